// SPDX-License-Identifier: Apache-2.0
// What crosses the units of the multi-GPU exchange (transport.cpp, range_partition.hip, shuffle.cpp, collectives.hip): the flat-column
// form of a table, its hash-range split with the side stream of a pipelined shuffle, and the control round of the collectives.
#pragma once
#include <cudf/distributed.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime_api.h>

#include <cstdint>
#include <memory>
#include <span>
#include <utility>
#include <vector>

namespace cudf {
namespace distributed {
namespace detail {

constexpr int RP_MAX_PARTS = 64;  // destinations of one split = ranks of one communicator (the scan kernel gives each one lane of a wave)

// The columns that travel: the input columns, then one validity-byte column per column listed in `with_validity`.
struct flat_table {
  std::vector<column_view> cols;            // what is partitioned / exchanged
  std::vector<int> validity_of;             // cols[ninput + j] holds the validity bytes of input column validity_of[j]
  std::vector<rmm::device_buffer> temps;    // the byte columns' storage
  int ninput{0};
};
// validity-carrying columns of `t` as the bits `flatten` takes
uint64_t nullable_bits(table_view const& t);
flat_table flatten(table_view const& input, uint64_t with_validity, hipStream_t s);
// buffers of the flat columns (nrows rows each) -> owning table with the input's types and re-packed validity
std::unique_ptr<table> assemble(table_view const& like, flat_table const& f, std::vector<rmm::device_buffer>&& bufs, int64_t nrows,
                                stream_ref stream, rmm::device_async_resource_ref mr);

// The side stream of a pipelined shuffle: column c of the local split is scattered there while the exchange of the columns before it
// runs on the caller's stream; column_ready[c] is recorded behind column c's scatter (reference: the chunked pipeline of
// cpp/libcudf_streaming/src/partition.cpp:20-88 overlaps partition and exchange chunk by chunk; here the unit is a column).
struct scatter_pipeline {
  hipStream_t side{nullptr};
  hipEvent_t scan_done{nullptr};
  std::vector<hipEvent_t> column_ready;
  scatter_pipeline() = default;
  scatter_pipeline(scatter_pipeline const&)            = delete;
  scatter_pipeline& operator=(scatter_pipeline const&) = delete;
  void open(std::size_t ncols)
  {
    CUDF_HIP_TRY(hipStreamCreateWithFlags(&side, hipStreamNonBlocking));
    CUDF_HIP_TRY(hipEventCreateWithFlags(&scan_done, hipEventDisableTiming));
    column_ready.assign(ncols, nullptr);
    for (auto& e : column_ready) CUDF_HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  ~scatter_pipeline()
  {
    if (side != nullptr) (void)hipStreamSynchronize(side);  // (nothing of this call may outlive its buffers, whatever path left the scope)
    for (auto e : column_ready)
      if (e != nullptr) (void)hipEventDestroy(e);
    if (scan_done != nullptr) (void)hipEventDestroy(scan_done);
    if (side != nullptr) (void)hipStreamDestroy(side);
  }
};

// Partitions the flat columns by the hash range of `hashed`'s rows; returns one buffer per flat column and N + 1 offsets.
// pipe != nullptr: the offsets are final on return but the columns are not - column c's buffer is complete once pipe->column_ready[c]
// has happened (the caller makes its stream wait for that event before it reads the buffer).
std::pair<std::vector<rmm::device_buffer>, std::vector<int64_t>> partition_flat(flat_table const& f, table_view const& hashed, int N,
                                                                                stream_ref stream, rmm::device_async_resource_ref mr,
                                                                                scatter_pipeline* pipe = nullptr);

// One control round: every rank contributes `mine` (the same length on every rank) and receives the contributions of ranks 0, 1, ...
// back to back on the host. One host-to-device copy, one all_gather, one device-to-host copy, one synchronisation of `s`.
std::vector<int64_t> all_gather_host(communicator& comm, std::span<int64_t const> mine, hipStream_t s);

}  // namespace detail
}  // namespace distributed
}  // namespace cudf

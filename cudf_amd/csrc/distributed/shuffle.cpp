// SPDX-License-Identifier: Apache-2.0
// The exchange of table rows by key ownership (include/cudf/distributed.hpp): control rounds, the host-side plan, and the payload
// rounds of point-to-point messages over a `transport`. Role of the reference's cpp/libcudf_streaming/src/partition_utils.cpp:72-185
// (hash_partition -> pack -> shuffle -> unpack). Host code only: the kernels of the local split are in range_partition.hip.
#include "../common/device_table.hpp"
#include "../common/profiler.hpp"
#include "detail.hpp"

#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <limits>

namespace cudf {
namespace distributed {
namespace {
using cudf::detail::MAX_COLS;

// Closes an open group when the scope is left by an exception (a failed Send between GroupStart and GroupEnd used to leave the
// group open for ever).
class group_scope {
 public:
  explicit group_scope(transport& t) : _t{t} { _t.group_start(); }
  void end()
  {
    _open = false;
    _t.group_end();
  }
  ~group_scope()
  {
    if (_open) {
      try {
        _t.group_end();
      } catch (...) {
      }
    }
  }
  group_scope(group_scope const&)            = delete;
  group_scope& operator=(group_scope const&) = delete;

 private:
  transport& _t;
  bool _open{true};
};
}  // namespace

std::vector<int64_t> detail::all_gather_host(communicator& comm, std::span<int64_t const> mine, hipStream_t s)
{
  auto tmp = cudf::get_current_device_resource_ref();
  rmm::device_buffer d_mine{mine.size_bytes(), s, tmp}, d_all{mine.size_bytes() * comm.size(), s, tmp};
  std::vector<int64_t> h_all(mine.size() * comm.size(), 0);
  CUDF_HIP_TRY(hipMemcpyAsync(d_mine.data(), mine.data(), d_mine.size(), hipMemcpyHostToDevice, s));
  comm.link().all_gather(d_mine.data(), d_all.data(), mine.size(), s);
  CUDF_HIP_TRY(hipMemcpyAsync(h_all.data(), d_all.data(), d_all.size(), hipMemcpyDeviceToHost, s));
  CUDF_HIP_TRY(hipStreamSynchronize(s));
  return h_all;
}

exchange_plan plan_exchange(std::vector<std::int64_t> const& counts, int world, int me)
{
  CUDF_EXPECTS(world >= 1 && me >= 0 && me < world && counts.size() == static_cast<std::size_t>(world) * world,
               "plan_exchange: a world x world count matrix and a rank inside the world", std::invalid_argument);
  exchange_plan ep;
  ep.recv_count.resize(world);
  ep.recv_offset.assign(static_cast<std::size_t>(world) + 1, 0);
  for (int p = 0; p < world; ++p) {
    ep.recv_count[p]      = counts[static_cast<std::size_t>(p) * world + me];
    ep.recv_offset[p + 1] = ep.recv_offset[p] + ep.recv_count[p];
    for (int q = 0; q < world; ++q)
      if (p != q) ep.biggest = std::max(ep.biggest, counts[static_cast<std::size_t>(p) * world + q]);  // (the own slice is a device copy)
  }
  return ep;
}

// ------------------------------------------------------------------ shuffle
std::unique_ptr<table> shuffle(table_view const& input, std::vector<size_type> const& key_columns, communicator& comm, stream_ref stream,
                               rmm::device_async_resource_ref mr)
{
  CUDF_FUNC_RANGE();
  try {
    hipStream_t const s = stream.value();
    int const N = comm.size(), me = comm.rank();
    transport& link = comm.link();
    auto tmp        = cudf::get_current_device_resource_ref();
    // (the exact limit - 16 flat columns, a column with nulls on any rank counting twice - is known after round 0; flatten checks it
    // on every rank with the same verdict)
    CUDF_EXPECTS(input.num_columns() >= 1 && input.num_columns() <= MAX_COLS,
                 "shuffle: 1 to 16 flat columns (a column with nulls on any rank counts twice: its validity travels as a byte column)",
                 std::invalid_argument);
    auto const hashed = input.select(key_columns);
    CUDF_EXPECTS(hashed.num_columns() >= 1, "shuffle: at least one key column", std::invalid_argument);

    // ---- round 0 of the control traffic: which columns carry nulls on ANY rank (they travel with validity bytes everywhere)
    // (both rounds carry N + 1 values per rank: the rows for every destination, then the null bits)
    std::vector<int64_t> h_send(static_cast<std::size_t>(N) + 1, 0);
    h_send[N]  = static_cast<int64_t>(detail::nullable_bits(input));
    auto h_all = detail::all_gather_host(comm, h_send, s);
    uint64_t with_validity = 0;
    for (int p = 0; p < N; ++p) with_validity |= static_cast<uint64_t>(h_all[static_cast<std::size_t>(p) * (N + 1) + N]);

    // ---- local split by owner rank
    auto f = detail::flatten(input, with_validity, s);
    // (the columns are scattered one per launch on a side stream: the count exchange below and the payload rounds of column c run
    // beside the scatter of the columns after c; one column takes one fused scatter on the caller's stream.)
    detail::scatter_pipeline pipe;  // (partition_flat returns with `s` waiting for the last column's event: buffers released on `s` are safe)
    if (f.cols.size() > 1) pipe.open(f.cols.size());
    auto [bufs, off] = detail::partition_flat(f, hashed, N, stream, tmp, pipe.side != nullptr ? &pipe : nullptr);

    // ---- counts: every rank learns what every rank sends to every rank
    for (int p = 0; p < N; ++p) h_send[p] = off[p + 1] - off[p];
    h_all = detail::all_gather_host(comm, h_send, s);
    std::vector<int64_t> matrix(static_cast<std::size_t>(N) * N);
    for (int p = 0; p < N; ++p)
      for (int q = 0; q < N; ++q) matrix[static_cast<std::size_t>(p) * N + q] = h_all[static_cast<std::size_t>(p) * (N + 1) + q];
    exchange_plan const ep    = plan_exchange(matrix, N, me);
    auto const& rcnt          = ep.recv_count;
    auto const& roff          = ep.recv_offset;
    int64_t const biggest     = ep.biggest;  // the largest (sender, receiver) message in rows: every rank runs the same number of rounds
    int64_t const total       = roff[N];
    CUDF_EXPECTS(total <= std::numeric_limits<size_type>::max(), "shuffle: a rank would receive more rows than a column holds", std::overflow_error);

    // ---- payload: per column, group_start { send / recv per peer } group_end in rounds of bounded messages (RCCL: ncclGroupStart /
    // ncclSend / ncclRecv / ncclGroupEnd); the own slice is a device copy
    int64_t const max_message_bytes = comm.max_message_bytes();
    std::vector<rmm::device_buffer> recv;
    cudf::detail::prof::scope p_{"shuffle_exchange", s};
    for (std::size_t c = 0; c < f.cols.size(); ++c) {
      int64_t const w = static_cast<int64_t>(size_of_id(f.cols[c].type().id()));
      if (pipe.side != nullptr) CUDF_HIP_TRY(hipStreamWaitEvent(s, pipe.column_ready[c], 0));  // column c has been scattered
      recv.emplace_back(static_cast<std::size_t>(std::max<int64_t>(total, 1) * w), s, c < static_cast<std::size_t>(f.ninput) ? mr : tmp);
      char const* src = static_cast<char const*>(bufs[c].data());
      char* dst       = static_cast<char*>(recv.back().data());
      if (h_send[me] > 0)
        CUDF_HIP_TRY(hipMemcpyAsync(dst + roff[me] * w, src + off[me] * w, static_cast<std::size_t>(h_send[me] * w), hipMemcpyDeviceToDevice, s));
      int64_t const chunk = std::max<int64_t>(1, max_message_bytes / w);
      for (int64_t done = 0; done < biggest; done += chunk) {
        group_scope group{link};  // (closed on every path out of this scope: a failed send does not leave the group open)
        for (int p = 0; p < N; ++p) {
          if (p == me) continue;
          int64_t const sb = std::min(done, h_send[p]), se = std::min(done + chunk, h_send[p]);
          if (se > sb) link.send(src + (off[p] + sb) * w, static_cast<std::size_t>((se - sb) * w), p, s);
          int64_t const rb = std::min(done, rcnt[p]), re = std::min(done + chunk, rcnt[p]);
          if (re > rb) link.recv(dst + (roff[p] + rb) * w, static_cast<std::size_t>((re - rb) * w), p, s);
        }
        group.end();
      }
    }
    return detail::assemble(input, f, std::move(recv), total, stream, mr);
  } catch (...) {
    comm.link().abort();  // (validation, an allocation, a too-long receive: the peers are told instead of waiting in the next collective)
    throw;
  }
}

}  // namespace distributed
}  // namespace cudf

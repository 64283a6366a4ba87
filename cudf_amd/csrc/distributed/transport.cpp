// SPDX-License-Identifier: Apache-2.0
// The communication layer of the multi-GPU exchange (include/cudf/distributed.hpp): RCCL bound at run time, the RCCL and LOOPBACK
// implementations of `transport`, and `communicator`. Host code only: HIP runtime calls, no kernels.
#include "../common/env.hpp"
#include "detail.hpp"

#include <cudf/distributed.hpp>
#include <cudf/utilities/error.hpp>

#include <dlfcn.h>
#include <hip/hip_runtime_api.h>
#include <rccl/rccl.h>

#include <chrono>
#include <condition_variable>
#include <cstring>
#include <mutex>
#include <string>

namespace cudf {
namespace distributed {
namespace {
// ------------------------------------------------------------------ RCCL, resolved at run time
struct rccl_api {
  decltype(&ncclGetUniqueId) GetUniqueId{};
  decltype(&ncclCommInitRank) CommInitRank{};
  decltype(&ncclCommDestroy) CommDestroy{};
  decltype(&ncclAllGather) AllGather{};
  decltype(&ncclSend) Send{};
  decltype(&ncclRecv) Recv{};
  decltype(&ncclGroupStart) GroupStart{};
  decltype(&ncclGroupEnd) GroupEnd{};
  decltype(&ncclGetErrorString) GetErrorString{};
};
rccl_api const& rccl()
{
  static rccl_api api = [] {
    rccl_api a{};
    // a copy already in the process (torch.distributed's) is reused; otherwise ROCm's
    void* h = nullptr;
    for (char const* name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
      h = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
      if (h != nullptr) break;
    }
    CUDF_EXPECTS(h != nullptr, "librccl.so could not be loaded: the multi-GPU exchange needs RCCL");
    auto sym = [&](char const* n) {
      void* p = dlsym(h, n);
      CUDF_EXPECTS(p != nullptr, std::string{"librccl.so lacks "} + n);
      return p;
    };
    a.GetUniqueId    = reinterpret_cast<decltype(a.GetUniqueId)>(sym("ncclGetUniqueId"));
    a.CommInitRank   = reinterpret_cast<decltype(a.CommInitRank)>(sym("ncclCommInitRank"));
    a.CommDestroy    = reinterpret_cast<decltype(a.CommDestroy)>(sym("ncclCommDestroy"));
    a.AllGather      = reinterpret_cast<decltype(a.AllGather)>(sym("ncclAllGather"));
    a.Send           = reinterpret_cast<decltype(a.Send)>(sym("ncclSend"));
    a.Recv           = reinterpret_cast<decltype(a.Recv)>(sym("ncclRecv"));
    a.GroupStart     = reinterpret_cast<decltype(a.GroupStart)>(sym("ncclGroupStart"));
    a.GroupEnd       = reinterpret_cast<decltype(a.GroupEnd)>(sym("ncclGroupEnd"));
    a.GetErrorString = reinterpret_cast<decltype(a.GetErrorString)>(sym("ncclGetErrorString"));
    return a;
  }();
  return api;
}
#define CUDF_RCCL_TRY(call)                                                                              \
  do {                                                                                                   \
    ncclResult_t const r_ = (call);                                                                      \
    if (r_ != ncclSuccess) CUDF_FAIL(std::string{"RCCL error: "} + rccl().GetErrorString(r_) + " in " #call); \
  } while (0)

// ------------------------------------------------------------------ transports
class rccl_transport final : public transport {
 public:
  rccl_transport(unique_id const& id, int world_size, int rank)
  {
    ncclUniqueId nid;
    std::memcpy(&nid, id.data(), sizeof(nid));
    CUDF_RCCL_TRY(rccl().CommInitRank(&_comm, world_size, nid, rank));
  }
  ~rccl_transport() override
  {
    if (_comm != nullptr) (void)rccl().CommDestroy(_comm);
  }
  void all_gather(void const* send, void* recv, std::size_t count_int64, hipStream_t stream) override
  {
    CUDF_RCCL_TRY(rccl().AllGather(send, recv, count_int64, ncclInt64, _comm, stream));
  }
  void group_start() override { CUDF_RCCL_TRY(rccl().GroupStart()); }
  void send(void const* buf, std::size_t bytes, int peer, hipStream_t stream) override
  {
    CUDF_RCCL_TRY(rccl().Send(buf, bytes, ncclInt8, peer, _comm, stream));
  }
  void recv(void* buf, std::size_t bytes, int peer, hipStream_t stream) override
  {
    CUDF_RCCL_TRY(rccl().Recv(buf, bytes, ncclInt8, peer, _comm, stream));
  }
  void group_end() override { CUDF_RCCL_TRY(rccl().GroupEnd()); }
  [[nodiscard]] void* native_handle() const noexcept override { return _comm; }

 private:
  ncclComm_t _comm{};
};

// Loopback: V virtual ranks in one process on one device, one host thread per rank. A collective is a rendezvous of the V
// threads: every rank drains its stream (its buffers are complete), publishes its pointers, and after the barrier copies what it
// RECEIVES with device copies on its own stream; a second barrier releases the senders' buffers. Sends and receives between two
// ranks match in the order they were posted, as RCCL's do.
struct loopback_hub {
  explicit loopback_hub(int v) : world{v}, ag_send(v, nullptr), sends(v) {}
  struct posted {
    int peer;
    void const* buf;
    std::size_t bytes;
  };
  int const world;
  std::mutex mu;
  std::condition_variable cv;
  int arrived{0};
  std::uint64_t generation{0};
  bool failed{false};
  std::vector<void const*> ag_send;         // all_gather: every rank's send buffer
  std::vector<std::vector<posted>> sends;   // group: what every rank sends, in posting order
  void barrier()
  {
    std::unique_lock<std::mutex> lk{mu};
    CUDF_EXPECTS(!failed, "loopback transport: another rank failed");
    std::uint64_t const gen = generation;
    if (++arrived == world) {
      arrived = 0;
      ++generation;
      cv.notify_all();
      return;
    }
    // (a deadline as well: a rank that died without telling anybody must not park its peers - and the device buffers they hold - for ever)
    bool const released = cv.wait_for(lk, std::chrono::seconds(barrier_timeout_s()), [&] { return generation != gen || failed; });
    if (!released) {
      failed = true;
      cv.notify_all();
    }
    CUDF_EXPECTS(released, "loopback transport: a rank did not reach the collective within CUDF_AMD_LOOPBACK_TIMEOUT_S");
    CUDF_EXPECTS(!failed || generation != gen, "loopback transport: another rank failed");
  }
  void fail()
  {
    std::lock_guard<std::mutex> lk{mu};
    failed = true;
    cv.notify_all();
  }
  static long barrier_timeout_s()
  {
    int64_t const x = cudf::detail::env_i64("CUDF_AMD_LOOPBACK_TIMEOUT_S", 0);
    return x > 0 ? static_cast<long>(x) : 120L;
  }
};
class loopback_transport final : public transport {
 public:
  loopback_transport(std::shared_ptr<loopback_hub> hub, int rank) : _hub{std::move(hub)}, _rank{rank} {}
  void all_gather(void const* send, void* recv, std::size_t count_int64, hipStream_t stream) override
  {
    guarded([&] {
      CUDF_HIP_TRY(hipStreamSynchronize(stream));
      _hub->ag_send[_rank] = send;
      _hub->barrier();
      std::size_t const bytes = count_int64 * sizeof(int64_t);
      for (int p = 0; p < _hub->world; ++p)
        CUDF_HIP_TRY(hipMemcpyAsync(static_cast<char*>(recv) + p * bytes, _hub->ag_send[p], bytes, hipMemcpyDeviceToDevice, stream));
      CUDF_HIP_TRY(hipStreamSynchronize(stream));
      _hub->barrier();
    });
  }
  void group_start() override
  {
    CUDF_EXPECTS(!_open, "loopback transport: group already open");
    _open = true;
    _sends.clear();
    _recvs.clear();
    _stream = nullptr;
  }
  void send(void const* buf, std::size_t bytes, int peer, hipStream_t stream) override
  {
    CUDF_EXPECTS(_open && peer >= 0 && peer < _hub->world, "loopback transport: send outside a group or to a rank outside the world");
    _sends.push_back({peer, buf, bytes});
    _stream = stream;
  }
  void recv(void* buf, std::size_t bytes, int peer, hipStream_t stream) override
  {
    CUDF_EXPECTS(_open && peer >= 0 && peer < _hub->world, "loopback transport: recv outside a group or from a rank outside the world");
    _recvs.push_back({peer, buf, bytes});
    _stream = stream;
  }
  void group_end() override
  {
    CUDF_EXPECTS(_open, "loopback transport: no open group");
    _open = false;
    guarded([&] {
      CUDF_HIP_TRY(hipStreamSynchronize(_stream));  // what this rank sends is complete
      _hub->sends[_rank] = _sends;
      _hub->barrier();
      std::vector<std::size_t> next(static_cast<std::size_t>(_hub->world), 0);  // per source: its next unmatched send to this rank
      for (auto const& r : _recvs) {
        auto const& from = _hub->sends[r.peer];
        std::size_t& i   = next[r.peer];
        while (i < from.size() && from[i].peer != _rank) ++i;
        CUDF_EXPECTS(i < from.size(), "loopback transport: a receive without a matching send");
        CUDF_EXPECTS(from[i].bytes == r.bytes, "loopback transport: send and receive sizes differ");
        CUDF_HIP_TRY(hipMemcpyAsync(const_cast<void*>(r.buf), from[i].buf, r.bytes, hipMemcpyDeviceToDevice, _stream));
        ++i;
      }
      for (int p = 0; p < _hub->world; ++p) {  // every send to this rank must have been received
        auto const& from = _hub->sends[p];
        std::size_t i    = next[p];
        while (i < from.size() && from[i].peer != _rank) ++i;
        CUDF_EXPECTS(i == from.size(), "loopback transport: a send without a matching receive");
      }
      CUDF_HIP_TRY(hipStreamSynchronize(_stream));
      _hub->barrier();  // the senders' buffers are free again
    });
  }

 private:
  template <typename F>
  void guarded(F&& f)
  {
    try {
      f();
    } catch (...) {
      _hub->fail();  // the other ranks leave their barriers with an error instead of waiting for ever
      throw;
    }
  }

 public:
  void abort() noexcept override { _hub->fail(); }

 private:
  std::shared_ptr<loopback_hub> _hub;
  int _rank;
  bool _open{false};
  std::vector<loopback_hub::posted> _sends, _recvs;
  hipStream_t _stream{nullptr};
};
}  // namespace

// ------------------------------------------------------------------ communicator
unique_id communicator::make_unique_id()
{
  ncclUniqueId id;
  CUDF_RCCL_TRY(rccl().GetUniqueId(&id));
  unique_id out{};
  static_assert(sizeof(id) == UNIQUE_ID_BYTES);
  std::memcpy(out.data(), &id, sizeof(id));
  return out;
}
communicator::communicator(std::unique_ptr<transport> t, int world_size, int rank) : _transport{std::move(t)}, _world{world_size}, _rank{rank} {}
communicator::communicator(unique_id const& id, int world_size, int rank) : _world{world_size}, _rank{rank}
{
  CUDF_EXPECTS(world_size >= 1 && rank >= 0 && rank < world_size, "communicator: rank outside the world", std::invalid_argument);
  _transport = std::make_unique<rccl_transport>(id, world_size, rank);
}
std::vector<std::unique_ptr<communicator>> communicator::make_loopback(int world_size)
{
  CUDF_EXPECTS(world_size >= 1 && world_size <= detail::RP_MAX_PARTS, "communicator: a loopback world of 1 to 64 ranks", std::invalid_argument);
  auto hub = std::make_shared<loopback_hub>(world_size);
  std::vector<std::unique_ptr<communicator>> out;
  for (int r = 0; r < world_size; ++r)
    out.push_back(std::unique_ptr<communicator>{new communicator{std::make_unique<loopback_transport>(hub, r), world_size, r}});
  return out;
}
communicator::~communicator() = default;
void communicator::set_max_message_bytes(std::int64_t bytes)
{
  CUDF_EXPECTS(bytes >= 8, "communicator: a message holds at least one 8-byte element", std::invalid_argument);
  _max_message_bytes = bytes;
}

}  // namespace distributed
}  // namespace cudf

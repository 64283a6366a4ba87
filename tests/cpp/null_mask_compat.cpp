// The null-mask functions of include/cudf/null_mask.hpp called directly, at the bit offsets and sizes where their kernels change
// path: cudf::null_count (k_count_unset: the funnel shift across a word boundary up to the last word, the tail of fewer than 32 live
// bits, the second round of the grid-stride loop), cudf::bitmask_and (k_bitmask_and: one to three sliced masks, one block of words
// and one bit more), cudf::column{sliced view} (the mask rebased to bit 0, the null count of the slice), cudf::create_null_mask and
// cudf::bitmask_allocation_size_bytes. Host masks come from a fixed LCG; every result is compared with a plain host bit loop.
// Every device mask is sized with bitmask_allocation_size_bytes, as a caller would size it.
#include <cudf/column/column.hpp>
#include <cudf/null_mask.hpp>
#include <cudf/table/table_view.hpp>
#include <cudf/utilities/error.hpp>

#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <vector>

#define CHECK(cond)                                                            \
  do {                                                                         \
    if (!(cond)) {                                                             \
      std::fprintf(stderr, "FAILED %s at %s:%d\n", #cond, __FILE__, __LINE__); \
      return 1;                                                                \
    }                                                                          \
  } while (0)
#define HIP_OK(call) CHECK((call) == hipSuccess)

using cudf::bitmask_type;
using cudf::size_type;

static uint64_t g_lcg = 0x9e3779b97f4a7c15ull;
static uint32_t next_word()
{
  g_lcg = g_lcg * 6364136223846793005ull + 1442695040888963407ull;
  return static_cast<uint32_t>(g_lcg >> 32);
}

// A host mask of `bits` bits in an allocation of bitmask_allocation_size_bytes(bits), every word of it random, and its device copy.
struct mask {
  std::vector<bitmask_type> host;
  bitmask_type* dev{};
  explicit mask(size_type bits, bool dense = false) : host(cudf::bitmask_allocation_size_bytes(bits) / sizeof(bitmask_type))
  {
    for (auto& w : host) {
      w = next_word();
      if (dense) w |= next_word();  // (denser masks: an AND of three keeps some set bits)
    }
    (void)hipMalloc(&dev, host.size() * sizeof(bitmask_type));
    (void)hipMemcpy(dev, host.data(), host.size() * sizeof(bitmask_type), hipMemcpyHostToDevice);
  }
  ~mask() { (void)hipFree(dev); }
  mask(mask const&)            = delete;
  mask& operator=(mask const&) = delete;
  [[nodiscard]] bool bit(int64_t i) const { return (host[i >> 5] >> (i & 31)) & 1u; }
  [[nodiscard]] int64_t unset(int64_t start, int64_t stop) const
  {
    int64_t n = 0;
    for (int64_t i = start; i < stop; ++i) n += !bit(i);
    return n;
  }
};

static std::vector<bitmask_type> words_of(void const* dev, std::size_t bytes)
{
  std::vector<bitmask_type> h(bytes / sizeof(bitmask_type));
  (void)hipMemcpy(h.data(), dev, h.size() * sizeof(bitmask_type), hipMemcpyDeviceToHost);
  return h;
}

static int test_allocation_and_create()
{
  CHECK(cudf::bitmask_allocation_size_bytes(0) == 0);
  CHECK(cudf::bitmask_allocation_size_bytes(1) == 64);
  CHECK(cudf::bitmask_allocation_size_bytes(512) == 64);
  CHECK(cudf::bitmask_allocation_size_bytes(513) == 128);
  for (size_type n : {1, 63, 64, 65, 513}) {
    for (auto state : {cudf::mask_state::ALL_VALID, cudf::mask_state::ALL_NULL}) {
      auto buf = cudf::create_null_mask(n, state);
      CHECK(buf.size() == cudf::bitmask_allocation_size_bytes(n));
      HIP_OK(hipDeviceSynchronize());
      auto const h = words_of(buf.data(), buf.size());
      for (size_type i = 0; i < n; ++i) CHECK(((h[i >> 5] >> (i & 31)) & 1u) == (state == cudf::mask_state::ALL_VALID ? 1u : 0u));
      CHECK(cudf::null_count(static_cast<bitmask_type const*>(buf.data()), 0, n) == (state == cudf::mask_state::ALL_VALID ? 0 : n));
    }
  }
  CHECK(cudf::create_null_mask(100, cudf::mask_state::UNALLOCATED).size() == 0);
  CHECK(cudf::create_null_mask(100, cudf::mask_state::UNINITIALIZED).size() == 64);
  return 0;
}

static int test_null_count()
{
  mask const m{9000};
  size_type const edges[] = {0, 1, 31, 32, 33, 63, 64, 65, 8191, 8192, 8193};
  for (size_type start : edges) {
    for (size_type stop : edges) {
      if (start > stop) {
        bool threw = false;
        try {
          (void)cudf::null_count(m.dev, start, stop);
        } catch (cudf::logic_error const&) {
          threw = true;
        }
        CHECK(threw);
        continue;
      }
      size_type const got = cudf::null_count(m.dev, start, stop);
      if (got != m.unset(start, stop)) {
        std::fprintf(stderr, "null_count(%d, %d) = %d, the host counts %lld\n", start, stop, got, static_cast<long long>(m.unset(start, stop)));
        return 1;
      }
      if (start == stop) CHECK(got == 0);
    }
  }
  CHECK(cudf::null_count(nullptr, 0, 9000) == 0);
  CHECK(cudf::null_count(nullptr, 5, 5) == 0);
  // 2^24 + 1056 bits from bit 5: 524,321 words against a grid of 2048 * 256 = 524,288 threads - the grid-stride loop's second round
  // holds the last 33 words, the last of them with 0 < live < 32 bits and its high half taken from the mask's last word
  size_type const big = (1 << 24) + 1061;
  mask const b{big};
  CHECK(cudf::null_count(b.dev, 5, big) == b.unset(5, big));
  CHECK(cudf::null_count(b.dev, 0, big) == b.unset(0, big));
  return 0;
}

static int test_bitmask_and()
{
  size_type const offsets[] = {0, 1, 31, 32, 37};
  cudf::data_type const i8{cudf::type_id::INT8};
  for (size_type n : {1, 31, 32, 33, 64, 65, 8191, 8192, 8193}) {
    mask const m0{n + 37, true}, m1{n + 37, true}, m2{n + 37, true};
    mask const* const ms[] = {&m0, &m1, &m2};
    void* data{};
    HIP_OK(hipMalloc(&data, static_cast<std::size_t>(n) + 37));  // (the data is never read: bitmask_and looks at masks only)
    for (int k = 1; k <= 3; ++k) {
      int combos = 1;
      for (int i = 0; i < k; ++i) combos *= 5;
      for (int combo = 0; combo < combos; ++combo) {
        size_type off[3] = {0, 0, 0};
        for (int i = 0, c = combo; i < k; ++i, c /= 5) off[i] = offsets[c % 5];
        std::vector<cudf::column_view> cols;
        for (int i = 0; i < k; ++i) {
          if (i == combo % (k + 1)) cols.emplace_back(i8, n, data, nullptr, 0, off[i]);  // a non-nullable column mixed in
          cols.emplace_back(i8, n, data, ms[i]->dev, static_cast<size_type>(ms[i]->unset(off[i], off[i] + n)), off[i]);
        }
        auto [buf, nulls] = cudf::bitmask_and(cudf::table_view{cols});
        CHECK(buf.size() == cudf::bitmask_allocation_size_bytes(n));
        auto const h      = words_of(buf.data(), buf.size());
        size_type unset   = 0;
        for (size_type r = 0; r < n; ++r) {
          bool expect = true;
          for (int i = 0; i < k; ++i) expect = expect && ms[i]->bit(static_cast<int64_t>(off[i]) + r);
          unset += !expect;
          if (((h[r >> 5] >> (r & 31)) & 1u) != (expect ? 1u : 0u)) {
            std::fprintf(stderr, "bitmask_and: n %d, %d masks at offsets %d %d %d: bit %d is %d\n", n, k, off[0], off[1], off[2], r, !expect);
            return 1;
          }
        }
        if (nulls != unset) {
          std::fprintf(stderr, "bitmask_and: n %d, %d masks at offsets %d %d %d: count %d, the host counts %d\n", n, k, off[0], off[1], off[2], nulls, unset);
          return 1;
        }
      }
    }
    // no nullable column: an empty buffer and a count of 0
    auto [none, zero] = cudf::bitmask_and(cudf::table_view{{cudf::column_view{i8, n, data, nullptr, 0, 3}}});
    CHECK(none.size() == 0 && zero == 0);
    HIP_OK(hipFree(data));
  }
  // no rows
  mask const m{64};
  auto [empty, zero] = cudf::bitmask_and(cudf::table_view{{cudf::column_view{i8, 0, nullptr, m.dev, 0, 0}}});
  CHECK(empty.size() == 0 && zero == 0);
  auto [nothing, zero2] = cudf::bitmask_and(cudf::table_view{});
  CHECK(nothing.size() == 0 && zero2 == 0);
  return 0;
}

static int test_column_copy_of_a_slice()
{
  for (size_type n : {1, 31, 32, 33, 64, 65, 8191, 8192, 8193}) {
    for (size_type off : {1, 37}) {
      mask const m{n + off};
      std::vector<int16_t> values(static_cast<std::size_t>(n) + off);
      for (auto& v : values) v = static_cast<int16_t>(next_word());
      int16_t* data{};
      HIP_OK(hipMalloc(&data, values.size() * sizeof(int16_t)));
      HIP_OK(hipMemcpy(data, values.data(), values.size() * sizeof(int16_t), hipMemcpyHostToDevice));
      size_type const nulls = static_cast<size_type>(m.unset(off, static_cast<int64_t>(off) + n));
      cudf::column_view const sliced{cudf::data_type{cudf::type_id::INT16}, n, data, m.dev, nulls, off};
      cudf::column const copy{sliced};
      HIP_OK(hipDeviceSynchronize());
      cudf::column_view const v = copy.view();
      CHECK(v.size() == n && v.offset() == 0 && v.nullable());
      CHECK(copy.null_count() == nulls && v.null_count() == nulls);
      CHECK(cudf::null_count(v.null_mask(), 0, n) == nulls);
      auto const h = words_of(v.null_mask(), cudf::bitmask_allocation_size_bytes(n));
      for (size_type r = 0; r < n; ++r) CHECK(((h[r >> 5] >> (r & 31)) & 1u) == (m.bit(static_cast<int64_t>(off) + r) ? 1u : 0u));
      std::vector<int16_t> got(n);
      HIP_OK(hipMemcpy(got.data(), v.head<int16_t>(), got.size() * sizeof(int16_t), hipMemcpyDeviceToHost));
      for (size_type r = 0; r < n; ++r) CHECK(got[r] == values[static_cast<std::size_t>(off) + r]);
      HIP_OK(hipFree(data));
    }
  }
  return 0;
}

int main()
{
  if (test_allocation_and_create()) return 1;
  if (test_null_count()) return 1;
  if (test_bitmask_and()) return 1;
  if (test_column_copy_of_a_slice()) return 1;
  HIP_OK(hipDeviceSynchronize());
  std::printf("null_mask_compat OK\n");
  return 0;
}

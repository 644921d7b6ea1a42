// The general-comparator tier of shp::sort / shp::stable_sort (dr/shp/
// merge_sort.hpp, detail::sort_general in dr/shp/sort.hpp) against
// std::stable_sort on a host copy.  The tier's result is bit-defined, so every
// check is a memcmp of the whole vector: no tolerance anywhere.  Everything
// goes through the public shp:: API, and no size below is taken from the
// header, so the suite keeps its value when the kernels underneath change.
//
// Every comparator looks at part of the element only (a few bits, or a key
// field with few distinct values) and the other bytes tell equivalent
// elements apart: a lost tie order, a dropped or a duplicated element changes
// the bytes.  The runner takes --devicesCount N (N segments duplicated on one
// GPU), --devices a,b,... (explicit device ids), --filter NAME and --modulus M
// as the sibling suites do.  Built twice: as is, and with
// -DDR_SHP_MSORT_SORT_THREADS=512 (first runs twice the merge tile).
#include <dr/shp.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <future>
#include <limits>
#include <random>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

struct TestCase {
  const char *name;
  void (*fn)();
};
static std::vector<TestCase> &registry() {
  static std::vector<TestCase> r;
  return r;
}
static bool g_cur_failed = false;
static long g_cases = 0, g_reported = 0;
#define TEST(N)                                                        \
  static void N();                                                     \
  static const int N##_reg = (registry().push_back({#N, &N}), 0);      \
  static void N()
#define EXPECT_TRUE(c)                                                            \
  do {                                                                            \
    if (!(c)) {                                                                   \
      std::printf("  %s:%d: EXPECT_TRUE(%s) failed\n", __FILE__, __LINE__, #c);   \
      g_cur_failed = true;                                                        \
    }                                                                             \
  } while (0)

// ------------------------------------------------------------ element types
// thirteen size classes; none has padding, so memcmp compares values
struct e3 {
  std::uint8_t k, a, b;
};
struct e12 {
  std::uint32_t key, wbits, serial; // wbits: a float's bit pattern
};
struct e16 {
  std::uint32_t key, serial, a, b;
};
struct e24 {
  std::uint64_t key, serial, c;
};
template <std::size_t S, std::size_t A> struct alignas(A) wide {
  std::uint32_t key, serial;
  std::uint8_t fill[S - 8];
};
using e32 = wide<32, 4>;
using e40 = wide<40, 4>;
using e64 = wide<64, 64>;
using e128 = wide<128, 4>;
using e256 = wide<256, 4>;

template <typename T, std::size_t S, std::size_t A> constexpr bool plain_bytes() {
  return std::has_unique_object_representations_v<T> && std::is_trivially_copyable_v<T> && sizeof(T) == S && alignof(T) == A;
}
static_assert(plain_bytes<std::uint8_t, 1, 1>());
static_assert(plain_bytes<std::uint16_t, 2, 2>());
static_assert(plain_bytes<e3, 3, 1>());
static_assert(plain_bytes<std::uint32_t, 4, 4>());
static_assert(plain_bytes<std::uint64_t, 8, 8>());
static_assert(plain_bytes<e12, 12, 4>());
static_assert(plain_bytes<e16, 16, 4>());
static_assert(plain_bytes<e24, 24, 8>());
static_assert(plain_bytes<e32, 32, 4>());
static_assert(plain_bytes<e40, 40, 4>());
static_assert(plain_bytes<e64, 64, 64>());
static_assert(plain_bytes<e128, 128, 4>());
static_assert(plain_bytes<e256, 256, 4>());
// float itself has no unique object representation (+0.0 == -0.0); it is
// compared through its bit pattern, which memcmp does
static_assert(sizeof(float) == 4 && std::numeric_limits<float>::is_iec559);

static const float kFloats[] = {0.0f, -0.0f, 1.5f, -1.5f, 0.0f, -0.0f, 2.0f, -3.25f, 1e-40f, -1e-40f, 1024.0f, 0.0f, -0.0f};
constexpr std::uint32_t kKeys = 17; // distinct keys of a random fill (16 where only 4 bits order)

static std::uint64_t mix(std::uint64_t x) {
  x += 0x9E3779B97F4A7C15ull;
  x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
  x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
  return x ^ (x >> 31);
}

// element number i with key k; r: random bits for the types too small for a serial
template <typename T> static T make(std::uint64_t i, std::uint32_t k, std::uint64_t r) {
  if constexpr (std::is_same_v<T, std::uint8_t>) return (std::uint8_t)(((k & 15) << 4) | (r & 15));
  else if constexpr (std::is_same_v<T, std::uint16_t>) return (std::uint16_t)(((k & 0xFF) << 8) | (r & 0xFF));
  else if constexpr (std::is_same_v<T, e3>) return e3{(std::uint8_t)k, (std::uint8_t)r, (std::uint8_t)(r >> 8)};
  else if constexpr (std::is_same_v<T, std::uint32_t>) return (std::uint32_t)(i << 4) | (k & 15);
  else if constexpr (std::is_same_v<T, float>) return kFloats[k % (sizeof(kFloats) / sizeof(float))];
  else if constexpr (std::is_same_v<T, std::uint64_t>) return (i << 8) | (k & 0xFF);
  else if constexpr (std::is_same_v<T, e12>) {
    const float w = 0.25f * (float)(i % 7) - 0.5f;
    std::uint32_t wb;
    std::memcpy(&wb, &w, 4);
    return e12{k, wb, (std::uint32_t)i};
  } else if constexpr (std::is_same_v<T, e16>) return e16{k, (std::uint32_t)i, ~(std::uint32_t)i, (std::uint32_t)i * 2654435761u};
  else if constexpr (std::is_same_v<T, e24>) return e24{k, i, ~i};
  else {
    T x;
    x.key = k;
    x.serial = (std::uint32_t)i;
    for (std::size_t j = 0; j < sizeof(x.fill); j++) x.fill[j] = (std::uint8_t)(i * 7 + j * 13 + (i >> 8));
    return x;
  }
}

// the order of every type: part of the element only
template <typename T> struct key_less {
  __host__ __device__ bool operator()(const T &a, const T &b) const {
    if constexpr (std::is_same_v<T, std::uint8_t>) return (a >> 4) < (b >> 4);
    else if constexpr (std::is_same_v<T, std::uint16_t>) return (a >> 8) < (b >> 8);
    else if constexpr (std::is_same_v<T, e3>) return a.k < b.k;
    else if constexpr (std::is_same_v<T, std::uint32_t>) return (a & 15) < (b & 15);
    else if constexpr (std::is_same_v<T, std::uint64_t>) return (a & 0xFF) < (b & 0xFF);
    else return a.key < b.key;
  }
};
template <typename T> static auto order_of() {
  if constexpr (std::is_same_v<T, float>) return [](float a, float b) { return a < b; };
  else return key_less<T>{};
}

template <typename T> static std::vector<T> random_fill(std::size_t n, std::uint64_t seed) {
  std::vector<T> h(n);
  for (std::size_t i = 0; i < n; i++) {
    const std::uint64_t r = mix(seed * 0x100000001B3ull + i);
    h[i] = make<T>(i, (std::uint32_t)(r % kKeys), r >> 20);
  }
  return h;
}

// ------------------------------------------------------------ the one helper
enum class api { sort, stable };

template <typename T> static bool same_bytes(const char *what, const std::vector<T> &got, const std::vector<T> &want) {
  const std::size_t n = want.size();
  if (got.size() == n && (n == 0 || std::memcmp(got.data(), want.data(), n * sizeof(T)) == 0)) return true;
  g_cur_failed = true;
  if (g_reported++ < 12) {
    std::size_t i = 0;
    while (i < n && i < got.size() && std::memcmp(&got[i], &want[i], sizeof(T)) == 0) i++;
    std::printf("  %s: %zu-byte elements, n = %zu, %zu segments: first difference at element %zu\n", what, sizeof(T), n,
                shp::nprocs(), i);
  }
  return false;
}

// std::stable_sort of [first, last).  Wide elements are sorted through their
// indices and gathered: the same order with less copying, and
// std::stable_sort's temporary buffer never holds an over-aligned element
// (it comes from a plain operator new).
template <typename T, typename Comp> static void host_stable_sort(T *first, T *last, Comp comp) {
  if constexpr (sizeof(T) >= 64 || alignof(T) > __STDCPP_DEFAULT_NEW_ALIGNMENT__) {
    std::vector<std::uint32_t> idx((std::size_t)(last - first));
    for (std::size_t i = 0; i < idx.size(); i++) idx[i] = (std::uint32_t)i;
    std::stable_sort(idx.begin(), idx.end(), [&](std::uint32_t a, std::uint32_t b) { return comp(first[a], first[b]); });
    std::vector<T> out(idx.size());
    for (std::size_t i = 0; i < idx.size(); i++) out[i] = first[idx[i]];
    std::copy(out.begin(), out.end(), first);
  } else {
    std::stable_sort(first, last, comp);
  }
}

// host vector -> distributed_vector, shp::sort / shp::stable_sort of
// [begin + a, end - b) under comp, std::stable_sort of the same stretch of the
// host copy, all bytes compared (so what lies outside must be unchanged)
template <typename T, typename Comp>
static bool sort_case(const char *what, std::vector<T> h, Comp comp, api which = api::sort, std::size_t a = 0,
                      std::size_t b = 0) {
  g_cases++;
  const std::size_t n = h.size();
  if (a + b > n) throw std::logic_error("sort_case: sub-range outside the vector");
  shp::distributed_vector<T> dv(n);
  if (n) shp::copy(h.begin(), h.end(), dv.begin());
  auto host = [&] { host_stable_sort(h.data() + a, h.data() + (n - b), comp); };
  // the host's sort runs beside the device's when it is long enough to matter
  std::future<void> ref;
  if (n >= 8192) ref = std::async(std::launch::async, host);
  else host();
  try {
    if (a == 0 && b == 0) {
      if (which == api::stable) shp::stable_sort(shp::par_unseq, dv, comp);
      else shp::sort(shp::par_unseq, dv, comp);
    } else {
      if (which == api::stable) shp::stable_sort(shp::par_unseq, dv.begin() + (std::ptrdiff_t)a, dv.end() - (std::ptrdiff_t)b, comp);
      else shp::sort(shp::par_unseq, dv.begin() + (std::ptrdiff_t)a, dv.end() - (std::ptrdiff_t)b, comp);
    }
  } catch (...) {
    if (ref.valid()) ref.get();
    throw;
  }
  if (ref.valid()) ref.get();
  std::vector<T> got(n);
  if (n) shp::copy(dv.begin(), dv.end(), got.data());
  return same_bytes(what, got, h);
}

// ------------------------------------------------------------ sizes
static const std::size_t kTileMultiples[] = {256, 512, 768, 1024, 2048, 4096, 6144, 8192, 10240, 14336};
static const std::size_t kTileMultiplesSmall[] = {32768, 34816}; // element types of at most 16 bytes

// n = P m + d, d in {-1, 0, +1}: every segment ends on a tile edge, one past it, or one short of it
template <typename T> static void boundary_list(const char *what) {
  const std::size_t P = shp::nprocs();
  std::vector<std::size_t> ms(std::begin(kTileMultiples), std::end(kTileMultiples));
  if (sizeof(T) <= 16) ms.insert(ms.end(), std::begin(kTileMultiplesSmall), std::end(kTileMultiplesSmall));
  int c = 0;
  for (std::size_t m : ms)
    for (int d : {-1, 0, 1}) {
      const std::size_t n = P * m + (std::size_t)(std::ptrdiff_t)d;
      sort_case(what, random_fill<T>(n, 1000 * sizeof(T) + n), order_of<T>(), (c++ & 1) ? api::stable : api::sort);
    }
  // fewer elements than segments, empty segments
  if (P > 1)
    for (std::size_t n = 0; n <= 3 * P + 2; n++)
      sort_case(what, random_fill<T>(n, 77 * sizeof(T) + n), order_of<T>(), (n & 1) ? api::stable : api::sort);
}

TEST(DenseSweep) {
  if (shp::nprocs() > 1) return; // with more segments: [0, 3 P + 2] for every type, in the boundary tests
  for (std::size_t n = 0; n <= 4100; n++)
    sort_case("dense u32", random_fill<std::uint32_t>(n, 5 + n), order_of<std::uint32_t>(), (n & 1) ? api::stable : api::sort);
  for (std::size_t n = 0; n <= 2100; n++)
    sort_case("dense e16", random_fill<e16>(n, 9 + n), order_of<e16>(), (n & 1) ? api::stable : api::sort);
}

TEST(Boundary1) { boundary_list<std::uint8_t>("u8 by the high nibble"); }
TEST(Boundary2) { boundary_list<std::uint16_t>("u16 by the high byte"); }
TEST(Boundary3) { boundary_list<e3>("3-byte struct by its first byte"); }
TEST(Boundary4) { boundary_list<std::uint32_t>("u32 by the low 4 bits"); }
TEST(Boundary4Float) { boundary_list<float>("float under a < b with signed zeros"); }
TEST(Boundary8) { boundary_list<std::uint64_t>("u64 by the low 8 bits"); }
TEST(Boundary12) { boundary_list<e12>("12-byte key / float / serial"); }
TEST(Boundary16) { boundary_list<e16>("16-byte struct by key"); }
TEST(Boundary24) { boundary_list<e24>("24-byte struct by key"); }
TEST(Boundary32) { boundary_list<e32>("32-byte struct by key"); }
TEST(Boundary40) { boundary_list<e40>("40-byte struct by key"); }
TEST(Boundary64) { boundary_list<e64>("64-byte struct, 64-byte aligned, by key"); }
TEST(Boundary128) { boundary_list<e128>("128-byte struct by key"); }
TEST(Boundary256) { boundary_list<e256>("256-byte struct by key"); }

// nine or more global passes
TEST(LongCase) {
  const std::size_t n = (std::size_t(1) << 20) + 3;
  sort_case("long u32", random_fill<std::uint32_t>(n, 4242), order_of<std::uint32_t>(), api::sort);
}

// ------------------------------------------------------------ key patterns
// value i of pattern p over n elements, and the pattern's greatest value
static const char *const kPatterns[] = {"ascending",     "descending", "all equal",       "two alternating", "sawtooth 2048",
                                        "sawtooth 2049", "organ pipe", "minimum is last", "maximum is first"};
static std::uint32_t pattern_value(int p, std::size_t i, std::size_t n) {
  switch (p) {
  case 0: return (std::uint32_t)i;
  case 1: return (std::uint32_t)(n - 1 - i);
  case 2: return 7;
  case 3: return (std::uint32_t)(i & 1);
  case 4: return (std::uint32_t)(i % 2048);
  case 5: return (std::uint32_t)(i % 2049);
  case 6: return (std::uint32_t)std::min(i, n - 1 - i);
  case 7: return i + 1 == n ? 0u : (std::uint32_t)(i + 1); // a one-element B survives every pass
  default: return i == 0 ? (std::uint32_t)n : (std::uint32_t)i;
  }
}

TEST(KeyPatterns) {
  const std::size_t P = shp::nprocs();
  for (std::size_t n : {P * 10240 + 1, P * 8192})
    for (int p = 0; p < 9; p++) {
      std::uint32_t vmax = 1;
      for (std::size_t i = 0; i < n; i++) vmax = std::max(vmax, pattern_value(p, i, n));
      // the pattern at full resolution (strictly monotone where it says so) ...
      std::vector<float> hf(n);
      std::vector<e16> hs(n);
      // ... and squeezed into few levels (0 stays alone at level 0): long runs of ties in the same shape
      std::vector<std::uint32_t> hu(n);
      std::vector<e16> hl(n);
      for (std::size_t i = 0; i < n; i++) {
        const std::uint32_t v = pattern_value(p, i, n);
        const std::uint32_t lvl = (std::uint32_t)(((std::uint64_t)v * 15 + vmax - 1) / vmax);
        hf[i] = p == 2 ? kFloats[i % 2] : (float)v - 100.0f; // all equal: +0.0 and -0.0 in turn
        hs[i] = make<e16>(i, v, 0);
        hu[i] = make<std::uint32_t>(i, lvl, 0);
        hl[i] = make<e16>(i, lvl, 0);
      }
      if (p == 2) { // equivalent throughout: the sort must move nothing
        auto lt = key_less<e16>{};
        for (std::size_t i = 1; i < n; i++) EXPECT_TRUE(!lt(hs[i - 1], hs[i]) && !lt(hs[i], hs[i - 1]));
      }
      sort_case(kPatterns[p], hf, order_of<float>(), api::sort);
      sort_case(kPatterns[p], hs, order_of<e16>(), api::stable);
      sort_case(kPatterns[p], hu, order_of<std::uint32_t>(), api::stable);
      sort_case(kPatterns[p], hl, order_of<e16>(), api::sort);
    }
}

// ------------------------------------------------------------ comparators with state
static volatile std::uint32_t g_modulus = 13; // --modulus: never a compile-time constant
struct by_modulus {
  std::uint32_t m;
  __host__ __device__ bool operator()(std::uint32_t a, std::uint32_t b) const { return a % m < b % m; }
};
// indices ordered by the table entry they name; the table is pinned host
// memory, so the host-side splitting and every device read the same bytes
struct by_table {
  const std::uint32_t *table;
  __host__ __device__ bool operator()(std::uint32_t a, std::uint32_t b) const { return table[a] < table[b]; }
};

static std::vector<std::size_t> state_sizes() {
  const std::size_t P = shp::nprocs();
  return {3 * P + 1, P * 2048 + 1, P * 10240 - 1, P * 14336};
}

TEST(RuntimeModulus) {
  const by_modulus comp{g_modulus};
  EXPECT_TRUE(comp.m >= 2);
  for (std::size_t n : state_sizes()) {
    std::vector<std::uint32_t> h(n);
    for (std::size_t i = 0; i < n; i++) h[i] = (std::uint32_t)mix(31 * n + i);
    sort_case("runtime modulus", h, comp, api::sort);
    sort_case("runtime modulus", h, comp, api::stable);
  }
}

TEST(IndirectThroughTable) {
  for (std::size_t n : state_sizes()) {
    std::uint32_t *table = nullptr;
    if (hipHostMalloc((void **)&table, n * sizeof(std::uint32_t), hipHostMallocPortable | hipHostMallocMapped) != hipSuccess)
      throw std::runtime_error("hipHostMalloc");
    for (std::size_t i = 0; i < n; i++) table[i] = (std::uint32_t)(mix(57 * n + i) % 11);
    std::vector<std::uint32_t> h(n);
    for (std::size_t i = 0; i < n; i++) h[i] = (std::uint32_t)i;
    std::mt19937_64 g(n);
    std::shuffle(h.begin(), h.end(), g);
    sort_case("indirect", h, by_table{table}, api::sort);
    sort_case("indirect", h, by_table{table}, api::stable);
    (void)hipHostFree(table);
  }
}

// ------------------------------------------------------------ segmentations
// [begin + a, end - b): pieces that start and end mid-segment
TEST(IteratorSubranges) {
  const std::size_t n = shp::nprocs() * 8192 + 5;
  int c = 0;
  for (std::size_t a : {1, 3, 2047, 2049})
    for (std::size_t b : {1, 3, 2047, 2049})
      sort_case("sub-range", random_fill<e16>(n, 600 + 10 * a + b), order_of<e16>(), (c++ & 1) ? api::stable : api::sort, a, b);
}

struct part_spec {
  std::size_t seg, off, len; // [off, off + len) of the vector's segment number seg
};
// a distributed_span over `parts` of a vector of nprocs() segments of S
// elements: the parts, in order, are one range; the rest of the vector stays
template <typename T> static void span_case(const char *what, std::size_t S, const std::vector<part_spec> &specs, std::uint64_t seed) {
  g_cases++;
  const std::size_t n = shp::nprocs() * S;
  std::vector<T> h = random_fill<T>(n, seed);
  shp::distributed_vector<T> dv(n);
  shp::copy(h.begin(), h.end(), dv.begin());
  const auto segs = dv.segments();
  std::vector<shp::device_span<T>> parts;
  std::vector<T> run;
  for (const part_spec &p : specs) {
    if (p.seg >= segs.size() || p.off + p.len > segs[p.seg].size()) throw std::logic_error("span_case: part outside its segment");
    parts.emplace_back(segs[p.seg].data() + p.off, p.len, segs[p.seg].rank());
    run.insert(run.end(), h.begin() + (std::ptrdiff_t)(p.seg * S + p.off), h.begin() + (std::ptrdiff_t)(p.seg * S + p.off + p.len));
  }
  shp::distributed_span ds(parts);
  EXPECT_TRUE(ds.size() == run.size());
  shp::sort(shp::par_unseq, ds, order_of<T>());
  host_stable_sort(run.data(), run.data() + run.size(), order_of<T>());
  std::size_t at = 0;
  for (const part_spec &p : specs) {
    std::copy(run.begin() + (std::ptrdiff_t)at, run.begin() + (std::ptrdiff_t)(at + p.len), h.begin() + (std::ptrdiff_t)(p.seg * S + p.off));
    at += p.len;
  }
  std::vector<T> got(n);
  shp::copy(dv.begin(), dv.end(), got.data());
  same_bytes(what, got, h);
}

TEST(SpanSegmentations) {
  const std::size_t P = shp::nprocs(), S = 10243;
  std::vector<part_spec> two, tiny, uneven;
  for (std::size_t r = 0; r < P; r++) {
    two.push_back({r, 0, S / 3});
    two.push_back({r, S / 3, S - S / 3});
    // zero-length and one-element parts; elements S - 3 and S - 1 of every segment stay out
    tiny.push_back({r, 5, 0});
    tiny.push_back({r, 5, 1});
    tiny.push_back({r, 6, 1});
    tiny.push_back({r, 7, S - 10});
    tiny.push_back({r, S - 3, 0});
    tiny.push_back({r, S - 2, 1});
  }
  // one part with 90 % of the elements, the rest in slivers
  const std::size_t big = 9 * S / 10, t = std::max<std::size_t>(1, S / (10 * P));
  uneven.push_back({0, 0, big});
  uneven.push_back({0, big, t});
  for (std::size_t r = 1; r < P; r++) uneven.push_back({r, 0, t});
  span_case<e16>("two parts per rank", S, two, 801);
  span_case<e16>("zero-length and one-element parts", S, tiny, 802);
  span_case<e16>("one part with 90 %", S, uneven, 803);
  span_case<e40>("two parts per rank", S, two, 804);
  span_case<e40>("zero-length and one-element parts", S, tiny, 805);
  span_case<e40>("one part with 90 %", S, uneven, 806);
  // nothing but empty parts
  span_case<e16>("only zero-length parts", S, {{0, 3, 0}, {P - 1, 9, 0}}, 807);
}

// ------------------------------------------------------------ radix tier, signed zeros
// equivalent keys may come out in any order there: the bit patterns are a
// permutation of the input's and the result is sorted under the comparator
template <typename F, typename U, typename Comp> static void signed_zero_case(std::size_t n, Comp comp, bool with_comp) {
  g_cases++;
  using L = std::numeric_limits<F>;
  const F vals[] = {F(0), -F(0), L::infinity(), -L::infinity(), L::denorm_min(), -L::denorm_min(), L::min() / 4, -L::min() / 4,
                    F(1), F(-1), F(3.5), F(-2.25), L::max(), -L::max(), L::min(), F(0), -F(0)};
  std::vector<F> h(n);
  for (std::size_t i = 0; i < n; i++) h[i] = vals[mix(91 * n + i) % (sizeof(vals) / sizeof(F))];
  shp::distributed_vector<F> dv(n);
  shp::copy(h.begin(), h.end(), dv.begin());
  if (with_comp) shp::sort(shp::par_unseq, dv, comp);
  else shp::sort(shp::par_unseq, dv);
  std::vector<F> got(n);
  shp::copy(dv.begin(), dv.end(), got.data());
  EXPECT_TRUE(std::is_sorted(got.begin(), got.end(), comp));
  std::vector<U> a(n), b(n);
  std::memcpy(a.data(), h.data(), n * sizeof(F));
  std::memcpy(b.data(), got.data(), n * sizeof(F));
  std::sort(a.begin(), a.end());
  std::sort(b.begin(), b.end());
  EXPECT_TRUE(a == b);
}

TEST(RadixSignedZeros) {
  const std::size_t P = shp::nprocs();
  for (std::size_t n : {3 * P + 1, std::size_t(1000), P * 4096 + 1, std::size_t(100003)}) {
    signed_zero_case<float, std::uint32_t>(n, std::less<>{}, false);
    signed_zero_case<float, std::uint32_t>(n, std::greater<>{}, true);
    signed_zero_case<double, std::uint64_t>(n, std::less<>{}, false);
    signed_zero_case<double, std::uint64_t>(n, std::greater<>{}, true);
  }
}

int main(int argc, char **argv) {
  unsigned dev_num = 0;
  std::string filter, dev_list;
  for (int i = 1; i < argc; i++) {
    std::string a = argv[i];
    if ((a == "-d" || a == "--devicesCount") && i + 1 < argc) dev_num = (unsigned)std::atoi(argv[++i]);
    else if (a.rfind("--devicesCount=", 0) == 0) dev_num = (unsigned)std::atoi(a.c_str() + 15);
    else if (a == "--filter" && i + 1 < argc) filter = argv[++i];
    else if (a == "--devices" && i + 1 < argc) dev_list = argv[++i];
    else if (a == "--modulus" && i + 1 < argc) g_modulus = (std::uint32_t)std::atoi(argv[++i]);
  }
  auto devices = shp::get_numa_devices();
  if (devices.empty()) {
    std::printf("no HIP device\n");
    return 2;
  }
  if (!dev_list.empty()) {
    std::vector<int> ids;
    for (std::size_t p = 0; p < dev_list.size();) {
      std::size_t q = dev_list.find(',', p);
      if (q == std::string::npos) q = dev_list.size();
      ids.push_back(std::atoi(dev_list.substr(p, q - p).c_str()));
      p = q + 1;
    }
    devices = ids;
  } else if (dev_num > 0) {
    devices = shp::get_duplicated_devices(devices, dev_num);
  }
  shp::init(devices);
  std::printf("segments: %zu on devices:", shp::nprocs());
  for (int d : shp::devices()) std::printf(" %d", d);
  std::printf("\nblock-sort threads: %d\n", (int)DR_SHP_MSORT_SORT_THREADS);
  int run = 0, failed = 0;
  for (auto &t : registry()) {
    if (!filter.empty() && std::string(t.name).find(filter) == std::string::npos) continue;
    g_cur_failed = false;
    try {
      t.fn();
    } catch (const std::exception &e) {
      std::printf("  exception: %s\n", e.what());
      g_cur_failed = true;
    }
    std::printf("[%s] MergeSort.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    std::fflush(stdout);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%ld sorts compared\n%d tests, %d failed\n", g_cases, run, failed);
  return failed ? 1 : 0;
}

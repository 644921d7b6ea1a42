// shp::reduce_by_key / run_length_encode / unique_copy
// (dr/shp/reduce_by_key.hpp) against a host loop over the host copy.  The
// reference has no by-key algorithm, so there is no gtest to restate; the
// runner takes --devicesCount N (N segments duplicated on one GPU) and
// --devices a,b,... (explicit device ids) as copy_if_tests does.
#include <dr/shp.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
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

// a key compared on `a` only: which key of a run is written is observable in b
struct pairkey {
  int a, b;
};
struct same_a {
  __host__ __device__ bool operator()(const pairkey &x, const pairkey &y) const { return x.a == y.a; }
};
// x -> a x + b (wrapping); compose(f, g) applies f first: associative, not commutative
struct affine {
  std::uint32_t a, b;
};
struct compose {
  __host__ __device__ affine operator()(const affine &f, const affine &g) const { return {f.a * g.a, f.b * g.a + g.b}; }
};
static_assert(sizeof(pairkey) == 8 && sizeof(affine) == 8);

template <typename T> static std::vector<T> to_host(const shp::distributed_vector<T> &dv) {
  std::vector<T> h(dv.size());
  shp::copy(dv.begin(), dv.end(), h.begin());
  return h;
}
template <typename T> static bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}
template <typename T> static T sentinel() {
  T t;
  std::memset(&t, 0xA5, sizeof(T));
  return t;
}
template <typename T> static shp::distributed_vector<T> to_device(const std::vector<T> &h) {
  shp::distributed_vector<T> d(h.size());
  shp::copy(h.begin(), h.end(), d.begin());
  return d;
}

// the host loop
template <typename K, typename V, typename Eq, typename Op>
static void host_rbk(const std::vector<K> &k, const std::vector<V> &v, std::vector<K> &ko, std::vector<V> &vo, Eq eq, Op op) {
  for (std::size_t i = 0; i < k.size(); i++) {
    if (i == 0 || !eq(k[i - 1], k[i])) {
      ko.push_back(k[i]);
      vo.push_back(v[i]);
    } else {
      vo.back() = op(vo.back(), v[i]);
    }
  }
}

// keys whose runs have the given mean length; neighbouring runs differ
static std::vector<int> run_keys(std::size_t n, double mean, std::uint64_t seed) {
  std::vector<int> k(n);
  std::mt19937_64 g(seed);
  std::bernoulli_distribution head(1.0 / mean);
  int cur = 0;
  for (std::size_t i = 0; i < n; i++) {
    if (i && head(g)) cur = (cur + 1 + (int)(g() % 5)) % 1000;
    k[i] = cur - 500;
  }
  return k;
}

// reduce_by_key, run_length_encode and unique_copy of (k, v) into whole
// outputs with room for n + 1, and into outputs that start `drop` elements
// into longer vectors (segmented differently from the inputs)
template <typename K, typename V, typename Eq, typename Op>
static void whole_case(const std::vector<K> &k, const std::vector<V> &v, Eq eq, Op op) {
  const std::size_t n = k.size();
  std::vector<K> wk;
  std::vector<V> wv;
  host_rbk(k, v, wk, wv, eq, op);
  std::vector<std::uint64_t> ones(n, 1), wc;
  {
    std::vector<K> tmp;
    host_rbk(k, ones, tmp, wc, eq, std::plus<>{});
  }
  const std::size_t runs = wk.size();
  auto dk = to_device(k);
  auto dv = to_device(v);
  for (std::size_t drop : {std::size_t(0), n / 3 + 1}) {
    const std::size_t len = n + 1 + drop;
    shp::distributed_vector<K> ok(len, sentinel<K>());
    shp::distributed_vector<V> ov(len, sentinel<V>());
    shp::distributed_vector<std::uint64_t> oc(len, sentinel<std::uint64_t>());
    std::vector<K> ek(len, sentinel<K>());
    std::vector<V> evv(len, sentinel<V>());
    std::vector<std::uint64_t> ec(len, sentinel<std::uint64_t>());
    std::copy(wk.begin(), wk.end(), ek.begin() + (std::ptrdiff_t)drop);
    std::copy(wv.begin(), wv.end(), evv.begin() + (std::ptrdiff_t)drop);
    std::copy(wc.begin(), wc.end(), ec.begin() + (std::ptrdiff_t)drop);
    {
      auto okv = ok | shp::views::drop(drop);
      auto ovv = ov | shp::views::drop(drop);
      auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk, dv, okv, ovv, eq, op);
      EXPECT_TRUE(ik == std::ranges::begin(okv) + (std::ptrdiff_t)runs);
      EXPECT_TRUE(iv == std::ranges::begin(ovv) + (std::ptrdiff_t)runs);
      EXPECT_TRUE(same_bits(to_host(ok), ek)); // the runs, then sentinels
      EXPECT_TRUE(same_bits(to_host(ov), evv));
    }
    {
      shp::distributed_vector<K> ok2(len, sentinel<K>());
      auto okv = ok2 | shp::views::drop(drop);
      auto ocv = oc | shp::views::drop(drop);
      auto [ik, ic] = shp::run_length_encode(shp::par_unseq, dk, okv, ocv, eq);
      EXPECT_TRUE(ik == std::ranges::begin(okv) + (std::ptrdiff_t)runs);
      EXPECT_TRUE(ic == std::ranges::begin(ocv) + (std::ptrdiff_t)runs);
      EXPECT_TRUE(same_bits(to_host(ok2), ek));
      EXPECT_TRUE(same_bits(to_host(oc), ec));
    }
    {
      shp::distributed_vector<K> ok3(len, sentinel<K>());
      auto okv = ok3 | shp::views::drop(drop);
      auto it = shp::unique_copy(shp::par_unseq, dk, okv, eq);
      EXPECT_TRUE(it == std::ranges::begin(okv) + (std::ptrdiff_t)runs);
      EXPECT_TRUE(same_bits(to_host(ok3), ek));
    }
  }
}

template <typename V> static std::vector<V> small_values(std::size_t n, std::uint64_t seed) {
  std::vector<V> v(n);
  std::mt19937_64 g(seed);
  for (auto &x : v) x = (V)(g() % 8); // float sums stay exact
  return v;
}

// n not a multiple of the segment count, n smaller than it (empty pieces), larger sizes
static std::vector<std::size_t> sizes() {
  const std::size_t P = shp::nprocs();
  return {0, 1, 2, P - 1, P, P + 1, 1000, 100003, (std::size_t(1) << 20) + 13};
}

TEST(IntKeysIntValues) {
  for (std::size_t n : sizes())
    for (double mean : {1.0, 3.0, 1000.0})
      whole_case(run_keys(n, mean, 1 + n), small_values<int>(n, 2 + n), std::equal_to<>{}, std::plus<>{});
}

TEST(Int64KeysDoubleValues) {
  for (std::size_t n : sizes()) {
    const std::vector<int> k32 = run_keys(n, 5.0, 3 + n);
    std::vector<std::int64_t> k(k32.begin(), k32.end());
    whole_case(k, small_values<double>(n, 4 + n), std::equal_to<>{}, std::plus<>{});
  }
}

TEST(FloatValuesMixedSizes) {
  const std::size_t n = 100003;
  const std::vector<int> k32 = run_keys(n, 40.0, 5);
  std::vector<std::int64_t> k64(k32.begin(), k32.end());
  whole_case(k32, small_values<float>(n, 6), std::equal_to<>{}, std::plus<>{});
  whole_case(k64, small_values<float>(n, 7), std::equal_to<>{}, std::plus<>{});
  whole_case(k32, small_values<double>(n, 8), std::equal_to<>{}, std::plus<>{});
}

// one run across every segment: its count and sum exact
TEST(AllKeysEqual) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 20) + 13}) {
    std::vector<int> k(n, 42);
    std::vector<std::uint64_t> v(n);
    for (std::size_t i = 0; i < n; i++) v[i] = i;
    whole_case(k, v, std::equal_to<>{}, std::plus<>{});
    auto dk = to_device(k);
    auto dv = to_device(v);
    shp::distributed_vector<int> ok(n, -7);
    shp::distributed_vector<std::uint64_t> ov(n, 0), oc(n, 0);
    auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk, dv, ok, ov);
    EXPECT_TRUE(ik == ok.begin() + 1 && iv == ov.begin() + 1);
    EXPECT_TRUE(to_host(ov)[0] == (std::uint64_t)n * (n - 1) / 2);
    shp::run_length_encode(shp::par_unseq, dk, ok, oc);
    EXPECT_TRUE(to_host(oc)[0] == n && to_host(oc)[1] == 0);
  }
}

// runs that straddle every segment boundary, and runs that end exactly there
TEST(SegmentBoundaries) {
  const std::size_t n = 100003;
  shp::distributed_vector<int> probe(n);
  const std::size_t seg = probe.segment_size();
  for (int exact = 0; exact < 2; exact++) {
    std::vector<int> k(n);
    // straddle: a new key 3 elements before every boundary, running 3 past it;
    // exact: a new key exactly at every boundary (nothing may join), runs of 7 inside
    for (std::size_t i = 0; i < n; i++) {
      const std::size_t s = i / seg, o = i % seg;
      if (exact) k[i] = (int)(s * 100000 + o / 7);
      else k[i] = (int)((i + 3) / seg * 100000 + ((o + 3) % seg) / 50);
    }
    whole_case(k, small_values<int>(n, 9 + exact), std::equal_to<>{}, std::plus<>{});
    whole_case(k, small_values<float>(n, 11 + exact), std::equal_to<>{}, std::plus<>{});
  }
}

// Float sums that no float holds but every double does: the values are
// multiples of 2^-10 below 2^10, so every partial sum of up to 2^20 of them is
// exact in double, every association of the double fold gives the same
// double, and the one rounding at the output gives the same float on every
// segmentation -- the one-segment result, computed here by a host loop in
// double.  A run that was rounded once per piece it crosses would differ.
TEST(InexactFloatSumsRoundedOnce) {
  for (std::size_t n : {std::size_t(100003), (std::size_t(1) << 20) + 13}) {
    for (double mean : {1e12, 30000.0, 7.0}) { // all keys equal: one run across every segment
      const std::vector<int> k = run_keys(n, mean, 25 + n);
      std::vector<float> v(n);
      std::mt19937_64 g(26 + n);
      for (auto &x : v) x = (float)(g() % (1u << 20)) / 1024.f;
      std::vector<int> wk;
      std::vector<double> acc;
      for (std::size_t i = 0; i < n; i++) {
        if (i == 0 || k[i - 1] != k[i]) {
          wk.push_back(k[i]);
          acc.push_back(v[i]);
        } else {
          acc.back() += v[i];
        }
      }
      std::vector<float> wv(acc.begin(), acc.end());
      auto dk = to_device(k);
      auto dv = to_device(v);
      shp::distributed_vector<int> ok(n, -7);
      shp::distributed_vector<float> ov(n, -7.f);
      auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk, dv, ok, ov);
      EXPECT_TRUE(ik == ok.begin() + (std::ptrdiff_t)wk.size() && iv == ov.begin() + (std::ptrdiff_t)wk.size());
      wk.resize(n, -7);
      wv.resize(n, -7.f);
      EXPECT_TRUE(to_host(ok) == wk);
      EXPECT_TRUE(same_bits(to_host(ov), wv));
    }
  }
}

TEST(TooSmallOutputThrows) {
  const std::size_t n = 100003;
  const std::vector<int> k = run_keys(n, 3.0, 13);
  const std::vector<int> v = small_values<int>(n, 14);
  std::vector<int> wk, wv;
  host_rbk(k, v, wk, wv, std::equal_to<>{}, std::plus<>{});
  const std::size_t c = wk.size();
  auto dk = to_device(k);
  auto dv = to_device(v);
  for (int which = 0; which < 2; which++) { // the key output, then the value output, one short
    shp::distributed_vector<int> ok(c - (which == 0), -7), ov(c - (which == 1), -7);
    bool threw = false;
    try {
      shp::reduce_by_key(shp::par_unseq, dk, dv, ok, ov);
    } catch (const std::out_of_range &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    EXPECT_TRUE(to_host(ok) == std::vector<int>(ok.size(), -7)); // unchanged
    EXPECT_TRUE(to_host(ov) == std::vector<int>(ov.size(), -7));
  }
  {
    shp::distributed_vector<int> ok(c - 1, -7);
    bool threw = false;
    try {
      shp::unique_copy(shp::par_unseq, dk, ok);
    } catch (const std::out_of_range &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    EXPECT_TRUE(to_host(ok) == std::vector<int>(c - 1, -7));
  }
  // exactly enough room: fine
  shp::distributed_vector<int> fk(c, -7), fv(c, -7);
  auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk, dv, fk, fv);
  EXPECT_TRUE(ik == fk.end() && iv == fv.end());
  EXPECT_TRUE(to_host(fk) == wk && to_host(fv) == wv);
}

TEST(DifferentSegmentationThrows) {
  const std::size_t n = 100003;
  shp::distributed_vector<int> k(n, 1), v(n + 5, 1), ok(n, -7), ov(n, -7);
  bool threw = false;
  try {
    // same length, but v's pieces start 5 elements into its segments
    shp::reduce_by_key(shp::par_unseq, k, v | shp::views::drop(5), ok, ov);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  EXPECT_TRUE(threw || shp::nprocs() == 1); // one segment: one piece each, alike
  threw = false;
  try {
    shp::reduce_by_key(shp::par_unseq, k, v, ok, ov); // sizes differ
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
}

TEST(StructKeyFirstOfRun) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003)}) {
    const std::vector<int> a = run_keys(n, 6.0, 15 + n);
    std::vector<pairkey> k(n);
    for (std::size_t i = 0; i < n; i++) k[i] = {a[i], (int)i}; // b tells the elements of a run apart
    whole_case(k, small_values<int>(n, 16 + n), same_a{}, std::plus<>{});
  }
}

TEST(CapturingLambdaKeyEqual) {
  const int width = 10; // keys in one bucket of `width` share a run
  auto eq = [width] __host__ __device__(int x, int y) { return (x + 1000) / width == (y + 1000) / width; };
  for (std::size_t n : {std::size_t(1000), std::size_t(100003)}) {
    std::vector<int> k(n);
    std::mt19937_64 g(17 + n);
    int cur = 0;
    for (auto &x : k) {
      cur = std::clamp(cur + (int)(g() % 7) - 3, -900, 900);
      x = cur;
    }
    whole_case(k, small_values<std::int64_t>(n, 18 + n), eq, std::plus<>{});
  }
}

// affine-map composition: runs cross tile and segment boundaries, the order of the fold shows
TEST(NonCommutativeOp) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 20) + 13}) {
    for (double mean : {3.0, 5000.0, 1e9}) {
      const std::vector<int> k = run_keys(n, mean, 19 + n);
      std::vector<affine> v(n);
      std::mt19937_64 g(20 + n);
      for (auto &x : v) x = {(std::uint32_t)g() | 1u, (std::uint32_t)g()};
      whole_case(k, v, std::equal_to<>{}, compose{});
    }
  }
}

TEST(InputViews) {
  const std::size_t n = 100003;
  const std::vector<int> k = run_keys(n, 4.0, 21);
  const std::vector<int> v = small_values<int>(n, 22);
  auto dk = to_device(k);
  auto dv = to_device(v);
  {
    // a transform view as the value input
    auto twice = [] __host__ __device__(int x) { return 2 * x + 1; };
    std::vector<int> vt(n), wk, wv;
    std::transform(v.begin(), v.end(), vt.begin(), twice);
    host_rbk(k, vt, wk, wv, std::equal_to<>{}, std::plus<>{});
    shp::distributed_vector<int> ok(n, -7), ov(n, -7);
    auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk, lib::views::transform(dv, twice), ok, ov);
    EXPECT_TRUE(ik == ok.begin() + (std::ptrdiff_t)wk.size());
    wk.resize(n, -7);
    wv.resize(n, -7);
    EXPECT_TRUE(to_host(ok) == wk && to_host(ov) == wv);
  }
  {
    // drop(5) | take(n - 11): starts mid-segment, not 16-byte aligned
    auto kv = dk | shp::views::drop(5) | shp::views::take(n - 11);
    auto vv = dv | shp::views::drop(5) | shp::views::take(n - 11);
    std::vector<int> hk(k.begin() + 5, k.begin() + 5 + (std::ptrdiff_t)(n - 11)), hv(v.begin() + 5, v.begin() + 5 + (std::ptrdiff_t)(n - 11));
    std::vector<int> wk, wv;
    host_rbk(hk, hv, wk, wv, std::equal_to<>{}, std::plus<>{});
    shp::distributed_vector<int> ok(n, -7), ov(n, -7);
    auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, kv, vv, ok, ov);
    EXPECT_TRUE(iv == ov.begin() + (std::ptrdiff_t)wk.size());
    wk.resize(n, -7);
    wv.resize(n, -7);
    EXPECT_TRUE(to_host(ok) == wk && to_host(ov) == wv);
  }
}

TEST(IteratorForms) {
  const std::size_t n = 100003;
  const std::vector<int> k = run_keys(n, 4.0, 23);
  const std::vector<int> v = small_values<int>(n, 24);
  auto dk = to_device(k);
  auto dv = to_device(v);
  std::vector<int> hk(k.begin() + 100, k.end() - 200), hv(v.begin() + 100, v.end() - 200), wk, wv;
  host_rbk(hk, hv, wk, wv, std::equal_to<>{}, std::plus<>{});
  shp::distributed_vector<int> ok(n, -7), ov(n, -7);
  auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, dk.begin() + 100, dk.end() - 200, dv.begin() + 100, ok.begin() + 50,
                                     ov.begin() + 50);
  EXPECT_TRUE(ik == ok.begin() + 50 + (std::ptrdiff_t)wk.size() && iv == ov.begin() + 50 + (std::ptrdiff_t)wk.size());
  std::vector<int> ek(n, -7), evv(n, -7);
  std::copy(wk.begin(), wk.end(), ek.begin() + 50);
  std::copy(wv.begin(), wv.end(), evv.begin() + 50);
  EXPECT_TRUE(to_host(ok) == ek && to_host(ov) == evv);
  shp::distributed_vector<int> uk(n, -7);
  auto it = shp::unique_copy(shp::par_unseq, dk.begin() + 100, dk.end() - 200, uk.begin() + 50);
  EXPECT_TRUE(it == uk.begin() + 50 + (std::ptrdiff_t)wk.size());
  EXPECT_TRUE(to_host(uk) == ek);
}

// every segment cut at a third, both parts listed: two pieces per rank
template <typename T> static shp::distributed_span<T> cut_in_two(shp::distributed_vector<T> &dv) {
  std::vector<shp::device_span<T>> parts;
  for (auto &&s : dv.segments()) {
    const std::size_t a = s.size() / 3;
    parts.emplace_back(s.data(), a, s.rank());
    parts.emplace_back(s.data() + a, s.size() - a, s.rank());
  }
  return shp::distributed_span<T>(parts);
}

// two pieces share every rank's scratch block, each with its own runs and
// state; runs cross the cuts as they cross segment boundaries
TEST(SharedRankSegments) {
  const std::size_t n = (std::size_t(1) << 20) + 13;
  for (double mean : {3.0, 1000.0}) {
    const std::vector<int> k = run_keys(n, mean, 27);
    const std::vector<int> v = small_values<int>(n, 28);
    std::vector<int> wk, wv, tmp;
    std::vector<std::uint64_t> ones(n, 1), wc;
    host_rbk(k, v, wk, wv, std::equal_to<>{}, std::plus<>{});
    host_rbk(k, ones, tmp, wc, std::equal_to<>{}, std::plus<>{});
    const std::ptrdiff_t runs = (std::ptrdiff_t)wk.size();
    wk.resize(n, -7);
    wv.resize(n, -7);
    wc.resize(n, 0);
    auto dk = to_device(k);
    auto dv = to_device(v);
    auto ks = cut_in_two(dk);
    auto vs = cut_in_two(dv);
    {
      shp::distributed_vector<int> ok(n, -7), ov(n, -7);
      auto [ik, iv] = shp::reduce_by_key(shp::par_unseq, ks, vs, ok, ov);
      EXPECT_TRUE(ik == ok.begin() + runs && iv == ov.begin() + runs);
      EXPECT_TRUE(to_host(ok) == wk && to_host(ov) == wv);
    }
    {
      shp::distributed_vector<int> ok(n, -7);
      shp::distributed_vector<std::uint64_t> oc(n, 0);
      auto [ik, ic] = shp::run_length_encode(shp::par_unseq, ks, ok, oc);
      EXPECT_TRUE(ik == ok.begin() + runs && ic == oc.begin() + runs);
      EXPECT_TRUE(to_host(ok) == wk && to_host(oc) == wc);
    }
    {
      shp::distributed_vector<int> ok(n, -7);
      auto it = shp::unique_copy(shp::par_unseq, ks, ok);
      EXPECT_TRUE(it == ok.begin() + runs);
      EXPECT_TRUE(to_host(ok) == wk);
    }
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
  std::printf("\n");
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
    std::printf("[%s] ReduceByKey.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

// shp::inclusive_scan_by_key / exclusive_scan_by_key (dr/shp/scan_by_key.hpp)
// against a host loop over the host copy.  The reference has no by-key
// algorithm, so there is no gtest to restate; the runner takes
// --devicesCount N (N segments duplicated on one GPU) and --devices a,b,...
// (explicit device ids) as reduce_by_key_tests does.
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

// x -> a x + b (wrapping mod 2^32); compose(f, g) applies f first: associative, not commutative
struct affine {
  std::uint32_t a, b;
};
struct compose {
  __host__ __device__ affine operator()(const affine &f, const affine &g) const { return {f.a * g.a, f.b * g.a + g.b}; }
};
static_assert(sizeof(affine) == 8);

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

// the host loops
template <typename K, typename V, typename Eq, typename Op>
static std::vector<V> host_incl(const std::vector<K> &k, const std::vector<V> &v, Eq eq, Op op) {
  std::vector<V> o(v.size());
  for (std::size_t i = 0; i < k.size(); i++) o[i] = (i == 0 || !eq(k[i - 1], k[i])) ? v[i] : (V)op(o[i - 1], v[i]);
  return o;
}
template <typename K, typename V, typename Eq, typename Op>
static std::vector<V> host_excl(const std::vector<K> &k, const std::vector<V> &v, V init, Eq eq, Op op) {
  std::vector<V> o(v.size());
  V acc{};
  for (std::size_t i = 0; i < k.size(); i++) {
    const bool head = i == 0 || !eq(k[i - 1], k[i]);
    o[i] = head ? init : (V)op(init, acc);
    acc = head ? v[i] : (V)op(acc, v[i]);
  }
  return o;
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

// Both scans of (k, v): into a whole output of n + 1 elements (segmented like
// the input up to rounding of the segment size), into an output that starts
// `drop` elements into a longer vector (segmented differently from the input),
// and in place.
template <typename K, typename V, typename Eq, typename Op>
static void whole_case(const std::vector<K> &k, const std::vector<V> &v, V init, Eq eq, Op op) {
  const std::size_t n = k.size();
  const std::vector<V> wi = host_incl(k, v, eq, op), we = host_excl(k, v, init, eq, op);
  auto dk = to_device(k);
  auto dv = to_device(v);
  for (std::size_t drop : {std::size_t(0), n / 3 + 1}) {
    const std::size_t len = n + 1 + drop;
    std::vector<V> ei(len, sentinel<V>()), ee(len, sentinel<V>());
    std::copy(wi.begin(), wi.end(), ei.begin() + (std::ptrdiff_t)drop);
    std::copy(we.begin(), we.end(), ee.begin() + (std::ptrdiff_t)drop);
    shp::distributed_vector<V> oi(len, sentinel<V>()), oe(len, sentinel<V>());
    auto oiv = oi | shp::views::drop(drop);
    auto oev = oe | shp::views::drop(drop);
    shp::inclusive_scan_by_key(shp::par_unseq, dk, dv, oiv, eq, op);
    EXPECT_TRUE(same_bits(to_host(oi), ei)); // sentinels around the n results
    shp::exclusive_scan_by_key(shp::par_unseq, dk, dv, oev, init, eq, op);
    EXPECT_TRUE(same_bits(to_host(oe), ee));
  }
  {
    // an output of exactly the input's size is segmented like the input: written directly
    shp::distributed_vector<V> o(n, sentinel<V>());
    shp::inclusive_scan_by_key(shp::par_unseq, dk, dv, o, eq, op);
    EXPECT_TRUE(same_bits(to_host(o), wi));
    shp::exclusive_scan_by_key(shp::par_unseq, dk, dv, o, init, eq, op);
    EXPECT_TRUE(same_bits(to_host(o), we));
  }
  {
    auto d1 = to_device(v);
    shp::inclusive_scan_by_key(shp::par_unseq, dk, d1, d1, eq, op);
    EXPECT_TRUE(same_bits(to_host(d1), wi));
    auto d2 = to_device(v);
    shp::exclusive_scan_by_key(shp::par_unseq, dk, d2, d2, init, eq, op);
    EXPECT_TRUE(same_bits(to_host(d2), we));
    EXPECT_TRUE(same_bits(to_host(dv), v)); // the input of the other calls is untouched
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
      whole_case(run_keys(n, mean, 1 + n), small_values<int>(n, 2 + n), 5, std::equal_to<>{}, std::plus<>{});
}

TEST(Int64KeysDoubleValues) {
  for (std::size_t n : sizes()) {
    const std::vector<int> k32 = run_keys(n, 5.0, 3 + n);
    std::vector<std::int64_t> k(k32.begin(), k32.end());
    whole_case(k, small_values<double>(n, 4 + n), 5.0, std::equal_to<>{}, std::plus<>{});
  }
}

TEST(FloatValuesMixedSizes) {
  const std::size_t n = 100003;
  const std::vector<int> k32 = run_keys(n, 40.0, 5);
  std::vector<std::int64_t> k64(k32.begin(), k32.end());
  whole_case(k32, small_values<float>(n, 6), 5.f, std::equal_to<>{}, std::plus<>{});
  whole_case(k64, small_values<float>(n, 7), 5.f, std::equal_to<>{}, std::plus<>{});
  whole_case(k32, small_values<double>(n, 8), 5.0, std::equal_to<>{}, std::plus<>{});
  whole_case(k32, small_values<float>(n, 9), 3.f, std::equal_to<>{}, shp::maximum<>{});
}

// one run swallowing whole pieces: every piece but the first is all carry
TEST(AllKeysEqual) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 20) + 13}) {
    std::vector<int> k(n, 42);
    std::vector<std::uint64_t> v(n);
    for (std::size_t i = 0; i < n; i++) v[i] = i;
    whole_case(k, v, std::uint64_t(7), std::equal_to<>{}, std::plus<>{});
    // the rank inside the group: the exclusive scan of ones
    auto dk = to_device(k);
    shp::distributed_vector<std::uint64_t> ones(n, 1), r(n, 99);
    shp::exclusive_scan_by_key(shp::par_unseq, dk, ones, r, std::uint64_t(0));
    const auto hr = to_host(r);
    EXPECT_TRUE(hr[0] == 0 && hr[n / 2] == n / 2 && hr[n - 1] == n - 1);
  }
}

// runs that straddle every segment boundary, runs that end exactly there, and one run that covers the middle pieces
TEST(SegmentBoundaries) {
  const std::size_t n = 100003;
  shp::distributed_vector<int> probe(n);
  const std::size_t seg = probe.segment_size();
  for (int mode = 0; mode < 3; mode++) {
    std::vector<int> k(n);
    for (std::size_t i = 0; i < n; i++) {
      const std::size_t s = i / seg, o = i % seg;
      if (mode == 0) k[i] = (int)((i + 3) / seg * 100000 + ((o + 3) % seg) / 50); // straddle
      else if (mode == 1) k[i] = (int)(s * 100000 + o / 7);                        // a new key exactly at every boundary
      else k[i] = (i < seg / 2 || i >= n - seg / 2) ? (int)(i / 3) : -1;          // all but half of the end pieces
    }
    whole_case(k, small_values<int>(n, 9 + mode), 5, std::equal_to<>{}, std::plus<>{});
    whole_case(k, small_values<float>(n, 12 + mode), 5.f, std::equal_to<>{}, std::plus<>{});
  }
}

TEST(TooSmallOutputThrows) {
  const std::size_t n = 100003;
  auto dk = to_device(run_keys(n, 3.0, 13));
  auto dv = to_device(small_values<int>(n, 14));
  shp::distributed_vector<int> o(n - 1, -7);
  for (int excl = 0; excl < 2; excl++) {
    bool threw = false;
    try {
      if (excl) shp::exclusive_scan_by_key(shp::par_unseq, dk, dv, o, 5);
      else shp::inclusive_scan_by_key(shp::par_unseq, dk, dv, o);
    } catch (const std::out_of_range &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    EXPECT_TRUE(to_host(o) == std::vector<int>(n - 1, -7)); // unchanged
  }
}

TEST(DifferentSegmentationThrows) {
  const std::size_t n = 100003;
  shp::distributed_vector<int> k(n, 1), v(n + 5, 1), o(n + 5, -7);
  bool threw = false;
  try {
    // same length, but v's pieces start 5 elements into its segments
    shp::inclusive_scan_by_key(shp::par_unseq, k, v | shp::views::drop(5), o);
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  EXPECT_TRUE(threw || shp::nprocs() == 1); // one segment: one piece each, alike
  threw = false;
  try {
    shp::exclusive_scan_by_key(shp::par_unseq, k, v, o, 0); // sizes differ
  } catch (const std::invalid_argument &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
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
    whole_case(k, small_values<std::int64_t>(n, 18 + n), std::int64_t(5), eq, std::plus<>{});
  }
}

// affine-map composition: runs cross tile and segment boundaries, any reordering shows
TEST(NonCommutativeOp) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 20) + 13}) {
    for (double mean : {3.0, 5000.0, 1e9}) {
      const std::vector<int> k = run_keys(n, mean, 19 + n);
      std::vector<affine> v(n);
      std::mt19937_64 g(20 + n);
      for (auto &x : v) x = {(std::uint32_t)g() | 1u, (std::uint32_t)g()};
      whole_case(k, v, affine{3u, 11u}, std::equal_to<>{}, compose{});
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
    std::vector<int> vt(n);
    std::transform(v.begin(), v.end(), vt.begin(), twice);
    shp::distributed_vector<int> o(n, -7);
    shp::inclusive_scan_by_key(shp::par_unseq, dk, lib::views::transform(dv, twice), o);
    EXPECT_TRUE(to_host(o) == host_incl(k, vt, std::equal_to<>{}, std::plus<>{}));
    shp::exclusive_scan_by_key(shp::par_unseq, dk, lib::views::transform(dv, twice), o, 5);
    EXPECT_TRUE(to_host(o) == host_excl(k, vt, 5, std::equal_to<>{}, std::plus<>{}));
  }
  for (double mean : {4.0, 1e9}) {
    // drop(5) | take(n - 11): starts mid-segment, not 16-byte aligned; the output likewise (in step with the input),
    // and a whole vector (out of step)
    const std::vector<int> kk = run_keys(n, mean, 23);
    auto dkk = to_device(kk);
    auto kv = dkk | shp::views::drop(5) | shp::views::take(n - 11);
    auto vv = dv | shp::views::drop(5) | shp::views::take(n - 11);
    std::vector<int> hk(kk.begin() + 5, kk.begin() + 5 + (std::ptrdiff_t)(n - 11)), hv(v.begin() + 5, v.begin() + 5 + (std::ptrdiff_t)(n - 11));
    const auto wi = host_incl(hk, hv, std::equal_to<>{}, std::plus<>{});
    const auto we = host_excl(hk, hv, 5, std::equal_to<>{}, std::plus<>{});
    for (std::size_t odrop : {std::size_t(5), std::size_t(0)}) {
      std::vector<int> ei(n, -7), ee(n, -7);
      std::copy(wi.begin(), wi.end(), ei.begin() + (std::ptrdiff_t)odrop);
      std::copy(we.begin(), we.end(), ee.begin() + (std::ptrdiff_t)odrop);
      shp::distributed_vector<int> o(n, -7);
      shp::inclusive_scan_by_key(shp::par_unseq, kv, vv, o | shp::views::drop(odrop));
      EXPECT_TRUE(to_host(o) == ei);
      shp::distributed_vector<int> o2(n, -7);
      shp::exclusive_scan_by_key(shp::par_unseq, kv, vv, o2 | shp::views::drop(odrop), 5);
      EXPECT_TRUE(to_host(o2) == ee);
    }
  }
}

TEST(IteratorForms) {
  const std::size_t n = 100003;
  const std::vector<int> k = run_keys(n, 4.0, 23);
  const std::vector<int> v = small_values<int>(n, 24);
  auto dk = to_device(k);
  auto dv = to_device(v);
  std::vector<int> hk(k.begin() + 100, k.end() - 200), hv(v.begin() + 100, v.end() - 200);
  const auto wi = host_incl(hk, hv, std::equal_to<>{}, std::plus<>{});
  const auto we = host_excl(hk, hv, 5, std::equal_to<>{}, std::plus<>{});
  std::vector<int> ei(n, -7), ee(n, -7);
  std::copy(wi.begin(), wi.end(), ei.begin() + 50);
  std::copy(we.begin(), we.end(), ee.begin() + 50);
  shp::distributed_vector<int> o(n, -7), o2(n, -7);
  auto it = shp::inclusive_scan_by_key(shp::par_unseq, dk.begin() + 100, dk.end() - 200, dv.begin() + 100, o.begin() + 50);
  EXPECT_TRUE(it == o.begin() + 50 + (std::ptrdiff_t)hk.size());
  EXPECT_TRUE(to_host(o) == ei);
  auto it2 = shp::exclusive_scan_by_key(shp::par_unseq, dk.begin() + 100, dk.end() - 200, dv.begin() + 100, o2.begin() + 50, 5);
  EXPECT_TRUE(it2 == o2.begin() + 50 + (std::ptrdiff_t)hk.size());
  EXPECT_TRUE(to_host(o2) == ee);
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

// two pieces share every rank's scratch block: written directly (state only),
// through scratch (an output out of step with the input) and in place (the
// exclusive form keeps a copy of a piece's values there)
TEST(SharedRankSegments) {
  const std::size_t n = (std::size_t(1) << 20) + 13;
  for (double mean : {3.0, 1000.0}) {
    const std::vector<int> k = run_keys(n, mean, 25);
    const std::vector<int> v = small_values<int>(n, 26);
    const auto wi = host_incl(k, v, std::equal_to<>{}, std::plus<>{});
    const auto we = host_excl(k, v, 5, std::equal_to<>{}, std::plus<>{});
    auto dk = to_device(k);
    auto dv = to_device(v);
    auto ks = cut_in_two(dk);
    auto vs = cut_in_two(dv);
    {
      shp::distributed_vector<int> o(n, -7);
      shp::inclusive_scan_by_key(shp::par_unseq, ks, vs, o);
      EXPECT_TRUE(to_host(o) == wi);
      shp::exclusive_scan_by_key(shp::par_unseq, ks, vs, o, 5);
      EXPECT_TRUE(to_host(o) == we);
    }
    {
      const std::size_t drop = n / 3 + 1;
      std::vector<int> ei(n + drop, -7), ee(n + drop, -7);
      std::copy(wi.begin(), wi.end(), ei.begin() + (std::ptrdiff_t)drop);
      std::copy(we.begin(), we.end(), ee.begin() + (std::ptrdiff_t)drop);
      shp::distributed_vector<int> o(n + drop, -7), o2(n + drop, -7);
      shp::inclusive_scan_by_key(shp::par_unseq, ks, vs, o | shp::views::drop(drop));
      EXPECT_TRUE(to_host(o) == ei);
      shp::exclusive_scan_by_key(shp::par_unseq, ks, vs, o2 | shp::views::drop(drop), 5);
      EXPECT_TRUE(to_host(o2) == ee);
    }
    {
      auto d1 = to_device(v);
      auto s1 = cut_in_two(d1);
      shp::inclusive_scan_by_key(shp::par_unseq, ks, s1, s1);
      EXPECT_TRUE(to_host(d1) == wi);
      auto d2 = to_device(v);
      auto s2 = cut_in_two(d2);
      shp::exclusive_scan_by_key(shp::par_unseq, ks, s2, s2, 5);
      EXPECT_TRUE(to_host(d2) == we);
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
    std::printf("[%s] ScanByKey.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

// shp::sort_by_key (dr/shp/sort.hpp) against std::stable_sort of the (key,
// value) pairs by key.  The reference has no by-key sort, so there is no
// gtest to restate; the runner takes --devicesCount N (N segments duplicated
// on one GPU) and --devices a,b,... (explicit device ids) as shp_tests does.
#include <dr/shp.hpp>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <stdexcept>
#include <string>
#include <utility>
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

struct int2v {
  int a, b;
};
static_assert(sizeof(int2v) == 8);

template <typename T> static std::vector<T> to_host(const shp::distributed_vector<T> &dv) {
  std::vector<T> h(dv.size());
  shp::copy(dv.begin(), dv.end(), h.begin());
  return h;
}
template <typename T> static bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

// keys: random over the whole type (mod == 0) or in [0, mod); floats normal, no zero
template <typename K> static std::vector<K> make_keys(std::size_t n, std::uint64_t seed, std::uint64_t mod) {
  std::vector<K> h(n);
  std::mt19937_64 g(seed);
  for (auto &x : h) {
    if constexpr (std::is_floating_point_v<K>) {
      x = (K)std::normal_distribution<double>(0, 1e3)(g);
      if (mod) x = (K)((long)x % (long)mod); // few distinct values, negatives included
      if (x == 0) x = 1;
    } else {
      x = mod ? (K)(g() % mod) : (K)g();
    }
  }
  return h;
}
template <typename V> static V make_val(std::size_t i) {
  if constexpr (std::is_same_v<V, int2v>) return int2v{(int)i, (int)(~i)};
  else return (V)i;
}

// std::stable_sort of the pairs over [lo, hi), everything outside unchanged
template <typename K, typename V, typename Comp>
static void host_sort(std::vector<K> &k, std::vector<V> &v, std::size_t lo, std::size_t hi, Comp comp) {
  std::vector<std::pair<K, V>> p(hi - lo);
  for (std::size_t i = lo; i < hi; i++) p[i - lo] = {k[i], v[i]};
  std::stable_sort(p.begin(), p.end(), [&](const auto &x, const auto &y) { return comp(x.first, y.first); });
  for (std::size_t i = lo; i < hi; i++) {
    k[i] = p[i - lo].first;
    v[i] = p[i - lo].second;
  }
}

template <typename K, typename V, typename Comp = std::less<>>
static void pairs_case(std::size_t n, std::uint64_t seed, std::uint64_t mod, Comp comp = {}) {
  std::vector<K> hk = make_keys<K>(n, seed, mod);
  std::vector<V> hv(n);
  for (std::size_t i = 0; i < n; i++) hv[i] = make_val<V>(i);
  shp::distributed_vector<K> dk(n);
  shp::distributed_vector<V> dv(n);
  shp::copy(hk.begin(), hk.end(), dk.begin());
  shp::copy(hv.begin(), hv.end(), dv.begin());
  shp::sort_by_key(shp::par_unseq, dk, dv, comp);
  host_sort(hk, hv, 0, n, comp);
  EXPECT_TRUE(same_bits(to_host(dk), hk));
  EXPECT_TRUE(same_bits(to_host(dv), hv));
}

TEST(RandomU32) { pairs_case<std::uint32_t, std::uint32_t>(100003, 1, 0); }

// ties straddle every segment boundary: stability across segments decides
TEST(FewI32U64) { pairs_case<std::int32_t, std::uint64_t>(200001, 2, 5); }

TEST(ConstantKeys) {
  const std::size_t n = 50001;
  std::vector<std::uint32_t> hk(n, 12345u), hv(n);
  for (std::size_t i = 0; i < n; i++) hv[i] = (std::uint32_t)(i * 7);
  shp::distributed_vector<std::uint32_t> dk(n), dv(n);
  shp::copy(hk.begin(), hk.end(), dk.begin());
  shp::copy(hv.begin(), hv.end(), dv.begin());
  shp::sort_by_key(shp::par_unseq, dk, dv);
  EXPECT_TRUE(to_host(dk) == hk);
  EXPECT_TRUE(to_host(dv) == hv); // unchanged
}

TEST(FloatKeysFloatValues) {
  pairs_case<float, float>(150001, 3, 0);
  pairs_case<float, float>(70001, 4, 7); // few distinct, negatives included
}

TEST(DoubleKeysStructValues) {
  pairs_case<double, int2v>(90001, 5, 0);
  pairs_case<double, int2v>(40003, 6, 3);
}

TEST(Keys64) {
  pairs_case<std::int64_t, std::uint32_t>(65539, 7, 0);
  pairs_case<std::uint64_t, std::uint64_t>(65539, 8, 0);
  pairs_case<std::int64_t, std::uint64_t>(100001, 9, 4);
}

TEST(Greater) {
  pairs_case<std::uint32_t, std::uint32_t>(100003, 10, 0, std::greater<>());
  pairs_case<std::int32_t, std::uint64_t>(200001, 11, 5, std::greater<std::int32_t>());
  pairs_case<std::int32_t, std::uint32_t>(77777, 12, 5, std::ranges::greater{});
  pairs_case<float, std::uint32_t>(50001, 13, 6, std::greater<>());
}

TEST(TinySizes) {
  // 0, 1, and fewer elements than segments (some segments empty)
  for (std::size_t n : {std::size_t(0), std::size_t(1), std::size_t(5)}) {
    pairs_case<std::uint32_t, std::uint32_t>(n, 20 + n, 0);
    pairs_case<std::int64_t, std::uint64_t>(n, 30 + n, 2);
  }
}

TEST(IteratorSubrange) {
  const std::size_t n = 120007;
  std::vector<std::int32_t> hk = make_keys<std::int32_t>(n, 40, 9);
  std::vector<std::uint64_t> hv(n);
  for (std::size_t i = 0; i < n; i++) hv[i] = 1000 + i;
  shp::distributed_vector<std::int32_t> dk(n);
  shp::distributed_vector<std::uint64_t> dv(n);
  shp::copy(hk.begin(), hk.end(), dk.begin());
  shp::copy(hv.begin(), hv.end(), dv.begin());
  shp::sort_by_key(shp::par_unseq, dk.begin() + 100, dk.end() - 200, dv.begin() + 100);
  host_sort(hk, hv, 100, n - 200, std::less<>());
  EXPECT_TRUE(to_host(dk) == hk); // the elements outside unchanged
  EXPECT_TRUE(to_host(dv) == hv);
  shp::sort_by_key(shp::par_unseq, dk.begin() + 100, dk.end() - 200, dv.begin() + 100, std::greater<>());
  host_sort(hk, hv, 100, n - 200, std::greater<>());
  EXPECT_TRUE(to_host(dk) == hk);
  EXPECT_TRUE(to_host(dv) == hv);
}

TEST(ScratchReusedAndRegrown) {
  pairs_case<std::uint32_t, std::uint64_t>(60001, 50, 0);
  pairs_case<std::uint32_t, std::uint64_t>(60001, 51, 3);
  pairs_case<std::uint64_t, std::uint64_t>(400003, 52, 0); // larger: the cached scratch grows
  pairs_case<std::uint32_t, std::uint32_t>(1000, 53, 0);
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

// two pieces share every rank's scratch block: both exchange buffers of each
// must survive until its merge.  Few distinct keys, the value is the original
// index: ties across the pieces of one rank show in the values.
TEST(SharedRankSegments) {
  const std::size_t n = 4 * (std::size_t(1) << 16) + 321;
  std::vector<std::uint32_t> hk = make_keys<std::uint32_t>(n, 60, 1000), hv(n);
  for (std::size_t i = 0; i < n; i++) hv[i] = (std::uint32_t)i;
  shp::distributed_vector<std::uint32_t> dk(n), dv(n);
  shp::copy(hk.begin(), hk.end(), dk.begin());
  shp::copy(hv.begin(), hv.end(), dv.begin());
  shp::sort_by_key(shp::par_unseq, cut_in_two(dk), cut_in_two(dv));
  host_sort(hk, hv, 0, n, std::less<>());
  EXPECT_TRUE(same_bits(to_host(dk), hk));
  EXPECT_TRUE(same_bits(to_host(dv), hv));
}

TEST(MismatchesThrow) {
  shp::distributed_vector<std::uint32_t> dk(1000), dv(1000), ds(999);
  shp::fill(dk.begin(), dk.end(), 3u);
  shp::fill(dv.begin(), dv.end(), 4u);
  shp::fill(ds.begin(), ds.end(), 5u);
  bool size_threw = false, seg_threw = false;
  try {
    shp::sort_by_key(shp::par_unseq, dk, ds);
  } catch (const std::invalid_argument &) {
    size_threw = true;
  }
  EXPECT_TRUE(size_threw);
  // equal sizes, cut differently: keys without their first element against
  // values without their last
  try {
    shp::sort_by_key(shp::par_unseq, std::ranges::subrange(dk.begin() + 1, dk.end()),
                     std::ranges::subrange(dv.begin(), dv.end() - 1));
  } catch (const std::invalid_argument &) {
    seg_threw = true;
  }
  EXPECT_TRUE(seg_threw || shp::nprocs() == 1); // one segment: both cuts are one 999-element segment
  // both sides cut alike: fine
  shp::sort_by_key(shp::par_unseq, std::ranges::subrange(dk.begin() + 1, dk.end()),
                   std::ranges::subrange(dv.begin() + 1, dv.end()));
  EXPECT_TRUE(to_host(dk) == std::vector<std::uint32_t>(1000, 3u));
  EXPECT_TRUE(to_host(dv) == std::vector<std::uint32_t>(1000, 4u));
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
    std::printf("[%s] SortByKey.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

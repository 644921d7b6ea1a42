// shp::lower_bound / upper_bound / binary_search (vectorised and scalar),
// equal_range and partition_point (dr/shp/sorted_search.hpp) against their
// std:: counterparts on host copies; every expected value is an exact
// position or flag.  The reference has none of these algorithms, so there is
// no gtest to restate; the runner takes --devicesCount N (N segments
// duplicated on one GPU) and --devices a,b,... (explicit device ids) as
// search_tests does.
#include <dr/shp.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
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
#define EXPECT_EQ(a, b)                                                                                       \
  do {                                                                                                        \
    const long long a_ = (long long)(a), b_ = (long long)(b);                                                 \
    if (a_ != b_) {                                                                                           \
      std::printf("  %s:%d: EXPECT_EQ(%s, %s) failed: %lld vs %lld\n", __FILE__, __LINE__, #a, #b, a_, b_);   \
      g_cur_failed = true;                                                                                    \
    }                                                                                                         \
  } while (0)

struct rec {
  int key;
  float payload;
};
static_assert(sizeof(rec) == 8);

template <typename T> static shp::distributed_vector<T> to_device(const std::vector<T> &h) {
  shp::distributed_vector<T> dv(h.size());
  shp::copy(h.begin(), h.end(), dv.begin());
  return dv;
}
template <typename T> static std::vector<T> to_host(shp::distributed_vector<T> &dv) {
  std::vector<T> h(dv.size());
  if (!h.empty()) shp::copy(dv.begin(), dv.end(), h.data());
  return h;
}
// the global index of the first element of every piece after the first, for a vector of n elements
static std::vector<std::size_t> boundaries(std::size_t n, std::size_t seg) {
  std::vector<std::size_t> b;
  for (std::size_t x = seg; x < n; x += seg) b.push_back(x);
  return b;
}
static const std::size_t kSizes[] = {3, 1000, (std::size_t(1) << 20) + 7};

// sorted, `distinct` different values 10 apart (so +-1 of a value is absent)
static std::vector<int> sorted_ints(std::size_t n, std::uint64_t seed, int distinct) {
  std::vector<int> h(n);
  std::mt19937_64 g(seed);
  for (auto &x : h) x = (int)(g() % (unsigned)distinct) * 10 - 5 * distinct;
  std::sort(h.begin(), h.end());
  return h;
}
// below the least and above the greatest, the last element of every piece and the first of the next, each
// +-1, and random values; `count` random ones, so the needles' length differs from the haystack's
static std::vector<int> needles_for(const std::vector<int> &h, std::size_t seg, std::size_t count, std::uint64_t seed) {
  std::vector<int> v;
  const int lo = h.empty() ? 0 : h.front(), hi = h.empty() ? 0 : h.back();
  v.push_back(lo - 7);
  v.push_back(hi + 7);
  for (std::size_t b : boundaries(h.size(), seg))
    for (int x : {h[b - 1], h[b]})
      for (int d : {-1, 0, 1}) v.push_back(x + d);
  std::mt19937_64 g(seed);
  for (std::size_t i = 0; i < count; i++) v.push_back(lo - 20 + (int)(g() % (std::uint64_t)((long long)hi - lo + 41)));
  return v;
}

// The three vectorised forms of `hay` (host copy h, sorted under comp) against std::, into uint64 / uint32 / uint8.
template <typename T, typename H, typename Comp>
static void check_batch(const std::vector<T> &h, H &&hay, const std::vector<T> &nh, Comp comp) {
  const std::size_t m = nh.size();
  auto nd = to_device(nh);
  shp::distributed_vector<std::uint64_t> lo(m);
  shp::distributed_vector<std::uint32_t> up(m);
  shp::distributed_vector<std::uint8_t> fl(m);
  auto e1 = shp::lower_bound(shp::par_unseq, hay, nd, lo, comp);
  auto e2 = shp::upper_bound(shp::par_unseq, hay, nd, up, comp);
  auto e3 = shp::binary_search(shp::par_unseq, hay, nd, fl, comp);
  EXPECT_EQ(e1 - lo.begin(), m);
  EXPECT_EQ(e2 - up.begin(), m);
  EXPECT_EQ(e3 - fl.begin(), m);
  const auto glo = to_host(lo);
  const auto gup = to_host(up);
  const auto gfl = to_host(fl);
  std::size_t bad = 0;
  for (std::size_t i = 0; i < m; i++) {
    const std::size_t wl = (std::size_t)(std::lower_bound(h.begin(), h.end(), nh[i], comp) - h.begin());
    const std::size_t wu = (std::size_t)(std::upper_bound(h.begin(), h.end(), nh[i], comp) - h.begin());
    const bool wf = std::binary_search(h.begin(), h.end(), nh[i], comp);
    const bool ok = glo[i] == wl && gup[i] == wu && gfl[i] == (wf ? 1 : 0);
    if (!ok && bad++ < 4)
      std::printf("  needle %zu of %zu, n = %zu: got %llu %u %u, want %zu %zu %d\n", i, m, h.size(), (unsigned long long)glo[i],
                  gup[i], gfl[i], wl, wu, (int)wf);
  }
  EXPECT_EQ(bad, 0);
}

TEST(SizesDefaultOrder) {
  for (std::size_t n : kSizes) {
    for (int distinct : {3, 100000}) {
      const auto h = sorted_ints(n, 1 + n + distinct, distinct);
      auto dv = to_device(h);
      // needles shorter than the haystack, longer than it, and past one staging threshold
      for (std::size_t count : {std::size_t(5), n / 3 + 11, std::size_t(5000)}) {
        const auto nh = needles_for(h, dv.segment_size(), count, 7 * n + count);
        check_batch(h, dv, nh, std::less<int>{});
        // the default order
        auto nd = to_device(nh);
        shp::distributed_vector<std::uint64_t> lo(nh.size());
        shp::lower_bound(shp::par_unseq, dv, nd, lo);
        const auto got = to_host(lo);
        std::size_t bad = 0;
        for (std::size_t i = 0; i < nh.size(); i++)
          bad += got[i] != (std::uint64_t)(std::lower_bound(h.begin(), h.end(), nh[i]) - h.begin());
        EXPECT_EQ(bad, 0);
      }
    }
  }
}

// a run of equal elements across every seam: lower = 0, upper = n
TEST(ConstantHaystack) {
  for (std::size_t n : kSizes) {
    const std::vector<int> h(n, 42);
    auto dv = to_device(h);
    const std::vector<int> nh{41, 42, 43, 42, 42, 42, 41, 43, 42};
    check_batch(h, dv, nh, std::less<int>{});
    auto nd = to_device(nh);
    shp::distributed_vector<std::uint64_t> lo(nh.size()), up(nh.size());
    shp::lower_bound(shp::par_unseq, dv, nd, lo);
    shp::upper_bound(shp::par_unseq, dv, nd, up);
    const auto glo = to_host(lo), gup = to_host(up);
    EXPECT_EQ(glo[1], 0);
    EXPECT_EQ(gup[1], n);
    EXPECT_EQ(glo[0], 0);
    EXPECT_EQ(gup[0], 0);
    EXPECT_EQ(glo[2], n);
    EXPECT_EQ(gup[2], n);
    const auto er = shp::equal_range(shp::par_unseq, dv, 42);
    EXPECT_EQ(er.first - dv.begin(), 0);
    EXPECT_EQ(er.second - dv.begin(), n);
  }
}

TEST(GreaterOnDescending) {
  for (std::size_t n : kSizes) {
    auto h = sorted_ints(n, 50 + n, 1000);
    std::reverse(h.begin(), h.end());
    auto dv = to_device(h);
    auto asc = h;
    std::reverse(asc.begin(), asc.end());
    const auto nh = needles_for(asc, dv.segment_size(), 300, 9 * n);
    check_batch(h, dv, nh, std::greater<int>{});
    for (int v : {h.front() + 5, h.back() - 5, h[n / 2], h[n / 2] + 1}) {
      EXPECT_EQ(shp::lower_bound(shp::par_unseq, dv, v, std::greater<int>{}) - dv.begin(),
                std::lower_bound(h.begin(), h.end(), v, std::greater<int>{}) - h.begin());
      EXPECT_EQ(shp::upper_bound(shp::par_unseq, dv, v, std::greater<int>{}) - dv.begin(),
                std::upper_bound(h.begin(), h.end(), v, std::greater<int>{}) - h.begin());
    }
  }
}

// a comparator on the key of an 8-byte {key, payload}
TEST(StructUnderKeyLambda) {
  auto by_key = [] __host__ __device__(const rec &a, const rec &b) { return a.key < b.key; };
  for (std::size_t n : kSizes) {
    const auto keys = sorted_ints(n, 70 + n, 500);
    std::vector<rec> h(n);
    for (std::size_t i = 0; i < n; i++) h[i] = rec{keys[i], (float)i};
    auto dv = to_device(h);
    const auto nk = needles_for(keys, dv.segment_size(), 777, 11 * n);
    std::vector<rec> nh(nk.size());
    for (std::size_t i = 0; i < nk.size(); i++) nh[i] = rec{nk[i], -1.f};
    check_batch(h, dv, nh, by_key);
    const rec probe{keys[n / 2], 0.f};
    const auto er = shp::equal_range(shp::par_unseq, dv, probe, by_key);
    const auto hr = std::equal_range(h.begin(), h.end(), probe, by_key);
    EXPECT_EQ(er.first - dv.begin(), hr.first - h.begin());
    EXPECT_EQ(er.second - dv.begin(), hr.second - h.begin());
  }
}

// haystacks whose pieces start mid-segment (unaligned), lose pieces, or are computed on the fly
TEST(HaystackViews) {
  for (std::size_t n : {std::size_t(1000), (std::size_t(1) << 20) + 7}) {
    const auto h = sorted_ints(n, 90 + n, 4000);
    auto dv = to_device(h);
    const std::size_t seg = dv.segment_size();
    const auto nh = needles_for(h, seg, 1500, 13 * n);
    auto sub = [&](std::size_t lo, std::size_t hi) { return std::vector<int>(h.begin() + (long)lo, h.begin() + (long)hi); };
    check_batch(sub(1, n), dv | shp::views::drop(1), nh, std::less<int>{});
    check_batch(sub(5, n - 6), shp::views::slice(dv, {5, n - 6}), nh, std::less<int>{});
    check_batch(sub(0, seg + 1 < n ? seg + 1 : n), dv | shp::views::take(seg + 1 < n ? seg + 1 : n), nh, std::less<int>{});
    // monotone transform: the view is sorted too
    auto f = [] __host__ __device__(int x) { return 3 * x + 1; };
    std::vector<int> ht(n);
    std::transform(h.begin(), h.end(), ht.begin(), f);
    std::vector<int> nt(nh.size());
    for (std::size_t i = 0; i < nh.size(); i++) nt[i] = 3 * nh[i] + (int)(i % 3);
    auto v = lib::views::transform(dv, f);
    check_batch(ht, v, nt, std::less<int>{});
    EXPECT_EQ(shp::lower_bound(shp::par_unseq, v, ht[n / 2]) - std::ranges::begin(v),
              std::lower_bound(ht.begin(), ht.end(), ht[n / 2]) - ht.begin());
    auto d1 = dv | shp::views::drop(1);
    EXPECT_EQ(shp::upper_bound(shp::par_unseq, d1, h[n / 2]) - std::ranges::begin(d1),
              std::upper_bound(h.begin() + 1, h.end(), h[n / 2]) - (h.begin() + 1));
  }
}

TEST(EmptyInputs) {
  shp::distributed_vector<int> e(0);
  const std::vector<int> nh{-5, 0, 5, 7, 9};
  check_batch(std::vector<int>{}, e, nh, std::less<int>{});
  EXPECT_TRUE(shp::lower_bound(shp::par_unseq, e, 3) == e.begin());
  EXPECT_TRUE(shp::upper_bound(shp::par_unseq, e, 3) == e.begin());
  EXPECT_TRUE(!shp::binary_search(shp::par_unseq, e, 3));
  EXPECT_TRUE(shp::equal_range(shp::par_unseq, e, 3).second == e.begin());
  EXPECT_TRUE(shp::partition_point(shp::par_unseq, e, [] __host__ __device__(int) { return true; }) == e.begin());
  // no needles: nothing is written
  const auto h = sorted_ints(1000, 5, 100);
  auto dv = to_device(h);
  shp::distributed_vector<std::uint64_t> out(4, 77);
  auto end = shp::lower_bound(shp::par_unseq, dv, e, out);
  EXPECT_EQ(end - out.begin(), 0);
  for (auto x : to_host(out)) EXPECT_EQ(x, 77);
  // an empty view of a non-empty haystack
  auto v = dv | shp::views::take(0);
  check_batch(std::vector<int>{}, v, nh, std::less<int>{});
}

TEST(BoolOutputAndIteratorForms) {
  const std::size_t n = 100003;
  const auto h = sorted_ints(n, 21, 3000);
  auto dv = to_device(h);
  const auto nh = needles_for(h, dv.segment_size(), 2000, 23);
  const std::size_t m = nh.size();
  auto nd = to_device(nh);
  shp::distributed_vector<bool> fb(m);
  shp::binary_search(shp::par_unseq, dv, nd, fb);
  std::vector<std::uint8_t> got(m);
  shp::copy(fb.begin(), fb.end(), reinterpret_cast<bool *>(got.data()));
  std::size_t bad = 0;
  for (std::size_t i = 0; i < m; i++) bad += got[i] != (std::binary_search(h.begin(), h.end(), nh[i]) ? 1 : 0);
  EXPECT_EQ(bad, 0);
  // iterator forms, with and without a comparator; fewer needles than the output iterator's container holds
  shp::distributed_vector<std::uint64_t> lo(m, 5);
  auto e = shp::lower_bound(shp::par_unseq, dv.begin(), dv.end(), nd.begin(), nd.end() - 9, lo.begin());
  EXPECT_EQ(e - lo.begin(), m - 9);
  auto glo = to_host(lo);
  bad = 0;
  for (std::size_t i = 0; i < m - 9; i++)
    bad += glo[i] != (std::uint64_t)(std::lower_bound(h.begin(), h.end(), nh[i]) - h.begin());
  EXPECT_EQ(bad, 0);
  for (std::size_t i = m - 9; i < m; i++) EXPECT_EQ(glo[i], 5);
  shp::distributed_vector<std::uint32_t> up(m);
  shp::upper_bound(shp::par_unseq, dv.begin(), dv.end(), nd.begin(), nd.end(), up.begin(), std::less<int>{});
  auto gup = to_host(up);
  bad = 0;
  for (std::size_t i = 0; i < m; i++) bad += gup[i] != (std::uint32_t)(std::upper_bound(h.begin(), h.end(), nh[i]) - h.begin());
  EXPECT_EQ(bad, 0);
  const int v = h[n / 3];
  EXPECT_EQ(shp::lower_bound(shp::par_unseq, dv.begin(), dv.end(), v) - dv.begin(),
            std::lower_bound(h.begin(), h.end(), v) - h.begin());
  EXPECT_EQ(shp::upper_bound(shp::par_unseq, dv.begin(), dv.end(), v, std::less<int>{}) - dv.begin(),
            std::upper_bound(h.begin(), h.end(), v) - h.begin());
  EXPECT_TRUE(shp::binary_search(shp::par_unseq, dv.begin(), dv.end(), v));
  EXPECT_TRUE(!shp::binary_search(shp::par_unseq, dv.begin(), dv.end(), v + 1));
  const auto er = shp::equal_range(shp::par_unseq, dv.begin(), dv.end(), v);
  const auto hr = std::equal_range(h.begin(), h.end(), v);
  EXPECT_EQ(er.first - dv.begin(), hr.first - h.begin());
  EXPECT_EQ(er.second - dv.begin(), hr.second - h.begin());
  auto below = [v] __host__ __device__(int x) { return x < v; };
  EXPECT_EQ(shp::partition_point(shp::par_unseq, dv.begin(), dv.end(), below) - dv.begin(),
            std::partition_point(h.begin(), h.end(), below) - h.begin());
}

// a value below all elements, above all, present once, present across a seam, absent in the middle
TEST(ScalarFormsAndEqualRange) {
  for (std::size_t n : kSizes) {
    shp::distributed_vector<int> probe(n);
    const std::size_t seg = probe.segment_size();
    std::vector<int> h(n);
    for (std::size_t i = 0; i < n; i++) h[i] = 4 * (int)i; // strictly ascending: every value is present once
    std::vector<int> vals{-3, h.back() + 3, h[n / 2], h[n / 2] + 2, h[0], h.back()};
    for (std::size_t b : boundaries(n, seg)) {
      if (b >= 2 && b + 2 <= n) { // equal elements on both sides of the seam
        h[b - 2] = h[b - 1] = h[b] = h[b + 1 < n ? b + 1 : b];
        vals.push_back(h[b]);
      }
      vals.push_back(h[b - 1]);
      vals.push_back(h[b]);
      if (vals.size() > 40) break;
    }
    auto dv = to_device(h);
    for (int v : vals) {
      const auto hr = std::equal_range(h.begin(), h.end(), v);
      EXPECT_EQ(shp::lower_bound(shp::par_unseq, dv, v) - dv.begin(), hr.first - h.begin());
      EXPECT_EQ(shp::upper_bound(shp::par_unseq, dv, v) - dv.begin(), hr.second - h.begin());
      EXPECT_EQ(shp::binary_search(shp::par_unseq, dv, v), hr.first != hr.second);
      const auto er = shp::equal_range(shp::par_unseq, dv, v);
      EXPECT_EQ(er.first - dv.begin(), hr.first - h.begin());
      EXPECT_EQ(er.second - dv.begin(), hr.second - h.begin());
    }
  }
}

// x < k for k at 0, at every seam and at n
TEST(PartitionPointAtSeams) {
  for (std::size_t n : kSizes) {
    std::vector<int> h(n);
    for (std::size_t i = 0; i < n; i++) h[i] = (int)i;
    auto dv = to_device(h);
    std::vector<std::size_t> ks{0, n};
    for (std::size_t b : boundaries(n, dv.segment_size())) {
      ks.push_back(b - 1), ks.push_back(b), ks.push_back(b + 1);
      if (ks.size() > 40) break;
    }
    for (std::size_t k : ks) {
      const int kk = (int)k;
      auto pred = [kk] __host__ __device__(int x) { return x < kk; };
      EXPECT_EQ(shp::partition_point(shp::par_unseq, dv, pred) - dv.begin(),
                std::partition_point(h.begin(), h.end(), pred) - h.begin());
    }
  }
}

// elements of 2 KiB: the staged samples would not fit a workgroup's LDS, every level goes to global memory
struct wide {
  int key;
  char pad[2044];
};
TEST(WideElements) {
  auto by_key = [] __host__ __device__(const wide &a, const wide &b) { return a.key < b.key; };
  const std::size_t n = 301, m = 200;
  std::vector<wide> h(n), nh(m);
  for (std::size_t i = 0; i < n; i++) h[i].key = 3 * (int)(i / 2);
  for (std::size_t i = 0; i < m; i++) nh[i].key = (int)(i * 5 % 460) - 3;
  auto dv = to_device(h);
  check_batch(h, dv, nh, by_key);
}

TEST(Exceptions) {
  const std::size_t n = 1000, m = 500;
  const auto h = sorted_ints(n, 31, 100);
  auto dv = to_device(h);
  const auto nh = sorted_ints(m, 32, 100);
  auto nd = to_device(nh);
  {
    shp::distributed_vector<std::uint64_t> small(m - 1, 99);
    bool threw = false;
    try {
      shp::lower_bound(shp::par_unseq, dv, nd, small);
    } catch (const std::out_of_range &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    for (auto x : to_host(small)) EXPECT_EQ(x, 99); // untouched
  }
  if (shp::nprocs() > 1) {
    // as long as the needles, segmented differently
    shp::distributed_vector<std::uint64_t> longer(m + 1, 99);
    bool threw = false;
    try {
      shp::upper_bound(shp::par_unseq, dv, nd, longer | shp::views::drop(1));
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    for (auto x : to_host(longer)) EXPECT_EQ(x, 99);
  }
  // alike: needles and output cut the same way
  shp::distributed_vector<std::uint64_t> out(m, 99);
  shp::lower_bound(shp::par_unseq, dv, nd | shp::views::drop(3), out | shp::views::drop(3));
  const auto got = to_host(out);
  std::size_t bad = 0;
  for (std::size_t i = 0; i < m; i++)
    bad += got[i] != (i < 3 ? 99 : (std::uint64_t)(std::lower_bound(h.begin(), h.end(), nh[i]) - h.begin()));
  EXPECT_EQ(bad, 0);
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
    std::printf("[%s] SortedSearch.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

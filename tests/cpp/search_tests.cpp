// shp::find / find_if / find_if_not / any_of / all_of / none_of /
// adjacent_find / is_sorted_until / is_sorted / min_element / max_element /
// minmax_element / mismatch / equal (dr/shp/search.hpp) against their std::
// counterparts on the host copy; returned iterators are compared by
// it - begin.  The reference has none of these algorithms, so there is no
// gtest to restate; the runner takes --devicesCount N (N segments duplicated
// on one GPU) and --devices a,b,... (explicit device ids) as copy_if_tests
// does.
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
#define EXPECT_EQ(a, b)                                                                                       \
  do {                                                                                                        \
    const long long a_ = (long long)(a), b_ = (long long)(b);                                                 \
    if (a_ != b_) {                                                                                           \
      std::printf("  %s:%d: EXPECT_EQ(%s, %s) failed: %lld vs %lld\n", __FILE__, __LINE__, #a, #b, a_, b_);   \
      g_cur_failed = true;                                                                                    \
    }                                                                                                         \
  } while (0)

struct rec {
  int id;
  float w;
};
static_assert(sizeof(rec) == 8);

// the sizes of the issue: 0, 1, 2, P-1, P, P+1, 1000, 100003, 2^21+13
static std::vector<std::size_t> sizes() {
  const std::size_t P = shp::nprocs();
  return {0, 1, 2, P - 1, P, P + 1, 1000, 100003, (std::size_t(1) << 21) + 13};
}

template <typename T> static shp::distributed_vector<T> to_device(const std::vector<T> &h) {
  shp::distributed_vector<T> dv(h.size());
  shp::copy(h.begin(), h.end(), dv.begin());
  return dv;
}

// the first-match algorithms of a unary predicate: r against its host copy h
template <typename T, typename R, typename Pred> static void check_pred(const std::vector<T> &h, R &&r, Pred pred) {
  auto b = std::ranges::begin(r);
  EXPECT_EQ(shp::find_if(shp::par_unseq, r, pred) - b, std::find_if(h.begin(), h.end(), pred) - h.begin());
  EXPECT_EQ(shp::find_if_not(shp::par_unseq, r, pred) - b, std::find_if_not(h.begin(), h.end(), pred) - h.begin());
  EXPECT_EQ(shp::any_of(shp::par_unseq, r, pred), std::any_of(h.begin(), h.end(), pred));
  EXPECT_EQ(shp::all_of(shp::par_unseq, r, pred), std::all_of(h.begin(), h.end(), pred));
  EXPECT_EQ(shp::none_of(shp::par_unseq, r, pred), std::none_of(h.begin(), h.end(), pred));
}
// the algorithms of an order comp and an equivalence eq
template <typename T, typename R, typename Comp, typename Eq>
static void check_order(const std::vector<T> &h, R &&r, Comp comp, Eq eq) {
  auto b = std::ranges::begin(r);
  EXPECT_EQ(shp::adjacent_find(shp::par_unseq, r, eq) - b, std::adjacent_find(h.begin(), h.end(), eq) - h.begin());
  EXPECT_EQ(shp::is_sorted_until(shp::par_unseq, r, comp) - b, std::is_sorted_until(h.begin(), h.end(), comp) - h.begin());
  EXPECT_EQ(shp::is_sorted(shp::par_unseq, r, comp), std::is_sorted(h.begin(), h.end(), comp));
  EXPECT_EQ(shp::min_element(shp::par_unseq, r, comp) - b, std::min_element(h.begin(), h.end(), comp) - h.begin());
  EXPECT_EQ(shp::max_element(shp::par_unseq, r, comp) - b, std::max_element(h.begin(), h.end(), comp) - h.begin());
  const auto mm = shp::minmax_element(shp::par_unseq, r, comp);
  const auto hm = std::minmax_element(h.begin(), h.end(), comp);
  EXPECT_EQ(mm.first - b, hm.first - h.begin());
  EXPECT_EQ(mm.second - b, hm.second - h.begin());
}
// the same with the defaults (operator<, operator==)
template <typename T, typename R> static void check_order_default(const std::vector<T> &h, R &&r) {
  auto b = std::ranges::begin(r);
  EXPECT_EQ(shp::adjacent_find(shp::par_unseq, r) - b, std::adjacent_find(h.begin(), h.end()) - h.begin());
  EXPECT_EQ(shp::is_sorted_until(shp::par_unseq, r) - b, std::is_sorted_until(h.begin(), h.end()) - h.begin());
  EXPECT_EQ(shp::is_sorted(shp::par_unseq, r), std::is_sorted(h.begin(), h.end()));
  EXPECT_EQ(shp::min_element(shp::par_unseq, r) - b, std::min_element(h.begin(), h.end()) - h.begin());
  EXPECT_EQ(shp::max_element(shp::par_unseq, r) - b, std::max_element(h.begin(), h.end()) - h.begin());
  const auto mm = shp::minmax_element(shp::par_unseq, r);
  const auto hm = std::minmax_element(h.begin(), h.end());
  EXPECT_EQ(mm.first - b, hm.first - h.begin());
  EXPECT_EQ(mm.second - b, hm.second - h.begin());
}

// few distinct values: ties for the extrema, adjacent equal pairs, early hits
template <typename T> static std::vector<T> few_values(std::size_t n, std::uint64_t seed, int distinct) {
  std::vector<T> h(n);
  std::mt19937_64 g(seed);
  for (auto &x : h) x = (T)((long long)(g() % (unsigned)distinct) - distinct / 2);
  return h;
}
// strictly ascending
template <typename T> static std::vector<T> ascending(std::size_t n) {
  std::vector<T> h(n);
  for (std::size_t i = 0; i < n; i++) h[i] = (T)(2 * (long long)i) - (T)1000;
  return h;
}
// the global index of the first element of every piece after the first, for a vector of n elements
static std::vector<std::size_t> boundaries(std::size_t n, std::size_t seg) {
  std::vector<std::size_t> b;
  for (std::size_t x = seg; x < n; x += seg) b.push_back(x);
  return b;
}

TEST(RandomInt) {
  for (std::size_t n : sizes()) {
    for (int distinct : {3, 1000}) {
      const auto h = few_values<int>(n, 1 + n + distinct, distinct);
      auto dv = to_device(h);
      check_order_default(h, dv);
      const int t = distinct / 2 - 1;
      check_pred(h, dv, [t] __host__ __device__(int x) { return x == t; });
      check_pred(h, dv, [] __host__ __device__(int x) { return x > 100000; }); // never
      check_pred(h, dv, [] __host__ __device__(int x) { return x < 100000; }); // always
      EXPECT_EQ(shp::find(shp::par_unseq, dv, t) - dv.begin(), std::find(h.begin(), h.end(), t) - h.begin());
      EXPECT_EQ(shp::find(shp::par_unseq, dv, 777777) - dv.begin(), (long long)n);
    }
  }
}

TEST(RandomDouble) {
  for (std::size_t n : sizes()) {
    const auto h = few_values<double>(n, 100 + n, 50);
    auto dv = to_device(h);
    check_order_default(h, dv);
    check_order(h, dv, [] __host__ __device__(double a, double b) { return a > b; },
                [] __host__ __device__(double a, double b) { return a == b; });
    check_pred(h, dv, [] __host__ __device__(double x) { return x == 24.0; });
  }
}

TEST(StructUnderLambdas) {
  auto by_id = [] __host__ __device__(const rec &a, const rec &b) { return a.id < b.id; };
  auto by_id_desc = [] __host__ __device__(const rec &a, const rec &b) { return a.id > b.id; };
  auto same_id = [] __host__ __device__(const rec &a, const rec &b) { return a.id == b.id; };
  for (std::size_t n : sizes()) {
    std::vector<rec> h(n);
    std::mt19937_64 g(200 + n);
    for (std::size_t i = 0; i < n; i++) h[i] = rec{(int)(g() % 40), (float)i};
    auto dv = to_device(h);
    check_order(h, dv, by_id, same_id);
    check_order(h, dv, by_id_desc, same_id);
    check_pred(h, dv, [] __host__ __device__(const rec &x) { return x.id == 39 && x.w > 10.f; });
  }
}

// a single hit as the last element of piece k and as the first of piece k + 1;
// hits in two pieces: the earlier piece wins though its hit is deep and the later one is at offset 0
TEST(HitsAtPieceBoundaries) {
  auto pred = [] __host__ __device__(int x) { return x == 7; };
  for (std::size_t n : {std::size_t(1000), std::size_t(100003)}) {
    shp::distributed_vector<int> probe(n);
    const std::size_t seg = probe.segment_size();
    for (std::size_t b : boundaries(n, seg)) {
      for (std::size_t at : {b - 1, b}) {
        std::vector<int> h(n, 0);
        h[at] = 7;
        auto dv = to_device(h);
        check_pred(h, dv, pred);
        EXPECT_EQ(shp::find(shp::par_unseq, dv.begin(), dv.end(), 7) - dv.begin(), (long long)at);
      }
      std::vector<int> h(n, 0);
      h[b] = 7; // offset 0 of the later piece
      h[b - 1 - (seg > 2 ? seg - 2 : 0) / 2] = 7; // deep in the piece before
      auto dv = to_device(h);
      check_pred(h, dv, pred);
    }
  }
}

// the only inversion, and the only adjacent equal pair, exactly at each piece boundary
TEST(SeamsAtPieceBoundaries) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003)}) {
    shp::distributed_vector<int> probe(n);
    const std::size_t seg = probe.segment_size();
    {
      const auto h = ascending<int>(n);
      auto dv = to_device(h);
      check_order_default(h, dv); // sorted, no equal pair
    }
    for (std::size_t b : boundaries(n, seg)) {
      {
        auto h = ascending<int>(n);
        h[b] = h[b - 1] - 1; // (b - 1, b) descends; (b, b + 1) still ascends
        auto dv = to_device(h);
        check_order_default(h, dv);
        EXPECT_EQ(shp::is_sorted_until(shp::par_unseq, dv) - dv.begin(), (long long)b);
        EXPECT_TRUE(!shp::is_sorted(shp::par_unseq, dv.begin(), dv.end()));
      }
      {
        auto h = ascending<int>(n);
        h[b] = h[b - 1];
        auto dv = to_device(h);
        check_order_default(h, dv);
        EXPECT_EQ(shp::adjacent_find(shp::par_unseq, dv) - dv.begin(), (long long)(b - 1));
        EXPECT_TRUE(shp::is_sorted(shp::par_unseq, dv));
      }
    }
  }
}

// the same straddling pair when drop / slice leaves a piece empty, cuts a piece to one element, or starts mid-segment
TEST(SeamsUnderViews) {
  const std::size_t n = 100003;
  shp::distributed_vector<int> probe(n);
  const std::size_t seg = probe.segment_size();
  for (std::size_t b : boundaries(n, seg)) {
    for (int what = 0; what < 2; what++) {
      auto h = ascending<int>(n);
      h[b] = what ? h[b - 1] : h[b - 1] - 1;
      auto dv = to_device(h);
      auto sub = [&](std::size_t lo, std::size_t hi) { return std::vector<int>(h.begin() + (long)lo, h.begin() + (long)hi); };
      {
        // one element of the piece before, one of the piece after
        auto v = shp::views::slice(dv, {b - 1, b + 1});
        check_order_default(sub(b - 1, b + 1), v);
      }
      {
        auto v = dv | shp::views::drop(5) | shp::views::take(n - 11); // starts mid-segment, unaligned
        check_order_default(sub(5, n - 6), v);
      }
      {
        auto v = dv | shp::views::drop(b - 1); // every piece before is empty or gone
        check_order_default(sub(b - 1, n), v);
      }
      {
        auto v = dv | shp::views::take(b + 1); // every later piece is empty or gone
        check_order_default(sub(0, b + 1), v);
        auto pred = [] __host__ __device__(int x) { return x > 0; };
        check_pred(sub(0, b + 1), v, pred);
      }
    }
  }
}

// the extreme value duplicated in the first and the last piece: min_element and max_element give the first,
// the maximum of minmax_element the last
TEST(ExtremaDuplicatedAcrossPieces) {
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 21) + 13}) {
    auto h = few_values<int>(n, 300 + n, 1000);
    const std::size_t a = 3, z = n - 2;
    h[a] = h[z] = 5000;
    h[a + 1] = h[z - 1] = -5000;
    auto dv = to_device(h);
    check_order_default(h, dv);
    EXPECT_EQ(shp::max_element(shp::par_unseq, dv) - dv.begin(), (long long)a);
    EXPECT_EQ(shp::min_element(shp::par_unseq, dv) - dv.begin(), (long long)(a + 1));
    const auto mm = shp::minmax_element(shp::par_unseq, dv.begin(), dv.end());
    EXPECT_EQ(mm.first - dv.begin(), (long long)(a + 1));
    EXPECT_EQ(mm.second - dv.begin(), (long long)z);
    // under greater the roles swap: the "least" is the greatest value
    auto gt = [] __host__ __device__(int x, int y) { return x > y; };
    check_order(h, dv, gt, [] __host__ __device__(int x, int y) { return x == y; });
    EXPECT_EQ(shp::min_element(shp::par_unseq, dv, gt) - dv.begin(), (long long)a);
    // a constant range: min 0, max 0, minmax (0, n - 1)
    std::vector<int> c(n, 4);
    auto dc = to_device(c);
    check_order_default(c, dc);
    EXPECT_EQ(shp::minmax_element(shp::par_unseq, dc).second - dc.begin(), (long long)(n - 1));
  }
}

TEST(TransformViewInput) {
  for (std::size_t n : {std::size_t(1000), (std::size_t(1) << 21) + 13}) {
    const auto h = few_values<int>(n, 400 + n, 100000);
    auto dv = to_device(h);
    auto f = [] __host__ __device__(int x) { return (x % 1000) * 2 + 1; };
    std::vector<int> ht(n);
    std::transform(h.begin(), h.end(), ht.begin(), f);
    auto v = lib::views::transform(dv, f);
    check_order_default(ht, v);
    check_pred(ht, v, [] __host__ __device__(int x) { return x == 1999; });
    check_pred(ht, v, [] __host__ __device__(int x) { return x == 2; }); // even: never
  }
}

TEST(MismatchAndEqual) {
  for (std::size_t n : sizes()) {
    const auto h = few_values<int>(n, 500 + n, 1000);
    auto a = to_device(h), b = to_device(h);
    EXPECT_TRUE(shp::equal(shp::par_unseq, a, b));
    auto mm = shp::mismatch(shp::par_unseq, a, b);
    EXPECT_EQ(mm.first - a.begin(), (long long)n);
    EXPECT_EQ(mm.second - b.begin(), (long long)n);
    if (!n) continue;
    // the first and the last element of every piece, alone and together with a later one
    const std::size_t seg = a.segment_size();
    std::vector<std::size_t> at{0, n - 1, n / 2};
    if (n <= 100003)
      for (std::size_t x : boundaries(n, seg)) at.push_back(x - 1), at.push_back(x);
    for (std::size_t p : at) {
      auto h2 = h;
      h2[p] += 1;
      if (p != n - 1) h2[n - 1] += 1; // a later difference does not win
      auto c = to_device(h2);
      mm = shp::mismatch(shp::par_unseq, a, c);
      EXPECT_EQ(mm.first - a.begin(), (long long)p);
      EXPECT_EQ(mm.second - c.begin(), (long long)p);
      EXPECT_TRUE(!shp::equal(shp::par_unseq, a.begin(), a.end(), c.begin(), c.end()));
      // under a predicate that forgives a difference of one
      auto near = [] __host__ __device__(int x, int y) { return x - y <= 1 && y - x <= 1; };
      EXPECT_TRUE(shp::equal(shp::par_unseq, a, c, near));
      EXPECT_EQ(shp::mismatch(shp::par_unseq, a.begin(), a.end(), c.begin(), c.end(), near).first - a.begin(), (long long)n);
    }
  }
}

TEST(EqualSizesAndSegmentation) {
  const std::size_t n = 100003;
  const auto h = few_values<int>(n, 600, 1000);
  auto a = to_device(h);
  shp::distributed_vector<int> shorter(n - 1), longer(n + 1);
  EXPECT_TRUE(!shp::equal(shp::par_unseq, a, shorter)); // false, no throw
  EXPECT_TRUE(!shp::equal(shp::par_unseq, longer, a));
  if (shp::nprocs() > 1) {
    // the same size, segmented differently
    bool threw = false;
    try {
      shp::equal(shp::par_unseq, a, longer | shp::views::drop(1));
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
    threw = false;
    try {
      shp::mismatch(shp::par_unseq, a, longer | shp::views::drop(1));
    } catch (const std::invalid_argument &) {
      threw = true;
    }
    EXPECT_TRUE(threw);
  }
  // alike: both views cut the same way
  auto b = to_device(h);
  EXPECT_TRUE(shp::equal(shp::par_unseq, a | shp::views::drop(3), b | shp::views::drop(3)));
}

TEST(EmptyRange) {
  shp::distributed_vector<int> e(0);
  auto t = [] __host__ __device__(int) { return true; };
  EXPECT_TRUE(!shp::any_of(shp::par_unseq, e, t));
  EXPECT_TRUE(shp::all_of(shp::par_unseq, e, t));
  EXPECT_TRUE(shp::none_of(shp::par_unseq, e, t));
  EXPECT_TRUE(shp::find_if(shp::par_unseq, e, t) == e.end());
  EXPECT_TRUE(shp::min_element(shp::par_unseq, e) == e.end());
  EXPECT_TRUE(shp::max_element(shp::par_unseq, e) == e.end());
  EXPECT_TRUE(shp::minmax_element(shp::par_unseq, e).first == e.end());
  EXPECT_TRUE(shp::minmax_element(shp::par_unseq, e).second == e.end());
  EXPECT_TRUE(shp::is_sorted(shp::par_unseq, e));
  EXPECT_TRUE(shp::adjacent_find(shp::par_unseq, e) == e.end());
  EXPECT_TRUE(shp::equal(shp::par_unseq, e, e));
  // an empty view of a non-empty vector
  shp::distributed_vector<int> d(1000, 1);
  auto v = d | shp::views::take(0);
  EXPECT_TRUE(shp::all_of(shp::par_unseq, v, t) && !shp::any_of(shp::par_unseq, v, t));
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
    std::printf("[%s] Search.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

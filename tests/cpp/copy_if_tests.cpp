// shp::copy_if / count_if / count (dr/shp/select.hpp) against std::copy_if /
// std::count_if / std::count on the host copy.  The reference has no
// selection algorithm, so there is no gtest to restate; the runner takes
// --devicesCount N (N segments duplicated on one GPU) and --devices a,b,...
// (explicit device ids) as sort_by_key_tests does.
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

struct rec {
  int id;
  float w;
};
static_assert(sizeof(rec) == 8);

template <typename T> static std::vector<T> to_host(const shp::distributed_vector<T> &dv) {
  std::vector<T> h(dv.size());
  shp::copy(dv.begin(), dv.end(), h.begin());
  return h;
}
template <typename T> static bool same_bits(const std::vector<T> &a, const std::vector<T> &b) {
  return a.size() == b.size() && (a.empty() || std::memcmp(a.data(), b.data(), a.size() * sizeof(T)) == 0);
}

template <typename T> static T make_elem(std::size_t i, std::mt19937_64 &g) {
  if constexpr (std::is_same_v<T, rec>) return rec{(int)(g() % 1000003), (float)(i % 977) - 400.f};
  else if constexpr (std::is_floating_point_v<T>) return (T)std::normal_distribution<double>(0, 100)(g);
  else return (T)(g() % 2000003) - (T)1000000;
}
template <typename T> static T sentinel() {
  if constexpr (std::is_same_v<T, rec>) return rec{-7, -7.f};
  else return (T)-7;
}
template <typename T> static std::vector<T> make_data(std::size_t n, std::uint64_t seed) {
  std::vector<T> h(n);
  std::mt19937_64 g(seed);
  for (std::size_t i = 0; i < n; i++) h[i] = make_elem<T>(i, g);
  return h;
}

// the sizes of the issue: 0, 1, 2, P-1, P, P+1, 1000, 100003, 2^21+13
static std::vector<std::size_t> sizes() {
  const std::size_t P = shp::nprocs();
  return {0, 1, 2, P - 1, P, P + 1, 1000, 100003, (std::size_t(1) << 21) + 13};
}

// copy_if of the whole vector into the whole output (room for n), and into
// out | drop(k): result, returned iterator, untouched tail, count_if
template <typename T, typename Pred> static void whole_case(std::size_t n, std::uint64_t seed, Pred pred) {
  const std::vector<T> h = make_data<T>(n, seed);
  std::vector<T> want;
  std::copy_if(h.begin(), h.end(), std::back_inserter(want), pred);
  shp::distributed_vector<T> in(n);
  shp::copy(h.begin(), h.end(), in.begin());
  EXPECT_TRUE(shp::count_if(shp::par_unseq, in, pred) == want.size());
  EXPECT_TRUE(shp::count_if(shp::par_unseq, in, pred) == (std::size_t)std::count_if(h.begin(), h.end(), pred));
  {
    shp::distributed_vector<T> out(n, sentinel<T>());
    auto it = shp::copy_if(shp::par_unseq, in, out, pred);
    EXPECT_TRUE(it == out.begin() + (std::ptrdiff_t)want.size());
    std::vector<T> exp(n, sentinel<T>());
    std::copy(want.begin(), want.end(), exp.begin());
    EXPECT_TRUE(same_bits(to_host(out), exp)); // the survivors, then sentinels
  }
  {
    // the output starts k elements in, so the pieces straddle the output's
    // segment boundaries differently from the input's
    const std::size_t k = n / 3 + 1;
    shp::distributed_vector<T> out(n + k, sentinel<T>());
    auto ov = out | shp::views::drop(k);
    auto it = shp::copy_if(shp::par_unseq, in, ov, pred);
    EXPECT_TRUE(it == std::ranges::begin(ov) + (std::ptrdiff_t)want.size());
    std::vector<T> exp(n + k, sentinel<T>());
    std::copy(want.begin(), want.end(), exp.begin() + (std::ptrdiff_t)k);
    EXPECT_TRUE(same_bits(to_host(out), exp));
  }
}

struct always_true {
  template <typename T> __host__ __device__ bool operator()(const T &) const { return true; }
};
struct always_false {
  template <typename T> __host__ __device__ bool operator()(const T &) const { return false; }
};

TEST(AlwaysTrueFalse) {
  for (std::size_t n : sizes()) {
    whole_case<int>(n, 1 + n, always_true{});
    whole_case<int>(n, 2 + n, always_false{});
  }
  whole_case<double>(100003, 3, always_true{});
  whole_case<rec>(100003, 4, always_false{});
}

TEST(CapturingLambdaInt) {
  const int k = 7, r = 3;
  auto pred = [k, r] __host__ __device__(int x) { return ((x % k) + k) % k == r; };
  for (std::size_t n : sizes()) whole_case<int>(n, 10 + n, pred);
}

TEST(CapturingLambdaInt64) {
  const std::int64_t k = 5, r = 1;
  auto pred = [k, r] __host__ __device__(std::int64_t x) { return ((x % k) + k) % k == r; };
  for (std::size_t n : sizes()) whole_case<std::int64_t>(n, 20 + n, pred);
}

TEST(ThresholdFloat) {
  const float t = 25.f;
  auto pred = [t] __host__ __device__(float x) { return x > t; };
  for (std::size_t n : sizes()) whole_case<float>(n, 30 + n, pred);
}

TEST(ThresholdDouble) {
  const double t = -10.0;
  auto pred = [t] __host__ __device__(double x) { return x < t; };
  for (std::size_t n : sizes()) whole_case<double>(n, 40 + n, pred);
}

TEST(StructElements) {
  const float t = 0.f;
  auto pred = [t] __host__ __device__(const rec &x) { return x.w > t && (x.id & 1); };
  for (std::size_t n : sizes()) whole_case<rec>(n, 50 + n, pred);
}

TEST(Count) {
  for (std::size_t n : sizes()) {
    std::vector<int> h(n);
    std::mt19937_64 g(60 + n);
    for (auto &x : h) x = (int)(g() % 5);
    shp::distributed_vector<int> in(n);
    shp::copy(h.begin(), h.end(), in.begin());
    EXPECT_TRUE(shp::count(shp::par_unseq, in, 3) == (std::size_t)std::count(h.begin(), h.end(), 3));
    EXPECT_TRUE(shp::count(shp::par_unseq, in.begin(), in.end(), 9) == 0);
  }
  std::vector<float> hf = make_data<float>(100003, 61);
  hf[17] = hf[50000] = hf[100002] = 2.5f;
  shp::distributed_vector<float> df(hf.size());
  shp::copy(hf.begin(), hf.end(), df.begin());
  EXPECT_TRUE(shp::count(shp::par_unseq, df, 2.5f) == (std::size_t)std::count(hf.begin(), hf.end(), 2.5f));
}

// input views: drop(5) | take(n - 11) (starts mid-segment, not 16-byte
// aligned), a slice inside one segment, a transform view
TEST(InputViews) {
  const int k = 3, r = 1;
  auto pred = [k, r] __host__ __device__(int x) { return ((x % k) + k) % k == r; };
  for (std::size_t n : {std::size_t(1000), std::size_t(100003), (std::size_t(1) << 21) + 13}) {
    const std::vector<int> h = make_data<int>(n, 70 + n);
    shp::distributed_vector<int> in(n);
    shp::copy(h.begin(), h.end(), in.begin());
    {
      auto v = in | shp::views::drop(5) | shp::views::take(n - 11);
      std::vector<int> want;
      std::copy_if(h.begin() + 5, h.begin() + 5 + (std::ptrdiff_t)(n - 11), std::back_inserter(want), pred);
      EXPECT_TRUE(shp::count_if(shp::par_unseq, v, pred) == want.size());
      shp::distributed_vector<int> out(n, -7);
      auto it = shp::copy_if(shp::par_unseq, v, out, pred);
      EXPECT_TRUE(it == out.begin() + (std::ptrdiff_t)want.size());
      std::vector<int> exp(n, -7);
      std::copy(want.begin(), want.end(), exp.begin());
      EXPECT_TRUE(to_host(out) == exp);
    }
    {
      // inside segment 0: [3, 3 + len)
      const std::size_t seg = in.segment_size(), len = seg > 10 ? seg - 10 : 0;
      auto v = shp::views::slice(in, {3, 3 + len});
      std::vector<int> want;
      std::copy_if(h.begin() + 3, h.begin() + 3 + (std::ptrdiff_t)len, std::back_inserter(want), pred);
      EXPECT_TRUE(shp::count_if(shp::par_unseq, v, pred) == want.size());
      shp::distributed_vector<int> out(n, -7);
      auto it = shp::copy_if(shp::par_unseq, v, out, pred);
      EXPECT_TRUE(it == out.begin() + (std::ptrdiff_t)want.size());
      std::vector<int> exp(n, -7);
      std::copy(want.begin(), want.end(), exp.begin());
      EXPECT_TRUE(to_host(out) == exp);
    }
    {
      auto twice = [] __host__ __device__(int x) { return 2 * x + 1; };
      auto v = lib::views::transform(in, twice);
      std::vector<int> ht(n), want;
      std::transform(h.begin(), h.end(), ht.begin(), twice);
      std::copy_if(ht.begin(), ht.end(), std::back_inserter(want), pred);
      EXPECT_TRUE(shp::count_if(shp::par_unseq, v, pred) == want.size());
      shp::distributed_vector<int> out(n, -7);
      auto it = shp::copy_if(shp::par_unseq, v, out, pred);
      EXPECT_TRUE(it == out.begin() + (std::ptrdiff_t)want.size());
      std::vector<int> exp(n, -7);
      std::copy(want.begin(), want.end(), exp.begin());
      EXPECT_TRUE(to_host(out) == exp);
    }
  }
}

TEST(IteratorForms) {
  const std::size_t n = 100003;
  const std::vector<int> h = make_data<int>(n, 80);
  auto pred = [] __host__ __device__(int x) { return (x & 3) == 0; };
  shp::distributed_vector<int> in(n), out(n, -7);
  shp::copy(h.begin(), h.end(), in.begin());
  std::vector<int> want;
  std::copy_if(h.begin() + 100, h.end() - 200, std::back_inserter(want), pred);
  EXPECT_TRUE(shp::count_if(shp::par_unseq, in.begin() + 100, in.end() - 200, pred) == want.size());
  auto it = shp::copy_if(shp::par_unseq, in.begin() + 100, in.end() - 200, out.begin() + 50, pred);
  EXPECT_TRUE(it == out.begin() + 50 + (std::ptrdiff_t)want.size());
  std::vector<int> exp(n, -7);
  std::copy(want.begin(), want.end(), exp.begin() + 50);
  EXPECT_TRUE(to_host(out) == exp);
}

TEST(TooSmallOutputThrows) {
  const std::size_t n = 100003;
  const std::vector<int> h = make_data<int>(n, 90);
  auto pred = [] __host__ __device__(int x) { return (x & 1) == 0; };
  const std::size_t c = (std::size_t)std::count_if(h.begin(), h.end(), pred);
  shp::distributed_vector<int> in(n), out(c - 1, -7);
  shp::copy(h.begin(), h.end(), in.begin());
  bool threw = false;
  try {
    shp::copy_if(shp::par_unseq, in, out, pred);
  } catch (const std::out_of_range &) {
    threw = true;
  }
  EXPECT_TRUE(threw);
  EXPECT_TRUE(to_host(out) == std::vector<int>(c - 1, -7)); // unchanged
  // exactly enough room: fine
  shp::distributed_vector<int> fit(c, -7);
  auto it = shp::copy_if(shp::par_unseq, in, fit, pred);
  EXPECT_TRUE(it == fit.end());
  std::vector<int> want;
  std::copy_if(h.begin(), h.end(), std::back_inserter(want), pred);
  EXPECT_TRUE(to_host(fit) == want);
}

TEST(ScratchReusedAndRegrown) {
  auto pred = [] __host__ __device__(int x) { return x > 0; };
  whole_case<int>(60001, 100, pred);
  whole_case<int>((std::size_t(1) << 21) + 13, 101, pred); // larger: the cached scratch grows
  whole_case<int>(1000, 102, pred);
}

// every input segment cut at a third, both parts listed: two pieces share
// every rank's scratch block, each with its own compacted piece and status
TEST(SharedRankSegments) {
  const std::size_t n = (std::size_t(1) << 21) + 13;
  const std::vector<int> h = make_data<int>(n, 110);
  auto pred = [] __host__ __device__(int x) { return (x & 3) != 0; };
  shp::distributed_vector<int> in(n), out(n, -7);
  shp::copy(h.begin(), h.end(), in.begin());
  std::vector<shp::device_span<int>> parts;
  for (auto &&s : in.segments()) {
    const std::size_t a = s.size() / 3;
    parts.emplace_back(s.data(), a, s.rank());
    parts.emplace_back(s.data() + a, s.size() - a, s.rank());
  }
  shp::distributed_span<int> ds(parts);
  std::vector<int> want;
  std::copy_if(h.begin(), h.end(), std::back_inserter(want), pred);
  EXPECT_TRUE(shp::count_if(shp::par_unseq, ds, pred) == want.size());
  auto it = shp::copy_if(shp::par_unseq, ds, out, pred);
  EXPECT_TRUE(it == out.begin() + (std::ptrdiff_t)want.size());
  want.resize(n, -7);
  EXPECT_TRUE(to_host(out) == want);
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
    std::printf("[%s] CopyIf.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

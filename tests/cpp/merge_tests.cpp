// shp::merge and shp::merge_by_key (dr/shp/merge.hpp) against std::merge on
// host copies, byte for byte: the merge is stable (a's element first on ties,
// each input in its own order), so every output is defined exactly.  The
// reference has neither algorithm, so there is no gtest to restate; the
// runner takes --devicesCount N (N segments duplicated on one GPU) and
// --devices a,b,... (explicit device ids) as sorted_search_tests does.
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

template <typename T> static shp::distributed_vector<T> to_device(const std::vector<T> &h) {
  shp::distributed_vector<T> dv(h.size());
  if (!h.empty()) shp::copy(h.begin(), h.end(), dv.begin());
  return dv;
}
template <typename T> static std::vector<T> to_host(shp::distributed_vector<T> &dv) {
  std::vector<T> h(dv.size());
  if (!h.empty()) shp::copy(dv.begin(), dv.end(), h.data());
  return h;
}
template <typename T> static bool same_bytes(const T *a, const T *b, std::size_t n) {
  return n == 0 || std::memcmp(a, b, n * sizeof(T)) == 0;
}
// the first position at which two arrays differ as bytes, or n
template <typename T> static std::size_t first_diff(const T *a, const T *b, std::size_t n) {
  for (std::size_t i = 0; i < n; i++)
    if (std::memcmp(a + i, b + i, sizeof(T))) return i;
  return n;
}
// above one tile of every element width, and not a multiple of anything
static const std::size_t kSizes[] = {3, 1000, (std::size_t(1) << 17) + 7};

// sorted, `distinct` different values: dense duplicates, so equal runs lie on every seam
static std::vector<int> sorted_ints(std::size_t n, std::uint64_t seed, int distinct) {
  std::vector<int> h(n);
  std::mt19937_64 g(seed);
  for (auto &x : h) x = (int)(g() % (unsigned)distinct) - distinct / 2;
  std::sort(h.begin(), h.end());
  return h;
}

// a {key, payload} of BYTES bytes; ordered by the key alone, so only stability decides the order of ties
template <int BYTES> struct rec {
  int key;
  int tag;
  char pad[BYTES - 8];
};
template <> struct rec<8> {
  int key;
  int tag;
};
struct by_key {
  template <typename R> __host__ __device__ bool operator()(const R &a, const R &b) const { return a.key < b.key; }
};
template <int BYTES> static std::vector<rec<BYTES>> recs(const std::vector<int> &keys, int tag0) {
  std::vector<rec<BYTES>> h(keys.size());
  std::memset(static_cast<void *>(h.data()), 0, h.size() * sizeof(rec<BYTES>));
  for (std::size_t i = 0; i < keys.size(); i++) {
    h[i].key = keys[i];
    h[i].tag = tag0 + (int)i;
    if constexpr (BYTES > 8) h[i].pad[BYTES - 9] = (char)(i * 7 + 1);
  }
  return h;
}

// merge(a, b) into an output whose pieces start `off` elements into a longer vector, against std::merge of the
// host copies ha and hb; the elements of the vector before and behind the merge must keep their fill
template <typename T, typename RA, typename RB, typename Comp>
static void check_merge(const std::vector<T> &ha, RA &&a, const std::vector<T> &hb, RB &&b, std::size_t off, Comp comp) {
  const std::size_t n = ha.size() + hb.size(), tail = 5;
  std::vector<T> want(n);
  std::merge(ha.begin(), ha.end(), hb.begin(), hb.end(), want.begin(), comp);
  std::vector<T> fill(off + n + tail);
  std::memset(static_cast<void *>(fill.data()), 0x5A, fill.size() * sizeof(T));
  auto dv = to_device(fill);
  auto out = dv | shp::views::drop(off);
  auto end = shp::merge(shp::par_unseq, a, b, out, comp);
  EXPECT_EQ(end - std::ranges::begin(out), n);
  const auto got = to_host(dv);
  const std::size_t d = first_diff(got.data() + off, want.data(), n);
  if (d != n) std::printf("  na = %zu, nb = %zu, off = %zu: the first difference is at %zu\n", ha.size(), hb.size(), off, d);
  EXPECT_EQ(d, n);
  EXPECT_TRUE(same_bytes(got.data(), fill.data(), off));
  EXPECT_TRUE(same_bytes(got.data() + off + n, fill.data() + off + n, tail));
}

// inputs built as drops and slices of longer vectors, so no seam of a, b and out lines up with another
TEST(DifferentSegmentations) {
  for (std::size_t n : kSizes) {
    for (int distinct : {4, 100000}) {
      const auto wa = sorted_ints(n + 7, 1 + n + distinct, distinct);
      const auto wb = sorted_ints(n / 2 + 11, 2 + n + distinct, distinct);
      auto da = to_device(wa);
      auto db = to_device(wb);
      const std::vector<int> ha(wa.begin() + 1, wa.end()), hb(wb.begin() + 5, wb.end() - 4);
      check_merge(ha, da | shp::views::drop(1), hb, shp::views::slice(db, {5, wb.size() - 4}), 3, std::less<int>{});
      check_merge(hb, shp::views::slice(db, {5, wb.size() - 4}), ha, da | shp::views::drop(1), 0, std::less<int>{});
      check_merge(wa, da, wb, db, 1, std::less<int>{});
      // the default order
      shp::distributed_vector<int> out(wa.size() + wb.size());
      shp::merge(shp::par_unseq, da, db, out);
      std::vector<int> want(wa.size() + wb.size());
      std::merge(wa.begin(), wa.end(), wb.begin(), wb.end(), want.begin());
      const auto got = to_host(out);
      EXPECT_TRUE(same_bytes(got.data(), want.data(), want.size()));
    }
  }
}

// 3 elements over all the segments: with 8 segments most pieces are empty
TEST(FewElementsManySegments) {
  const std::vector<int> ha{1, 5}, hb{3};
  auto da = to_device(ha);
  auto db = to_device(hb);
  check_merge(ha, da, hb, db, 0, std::less<int>{});
  check_merge(hb, db, ha, da, 0, std::less<int>{});
  const std::vector<int> hc{5, 5, 5};
  auto dc = to_device(hc);
  check_merge(ha, da, hc, dc, 2, std::less<int>{});
}

TEST(EmptyInputs) {
  shp::distributed_vector<int> e(0);
  const std::vector<int> none;
  for (std::size_t n : kSizes) {
    const auto h = sorted_ints(n, 9 + n, 50);
    auto dv = to_device(h);
    check_merge(none, e, h, dv, 1, std::less<int>{});
    check_merge(h, dv, none, e, 0, std::less<int>{});
    // an empty view of a non-empty vector
    check_merge(none, dv | shp::views::take(0), h, dv, 0, std::less<int>{});
  }
  check_merge(none, e, none, e, 2, std::less<int>{});
  shp::distributed_vector<int> out(0);
  auto end = shp::merge(shp::par_unseq, e, e, out);
  EXPECT_TRUE(end == out.begin());
}

// every key equal: one run across every seam of a, b and out; the tags show a's elements first, in order
TEST(EqualRunsAcrossSeams) {
  for (std::size_t n : kSizes) {
    const std::vector<int> ka(n, 7), kb(n + 3, 7);
    const auto ha = recs<8>(ka, 0), hb = recs<8>(kb, 1 << 30);
    auto da = to_device(ha);
    auto db = to_device(hb);
    check_merge(ha, da, hb, db, 1, by_key{});
    // three runs, the middle one in both inputs and across their seams
    std::vector<int> k3a(n), k3b(n);
    for (std::size_t i = 0; i < n; i++) k3a[i] = i < n / 5 ? 1 : 2, k3b[i] = i < 4 * n / 5 ? 2 : 3;
    const auto h3a = recs<8>(k3a, 0), h3b = recs<8>(k3b, 1 << 30);
    auto d3a = to_device(h3a);
    auto d3b = to_device(h3b);
    check_merge(h3a, d3a, h3b, d3b, 0, by_key{});
    check_merge(h3b, d3b, h3a, d3a, 2, by_key{});
  }
}

template <int BYTES> static void struct_case() {
  static_assert(sizeof(rec<BYTES>) == BYTES);
  for (std::size_t n : {std::size_t(3), std::size_t(1000), std::size_t(20011)}) {
    const auto ha = recs<BYTES>(sorted_ints(n, 40 + n + BYTES, 9), 0);
    const auto hb = recs<BYTES>(sorted_ints(n / 3 + 2, 41 + n + BYTES, 9), 1 << 30);
    auto da = to_device(ha);
    auto db = to_device(hb);
    check_merge(ha, da, hb, db, 1, by_key{});
  }
}
TEST(StructsUnderKeyComparator) {
  struct_case<8>();
  struct_case<16>();
  struct_case<24>();
  struct_case<64>();
  struct_case<256>();
}

TEST(GreaterOnDescending) {
  for (std::size_t n : kSizes) {
    auto ha = sorted_ints(n, 50 + n, 1000), hb = sorted_ints(2 * n + 1, 51 + n, 1000);
    std::reverse(ha.begin(), ha.end());
    std::reverse(hb.begin(), hb.end());
    auto da = to_device(ha);
    auto db = to_device(hb);
    check_merge(ha, da, hb, db, 0, std::greater<int>{});
  }
}

TEST(TransformViewInput) {
  for (std::size_t n : kSizes) {
    const auto ha = sorted_ints(n, 60 + n, 300), hb = sorted_ints(n + 9, 61 + n, 900);
    auto da = to_device(ha);
    auto db = to_device(hb);
    auto f = [] __host__ __device__(int x) { return 3 * x + 1; }; // monotone: the view is sorted too
    std::vector<int> hat(n);
    std::transform(ha.begin(), ha.end(), hat.begin(), f);
    check_merge(hat, lib::views::transform(da, f), hb, db, 1, std::less<int>{});
    check_merge(hb, db | shp::views::drop(0), hat, lib::views::transform(da | shp::views::drop(0), f), 0, std::less<int>{});
  }
}

struct v12 {
  std::uint32_t w[3];
};
template <typename V> static V value_of(std::uint64_t t) {
  V v;
  std::memset(static_cast<void *>(&v), 0, sizeof(V));
  t = t * 0x9E3779B97F4A7C15ull + 1; // distinct for distinct tags (truncated for 1 byte)
  std::memcpy(static_cast<void *>(&v), &t, sizeof(V) < 8 ? sizeof(V) : 8);
  return v;
}
// keys with dense ties, values that name their source element; `off`: the outputs start there in longer vectors
template <typename V> static void by_key_case(std::size_t na, std::size_t nb, std::size_t off) {
  const auto ka = sorted_ints(na, 70 + na, 12), kb = sorted_ints(nb, 71 + nb, 12);
  std::vector<V> va(na), vb(nb);
  for (std::size_t i = 0; i < na; i++) va[i] = value_of<V>(i);
  for (std::size_t i = 0; i < nb; i++) vb[i] = value_of<V>((std::uint64_t(1) << 40) + i);
  const std::size_t n = na + nb;
  // the expected order: merge {key, source}
  struct src {
    int key;
    std::uint64_t at; // bit 63: from b
  };
  std::vector<src> sa(na), sb(nb), sm(n);
  for (std::size_t i = 0; i < na; i++) sa[i] = {ka[i], i};
  for (std::size_t i = 0; i < nb; i++) sb[i] = {kb[i], (std::uint64_t(1) << 63) | i};
  std::merge(sa.begin(), sa.end(), sb.begin(), sb.end(), sm.begin(), [](const src &x, const src &y) { return x.key < y.key; });
  std::vector<int> wk(n);
  std::vector<V> wv(n);
  for (std::size_t i = 0; i < n; i++) {
    wk[i] = sm[i].key;
    wv[i] = sm[i].at >> 63 ? vb[sm[i].at & ~(std::uint64_t(1) << 63)] : va[sm[i].at];
  }
  auto dka = to_device(ka);
  auto dkb = to_device(kb);
  auto dva = to_device(va);
  auto dvb = to_device(vb);
  std::vector<int> fk(off + n + 3, -77);
  std::vector<V> fv(off + n + 3, value_of<V>(12345));
  auto dko = to_device(fk);
  auto dvo = to_device(fv);
  auto ends = shp::merge_by_key(shp::par_unseq, dka, dva, dkb, dvb, dko | shp::views::drop(off), dvo | shp::views::drop(off));
  EXPECT_EQ(ends.first - std::ranges::begin(dko | shp::views::drop(off)), n);
  EXPECT_EQ(ends.second - std::ranges::begin(dvo | shp::views::drop(off)), n);
  const auto gk = to_host(dko);
  const auto gv = to_host(dvo);
  EXPECT_EQ(first_diff(gk.data() + off, wk.data(), n), n);
  EXPECT_EQ(first_diff(gv.data() + off, wv.data(), n), n);
  EXPECT_TRUE(same_bytes(gk.data(), fk.data(), off) && same_bytes(gk.data() + off + n, fk.data() + off + n, 3));
  EXPECT_TRUE(same_bytes(gv.data(), fv.data(), off) && same_bytes(gv.data() + off + n, fv.data() + off + n, 3));
}
TEST(MergeByKeyValueWidths) {
  for (std::size_t n : kSizes) {
    by_key_case<std::uint8_t>(n, n / 2 + 1, 0);
    by_key_case<std::uint32_t>(n, n + 5, 1);
    by_key_case<std::uint64_t>(n / 2 + 1, n, 0);
    by_key_case<v12>(n, n, 2);
  }
  by_key_case<std::uint32_t>(0, 100, 0);
  by_key_case<std::uint64_t>(100, 0, 1);
  by_key_case<std::uint32_t>(0, 0, 0);
}

// merge_by_key under a comparator, keys and values cut alike by a drop
TEST(MergeByKeyGreaterAndViews) {
  const std::size_t n = 5000;
  auto ka = sorted_ints(n, 80, 30), kb = sorted_ints(n + 17, 81, 30);
  std::reverse(ka.begin(), ka.end());
  std::reverse(kb.begin(), kb.end());
  std::vector<std::uint32_t> va(ka.size()), vb(kb.size());
  for (std::size_t i = 0; i < va.size(); i++) va[i] = (std::uint32_t)i;
  for (std::size_t i = 0; i < vb.size(); i++) vb[i] = 0x80000000u + (std::uint32_t)i;
  auto dka = to_device(ka);
  auto dkb = to_device(kb);
  auto dva = to_device(va);
  auto dvb = to_device(vb);
  const std::size_t m = ka.size() - 2 + kb.size();
  shp::distributed_vector<int> ko(m);
  shp::distributed_vector<std::uint32_t> vo(m);
  shp::merge_by_key(shp::par_unseq, dka | shp::views::drop(2), dva | shp::views::drop(2), dkb, dvb, ko, vo, std::greater<int>{});
  const auto gk = to_host(ko);
  const auto gv = to_host(vo);
  // every value names its source: the keys follow, and ties must be a's first, each in order
  std::size_t bad = 0, ia = 2, ib = 0;
  for (std::size_t i = 0; i < m; i++) {
    const bool take_b = ib < kb.size() && (ia >= ka.size() || kb[ib] > ka[ia]);
    const int wk = take_b ? kb[ib] : ka[ia];
    const std::uint32_t wv = take_b ? vb[ib] : va[ia];
    (take_b ? ib : ia)++;
    bad += gk[i] != wk || gv[i] != wv;
  }
  EXPECT_EQ(bad, 0);
}

TEST(IteratorForms) {
  const std::size_t n = 30011;
  const auto ha = sorted_ints(n, 90, 500), hb = sorted_ints(n / 2, 91, 500);
  auto da = to_device(ha);
  auto db = to_device(hb);
  std::vector<int> want(ha.size() + hb.size() - 9);
  std::merge(ha.begin(), ha.end() - 9, hb.begin(), hb.end(), want.begin());
  shp::distributed_vector<int> out(ha.size() + hb.size(), -5);
  auto e = shp::merge(shp::par_unseq, da.begin(), da.end() - 9, db.begin(), db.end(), out.begin());
  EXPECT_EQ(e - out.begin(), want.size());
  auto got = to_host(out);
  EXPECT_EQ(first_diff(got.data(), want.data(), want.size()), want.size());
  for (std::size_t i = want.size(); i < got.size(); i++) EXPECT_EQ(got[i], -5);
  // with a comparator, into the middle of the output
  shp::distributed_vector<int> out2(ha.size() + hb.size() + 4, -5);
  auto e2 = shp::merge(shp::par_unseq, da.begin(), da.end() - 9, db.begin(), db.end(), out2.begin() + 4, std::less<int>{});
  EXPECT_EQ(e2 - out2.begin(), want.size() + 4);
  got = to_host(out2);
  EXPECT_EQ(first_diff(got.data() + 4, want.data(), want.size()), want.size());
  for (std::size_t i = 0; i < 4; i++) EXPECT_EQ(got[i], -5);
  // by key
  std::vector<std::uint64_t> va(ha.size()), vb(hb.size());
  for (std::size_t i = 0; i < va.size(); i++) va[i] = i;
  for (std::size_t i = 0; i < vb.size(); i++) vb[i] = (std::uint64_t(1) << 40) + i;
  auto dva = to_device(va);
  auto dvb = to_device(vb);
  shp::distributed_vector<int> ko(ha.size() + hb.size(), -5);
  shp::distributed_vector<std::uint64_t> vo(ha.size() + hb.size(), 99);
  auto ends = shp::merge_by_key(shp::par_unseq, da.begin(), da.end() - 9, db.begin(), db.end(), dva.begin(), dvb.begin(),
                                ko.begin(), vo.begin());
  EXPECT_EQ(ends.first - ko.begin(), want.size());
  EXPECT_EQ(ends.second - vo.begin(), want.size());
  const auto gk = to_host(ko);
  const auto gv = to_host(vo);
  EXPECT_EQ(first_diff(gk.data(), want.data(), want.size()), want.size());
  std::size_t bad = 0;
  for (std::size_t i = 0; i < want.size(); i++) {
    const bool from_b = gv[i] >> 40;
    const std::size_t at = (std::size_t)(gv[i] & 0xFFFFFFFFFFull);
    bad += from_b ? (at >= hb.size() || hb[at] != gk[i]) : (at >= ha.size() - 9 || ha[at] != gk[i]);
    // stability: among equal keys a's come first and sources ascend
    if (i && gk[i - 1] == gk[i]) bad += gv[i - 1] >= gv[i];
  }
  EXPECT_EQ(bad, 0);
  for (std::size_t i = want.size(); i < gk.size(); i++) EXPECT_TRUE(gk[i] == -5 && gv[i] == 99);
}

template <typename E, typename F> static bool throws(F &&f) {
  try {
    f();
  } catch (const E &) {
    return true;
  }
  return false;
}

TEST(Exceptions) {
  const std::size_t na = 1000, nb = 500;
  const auto ha = sorted_ints(na, 31, 100), hb = sorted_ints(nb, 32, 100);
  auto da = to_device(ha);
  auto db = to_device(hb);
  {
    shp::distributed_vector<int> small(na + nb - 1, 99);
    EXPECT_TRUE(throws<std::out_of_range>([&] { shp::merge(shp::par_unseq, da, db, small); }));
    for (auto x : to_host(small)) EXPECT_EQ(x, 99); // untouched
    shp::distributed_vector<int> ko(na + nb, 99);
    shp::distributed_vector<int> vsmall(na + nb - 1, 99);
    EXPECT_TRUE(throws<std::out_of_range>([&] { shp::merge_by_key(shp::par_unseq, da, da, db, db, ko, vsmall); }));
    for (auto x : to_host(ko)) EXPECT_EQ(x, 99);
    for (auto x : to_host(vsmall)) EXPECT_EQ(x, 99);
  }
  if (shp::nprocs() > 1) {
    // values as long as their keys, segmented differently: the inputs', then the outputs'
    shp::distributed_vector<int> longer(na + 1, 1);
    shp::distributed_vector<int> ko(na + nb, 99), vo(na + nb, 99), vlong(na + nb + 1, 99);
    EXPECT_TRUE(throws<std::invalid_argument>(
        [&] { shp::merge_by_key(shp::par_unseq, da, longer | shp::views::drop(1), db, db, ko, vo); }));
    EXPECT_TRUE(throws<std::invalid_argument>(
        [&] { shp::merge_by_key(shp::par_unseq, da, da, db, db, ko, vlong | shp::views::drop(1)); }));
    for (auto x : to_host(ko)) EXPECT_EQ(x, 99);
    for (auto x : to_host(vo)) EXPECT_EQ(x, 99);
    for (auto x : to_host(vlong)) EXPECT_EQ(x, 99);
  }
  {
    // the output inside an input's memory
    const auto big = sorted_ints(4 * na, 33, 100);
    auto dbig = to_device(big);
    auto a = dbig | shp::views::take(na);
    EXPECT_TRUE(throws<std::invalid_argument>([&] { shp::merge(shp::par_unseq, a, db, dbig); }));
    EXPECT_TRUE(throws<std::invalid_argument>([&] { shp::merge(shp::par_unseq, db, a, dbig); }));
    shp::distributed_vector<int> ko(na + nb, 99);
    EXPECT_TRUE(throws<std::invalid_argument>([&] { shp::merge_by_key(shp::par_unseq, a, a, db, db, ko, dbig); }));
    const auto got = to_host(dbig);
    EXPECT_TRUE(same_bytes(got.data(), big.data(), big.size()));
    for (auto x : to_host(ko)) EXPECT_EQ(x, 99);
    // a transform view's base counts as the input's memory
    auto f = [] __host__ __device__(int x) { return x; };
    EXPECT_TRUE(throws<std::invalid_argument>([&] { shp::merge(shp::par_unseq, lib::views::transform(a, f), db, dbig); }));
  }
  {
    // an output piece of 2^32 elements: spans that claim the size over a small allocation; the refusal comes
    // before anything is read or written
    shp::distributed_vector<char> block(64, 'x');
    char *p = block.segments()[0].data();
    const std::size_t half = std::size_t(1) << 31;
    std::vector<shp::device_span<char>> sa{shp::device_span<char>(p, half, 0)}, so{shp::device_span<char>(p, 2 * half, 0)};
    shp::distributed_span<char> fa(sa), fo(so);
    EXPECT_TRUE(throws<std::length_error>([&] { shp::merge(shp::par_unseq, fa, fa, fo); }));
    for (auto x : to_host(block)) EXPECT_EQ(x, 'x');
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
    std::printf("[%s] Merge.%s\n", g_cur_failed ? "FAILED" : "    OK", t.name);
    failed += g_cur_failed;
    run++;
  }
  shp::finalize();
  std::printf("%d tests, %d failed\n", run, failed);
  return failed ? 1 : 0;
}

// msort::merge_path (dr/shp/merge_sort.hpp) against its definition, on the
// host: the number of A elements among the first `diag` outputs of std::merge
// of sorted A and B, A first on ties.  Every merge of the comparator sort --
// inside a tile, between tiles, between segments -- rests on this one
// function.  Host-only: no kernel is launched and no HIP call is made.
//
//   1. exhaustive: every pair of sorted A, B with na, nb <= 10 over the keys
//      {0, 1, 2} (empty A and empty B included) and every diag in
//      [0, na + nb], with I = int and I = std::size_t, ascending under `<` and
//      descending under `>`;
//   2. consecutive diagonals on random inputs of a few thousand elements with
//      few distinct keys: the split at diag + TILE minus the split at diag
//      lies in [0, TILE], and so does B's share -- what staging a tile's A and
//      B pieces in TILE elements of LDS depends on.
// Only merge_path's contract is checked; the kernels' index arithmetic is not
// restated here.
#include <dr/shp/merge_sort.hpp>

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <functional>
#include <random>
#include <vector>

namespace ms = shp::detail::msort;

struct item {
  int key;
  int from_a; // 1: an element of A
};

static long g_checked = 0, g_bad = 0;

// prefix[d] = A elements among the first d outputs of std::merge(A, B), A first on ties
template <typename Less> static std::vector<std::size_t> definition(const std::vector<int> &a, const std::vector<int> &b, Less less) {
  std::vector<item> ia, ib, out(a.size() + b.size());
  for (int k : a) ia.push_back({k, 1});
  for (int k : b) ib.push_back({k, 0});
  std::merge(ia.begin(), ia.end(), ib.begin(), ib.end(), out.begin(),
             [&](const item &x, const item &y) { return less(x.key, y.key); });
  std::vector<std::size_t> prefix(out.size() + 1, 0);
  for (std::size_t d = 0; d < out.size(); d++) prefix[d + 1] = prefix[d] + (std::size_t)out[d].from_a;
  return prefix;
}

template <typename I, typename Less> static void check_pair(const std::vector<int> &a, const std::vector<int> &b, Less less) {
  const std::vector<std::size_t> want = definition(a, b, less);
  const I na = (I)a.size(), nb = (I)b.size();
  for (I diag = 0; diag <= na + nb; diag++) {
    const I got = ms::merge_path<I>(a.data(), na, b.data(), nb, diag, less);
    g_checked++;
    if ((std::size_t)got != want[(std::size_t)diag]) {
      if (g_bad++ < 10)
        std::printf("merge_path: na = %zu, nb = %zu, diag = %zu: got %zu, want %zu\n", a.size(), b.size(), (std::size_t)diag,
                    (std::size_t)got, want[(std::size_t)diag]);
    }
  }
}

// every non-decreasing sequence over {0, 1, 2} of length 0..10: c0 zeros, c1 ones, c2 twos
static std::vector<std::vector<int>> all_sorted(bool descending) {
  std::vector<std::vector<int>> r;
  for (int len = 0; len <= 10; len++)
    for (int c0 = 0; c0 <= len; c0++)
      for (int c1 = 0; c0 + c1 <= len; c1++) {
        std::vector<int> s;
        s.insert(s.end(), (std::size_t)c0, 0);
        s.insert(s.end(), (std::size_t)c1, 1);
        s.insert(s.end(), (std::size_t)(len - c0 - c1), 2);
        if (descending) std::reverse(s.begin(), s.end());
        r.push_back(s);
      }
  return r;
}

template <typename I, typename Less> static void consecutive_diagonals(std::size_t na, std::size_t nb, int distinct, std::size_t tile,
                                                                        std::uint64_t seed, Less less) {
  std::mt19937_64 g(seed);
  std::vector<int> a(na), b(nb);
  for (auto &x : a) x = (int)(g() % (unsigned)distinct);
  for (auto &x : b) x = (int)(g() % (unsigned)distinct);
  std::sort(a.begin(), a.end(), less);
  std::sort(b.begin(), b.end(), less);
  const std::vector<std::size_t> want = definition(a, b, less);
  const std::size_t total = na + nb;
  std::size_t d0 = 0, s0 = (std::size_t)ms::merge_path<I>(a.data(), (I)na, b.data(), (I)nb, (I)0, less);
  if (s0 != 0) g_bad++;
  while (d0 < total) {
    const std::size_t d1 = std::min(total, d0 + tile);
    const std::size_t s1 = (std::size_t)ms::merge_path<I>(a.data(), (I)na, b.data(), (I)nb, (I)d1, less);
    g_checked++;
    const bool ok = s1 == want[d1] && s1 >= s0 && s1 - s0 <= tile && (d1 - s1) >= (d0 - s0) && (d1 - s1) - (d0 - s0) <= tile &&
                    (s1 - s0) + ((d1 - s1) - (d0 - s0)) == d1 - d0 && s1 <= na && d1 - s1 <= nb;
    if (!ok && g_bad++ < 10)
      std::printf("diagonals: na = %zu, nb = %zu, tile = %zu, diag %zu -> %zu: split %zu -> %zu, want %zu\n", na, nb, tile, d0, d1,
                  s0, s1, want[d1]);
    d0 = d1;
    s0 = s1;
  }
  if (s0 != na) g_bad++; // the last diagonal has all of A
}

int main() {
  for (bool descending : {false, true}) {
    const auto seqs = all_sorted(descending);
    for (const auto &a : seqs)
      for (const auto &b : seqs) {
        if (descending) {
          check_pair<int>(a, b, std::greater<int>{});
          check_pair<std::size_t>(a, b, std::greater<int>{});
        } else {
          check_pair<int>(a, b, std::less<int>{});
          check_pair<std::size_t>(a, b, std::less<int>{});
        }
      }
  }
  const long exhaustive = g_checked;
  std::uint64_t seed = 1;
  const std::vector<std::pair<std::size_t, std::size_t>> shapes{{4096, 4096}, {5000, 3001}, {1, 6000}, {6000, 1},
                                                               {0, 4097},    {4097, 0},    {2048, 2049}};
  for (std::size_t tile : {256, 512, 1024, 2048})
    for (int distinct : {1, 2, 5, 17, 1000})
      for (auto [na, nb] : shapes) {
        consecutive_diagonals<int>(na, nb, distinct, tile, seed++, std::less<int>{});
        consecutive_diagonals<std::size_t>(na, nb, distinct, tile, seed++, std::less<int>{});
        consecutive_diagonals<std::size_t>(na, nb, distinct, tile, seed++, std::greater<int>{});
      }
  std::printf("merge_path: %ld (A, B, diag) triples checked exhaustively, %ld tile diagonals on random inputs, %ld wrong\n", exhaustive,
              g_checked - exhaustive, g_bad);
  if (g_checked == 0 || exhaustive == 0) return 1;
  std::printf("%s\n", g_bad ? "FAILED" : "PASSED");
  return g_bad ? 1 : 0;
}

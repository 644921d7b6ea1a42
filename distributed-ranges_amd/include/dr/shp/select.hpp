// dr/shp/select.hpp -- shp::count_if, shp::count and shp::copy_if: selection
// by a predicate over a distributed range.
//
// Absent from the reference (its shp algorithms are for_each, reduce,
// inclusive_scan, gemv); defined with the semantics of std::count_if /
// std::count / std::copy_if over the whole range: the survivors appear in
// input order, contiguously from begin(out), across output segment
// boundaries wherever those fall.
//
// `pred` is any trivially copyable device callable (captures included); the
// kernel template (dr/details/select_kernel.hpp, the one the C-ABI's
// drhip_copy_if / drhip_count_if are built from) is instantiated here, in the
// user's translation unit, like the look-back scan of dr/shp/scan.hpp.  The
// input is any range the template reduce accepts: a distributed_vector, its
// take / drop / slice subranges (16-byte loads when a piece is 16-byte
// aligned, element loads through the accessor otherwise) and a transform
// view over those.  A zipped input is not supported.
//
// copy_if:
//   1. every input piece is compacted on its own segment stream, all pieces
//      concurrently, into that segment's detail::device_scratch(); its count
//      goes to a pinned slot;
//   2. one wait; the host takes the exclusive prefix of the P counts;
//   3. a total above size(out) throws std::out_of_range before anything is
//      written to out;
//   4. each compacted piece is copied into out with drhip_memcpy_d2d, split
//      at output segment boundaries (peer copies when devices differ);
//   5. sync.
// One look-back pass and bulk copies; the temporary is as large as the piece
// (DESIGN.md "Selection" has the alternative that avoids it).  A piece of
// 2^32 elements or more throws std::length_error; an empty piece contributes
// 0 and launches nothing.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <type_traits>
#include <vector>

#include "../details/select_kernel.hpp"
#include "algorithms.hpp"

namespace shp {

namespace detail {

// pred(x) as the kernel's pred(x, index)
template <typename Pred> struct sel_value_pred {
  Pred p;
  template <typename T> __device__ __forceinline__ bool operator()(const T &x, std::size_t) const {
    return static_cast<bool>(p(x));
  }
};
template <typename T> struct sel_equal_to {
  T value;
  __device__ __forceinline__ bool operator()(const T &x) const { return x == value; }
};

constexpr unsigned kSelCountGrid = 512; // count_if's grid limit: 2 blocks per CU of a 256-CU device
inline std::size_t sel_round(std::size_t b) { return (b + 255) & ~std::size_t(255); }

// Enqueue the selection (MODE: a store variant) or the count (SEL_COUNT) of
// the non-empty piece s on its segment's stream; `state` is device memory of
// that segment, sel_state_bytes (SEL_COUNT: kSelHeadBytes) long.
template <typename V, int MODE, typename Seg, typename Pred>
void select_launch(const Seg &s, V *out, Pred pred, char *state, unsigned long long *total, unsigned *err) {
  using namespace dr_select;
  const std::size_t n = s.size();
  hipStream_t st = stream(s.rank());
  const std::size_t bytes = MODE == SEL_COUNT ? kSelHeadBytes : sel_state_bytes<V>(n);
  hip_check(hipMemsetAsync(state, 0, bytes, st), "selection status clear");
  const sel_args a{state, total, err};
  const sel_value_pred<Pred> p{pred};
  if constexpr (is_device_span<Seg>) {
    using E = std::remove_const_t<typename Seg::value_type>;
    if constexpr (std::is_same_v<E, V>) {
      hip_check(sel_launch_span<V, MODE>(st, static_cast<const V *>(s.data()), out, n, p, a, kSelCountGrid),
                "selection launch");
      return;
    }
  }
  hip_check(sel_launch_accessor<V, MODE>(st, accessor_of(s), out, n, p, a, kSelCountGrid), "selection launch");
}

inline void select_check(unsigned err) {
  if (err & dr_select::SEL_ERR_CLAIM)
    throw std::runtime_error("shp: selection: a tile claim past the grid (counter not reset)");
  if (err) throw std::runtime_error("shp: selection: a bounded in-kernel spin timed out");
}

template <typename Segs> void select_sync(const Segs &segs) {
  std::vector<std::size_t> ranks;
  for (auto &s : segs)
    if (s.size()) ranks.push_back(s.rank());
  std::sort(ranks.begin(), ranks.end());
  ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
  for (auto rk : ranks) sync(rk);
}

template <typename Seg> void select_check_piece(const Seg &s) {
  if (static_cast<unsigned long long>(s.size()) >= (1ull << 32))
    throw std::length_error("shp: selection: a piece of 2^32 elements or more on one segment");
}

} // namespace detail

template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
std::size_t count_if(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  if (segs.empty()) return 0;
  using Seg = std::remove_cvref_t<decltype(segs[0])>;
  using V = typename decltype(detail::value_type_of_segment<Seg>())::type;
  const std::size_t P = segs.size();
  for (auto &s : segs) detail::select_check_piece(s);
  detail::pinned<unsigned long long> cnt(P);
  detail::pinned<unsigned> err(1);
  err[0] = 0;
  for (std::size_t k = 0; k < P; k++) {
    cnt[k] = 0;
    if (!segs[k].size()) continue;
    char *state = static_cast<char *>(detail::device_scratch().get(segs[k].rank(), dr_select::kSelHeadBytes));
    detail::select_launch<V, dr_select::SEL_COUNT>(segs[k], static_cast<V *>(nullptr), pred, state, &cnt[k],
                                                   err.data());
  }
  detail::select_sync(segs);
  detail::select_check(err[0]);
  std::size_t total = 0;
  for (std::size_t k = 0; k < P; k++) total += static_cast<std::size_t>(cnt[k]);
  return total;
}

template <typename ExecutionPolicy, lib::distributed_range R, typename T>
std::size_t count(ExecutionPolicy &&policy, R &&r, const T &value) {
  using Seg = std::remove_cvref_t<decltype(lib::ranges::segments(r)[0])>;
  using V = typename decltype(detail::value_type_of_segment<Seg>())::type;
  return shp::count_if(std::forward<ExecutionPolicy>(policy), std::forward<R>(r),
                       detail::sel_equal_to<V>{static_cast<V>(value)});
}

// Returns begin(out) + the number copied.
template <typename ExecutionPolicy, lib::distributed_range R, lib::distributed_contiguous_range O, typename Pred>
auto copy_if(ExecutionPolicy &&, R &&r, O &&out, Pred pred) {
  auto segs = lib::ranges::segments(r);
  auto osegs = lib::ranges::segments(out);
  using Seg = std::remove_cvref_t<decltype(segs[0])>;
  using V = typename decltype(detail::value_type_of_segment<Seg>())::type;
  static_assert(std::is_same_v<std::remove_cv_t<std::ranges::range_value_t<O>>, std::remove_cv_t<V>>,
                "shp::copy_if: the output's value type must be the input's");
  static_assert(std::is_trivially_copyable_v<V>, "shp::copy_if: elements move as bits");
  const std::size_t P = segs.size();
  for (auto &s : segs) detail::select_check_piece(s);

  // per segment: [compacted piece | status words] for each of its pieces
  struct piece {
    std::size_t tmp = 0, state = 0;
  };
  std::vector<piece> lay(P);
  std::vector<std::size_t> need(nprocs(), 0);
  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = segs[k].size();
    if (!n) continue;
    std::size_t &b = need.at(segs[k].rank());
    lay[k].tmp = b;
    b += detail::sel_round(n * sizeof(V));
    lay[k].state = b;
    b += detail::sel_round(dr_select::sel_state_bytes<V>(n));
  }
  std::vector<char *> base(need.size(), nullptr);
  for (std::size_t rk = 0; rk < need.size(); rk++)
    if (need[rk]) base[rk] = static_cast<char *>(detail::device_scratch().get(rk, need[rk]));

  detail::pinned<unsigned long long> cnt(P);
  detail::pinned<unsigned> err(1);
  err[0] = 0;
  for (std::size_t k = 0; k < P; k++) {
    cnt[k] = 0;
    if (!segs[k].size()) continue;
    char *b = base[segs[k].rank()];
    detail::select_launch<V, dr_select::kSelMode>(segs[k], reinterpret_cast<V *>(b + lay[k].tmp), pred,
                                                  b + lay[k].state, &cnt[k], err.data());
  }
  detail::select_sync(segs);
  detail::select_check(err[0]);

  std::size_t total = 0;
  for (std::size_t k = 0; k < P; k++) total += static_cast<std::size_t>(cnt[k]);
  if (total > static_cast<std::size_t>(std::ranges::size(out)))
    throw std::out_of_range("shp::copy_if: " + std::to_string(total) + " elements selected, the output holds " +
                            std::to_string(std::ranges::size(out)));

  // the compacted pieces, in order, into the output's segments
  std::size_t oi = 0, ooff = 0;
  for (std::size_t k = 0; k < P; k++) {
    std::size_t c = static_cast<std::size_t>(cnt[k]);
    if (!c) continue;
    const V *src = reinterpret_cast<const V *>(base[segs[k].rank()] + lay[k].tmp);
    while (c) {
      if (ooff == osegs[oi].size()) {
        oi++;
        ooff = 0;
        continue;
      }
      const std::size_t m = std::min(c, osegs[oi].size() - ooff);
      detail::check(drhip_memcpy_d2d(static_cast<int>(segs[k].rank()), osegs[oi].data() + ooff, src, m * sizeof(V)),
                    "drhip_memcpy_d2d");
      src += m;
      ooff += m;
      c -= m;
    }
  }
  detail::select_sync(segs);
  return std::ranges::begin(out) + static_cast<std::ranges::range_difference_t<O>>(total);
}

// iterator forms
template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename Pred>
std::size_t count_if(ExecutionPolicy &&policy, Iter first, Iter last, Pred pred) {
  return shp::count_if(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), pred);
}
template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename T>
std::size_t count(ExecutionPolicy &&policy, Iter first, Iter last, const T &value) {
  return shp::count(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), value);
}
// std::copy_if's form: the output starts at d_first and has room for the
// elements selected (at most last - first are written; the output is taken
// to end with d_first's container if that comes sooner)
template <typename ExecutionPolicy, lib::distributed_iterator Iter, lib::distributed_iterator OutputIter, typename Pred>
OutputIter copy_if(ExecutionPolicy &&policy, Iter first, Iter last, OutputIter d_first, Pred pred) {
  std::size_t room = 0;
  for (auto &s : d_first.segments()) room += s.size();
  const std::size_t len = std::min(room, static_cast<std::size_t>(last - first));
  return shp::copy_if(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last),
                      std::ranges::subrange(d_first, d_first + static_cast<std::ptrdiff_t>(len)), pred);
}

} // namespace shp

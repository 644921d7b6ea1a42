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
//      concurrently, into its slice of that segment's device scratch
//      (detail::carve_scratch); its count goes to a pinned slot;
//   2. one wait; the host takes the exclusive prefix of the P counts;
//   3. a total above size(out) throws std::out_of_range before anything is
//      written to out;
//   4. each compacted piece is copied into out with drhip_memcpy_d2d, split
//      at output segment boundaries (peer copies when devices differ);
//   5. sync.
// The plumbing the by-key algorithms (reduce_by_key.hpp, scan_by_key.hpp)
// share with copy_if is here too: the walk over output segments
// (detail::out_cursor), the argument checks (check_piece_sizes,
// check_segmented_alike) and the output of an iterator form (out_from).
// One look-back pass and bulk copies; the temporary is as large as the piece
// (DESIGN.md "Selection" has the alternative that avoids it).  A piece of
// 2^32 elements or more throws std::length_error; an empty piece contributes
// 0 and launches nothing.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
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

// the kernels of this family index a piece with 32 bits
template <typename Segs> void check_piece_sizes(const char *what, const Segs &segs) {
  for (auto &s : segs)
    if (static_cast<unsigned long long>(s.size()) >= (1ull << 32))
      throw std::length_error(std::string(what) + ": a piece of 2^32 elements or more on one segment");
}

// a value travels beside its key: piece k of both on one rank, equally long
template <typename KSegs, typename VSegs>
void check_segmented_alike(const char *what, const KSegs &ksegs, const VSegs &vsegs) {
  bool alike = ksegs.size() == vsegs.size();
  for (std::size_t k = 0; alike && k < ksegs.size(); k++)
    alike = ksegs[k].size() == vsegs[k].size() && ksegs[k].rank() == vsegs[k].rank();
  if (!alike) throw std::invalid_argument(std::string(what) + ": keys and values are segmented differently");
}

// A position in a list of output segments (contiguous device spans).
template <typename OSegs> struct out_cursor {
  const OSegs *segs = nullptr;
  std::size_t seg = 0, off = 0;
  // the segment that holds the next element (exhausted and empty segments are passed over; an element must be left),
  // the next element, and the room from it to that segment's end
  const auto &segment() {
    while (off == (*segs)[seg].size()) {
      seg++;
      off = 0;
    }
    return (*segs)[seg];
  }
  auto *next() { return segment().data() + off; }
  std::size_t room() { return segment().size() - off; }
  // the position c elements further
  void advance(std::size_t c) {
    walk(c, [](auto *, std::size_t) {});
  }
  // c elements of src (device memory of segment rank rk) to the position and past them, split at segment
  // boundaries (peer copies when devices differ)
  template <typename T> void emit(std::size_t rk, const T *src, std::size_t c) {
    walk(c, [&](auto *dst, std::size_t m) {
      check(drhip_memcpy_d2d(static_cast<int>(rk), dst, src, m * sizeof(T)), "drhip_memcpy_d2d");
      src += m;
    });
  }
  // the element passed last (after an advance or emit of c > 0)
  auto *last() const { return (*segs)[seg].data() + (off - 1); }

private:
  template <typename F> void walk(std::size_t c, F &&f) {
    while (c) {
      const std::size_t m = std::min(c, room());
      f(next(), m);
      off += m;
      c -= m;
    }
  }
};

// An output given by its first iterator: it has room for at most n elements
// and is taken to end with the iterator's container if that comes sooner.
template <typename OutputIter> auto out_from(OutputIter d_first, std::size_t n) {
  std::size_t room = 0;
  for (auto &s : d_first.segments()) room += s.size();
  return std::ranges::subrange(d_first, d_first + static_cast<std::ptrdiff_t>(std::min(room, n)));
}

} // namespace detail

template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
std::size_t count_if(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  if (segs.empty()) return 0;
  using Seg = std::remove_cvref_t<decltype(segs[0])>;
  using V = typename decltype(detail::value_type_of_segment<Seg>())::type;
  const std::size_t P = segs.size();
  detail::check_piece_sizes("shp: selection", segs);
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
  detail::check_piece_sizes("shp: selection", segs);

  // per non-empty piece: [compacted piece | status words]
  enum { TMP, STATE };
  std::vector<detail::scratch_layout<2>> lay(P);
  std::vector<std::size_t> rank(P);
  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = segs[k].size();
    rank[k] = segs[k].rank();
    if (n) lay[k] = {n * sizeof(V), dr_select::sel_state_bytes<V>(n)};
  }
  const std::vector<char *> base = detail::carve_scratch(rank, lay);

  detail::pinned<unsigned long long> cnt(P);
  detail::pinned<unsigned> err(1);
  err[0] = 0;
  for (std::size_t k = 0; k < P; k++) {
    cnt[k] = 0;
    if (!segs[k].size()) continue;
    detail::select_launch<V, dr_select::kSelMode>(segs[k], lay[k].template at<V>(base[k], TMP), pred,
                                                  lay[k].at(base[k], STATE), &cnt[k], err.data());
  }
  detail::select_sync(segs);
  detail::select_check(err[0]);

  std::size_t total = 0;
  for (std::size_t k = 0; k < P; k++) total += static_cast<std::size_t>(cnt[k]);
  if (total > static_cast<std::size_t>(std::ranges::size(out)))
    throw std::out_of_range("shp::copy_if: " + std::to_string(total) + " elements selected, the output holds " +
                            std::to_string(std::ranges::size(out)));

  // the compacted pieces, in order, into the output's segments
  detail::out_cursor<decltype(osegs)> cur{&osegs};
  for (std::size_t k = 0; k < P; k++)
    if (cnt[k]) cur.emit(segs[k].rank(), lay[k].template at<const V>(base[k], TMP), static_cast<std::size_t>(cnt[k]));
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
// elements selected (at most last - first are written)
template <typename ExecutionPolicy, lib::distributed_iterator Iter, lib::distributed_iterator OutputIter, typename Pred>
OutputIter copy_if(ExecutionPolicy &&policy, Iter first, Iter last, OutputIter d_first, Pred pred) {
  return shp::copy_if(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last),
                      detail::out_from(d_first, static_cast<std::size_t>(last - first)), pred);
}

} // namespace shp

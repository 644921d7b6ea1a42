// dr/shp/search.hpp -- the algorithms that answer a question about a
// distributed range with a position or a bool: find, find_if, find_if_not,
// any_of, all_of, none_of, adjacent_find, is_sorted_until, is_sorted,
// min_element, max_element, minmax_element, mismatch, equal.
//
// Absent from the reference (its shp algorithms are for_each, reduce,
// inclusive_scan, gemv); defined with the semantics of their std:: namesakes
// over the whole range.  Each takes an execution policy first and has a range
// and an iterator-pair form; a position is returned as an iterator of the
// range, begin(r) + k, or end(r).  minmax_element returns {first least, LAST
// greatest}, as std::minmax_element does.  mismatch and equal take two ranges
// of one value type: equal returns false at once for unequal sizes; otherwise
// the ranges must be segmented alike (detail::check_segmented_alike:
// std::invalid_argument), as keys and values are in the by-key family.  The
// iterator forms of mismatch and equal take both ends: (first1, last1,
// first2, last2[, pred]).
//
// Callables (pred, comp) are trivially copyable device callables, captures
// included; they are only ever called on the device.  The kernel templates
// (dr/details/search_kernel.hpp, the ones the C-ABI's drhip_find_if ...
// drhip_minmax_element are built from) are instantiated here, in the user's
// translation unit.  The input is what count_if accepts: a
// distributed_vector, its take / drop / slice subranges (16-byte loads when a
// piece is 16-byte aligned, element loads through the accessor otherwise) and
// a transform view over those.  A zipped input is not supported.
//
// Across pieces: every non-empty piece is searched on its own segment stream,
// all pieces concurrently, the kernels' state in the segment's device scratch
// (detail::carve_scratch), every result in a pinned slot; one wait; the host
// only adds offsets and picks among P numbers.
//   * first match: the answer is the hit of the lowest piece that has one,
//     plus that piece's offset in the range.  There is no early exit ACROSS
//     pieces: a piece does not learn of a hit in an earlier piece and reads on
//     to its own first hit (inside a piece the kernel stops early).
//   * adjacent_find, is_sorted_until: the pair that straddles two pieces --
//     the last element of a non-empty piece and the first of the next
//     non-empty piece, empty pieces in between skipped -- is seen by neither
//     launch.  Every piece leaves its first and last element in a pinned
//     record (one thread, behind its search); one thread on the first piece's
//     stream, behind an event of every other piece, evaluates the seams on
//     the device.  A seam's hit competes with the in-piece hits by its
//     position in the range.
//   * extrema: each piece yields its winner's local index and, stored by the
//     same finishing kernel into one pinned array in piece order, its
//     winner's value.  The arg-extremum kernel then runs over those P values
//     on the first piece's stream, behind an event of every other piece: its
//     tie rule picks the earliest piece for min and max and the latest for
//     the maximum of minmax_element.  comp never runs on the host.
// A piece of 2^32 elements or more throws std::length_error; an empty piece
// launches nothing.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../details/search_kernel.hpp"
#include "reduce_by_key.hpp"
#include "select.hpp"

namespace shp {

namespace detail {

constexpr unsigned kSrchGrid = 512; // the searches' grid limit: count_if's (kSelCountGrid)
constexpr std::size_t kSrchNoPos = ~std::size_t(0);

// pred(x) as the kernel's pred(x, index); NEG: its negation
template <typename Pred, bool NEG> struct srch_value_pred {
  Pred p;
  template <typename T> __device__ __forceinline__ bool operator()(const T &x, std::size_t) const {
    return static_cast<bool>(p(x)) != NEG;
  }
};
template <typename Pred2, bool NEG> struct srch_pair_pred {
  Pred2 p;
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const {
    return static_cast<bool>(p(a, b)) != NEG;
  }
};
// the pair (a, b) ends a prefix sorted under comp
template <typename Comp> struct srch_descent {
  Comp c;
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const {
    return static_cast<bool>(c(b, a));
  }
};
struct srch_less {
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const { return a < b; }
};
struct srch_equal_to {
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const { return a == b; }
};

template <typename Seg, typename V> constexpr bool srch_span_of() {
  if constexpr (is_device_span<Seg>) return std::is_same_v<std::remove_const_t<typename Seg::value_type>, V>;
  else return false;
}

// a piece's ends, in pinned memory
template <typename V> struct srch_edge {
  unsigned long long n; // the piece's size (host); 0: an empty piece
  V first, last;
};
template <typename V, typename Acc> __global__ void srch_edge_kernel(Acc in, std::size_t n, srch_edge<V> *e) {
  e->first = static_cast<V>(in(0));
  e->last = static_cast<V>(in(n - 1));
}
// One thread walks the P records: seam[k] = pred(last element before piece k, first element of piece k).
template <typename V, typename Pred2>
__global__ void srch_seam_kernel(const srch_edge<V> *e, std::size_t P, Pred2 pred, unsigned long long *seam) {
  long prev = -1;
  for (std::size_t k = 0; k < P; k++) {
    if (!e[k].n) continue;
    seam[k] = prev >= 0 && pred(e[prev].last, e[k].first) ? 1 : 0;
    prev = (long)k;
  }
}

// The position in the range of the first match, or kSrchNoPos.  segs2 is read by SRCH_TWO only.
template <int KIND, typename Segs, typename Segs2, typename Pred>
std::size_t search_first(const char *what, const Segs &segs, const Segs2 &segs2, Pred pred) {
  using namespace dr_search;
  if (segs.empty()) return kSrchNoPos;
  using Seg = std::remove_cvref_t<decltype(segs[0])>;
  using Seg2 = std::remove_cvref_t<decltype(segs2[0])>;
  using V = typename decltype(value_type_of_segment<Seg>())::type;
  static_assert(std::is_same_v<V, typename decltype(value_type_of_segment<Seg2>())::type>,
                "shp: the two ranges of mismatch / equal have one value type");
  static_assert(std::is_trivially_copyable_v<V>, "shp: the searches read elements as bits");
  static_assert(std::is_trivially_copyable_v<Pred>, "shp: callables are passed to the device by value");
  const std::size_t P = segs.size();
  check_piece_sizes(what, segs);

  std::vector<scratch_layout<1>> lay(P);
  std::vector<std::size_t> rank(P);
  for (std::size_t k = 0; k < P; k++) {
    rank[k] = segs[k].rank();
    if (segs[k].size()) lay[k] = {kSrchHeadBytes};
  }
  const std::vector<char *> base = carve_scratch(rank, lay);

  constexpr bool ADJ = KIND == SRCH_ADJACENT;
  pinned<unsigned long long> hit(P), seam(P);
  pinned<srch_edge<V>> edge(ADJ ? P : 1);
  by_key_events events;
  long first = -1;
  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = segs[k].size();
    hit[k] = kSrchNone;
    seam[k] = 0;
    if constexpr (ADJ) edge[k].n = n;
    if (!n) continue;
    hipStream_t st = stream(rank[k]);
    const srch_first_args a{base[k], &hit[k], kSrchNone, 0, kSrchGrid};
    if constexpr (srch_span_of<Seg, V>() && srch_span_of<Seg2, V>())
      hip_check((srch_first_span<V, KIND>(st, static_cast<const V *>(segs[k].data()),
                                          static_cast<const V *>(segs2[k].data()), n, pred, a)),
                what);
    else
      hip_check((srch_first_accessor<V, KIND>(st, accessor_of(segs[k]), accessor_of(segs2[k]), n, pred, a)), what);
    if constexpr (ADJ) {
      auto acc = accessor_of(segs[k]);
      hipLaunchKernelGGL((srch_edge_kernel<V, decltype(acc)>), dim3(1), dim3(1), 0, st, acc, n, &edge[k]);
      hip_check(hipGetLastError(), what);
      if (first >= 0 && rank[k] != rank[first]) events.record(st);
    }
    if (first < 0) first = (long)k;
  }
  if (first < 0) return kSrchNoPos;
  if constexpr (ADJ) {
    hipStream_t st = stream(rank[first]);
    events.wait_on(st);
    hipLaunchKernelGGL((srch_seam_kernel<V, Pred>), dim3(1), dim3(1), 0, st, edge.data(), P, pred, seam.data());
    hip_check(hipGetLastError(), what);
  }
  select_sync(segs); // the one wait

  std::size_t off = 0;
  for (std::size_t k = 0; k < P; k++) {
    if (seam[k]) return off - 1; // the pair (last element before piece k, its first element)
    if (hit[k] != kSrchNone) return off + static_cast<std::size_t>(hit[k]);
    off += segs[k].size();
  }
  return kSrchNoPos;
}

// The positions in the range of the extrema of MODE ({min}, {max}, {min, last max}); kSrchNoPos for an empty range.
template <int MODE, typename Segs, typename Comp>
std::pair<std::size_t, std::size_t> search_extremum(const char *what, const Segs &segs, Comp comp) {
  using namespace dr_search;
  const std::pair<std::size_t, std::size_t> none{kSrchNoPos, kSrchNoPos};
  if (segs.empty()) return none;
  using Seg = std::remove_cvref_t<decltype(segs[0])>;
  using V = typename decltype(value_type_of_segment<Seg>())::type;
  static_assert(std::is_trivially_copyable_v<V>, "shp: the searches read elements as bits");
  static_assert(std::is_trivially_copyable_v<Comp>, "shp: callables are passed to the device by value");
  constexpr bool TWO = MODE == SRCH_MINMAX;
  const std::size_t P = segs.size();
  check_piece_sizes(what, segs);

  // per non-empty piece the kernel's state; the first one also holds the state of the fold over the winners
  enum { STATE, TOP };
  std::vector<scratch_layout<2>> lay(P);
  std::vector<std::size_t> rank(P), piece, off(P, 0);
  for (std::size_t k = 0, o = 0; k < P; k++) {
    rank[k] = segs[k].rank();
    off[k] = o;
    o += segs[k].size();
    if (!segs[k].size()) continue;
    lay[k] = {srch_ext_state_bytes<V>(kSrchGrid), piece.empty() ? srch_ext_state_bytes<V>(kSrchGrid) : 0};
    piece.push_back(k);
  }
  const std::size_t Q = piece.size();
  if (!Q) return none;
  const std::vector<char *> base = carve_scratch(rank, lay);

  pinned<unsigned long long> idx(2 * Q), top(4);
  pinned<V> val(2 * Q); // the pieces' winners in piece order: [0, Q) of end 0, [Q, 2Q) the maxima of MINMAX
  by_key_events events;
  for (std::size_t c = 0; c < Q; c++) {
    const std::size_t k = piece[c], n = segs[k].size();
    hipStream_t st = stream(rank[k]);
    srch_ext_args a{lay[k].at(base[k], STATE), &idx[2 * c], kSrchGrid};
    a.value[0] = &val[c];
    a.value[1] = &val[Q + c];
    if constexpr (srch_span_of<Seg, V>())
      hip_check((srch_extremum_span<V, MODE>(st, static_cast<const V *>(segs[k].data()), n, comp, a)), what);
    else
      hip_check((srch_extremum_accessor<V, MODE>(st, accessor_of(segs[k]), n, comp, a)), what);
    if (c && rank[k] != rank[piece[0]]) events.record(st);
  }
  top[0] = top[3] = 0;
  if (Q > 1) {
    const std::size_t k = piece[0];
    hipStream_t st = stream(rank[k]);
    events.wait_on(st);
    const srch_ext_args a{lay[k].at(base[k], TOP), &top[0], kSrchGrid};
    const srch_ext_args b{lay[k].at(base[k], TOP), &top[2], kSrchGrid};
    hip_check((srch_extremum_span<V, TWO ? SRCH_MIN : MODE>(st, static_cast<const V *>(val.data()), Q, comp, a)), what);
    if constexpr (TWO) // the last greatest of the pieces' last greatest
      hip_check((srch_extremum_span<V, SRCH_MINMAX>(st, static_cast<const V *>(val.data()) + Q, Q, comp, b)), what);
  }
  select_sync(segs); // the one wait

  const std::size_t ca = static_cast<std::size_t>(top[0]), cb = static_cast<std::size_t>(top[3]);
  return {off[piece[ca]] + static_cast<std::size_t>(idx[2 * ca]),
          TWO ? off[piece[cb]] + static_cast<std::size_t>(idx[2 * cb + 1]) : kSrchNoPos};
}

template <typename R> auto srch_iter(R &&r, std::size_t pos) {
  return pos == kSrchNoPos ? std::ranges::begin(r) + static_cast<std::ranges::range_difference_t<R>>(std::ranges::size(r))
                           : std::ranges::begin(r) + static_cast<std::ranges::range_difference_t<R>>(pos);
}
template <typename R> using srch_value_t =
    typename decltype(value_type_of_segment<std::remove_cvref_t<decltype(lib::ranges::segments(std::declval<R &>())[0])>>())::type;

} // namespace detail

// ---------------------------------------------------------------- find
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
auto find_if(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  return detail::srch_iter(r, detail::search_first<dr_search::SRCH_UNARY>("shp::find_if", segs, segs,
                                                                           detail::srch_value_pred<Pred, false>{pred}));
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
auto find_if_not(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  return detail::srch_iter(r, detail::search_first<dr_search::SRCH_UNARY>("shp::find_if_not", segs, segs,
                                                                           detail::srch_value_pred<Pred, true>{pred}));
}
template <typename ExecutionPolicy, lib::distributed_range R, typename T>
auto find(ExecutionPolicy &&policy, R &&r, const T &value) {
  using V = detail::srch_value_t<R>;
  return shp::find_if(std::forward<ExecutionPolicy>(policy), std::forward<R>(r),
                      detail::sel_equal_to<V>{static_cast<V>(value)});
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
bool any_of(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  return detail::search_first<dr_search::SRCH_UNARY>("shp::any_of", segs, segs,
                                                     detail::srch_value_pred<Pred, false>{pred}) != detail::kSrchNoPos;
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
bool none_of(ExecutionPolicy &&policy, R &&r, Pred pred) {
  return !shp::any_of(std::forward<ExecutionPolicy>(policy), std::forward<R>(r), pred);
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
bool all_of(ExecutionPolicy &&, R &&r, Pred pred) {
  auto segs = lib::ranges::segments(r);
  return detail::search_first<dr_search::SRCH_UNARY>("shp::all_of", segs, segs,
                                                     detail::srch_value_pred<Pred, true>{pred}) == detail::kSrchNoPos;
}

// ------------------------------------------------------ adjacent pairs
// the first i with pred(r[i], r[i + 1])
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred2 = detail::srch_equal_to>
auto adjacent_find(ExecutionPolicy &&, R &&r, Pred2 pred = Pred2{}) {
  auto segs = lib::ranges::segments(r);
  return detail::srch_iter(r, detail::search_first<dr_search::SRCH_ADJACENT>("shp::adjacent_find", segs, segs,
                                                                              detail::srch_pair_pred<Pred2, false>{pred}));
}
// the end of the longest prefix sorted under comp
template <typename ExecutionPolicy, lib::distributed_range R, typename Comp = detail::srch_less>
auto is_sorted_until(ExecutionPolicy &&, R &&r, Comp comp = Comp{}) {
  auto segs = lib::ranges::segments(r);
  const std::size_t pos = detail::search_first<dr_search::SRCH_ADJACENT>("shp::is_sorted_until", segs, segs,
                                                                         detail::srch_descent<Comp>{comp});
  return detail::srch_iter(r, pos == detail::kSrchNoPos ? pos : pos + 1);
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Comp = detail::srch_less>
bool is_sorted(ExecutionPolicy &&, R &&r, Comp comp = Comp{}) {
  auto segs = lib::ranges::segments(r);
  return detail::search_first<dr_search::SRCH_ADJACENT>("shp::is_sorted", segs, segs, detail::srch_descent<Comp>{comp}) ==
         detail::kSrchNoPos;
}

// -------------------------------------------------------------- extrema
template <typename ExecutionPolicy, lib::distributed_range R, typename Comp = detail::srch_less>
auto min_element(ExecutionPolicy &&, R &&r, Comp comp = Comp{}) {
  auto segs = lib::ranges::segments(r);
  return detail::srch_iter(r, detail::search_extremum<dr_search::SRCH_MIN>("shp::min_element", segs,
                                                                          detail::srch_pair_pred<Comp, false>{comp}).first);
}
template <typename ExecutionPolicy, lib::distributed_range R, typename Comp = detail::srch_less>
auto max_element(ExecutionPolicy &&, R &&r, Comp comp = Comp{}) {
  auto segs = lib::ranges::segments(r);
  return detail::srch_iter(r, detail::search_extremum<dr_search::SRCH_MAX>("shp::max_element", segs,
                                                                          detail::srch_pair_pred<Comp, false>{comp}).first);
}
// {first least, last greatest}
template <typename ExecutionPolicy, lib::distributed_range R, typename Comp = detail::srch_less>
auto minmax_element(ExecutionPolicy &&, R &&r, Comp comp = Comp{}) {
  auto segs = lib::ranges::segments(r);
  const auto p = detail::search_extremum<dr_search::SRCH_MINMAX>("shp::minmax_element", segs,
                                                                 detail::srch_pair_pred<Comp, false>{comp});
  return std::pair(detail::srch_iter(r, p.first), detail::srch_iter(r, p.second));
}

// ------------------------------------------------------ mismatch, equal
namespace detail {
template <typename R1, typename R2, typename Pred2>
std::size_t mismatch_pos(const char *what, R1 &&r1, R2 &&r2, Pred2 pred) {
  auto segs1 = lib::ranges::segments(r1);
  auto segs2 = lib::ranges::segments(r2);
  check_segmented_alike(what, segs1, segs2);
  return search_first<dr_search::SRCH_TWO>(what, segs1, segs2, srch_pair_pred<Pred2, true>{pred});
}
} // namespace detail

// {begin(r1) + k, begin(r2) + k} for the first k with !pred(r1[k], r2[k]), or both ends
template <typename ExecutionPolicy, lib::distributed_range R1, lib::distributed_range R2,
          typename Pred2 = detail::srch_equal_to>
auto mismatch(ExecutionPolicy &&, R1 &&r1, R2 &&r2, Pred2 pred = Pred2{}) {
  const std::size_t pos = detail::mismatch_pos("shp::mismatch", r1, r2, pred);
  return std::pair(detail::srch_iter(r1, pos), detail::srch_iter(r2, pos));
}
template <typename ExecutionPolicy, lib::distributed_range R1, lib::distributed_range R2,
          typename Pred2 = detail::srch_equal_to>
bool equal(ExecutionPolicy &&, R1 &&r1, R2 &&r2, Pred2 pred = Pred2{}) {
  if (std::ranges::size(r1) != std::ranges::size(r2)) return false;
  return detail::mismatch_pos("shp::equal", r1, r2, pred) == detail::kSrchNoPos;
}

// ------------------------------------------------------- iterator forms
#define DR_SHP_SEARCH_ITER_FORM(NAME)                                                                       \
  template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename... Args>                     \
  auto NAME(ExecutionPolicy &&policy, Iter first, Iter last, Args... args) {                                \
    return shp::NAME(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), args...);   \
  }
DR_SHP_SEARCH_ITER_FORM(find)
DR_SHP_SEARCH_ITER_FORM(find_if)
DR_SHP_SEARCH_ITER_FORM(find_if_not)
DR_SHP_SEARCH_ITER_FORM(any_of)
DR_SHP_SEARCH_ITER_FORM(all_of)
DR_SHP_SEARCH_ITER_FORM(none_of)
DR_SHP_SEARCH_ITER_FORM(adjacent_find)
DR_SHP_SEARCH_ITER_FORM(is_sorted_until)
DR_SHP_SEARCH_ITER_FORM(is_sorted)
DR_SHP_SEARCH_ITER_FORM(min_element)
DR_SHP_SEARCH_ITER_FORM(max_element)
DR_SHP_SEARCH_ITER_FORM(minmax_element)
#undef DR_SHP_SEARCH_ITER_FORM

template <typename ExecutionPolicy, lib::distributed_iterator Iter1, lib::distributed_iterator Iter2,
          typename Pred2 = detail::srch_equal_to>
auto mismatch(ExecutionPolicy &&policy, Iter1 first1, Iter1 last1, Iter2 first2, Iter2 last2, Pred2 pred = Pred2{}) {
  return shp::mismatch(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first1, last1),
                       std::ranges::subrange(first2, last2), pred);
}
template <typename ExecutionPolicy, lib::distributed_iterator Iter1, lib::distributed_iterator Iter2,
          typename Pred2 = detail::srch_equal_to>
bool equal(ExecutionPolicy &&policy, Iter1 first1, Iter1 last1, Iter2 first2, Iter2 last2, Pred2 pred = Pred2{}) {
  return shp::equal(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first1, last1),
                    std::ranges::subrange(first2, last2), pred);
}

} // namespace shp

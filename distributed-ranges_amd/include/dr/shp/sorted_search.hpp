// dr/shp/sorted_search.hpp -- the searches of a sorted distributed range:
// lower_bound, upper_bound, binary_search, equal_range, partition_point.
//
// Absent from the reference; they are what follows shp::sort, sort_by_key,
// reduce_by_key and unique_copy in a pipeline (rank a batch of values, join
// two key sets, bin against sorted edges, turn sorted COO rows into a CSR
// rowptr, test membership).  Each takes an execution policy first and has a
// range and an iterator form.  The haystack is partitioned with respect to
// every needle under the strict weak order comp (default: <), in practice
// sorted by it; -0.0 and +0.0 are equal under <, +-inf are ordinary values; a
// NaN or an unpartitioned haystack gives unspecified positions, still in
// [0, size(hay)].
//
// Vectorised forms (the semantics of thrust's):
//   lower_bound(policy, hay, needles, out[, comp])      out[i] = the position of
//   upper_bound(policy, hay, needles, out[, comp])      needles[i], an offset from
//   binary_search(policy, hay, needles, out[, comp])    begin(hay); or a 0 / 1 flag
//   (policy, first, last, values_first, values_last, result[, comp])
// out's value type is a 4- or 8-byte integer for positions (4 bytes with
// size(hay) >= 2^32: std::length_error) and any 1-byte type, bool included,
// for binary_search.  needles and out are segmented alike over the needles'
// length (detail::check_segmented_alike: std::invalid_argument), as keys and
// values are in the by-key family; an out shorter than needles throws
// std::out_of_range before anything is written.  The haystack may be
// segmented in any way, independent of the needles.  They return the end of
// the written output, begin(out) + size(needles).
//
// Scalar forms (the semantics of std's): lower_bound / upper_bound(policy,
// hay, value[, comp]) return an iterator of hay, binary_search a bool,
// equal_range a pair of iterators (ONE launch resolves both bounds),
// partition_point(policy, r, pred) an iterator.  The third argument selects
// the overload: a distributed range is a batch of needles, anything else a
// value (converted to the haystack's value type).
//
// Callables (comp, pred) are trivially copyable device callables, captures
// included, only ever called on the device; elements are any trivially
// copyable type, so a comparator over a {key, payload} struct works.  The
// haystack is what count_if accepts: a distributed_vector, its take / drop /
// slice subranges and a transform view over those; not a zip.
//
// Across pieces: the haystack's non-empty pieces form a table {accessor,
// first global index}, built once on the host and copied to the device
// scratch (detail::carve_scratch) of every segment that holds needles.  Every
// non-empty needle piece then launches ONE kernel (dr/details/
// bsearch_kernel.hpp, the one behind drhip_lower_bound) on its own segment's
// stream, all pieces concurrently; it searches the virtual concatenation of
// the haystack's pieces and so writes global positions straight into its out
// piece, whatever runs of equal elements span the seams; one wait.  A scalar
// form is one such launch of 1 or 2 searches, on the segment of the
// haystack's first non-empty piece, into a pinned slot; every call lists the
// pieces on the host again and takes its slot (and, with two or more pieces,
// the table's staging block) from the pinned pool, which a batch amortises
// and a loop of scalar calls does not.  Haystack pieces on
// another device are read through peer access (drhip_malloc memory is
// peer-visible, drhip.h): correct, but every probe crosses the fabric.
// A needle piece of 2^32 elements or more throws std::length_error.
#pragma once

#include <array>
#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../details/bsearch_kernel.hpp"
#include "search.hpp"
#include "select.hpp"

namespace shp {

namespace detail {

constexpr unsigned kBsGrid = kSelCountGrid; // the sorted searches' grid limit: count_if's

// The haystack of one call: its non-empty pieces and where the kernels find them.
template <typename HSegs> struct bs_haystack {
  using Seg = std::remove_cvref_t<decltype(std::declval<const HSegs &>()[0])>;
  using V = typename decltype(value_type_of_segment<Seg>())::type;
  using Acc = decltype(accessor_of(std::declval<const Seg &>()));
  using piece = dr_bsearch::bs_piece<Acc>;
  static_assert(std::is_trivially_copyable_v<V>, "shp: the sorted searches read elements as bits");
  static_assert(std::is_trivially_copyable_v<Acc>, "shp: callables are passed to the device by value");

  std::vector<piece> pieces;
  std::size_t n = 0, first_rank = 0;
  std::vector<piece *> table; // per rank: the device copy of `pieces`, or null
  std::unique_ptr<pinned<unsigned char>> staged; // the table on its way to the devices; none for one piece

  explicit bs_haystack(const HSegs &hsegs) {
    for (auto &s : hsegs) {
      if (!s.size()) continue;
      if (pieces.empty()) first_rank = s.rank();
      pieces.push_back(piece{accessor_of(s), static_cast<unsigned long long>(n)});
      n += s.size();
    }
  }
  // The table on every rank of `ranks` (the segments that will launch), behind whatever their streams hold.
  void place(const char *what, std::vector<std::size_t> ranks) {
    if (pieces.size() < 2) return; // one piece travels in the kernel arguments
    const std::size_t bytes = pieces.size() * sizeof(piece);
    staged = std::make_unique<pinned<unsigned char>>(bytes);
    std::memcpy(staged->data(), static_cast<const void *>(pieces.data()), bytes);
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    std::vector<scratch_layout<1>> lay(ranks.size(), scratch_layout<1>{bytes});
    const std::vector<char *> base = carve_scratch(ranks, lay);
    table.assign(device_list().size(), nullptr);
    for (std::size_t k = 0; k < ranks.size(); k++) {
      hip_check(hipMemcpyAsync(base[k], staged->data(), bytes, hipMemcpyHostToDevice, stream(ranks[k])), what);
      table[ranks[k]] = reinterpret_cast<piece *>(base[k]);
    }
  }
  // launch(h): h is the callable g -> hay[g] for a kernel on segment `rank`
  template <typename F> void with(std::size_t rank, F &&launch) const {
    if (pieces.size() == 1) launch(dr_bsearch::bs_one<V, Acc>{pieces[0].a});
    else
      launch(dr_bsearch::bs_table<V, Acc>{table[rank], static_cast<unsigned>(pieces.size()),
                                          dr_bsearch::bs_table_top(static_cast<unsigned>(pieces.size()))});
  }
};

// out[i] = the position (or the flag) of needles[i], piece by piece
template <int MODE, typename H, typename Nd, typename O, typename Order>
auto sorted_search(const char *what, H &&hay, Nd &&needles, O &&out, Order ord) {
  using namespace dr_bsearch;
  auto hsegs = lib::ranges::segments(hay);
  auto nsegs = lib::ranges::segments(needles);
  auto osegs = lib::ranges::segments(out);
  using NSeg = std::remove_cvref_t<decltype(nsegs[0])>;
  using OSeg = std::remove_cvref_t<decltype(osegs[0])>;
  using N = typename decltype(value_type_of_segment<NSeg>())::type;
  using Out = std::remove_cv_t<std::ranges::range_value_t<O>>;
  static_assert(std::is_trivially_copyable_v<N>, "shp: the sorted searches read elements as bits");
  static_assert(std::is_trivially_copyable_v<Order>, "shp: callables are passed to the device by value");
  if constexpr (MODE == BS_FOUND)
    static_assert(sizeof(Out) == 1, "shp::binary_search: the output's value type is 1 byte wide (bool, char, uint8_t)");
  else
    static_assert(std::is_integral_v<Out> && (sizeof(Out) == 4 || sizeof(Out) == 8),
                  "shp: positions are stored as 4- or 8-byte integers");

  const std::size_t m = static_cast<std::size_t>(std::ranges::size(needles));
  const auto end = std::ranges::begin(out) + static_cast<std::ranges::range_difference_t<O>>(m);
  if (static_cast<std::size_t>(std::ranges::size(out)) < m)
    throw std::out_of_range(std::string(what) + ": " + std::to_string(m) + " needles, the output holds " +
                            std::to_string(std::ranges::size(out)));
  // the first m elements of out, and both lists without their empty tails
  std::vector<NSeg> np(nsegs.begin(), nsegs.end());
  std::vector<OSeg> op;
  for (std::size_t k = 0, left = m; k < osegs.size(); k++) {
    const std::size_t c = std::min<std::size_t>(left, osegs[k].size());
    op.push_back(osegs[k].subspan(0, c));
    left -= c;
  }
  while (!np.empty() && !np.back().size()) np.pop_back();
  while (!op.empty() && !op.back().size()) op.pop_back();
  check_segmented_alike(what, np, op);
  check_piece_sizes(what, np);

  if (MODE == BS_POS && sizeof(Out) == 4 && static_cast<std::size_t>(std::ranges::size(hay)) >= (std::size_t(1) << 32))
    throw std::length_error(std::string(what) + ": positions in a haystack of 2^32 elements or more need an 8-byte type");
  if (!m) return end; // nothing to search: no piece list, no scratch, no launch
  bs_haystack<decltype(hsegs)> hs(hsegs);
  using V = typename bs_haystack<decltype(hsegs)>::V;
  std::vector<std::size_t> ranks;
  for (auto &s : np)
    if (s.size()) ranks.push_back(s.rank());
  hs.place(what, ranks);

  for (std::size_t k = 0; k < np.size(); k++) {
    const std::size_t mk = np[k].size(), rk = np[k].rank();
    if (!mk) continue;
    hip_check(hipSetDevice(device_list().at(rk)), "hipSetDevice");
    hipStream_t st = stream(rk);
    Out *dst = const_cast<Out *>(static_cast<const Out *>(op[k].data()));
    if (!hs.n) { // every position is 0, nothing is found
      hip_check(hipMemsetAsync(dst, 0, mk * sizeof(Out), st), what);
      continue;
    }
    hs.with(rk, [&](auto h) {
      if constexpr (srch_span_of<NSeg, N>())
        hip_check((bs_enqueue<V, MODE>(st, h, hs.n, bs_span<N>{static_cast<const N *>(np[k].data())}, mk, ord, dst, kBsGrid)),
                  what);
      else {
        auto acc = accessor_of(np[k]);
        hip_check((bs_enqueue<V, MODE>(st, h, hs.n, bs_acc<N, decltype(acc)>{acc}, mk, ord, dst, kBsGrid)), what);
      }
    });
  }
  select_sync(np); // the one wait
  return end;
}

// `count` (1 or 2) searches of one value, into a pinned slot: positions (MODE == BS_POS) or the flag
template <int MODE, typename HSegs, typename N, typename Order>
std::array<std::size_t, 2> sorted_search_value(const char *what, const HSegs &hsegs, const N &value, std::size_t count,
                                               Order ord) {
  using namespace dr_bsearch;
  static_assert(std::is_trivially_copyable_v<N>, "shp: the sorted searches read elements as bits");
  static_assert(std::is_trivially_copyable_v<Order>, "shp: callables are passed to the device by value");
  bs_haystack<HSegs> hs(hsegs);
  using V = typename bs_haystack<HSegs>::V;
  using Out = std::conditional_t<MODE == BS_FOUND, unsigned char, unsigned long long>;
  if (!hs.n) return {0, 0};
  const std::size_t rk = hs.first_rank;
  hs.place(what, {rk});
  pinned<Out> slot(2);
  slot[0] = slot[1] = 0;
  hip_check(hipSetDevice(device_list().at(rk)), "hipSetDevice");
  hs.with(rk, [&](auto h) {
    hip_check((bs_enqueue<V, MODE>(stream(rk), h, hs.n, bs_const<N>{value}, count, ord, slot.data(), kBsGrid)), what);
  });
  sync(rk);
  return {static_cast<std::size_t>(slot[0]), static_cast<std::size_t>(slot[1])};
}

template <typename R> auto bs_iter(R &&r, std::size_t pos) {
  return std::ranges::begin(r) + static_cast<std::ranges::range_difference_t<R>>(pos);
}
struct bs_nothing {}; // partition_point's needle

} // namespace detail

// ------------------------------------------------------------ vectorised
template <typename ExecutionPolicy, lib::distributed_range H, lib::distributed_range Nd, lib::distributed_contiguous_range O,
          typename Comp = dr_bsearch::bs_less>
auto lower_bound(ExecutionPolicy &&, H &&hay, Nd &&needles, O &&out, Comp comp = Comp{}) {
  return detail::sorted_search<dr_bsearch::BS_POS>("shp::lower_bound", hay, needles, out, dr_bsearch::bs_lower<Comp>{comp});
}
template <typename ExecutionPolicy, lib::distributed_range H, lib::distributed_range Nd, lib::distributed_contiguous_range O,
          typename Comp = dr_bsearch::bs_less>
auto upper_bound(ExecutionPolicy &&, H &&hay, Nd &&needles, O &&out, Comp comp = Comp{}) {
  return detail::sorted_search<dr_bsearch::BS_POS>("shp::upper_bound", hay, needles, out, dr_bsearch::bs_upper<Comp>{comp});
}
template <typename ExecutionPolicy, lib::distributed_range H, lib::distributed_range Nd, lib::distributed_contiguous_range O,
          typename Comp = dr_bsearch::bs_less>
auto binary_search(ExecutionPolicy &&, H &&hay, Nd &&needles, O &&out, Comp comp = Comp{}) {
  return detail::sorted_search<dr_bsearch::BS_FOUND>("shp::binary_search", hay, needles, out,
                                                     dr_bsearch::bs_lower<Comp>{comp});
}

// ---------------------------------------------------------------- scalar
template <typename ExecutionPolicy, lib::distributed_range H, typename T, typename Comp = dr_bsearch::bs_less>
  requires(!lib::distributed_range<T>)
auto lower_bound(ExecutionPolicy &&, H &&hay, const T &value, Comp comp = Comp{}) {
  using V = detail::srch_value_t<H>;
  return detail::bs_iter(hay, detail::sorted_search_value<dr_bsearch::BS_POS>("shp::lower_bound", lib::ranges::segments(hay),
                                                                             static_cast<V>(value), 1,
                                                                             dr_bsearch::bs_lower<Comp>{comp})[0]);
}
template <typename ExecutionPolicy, lib::distributed_range H, typename T, typename Comp = dr_bsearch::bs_less>
  requires(!lib::distributed_range<T>)
auto upper_bound(ExecutionPolicy &&, H &&hay, const T &value, Comp comp = Comp{}) {
  using V = detail::srch_value_t<H>;
  return detail::bs_iter(hay, detail::sorted_search_value<dr_bsearch::BS_POS>("shp::upper_bound", lib::ranges::segments(hay),
                                                                             static_cast<V>(value), 1,
                                                                             dr_bsearch::bs_upper<Comp>{comp})[0]);
}
template <typename ExecutionPolicy, lib::distributed_range H, typename T, typename Comp = dr_bsearch::bs_less>
  requires(!lib::distributed_range<T>)
bool binary_search(ExecutionPolicy &&, H &&hay, const T &value, Comp comp = Comp{}) {
  using V = detail::srch_value_t<H>;
  return detail::sorted_search_value<dr_bsearch::BS_FOUND>("shp::binary_search", lib::ranges::segments(hay),
                                                           static_cast<V>(value), 1, dr_bsearch::bs_lower<Comp>{comp})[0] != 0;
}
// {lower_bound, upper_bound} of value, both from one launch
template <typename ExecutionPolicy, lib::distributed_range H, typename T, typename Comp = dr_bsearch::bs_less>
  requires(!lib::distributed_range<T>)
auto equal_range(ExecutionPolicy &&, H &&hay, const T &value, Comp comp = Comp{}) {
  using V = detail::srch_value_t<H>;
  const auto p = detail::sorted_search_value<dr_bsearch::BS_POS>("shp::equal_range", lib::ranges::segments(hay),
                                                                 static_cast<V>(value), 2,
                                                                 dr_bsearch::bs_equal_range<Comp>{comp});
  return std::pair(detail::bs_iter(hay, p[0]), detail::bs_iter(hay, p[1]));
}
// the first element with !pred, in a range whose elements with pred come first
template <typename ExecutionPolicy, lib::distributed_range R, typename Pred>
auto partition_point(ExecutionPolicy &&, R &&r, Pred pred) {
  return detail::bs_iter(r, detail::sorted_search_value<dr_bsearch::BS_POS>("shp::partition_point", lib::ranges::segments(r),
                                                                           detail::bs_nothing{}, 1,
                                                                           dr_bsearch::bs_partition<Pred>{pred})[0]);
}

// -------------------------------------------------------- iterator forms
#define DR_SHP_SORTED_SEARCH_ITER_FORMS(NAME)                                                                          \
  template <typename ExecutionPolicy, lib::distributed_iterator Iter, lib::distributed_iterator VIter,                 \
            lib::distributed_iterator OIter, typename... Comp>                                                         \
    requires(sizeof...(Comp) <= 1)                                                                                     \
  auto NAME(ExecutionPolicy &&policy, Iter first, Iter last, VIter values_first, VIter values_last, OIter result,      \
            Comp... comp) {                                                                                            \
    const std::size_t m = static_cast<std::size_t>(values_last - values_first);                                        \
    auto out = detail::out_from(result, m);                                                                            \
    shp::NAME(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last),                               \
              std::ranges::subrange(values_first, values_last), out, comp...);                                         \
    return result + static_cast<std::ptrdiff_t>(m);                                                                    \
  }                                                                                                                    \
  template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename T, typename... Comp>                    \
    requires(sizeof...(Comp) <= 1 && !lib::distributed_iterator<T> && !lib::distributed_range<T>)                      \
  auto NAME(ExecutionPolicy &&policy, Iter first, Iter last, const T &value, Comp... comp) {                           \
    return shp::NAME(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), value, comp...);       \
  }
DR_SHP_SORTED_SEARCH_ITER_FORMS(lower_bound)
DR_SHP_SORTED_SEARCH_ITER_FORMS(upper_bound)
DR_SHP_SORTED_SEARCH_ITER_FORMS(binary_search)
#undef DR_SHP_SORTED_SEARCH_ITER_FORMS

template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename T, typename... Comp>
  requires(sizeof...(Comp) <= 1 && !lib::distributed_iterator<T>)
auto equal_range(ExecutionPolicy &&policy, Iter first, Iter last, const T &value, Comp... comp) {
  return shp::equal_range(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), value, comp...);
}
template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename Pred>
auto partition_point(ExecutionPolicy &&policy, Iter first, Iter last, Pred pred) {
  return shp::partition_point(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), pred);
}

} // namespace shp

// dr/shp/merge.hpp -- the stable merge of two sorted distributed ranges:
// merge and merge_by_key.
//
// Absent from the reference; they are what joins two results of shp::sort /
// sort_by_key (merge a sorted batch into a sorted range, join two key sets)
// without sorting the concatenation again.  Each takes an execution policy
// first and has a range and an iterator form:
//   merge(policy, a, b, out[, comp])              returns begin(out) + size(a) + size(b)
//   merge(policy, first1, last1, first2, last2, result[, comp])
//   merge_by_key(policy, keys_a, vals_a, keys_b, vals_b, keys_out, vals_out[, comp])
//                                                 returns the pair of ends
//   merge_by_key(policy, keys_first1, keys_last1, keys_first2, keys_last2,
//                vals_first1, vals_first2, keys_result, vals_result[, comp])
// The result is std::merge's: both inputs sorted under the strict weak order
// comp (default: <), on ties a's element first, each input in its own order.
// -0.0 and +0.0 are a tie under <, +-inf are ordinary values; NaNs or unsorted
// inputs give unspecified output values (and nothing worse).
//
// a and b are what count_if accepts: a distributed_vector, its take / drop /
// slice subranges and a transform view over those; not a zip.  Each may be
// segmented in any way, independently of the other and of out.  out is a
// distributed_contiguous_range of the same value type with size(out) >=
// size(a) + size(b) (shorter: std::out_of_range before anything is written);
// what lies beyond the merge in out is left alone.  In merge_by_key vals_x is
// segmented like keys_x and vals_out like keys_out over the merge's length
// (detail::check_segmented_alike: std::invalid_argument).  Elements and values
// are any trivially copyable type (at most 4 KiB), so a comparator over a
// {key, payload} struct works; comp is a trivially copyable device callable,
// captures included, only ever called on the device.  An output piece of 2^32
// elements or more throws std::length_error; an output piece that overlaps an
// input piece in memory throws std::invalid_argument.
//
// Across pieces: nothing is split on the host and nothing is stitched.  The
// non-empty pieces of a and of b (and of their values) each form a table
// {accessor, first global index}, as the sorted searches' haystack does; with
// one piece each the accessors travel in the kernel arguments, otherwise the
// tables are copied to the device scratch (detail::carve_scratch) of every
// segment that holds a piece of out.  Every non-empty output piece covering
// the output positions [g0, g1) then launches ONE kernel (dr/details/
// merge_kernel.hpp, the one behind drhip_merge) on its own segment's stream
// with the diagonal window [g0, g1): its workgroups find their splits on the
// merge path over the virtual concatenations, so runs of equal elements across
// any seam of a, b or out need nothing special.  All pieces run concurrently;
// one wait.  Input pieces on another device are read through peer access
// (drhip_malloc memory is peer-visible, drhip.h): correct, but every element
// crosses the fabric.
#pragma once

#include <cstdint>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../details/merge_kernel.hpp"
#include "sorted_search.hpp"

namespace shp {

namespace detail {

constexpr unsigned kMgGrid = 2048; // the merge's grid limit: 8 workgroups per CU of a 256-CU device

struct mg_absent {}; // merge without values

// the memory behind a piece (a transform view's: its base's): {first byte, bytes}
template <typename S> std::pair<std::uintptr_t, std::size_t> mg_extent(const S &s) {
  if constexpr (requires { s.data(); })
    return {reinterpret_cast<std::uintptr_t>(s.data()), s.size() * sizeof(*s.data())};
  else if constexpr (requires { s.base; }) return mg_extent(s.base);
  else return {0, 0};
}

// One input of a call: its non-empty pieces (the sorted searches' piece type) and the memory behind them.
template <typename Segs> struct mg_input {
  using Seg = std::remove_cvref_t<decltype(std::declval<const Segs &>()[0])>;
  using V = typename decltype(value_type_of_segment<Seg>())::type;
  using Acc = decltype(accessor_of(std::declval<const Seg &>()));
  using piece = dr_bsearch::bs_piece<Acc>;
  static_assert(std::is_trivially_copyable_v<V>, "shp::merge moves elements as bits");
  static_assert(std::is_trivially_copyable_v<Acc>, "shp: callables are passed to the device by value");

  std::vector<piece> pieces;
  std::vector<std::pair<std::uintptr_t, std::size_t>> extents;
  std::size_t n = 0;

  explicit mg_input(const Segs &segs) {
    for (auto &s : segs) {
      if (!s.size()) continue;
      pieces.push_back(piece{accessor_of(s), static_cast<unsigned long long>(n)});
      extents.push_back(mg_extent(s));
      n += s.size();
    }
  }
  std::size_t table_bytes() const { return pieces.size() * sizeof(piece); }
  auto one() const { return dr_bsearch::bs_one<V, Acc>{pieces[0].a}; }
  auto table(const char *dev) const {
    return dr_bsearch::bs_table<V, Acc>{reinterpret_cast<const piece *>(dev), static_cast<unsigned>(pieces.size()),
                                        dr_bsearch::bs_table_top(static_cast<unsigned>(pieces.size()))};
  }
};
struct mg_no_input { // the values of a merge without values
  using V = dr_merge::mg_none;
  std::vector<int> pieces;
  std::vector<std::pair<std::uintptr_t, std::size_t>> extents;
  std::size_t table_bytes() const { return 0; }
  auto one() const { return dr_merge::mg_no_values{}; }
  auto table(const char *) const { return dr_merge::mg_no_values{}; }
};
template <typename R> auto mg_input_of(R &r) {
  if constexpr (std::is_same_v<std::remove_cvref_t<R>, mg_absent>) return mg_no_input{};
  else {
    auto segs = lib::ranges::segments(r);
    return mg_input<decltype(segs)>(segs);
  }
}

// the pieces of the first n elements of out, without their empty tail
template <typename O> auto mg_out_pieces(O &out, std::size_t n) {
  auto osegs = lib::ranges::segments(out);
  using OSeg = std::remove_cvref_t<decltype(osegs[0])>;
  std::vector<OSeg> op;
  for (std::size_t k = 0, left = n; k < osegs.size(); k++) {
    const std::size_t c = std::min<std::size_t>(left, osegs[k].size());
    op.push_back(osegs[k].subspan(0, c));
    left -= c;
  }
  while (!op.empty() && !op.back().size()) op.pop_back();
  return op;
}

template <typename Ext> void mg_check_overlap(const char *what, std::pair<std::uintptr_t, std::size_t> o, const Ext &in) {
  for (auto &e : in)
    if (o.second && e.second && o.first < e.first + e.second && e.first < o.first + o.second)
      throw std::invalid_argument(std::string(what) + ": an output piece overlaps an input piece");
}

// va, vb, vo: ranges, or all three mg_absent
template <typename KA, typename VA, typename KB, typename VB, typename KO, typename VO, typename Comp>
void merge_impl(const char *what, KA &ka, VA &va, KB &kb, VB &vb, KO &ko, VO &vo, Comp comp) {
  using namespace dr_merge;
  constexpr bool VALS = !std::is_same_v<std::remove_cvref_t<VA>, mg_absent>;
  static_assert(std::is_trivially_copyable_v<Comp>, "shp: callables are passed to the device by value");
  const std::size_t n = static_cast<std::size_t>(std::ranges::size(ka)) + static_cast<std::size_t>(std::ranges::size(kb));
  if (static_cast<std::size_t>(std::ranges::size(ko)) < n)
    throw std::out_of_range(std::string(what) + ": " + std::to_string(n) + " elements, the output holds " +
                            std::to_string(std::ranges::size(ko)));
  auto A = mg_input_of(ka);
  auto B = mg_input_of(kb);
  auto VAl = mg_input_of(va);
  auto VBl = mg_input_of(vb);
  using T = typename decltype(A)::V;
  using V = typename decltype(VAl)::V;
  using Out = std::remove_cv_t<std::ranges::range_value_t<KO>>;
  static_assert(std::is_same_v<T, typename decltype(B)::V> && std::is_same_v<T, Out>,
                "shp::merge: both inputs and the output have one value type");
  auto op = mg_out_pieces(ko, n);
  check_piece_sizes(what, op);
  std::vector<Out *> kdst;
  for (auto &s : op) kdst.push_back(const_cast<Out *>(static_cast<const Out *>(s.data())));
  std::vector<V *> vdst(op.size(), nullptr);
  if constexpr (VALS) {
    static_assert(std::is_same_v<V, typename decltype(VBl)::V> && std::is_same_v<V, std::remove_cv_t<std::ranges::range_value_t<VO>>>,
                  "shp::merge_by_key: both inputs' values and the output's have one value type");
    if (static_cast<std::size_t>(std::ranges::size(vo)) < n)
      throw std::out_of_range(std::string(what) + ": " + std::to_string(n) + " elements, the values' output holds " +
                              std::to_string(std::ranges::size(vo)));
    check_segmented_alike(what, lib::ranges::segments(ka), lib::ranges::segments(va));
    check_segmented_alike(what, lib::ranges::segments(kb), lib::ranges::segments(vb));
    auto vop = mg_out_pieces(vo, n);
    check_segmented_alike(what, op, vop);
    for (std::size_t k = 0; k < vop.size(); k++) {
      vdst[k] = const_cast<V *>(static_cast<const V *>(vop[k].data()));
      const auto e = mg_extent(vop[k]);
      for (auto *in : {&A.extents, &B.extents, &VAl.extents, &VBl.extents}) mg_check_overlap(what, e, *in);
      for (auto &s : op) mg_check_overlap(what, e, std::vector{mg_extent(s)});
    }
  }
  for (auto &s : op)
    for (auto *in : {&A.extents, &B.extents, &VAl.extents, &VBl.extents}) mg_check_overlap(what, mg_extent(s), *in);
  if (!n) return; // nothing to merge: no piece list on a device, no launch

  // one piece each: the accessors travel in the kernel arguments; otherwise four tables on every launching rank
  const bool direct = A.pieces.size() == 1 && B.pieces.size() == 1 && (!VALS || (VAl.pieces.size() == 1 && VBl.pieces.size() == 1));
  const scratch_layout<4> lay{A.table_bytes(), B.table_bytes(), VAl.table_bytes(), VBl.table_bytes()};
  std::vector<std::size_t> ranks;
  std::vector<char *> base;
  std::unique_ptr<pinned<unsigned char>> staged; // the tables on their way to the devices
  if (!direct) {
    for (auto &s : op)
      if (s.size()) ranks.push_back(s.rank());
    std::sort(ranks.begin(), ranks.end());
    ranks.erase(std::unique(ranks.begin(), ranks.end()), ranks.end());
    staged = std::make_unique<pinned<unsigned char>>(lay.bytes);
    std::memset(staged->data(), 0, lay.bytes);
    auto put = [&](std::size_t field, const auto &in) {
      if (in.table_bytes()) std::memcpy(lay.at(reinterpret_cast<char *>(staged->data()), field), static_cast<const void *>(in.pieces.data()), in.table_bytes());
    };
    put(0, A), put(1, B), put(2, VAl), put(3, VBl);
    base = carve_scratch(ranks, std::vector<scratch_layout<4>>(ranks.size(), lay));
    for (std::size_t k = 0; k < ranks.size(); k++)
      hip_check(hipMemcpyAsync(base[k], staged->data(), lay.bytes, hipMemcpyHostToDevice, stream(ranks[k])), what);
  }

  std::size_t g0 = 0;
  for (std::size_t k = 0; k < op.size(); k++) {
    const std::size_t g1 = g0 + op[k].size(), rk = op[k].rank();
    if (g1 > g0) {
      hip_check(hipSetDevice(device_list().at(rk)), "hipSetDevice");
      hipStream_t st = stream(rk);
      if (direct) {
        hip_check((mg_enqueue<T, V>(st, A.one(), A.n, B.one(), B.n, VAl.one(), VBl.one(), g0, g1, kdst[k], vdst[k], comp, kMgGrid)),
                  what);
      } else {
        char *b = base[static_cast<std::size_t>(std::lower_bound(ranks.begin(), ranks.end(), rk) - ranks.begin())];
        hip_check((mg_enqueue<T, V>(st, A.table(lay.at(b, 0)), A.n, B.table(lay.at(b, 1)), B.n, VAl.table(lay.at(b, 2)),
                                    VBl.table(lay.at(b, 3)), g0, g1, kdst[k], vdst[k], comp, kMgGrid)),
                  what);
      }
    }
    g0 = g1;
  }
  select_sync(op); // the one wait
}

} // namespace detail

template <typename ExecutionPolicy, lib::distributed_range A, lib::distributed_range B, lib::distributed_contiguous_range O,
          typename Comp = dr_merge::mg_less>
auto merge(ExecutionPolicy &&, A &&a, B &&b, O &&out, Comp comp = Comp{}) {
  detail::mg_absent none;
  const std::size_t n = static_cast<std::size_t>(std::ranges::size(a)) + static_cast<std::size_t>(std::ranges::size(b));
  detail::merge_impl("shp::merge", a, none, b, none, out, none, comp);
  return std::ranges::begin(out) + static_cast<std::ranges::range_difference_t<O>>(n);
}

template <typename ExecutionPolicy, lib::distributed_range KA, lib::distributed_range VA, lib::distributed_range KB,
          lib::distributed_range VB, lib::distributed_contiguous_range KO, lib::distributed_contiguous_range VO,
          typename Comp = dr_merge::mg_less>
auto merge_by_key(ExecutionPolicy &&, KA &&keys_a, VA &&vals_a, KB &&keys_b, VB &&vals_b, KO &&keys_out, VO &&vals_out,
                  Comp comp = Comp{}) {
  const std::size_t n =
      static_cast<std::size_t>(std::ranges::size(keys_a)) + static_cast<std::size_t>(std::ranges::size(keys_b));
  detail::merge_impl("shp::merge_by_key", keys_a, vals_a, keys_b, vals_b, keys_out, vals_out, comp);
  return std::pair(std::ranges::begin(keys_out) + static_cast<std::ranges::range_difference_t<KO>>(n),
                   std::ranges::begin(vals_out) + static_cast<std::ranges::range_difference_t<VO>>(n));
}

// -------------------------------------------------------- iterator forms
template <typename ExecutionPolicy, lib::distributed_iterator I1, lib::distributed_iterator I2, lib::distributed_iterator OIter,
          typename... Comp>
  requires(sizeof...(Comp) <= 1)
auto merge(ExecutionPolicy &&policy, I1 first1, I1 last1, I2 first2, I2 last2, OIter result, Comp... comp) {
  const std::size_t n = static_cast<std::size_t>(last1 - first1) + static_cast<std::size_t>(last2 - first2);
  auto out = detail::out_from(result, n);
  shp::merge(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first1, last1), std::ranges::subrange(first2, last2),
             out, comp...);
  return result + static_cast<std::ptrdiff_t>(n);
}
template <typename ExecutionPolicy, lib::distributed_iterator K1, lib::distributed_iterator K2, lib::distributed_iterator V1,
          lib::distributed_iterator V2, lib::distributed_iterator KOIter, lib::distributed_iterator VOIter, typename... Comp>
  requires(sizeof...(Comp) <= 1)
auto merge_by_key(ExecutionPolicy &&policy, K1 keys_first1, K1 keys_last1, K2 keys_first2, K2 keys_last2, V1 vals_first1,
                  V2 vals_first2, KOIter keys_result, VOIter vals_result, Comp... comp) {
  const std::ptrdiff_t na = keys_last1 - keys_first1, nb = keys_last2 - keys_first2;
  const std::size_t n = static_cast<std::size_t>(na + nb);
  auto kout = detail::out_from(keys_result, n);
  auto vout = detail::out_from(vals_result, n);
  shp::merge_by_key(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(keys_first1, keys_last1),
                    std::ranges::subrange(vals_first1, vals_first1 + na), std::ranges::subrange(keys_first2, keys_last2),
                    std::ranges::subrange(vals_first2, vals_first2 + nb), kout, vout, comp...);
  return std::pair(keys_result + static_cast<std::ptrdiff_t>(n), vals_result + static_cast<std::ptrdiff_t>(n));
}

} // namespace shp

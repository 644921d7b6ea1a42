// dr/shp/scan_by_key.hpp -- shp::inclusive_scan_by_key and
// shp::exclusive_scan_by_key: every element of a distributed range receives
// the running fold of its own run of consecutive equal keys,
//   inclusive: out[i] = v[s] op ... op v[i]
//   exclusive: out[i] = init op v[s] op ... op v[i-1]   (out[s] = init)
// for the run that starts at s, across segment boundaries wherever those fall.
//
// Absent from the reference; defined with the semantics of
// thrust::inclusive_scan_by_key / thrust::exclusive_scan_by_key over the whole
// range.  The member of the sort_by_key / copy_if / reduce_by_key family that
// keeps every element: per-group running totals, the rank of an element inside
// its group (exclusive scan of ones), the offset of a COO entry inside its row.
//
// Keys and values are any trivially copyable 4- or 8-byte types; `key_equal`
// and `op` are any trivially copyable device callables (captures included;
// op must be associative, it need not commute, and no identity is assumed).
// The kernel template (dr/details/segscan_kernel.hpp, the one the C-ABI's
// drhip_inclusive_scan_by_key is built from) is instantiated here, in the
// user's translation unit.  Inputs are what reduce_by_key takes: a
// distributed_vector, its take / drop / slice subranges (16-byte loads when
// both spans of a piece are 16-byte aligned, element loads otherwise) and a
// transform view.  Keys and values must be segmented alike
// (std::invalid_argument otherwise).  `out` has the values' type and at least
// as many elements (std::out_of_range otherwise, before anything is written);
// it may be `values` itself (in place), not a shifted view of it.  Float
// values under std::plus / std::multiplies fold in double inside a piece.
//
//   1. every non-empty piece is scanned on its own segment stream, all pieces
//      concurrently.  Where the piece's stretch of `out` lies in one segment of
//      the piece's own rank it is written directly, with no extra pass;
//      otherwise the piece goes through its slice of the segment's device
//      scratch (detail::carve_scratch) and is copied out at the end, split at
//      the output's segment boundaries (detail::out_cursor, select.hpp);
//   2. a one-thread kernel behind it leaves the piece's edge record in pinned
//      memory: first and last key, the index of the piece's first break (its
//      size when the piece is one run) and the ACC fold of its last run, as
//      the kernel left them in the state's head;
//   3. one stitch kernel walks the P records behind event waits on the pieces'
//      streams.  Where the first key of a piece equals the last key of the
//      piece before it, the piece receives the fold that is open there as its
//      carry (in ACC); a piece without a break hands the carry on, folded with
//      its own, so a run may swallow whole pieces;
//   4. one wait for the records.  A piece with a carry gets it folded into the
//      elements before its first break.  Inclusive: out[i] = op(carry, out[i])
//      by a small kernel.  Exclusive: init cannot be taken out of a stored
//      op(init, x), so those elements are scanned again from the input with
//      op(init, carry) in place of init (formed by the stitch kernel; the
//      piece's first element receives exactly that); an in-place call keeps a
//      copy of such a piece's values for it.  Each element has one writer at a
//      time, in stream order, and the input order is kept;
//   5. copies of the pieces that went through scratch; sync.
// Everything carried between tiles and between segments is ACC.  An element
// that received a carry in the inclusive form has been rounded to the value
// type twice (once in its piece, once after the carry), so with float values
// whose folds are inexact the result can differ in the last place from a
// one-segment run; wherever every partial is representable the result does
// not depend on the segmentation.  A piece of 2^32 elements or more throws
// std::length_error; an empty piece launches nothing.
#pragma once

#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../details/segscan_kernel.hpp"
#include "reduce_by_key.hpp"

namespace shp {

namespace detail {

// a piece's edge record, in pinned memory (A = the kernel's ACC)
template <typename K, typename A> struct sbk_edge {
  unsigned long long n;           // the piece's size (host); 0: an empty piece
  unsigned long long first_break; // the smallest i > 0 with !eq(k[i-1], k[i]), or n
  K first_key, last_key;
  A last_acc; // the inclusive fold of the piece's last run inside the piece
  A carry;    // has_carry: the fold of the piece's first run's elements in earlier pieces
  A xinit;    // has_carry, exclusive: op(init, carry)
  unsigned has_carry;
};

template <typename K, typename A, typename KAcc>
__global__ void sbk_edge_kernel(KAcc kin, std::size_t n, const char *state, sbk_edge<K, A> *e) {
  e->first_key = static_cast<K>(kin(0));
  e->last_key = static_cast<K>(kin(n - 1));
  e->first_break = dr_segscan::ss_first_break(state, n);
  e->last_acc = *reinterpret_cast<const A *>(state + dr_segscan::kSsLastAcc);
}

// One thread walks the P records; `open` is the fold of the run that is open
// at the end of piece `prev`.
template <bool EXCL, typename K, typename A, typename Eq, typename Op>
__global__ void sbk_stitch_kernel(sbk_edge<K, A> *e, std::size_t P, A init, Eq eq, Op op) {
  long prev = -1;
  A open{};
  for (std::size_t k = 0; k < P; k++) {
    e[k].has_carry = 0;
    if (!e[k].n) continue;
    const bool j = prev >= 0 && eq(e[prev].last_key, e[k].first_key);
    if (j) {
      e[k].carry = open;
      if constexpr (EXCL) e[k].xinit = op(init, open);
      e[k].has_carry = 1;
    }
    open = (j && e[k].first_break == e[k].n) ? op(open, e[k].last_acc) : e[k].last_acc;
    prev = (long)k;
  }
}

// inclusive: the carry into the m elements before the piece's first break
template <typename V, typename A, typename Op> __global__ void sbk_carry_kernel(V *out, std::size_t m, A carry, Op op) {
  const std::size_t i = (std::size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m) out[i] = static_cast<V>(op(carry, static_cast<A>(out[i])));
}

template <bool EXCL, typename KR, typename VR, typename OR, typename T, typename Eq, typename Op>
void scan_by_key(const char *what, KR &&keys, VR &&values, OR &&out, T init_, Eq eq_, Op op_) {
  using namespace dr_segscan;
  auto ksegs = lib::ranges::segments(keys);
  auto vsegs = lib::ranges::segments(values);
  auto osegs = lib::ranges::segments(out);
  using KSeg = std::remove_cvref_t<decltype(ksegs[0])>;
  using VSeg = std::remove_cvref_t<decltype(vsegs[0])>;
  using K = typename decltype(value_type_of_segment<KSeg>())::type;
  using V = typename decltype(value_type_of_segment<VSeg>())::type;
  using A = by_key_acc_t<V, Op>;
  static_assert(sr_elem_type<K>, "shp: by-key algorithms take trivially copyable keys of 4 or 8 bytes");
  static_assert(sr_elem_type<V>, "shp: by-key algorithms take trivially copyable values of 4 or 8 bytes");
  static_assert(std::is_same_v<std::remove_cv_t<std::ranges::range_value_t<OR>>, V>,
                "shp: the output's value type must be the value input's");
  static_assert(std::is_trivially_copyable_v<Eq> && std::is_trivially_copyable_v<Op>,
                "shp: key_equal and op are passed to the device by value");
  const by_key_eq<Eq> eq{eq_};
  const by_key_op<A, Op> op{op_};
  const A init = static_cast<A>(static_cast<V>(init_));

  const std::size_t P = ksegs.size();
  const std::size_t total = static_cast<std::size_t>(std::ranges::size(keys));
  if (total != static_cast<std::size_t>(std::ranges::size(values)))
    throw std::invalid_argument(std::string(what) + ": keys and values differ in size");
  check_segmented_alike(what, ksegs, vsegs);
  check_piece_sizes(what, ksegs);
  if (total > static_cast<std::size_t>(std::ranges::size(out)))
    throw std::out_of_range(std::string(what) + ": " + std::to_string(total) + " elements, the output holds " +
                            std::to_string(std::ranges::size(out)));

  // per piece: where it is written (its stretch of `out`, or scratch), and its share of the segment's scratch:
  // [values of the piece, when it is not written directly | a copy of its input values, in-place exclusive | state]
  using Cursor = out_cursor<decltype(osegs)>;
  struct piece {
    V *dst = nullptr; // direct
    Cursor at;        // where its stretch of `out` starts
    bool save = false;
  };
  enum { TV, SV, STATE };
  std::vector<piece> pc(P);
  std::vector<scratch_layout<3>> lay(P);
  std::vector<std::size_t> rank(P);
  {
    Cursor cur{&osegs};
    long first = -1;
    for (std::size_t k = 0; k < P; k++) {
      const std::size_t n = ksegs[k].size();
      rank[k] = ksegs[k].rank();
      if (!n) continue;
      if (cur.room() >= n && cur.segment().rank() == rank[k]) pc[k].dst = static_cast<V *>(cur.next());
      pc[k].at = cur;
      cur.advance(n);
      if constexpr (EXCL && by_key_span_of<VSeg, V>())
        pc[k].save = first >= 0 && pc[k].dst == static_cast<const V *>(vsegs[k].data());
      lay[k] = {pc[k].dst ? 0 : n * sizeof(V), pc[k].save ? n * sizeof(V) : 0, ss_state_bytes_max<K, V>(n)};
      if (first < 0) first = (long)k;
    }
  }
  const std::vector<char *> base = carve_scratch(rank, lay);
  // where piece k is scanned into: its stretch of `out`, or scratch
  auto where = [&](std::size_t k) { return pc[k].dst ? pc[k].dst : lay[k].template at<V>(base[k], TV); };

  pinned<unsigned> err(1);
  err[0] = 0;
  // the scan of the first m elements of piece k into o, on the piece's stream
  auto launch = [&](std::size_t k, std::size_t m, V *o, A in, bool saved) {
    const std::size_t rk = ksegs[k].rank();
    hipStream_t st = stream(rk);
    const ss_args a{lay[k].at(base[k], STATE), err.data()};
    auto go = [&](auto vin, auto vin_is_span) {
      if constexpr (by_key_span_of<KSeg, K>()) {
        const K *kp = static_cast<const K *>(ksegs[k].data());
        if constexpr (decltype(vin_is_span)::value)
          hip_check((ss_launch_spans<K, V, A, EXCL>(st, kp, vin, m, o, in, eq, op, a)), what);
        else
          hip_check((ss_launch_keys_span<K, V, A, EXCL>(st, kp, vin, m, o, in, eq, op, a)), what);
      } else {
        if constexpr (decltype(vin_is_span)::value)
          hip_check((ss_launch<K, V, A, false, EXCL>(st, accessor_of(ksegs[k]), sr_ptr_accessor<V>{vin}, m, o, in, eq, op, a)), what);
        else
          hip_check((ss_launch<K, V, A, false, EXCL>(st, accessor_of(ksegs[k]), vin, m, o, in, eq, op, a)), what);
      }
    };
    if (saved) go(lay[k].template at<const V>(base[k], SV), std::true_type{});
    else if constexpr (by_key_span_of<VSeg, V>()) go(static_cast<const V *>(vsegs[k].data()), std::true_type{});
    else go(accessor_of(vsegs[k]), std::false_type{});
  };

  using Edge = sbk_edge<K, A>;
  pinned<Edge> edge(P);
  by_key_events events;
  long first = -1;
  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = ksegs[k].size();
    edge[k].n = n;
    edge[k].has_carry = 0;
    if (!n) continue;
    const std::size_t rk = ksegs[k].rank();
    hipStream_t st = stream(rk);
    if constexpr (by_key_span_of<VSeg, V>()) {
      if (pc[k].save)
        hip_check(hipMemcpyAsync(lay[k].at(base[k], SV), static_cast<const V *>(vsegs[k].data()), n * sizeof(V),
                                 hipMemcpyDeviceToDevice, st),
                  "scan_by_key copy");
    }
    launch(k, n, where(k), init, false);
    auto kacc = accessor_of(ksegs[k]);
    hipLaunchKernelGGL((sbk_edge_kernel<K, A, decltype(kacc)>), dim3(1), dim3(1), 0, st, kacc, n,
                       static_cast<const char *>(lay[k].at(base[k], STATE)), &edge[k]);
    hip_check(hipGetLastError(), "scan_by_key edge launch");
    if (first < 0) first = (long)k;
    else if (rk != ksegs[first].rank()) events.record(st);
  }
  if (first < 0) return;
  {
    const std::size_t rk = ksegs[first].rank();
    events.wait_on(stream(rk));
    hipLaunchKernelGGL((sbk_stitch_kernel<EXCL, K, A, by_key_eq<Eq>, by_key_op<A, Op>>), dim3(1), dim3(1), 0, stream(rk), edge.data(),
                       P, init, eq, op);
    hip_check(hipGetLastError(), "scan_by_key stitch launch");
    sync(rk); // the one wait: the stitch ran behind every piece
  }
  select_check(err[0]);

  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = ksegs[k].size();
    if (!n) continue;
    const std::size_t rk = ksegs[k].rank();
    V *o = where(k);
    if (edge[k].has_carry) {
      const std::size_t m = static_cast<std::size_t>(edge[k].first_break);
      if constexpr (EXCL) {
        launch(k, m, o, edge[k].xinit, pc[k].save);
      } else {
        hipLaunchKernelGGL((sbk_carry_kernel<V, A, by_key_op<A, Op>>), dim3((unsigned)((m + 255) / 256)), dim3(256), 0, stream(rk), o, m,
                           edge[k].carry, op);
        hip_check(hipGetLastError(), "scan_by_key carry launch");
      }
    }
    if (!pc[k].dst) pc[k].at.emit(rk, static_cast<const V *>(o), n);
  }
  select_sync(ksegs);
  select_check(err[0]);
}

} // namespace detail

// out[i] = the fold of the values of i's run up to and including i
template <typename ExecutionPolicy, lib::distributed_range KR, lib::distributed_range VR, lib::distributed_contiguous_range OR,
          typename KeyEqual = std::equal_to<>, typename Op = std::plus<>>
void inclusive_scan_by_key(ExecutionPolicy &&, KR &&keys, VR &&values, OR &&out, KeyEqual key_equal = KeyEqual{}, Op op = Op{}) {
  using V = std::remove_cv_t<std::ranges::range_value_t<OR>>;
  detail::scan_by_key<false>("shp::inclusive_scan_by_key", keys, values, out, V{}, key_equal, op);
}

// out[i] = init op the values of i's run before i; the first element of a run gets init
template <typename ExecutionPolicy, lib::distributed_range KR, lib::distributed_range VR, lib::distributed_contiguous_range OR,
          typename T, typename KeyEqual = std::equal_to<>, typename Op = std::plus<>>
void exclusive_scan_by_key(ExecutionPolicy &&, KR &&keys, VR &&values, OR &&out, T init, KeyEqual key_equal = KeyEqual{},
                           Op op = Op{}) {
  detail::scan_by_key<true>("shp::exclusive_scan_by_key", keys, values, out, init, key_equal, op);
}

// iterator forms: the output starts at d_first; returns d_first + (klast - kfirst)
template <typename ExecutionPolicy, lib::distributed_iterator KIter, lib::distributed_iterator VIter,
          lib::distributed_iterator OutputIter, typename KeyEqual = std::equal_to<>, typename Op = std::plus<>>
OutputIter inclusive_scan_by_key(ExecutionPolicy &&policy, KIter kfirst, KIter klast, VIter vfirst, OutputIter d_first,
                                 KeyEqual key_equal = KeyEqual{}, Op op = Op{}) {
  const std::size_t n = static_cast<std::size_t>(klast - kfirst);
  shp::inclusive_scan_by_key(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(kfirst, klast),
                             std::ranges::subrange(vfirst, vfirst + static_cast<std::ptrdiff_t>(n)),
                             detail::out_from(d_first, n), key_equal, op);
  return d_first + static_cast<std::ptrdiff_t>(n);
}
template <typename ExecutionPolicy, lib::distributed_iterator KIter, lib::distributed_iterator VIter,
          lib::distributed_iterator OutputIter, typename T, typename KeyEqual = std::equal_to<>, typename Op = std::plus<>>
OutputIter exclusive_scan_by_key(ExecutionPolicy &&policy, KIter kfirst, KIter klast, VIter vfirst, OutputIter d_first, T init,
                                 KeyEqual key_equal = KeyEqual{}, Op op = Op{}) {
  const std::size_t n = static_cast<std::size_t>(klast - kfirst);
  shp::exclusive_scan_by_key(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(kfirst, klast),
                             std::ranges::subrange(vfirst, vfirst + static_cast<std::ptrdiff_t>(n)),
                             detail::out_from(d_first, n), init, key_equal, op);
  return d_first + static_cast<std::ptrdiff_t>(n);
}

} // namespace shp

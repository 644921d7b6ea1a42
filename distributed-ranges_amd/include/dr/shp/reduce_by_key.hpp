// dr/shp/reduce_by_key.hpp -- shp::reduce_by_key, shp::run_length_encode and
// shp::unique_copy: every run of consecutive equal keys of a distributed range
// becomes one key (the run's first) and one value (the fold of the run's
// values in input order; its length; nothing).
//
// Absent from the reference; defined with the semantics of
// thrust::reduce_by_key / std::unique_copy over the whole range: the runs
// appear in input order, contiguously from begin(out), across input and
// output segment boundaries wherever those fall.  The second half of a
// sort_by_key pipeline: group-by, combining duplicate COO entries, row counts
// for a CSR rowptr (run_length_encode -> exclusive_scan).
//
// Keys and values are any trivially copyable 4- or 8-byte types; `key_equal`
// and `op` are any trivially copyable device callables (captures included;
// op must be associative, it need not commute).  The kernel template
// (dr/details/segreduce_kernel.hpp, the one the C-ABI's drhip_reduce_by_key is
// built from) is instantiated here, in the user's translation unit.  Inputs
// are what copy_if takes: a distributed_vector, its take / drop / slice
// subranges (16-byte loads when both spans of a piece are 16-byte aligned,
// element loads otherwise) and a transform view.  Keys and values must be
// segmented alike (std::invalid_argument otherwise, as sort_by_key).  Float
// values under std::plus / std::multiplies fold in double inside a piece.
//
//   1. every non-empty piece is reduced on its own segment stream, all pieces
//      concurrently, into its slice of that segment's device scratch
//      (detail::carve_scratch);
//   2. a one-thread kernel behind it leaves the piece's boundary record in
//      pinned memory: run count, first and last key, and the folds of the first
//      and last run in ACC (double for float values under the library's
//      functors), as the fix-up kernel left them before rounding;
//   3. key_equal and op are device callables, so whether the last run of piece
//      k and the first run of piece k + 1 are one run, and the fold of their
//      values, is decided by one tiny kernel over the P records (behind event
//      waits on the pieces' streams), chaining as far as the keys stay equal:
//      a run may swallow whole pieces.  It folds in ACC and leaves a `joined`
//      flag per piece and, where a later piece added to a piece's last run,
//      the folded edge value, rounded to the value type once;
//   4. one wait; the host takes the prefix of the adjusted counts; a total
//      above size(keys_out) or size(values_out) throws std::out_of_range before
//      anything is written;
//   5. each piece's runs are copied into the outputs with drhip_memcpy_d2d,
//      split at output segment boundaries (detail::out_cursor, select.hpp,
//      one per output); the first run of a joined piece is
//      skipped and the folded value replaces the previous owner's last;
//   6. sync.
// Everything carried between tiles and between segments is ACC and every
// output element is rounded once, so the result does not depend on the
// segmentation wherever the ACC folds are exact (for inexact double folds the
// association differs, as it does between tiles).  run_length_encode counts in
// counts_out's value type: with a 4-byte type a run of 2^32 elements or more
// (only possible across pieces) wraps; use a 64-bit type for such inputs.  A
// piece of 2^32 elements or more throws std::length_error; an empty piece
// launches nothing.
#pragma once

#include <cstdint>
#include <functional>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../details/segreduce_kernel.hpp"
#include "algorithms.hpp"
#include "select.hpp"

namespace shp {

namespace detail {

enum class by_key_mode { reduce, lengths, unique };

// a piece's boundary record, in pinned memory
// (A = the kernel's ACC: what crosses pieces is not yet rounded to the value type)
template <typename K, typename V, typename A> struct by_key_edge {
  unsigned long long count; // runs of the piece (written by the kernel); 0 for an empty piece
  K first_key, last_key;    // of the piece's INPUT (neighbouring elements are what key_equal compares)
  A first_val, last_val;    // of the piece's first and last run, in ACC
  V edge_val;               // has_edge: the value of the piece's last run with what later pieces added to it
  unsigned joined, has_edge; // joined: the piece's first run continues the run before it
};

// the ACC folds of the piece's first and last run are what the fix-up kernel left in the state's head
template <typename K, typename V, typename A, bool HASV, typename KAcc>
__global__ void by_key_edge_kernel(KAcc kin, std::size_t n, const char *state, by_key_edge<K, V, A> *e) {
  e->first_key = static_cast<K>(kin(0));
  e->last_key = static_cast<K>(kin(n - 1));
  if constexpr (HASV) {
    e->first_val = *reinterpret_cast<const A *>(state + dr_segreduce::kSrFirstAcc);
    e->last_val = *reinterpret_cast<const A *>(state + dr_segreduce::kSrLastAcc);
  }
}

// One thread walks the P records: `owner` is the piece whose last output run
// is still open, `open` its value so far (ACC; rounded to the value type once,
// when the run ends), `grown` whether a later piece has added to it.
template <typename K, typename V, typename A, bool HASV, typename Eq, typename Op>
__global__ void by_key_stitch_kernel(by_key_edge<K, V, A> *e, std::size_t P, Eq eq, Op op) {
  long owner = -1, prev = -1;
  A open{};
  bool grown = false;
  for (std::size_t k = 0; k < P; k++) {
    e[k].joined = 0;
    e[k].has_edge = 0;
    if (!e[k].count) continue;
    const bool j = prev >= 0 && eq(e[prev].last_key, e[k].first_key);
    e[k].joined = j;
    if constexpr (HASV) {
      if (j) {
        open = op(open, e[k].first_val);
        grown = true;
      }
      if (!j || e[k].count > 1) { // the open run ends here (in this piece's first run, or before it)
        if (owner >= 0 && grown) {
          e[owner].edge_val = static_cast<V>(open);
          e[owner].has_edge = 1;
        }
        owner = (long)k;
        open = e[k].last_val;
        grown = false;
      }
    }
    prev = (long)k;
  }
  if constexpr (HASV)
    if (owner >= 0 && grown) {
      e[owner].edge_val = static_cast<V>(open);
      e[owner].has_edge = 1;
    }
}

// events recorded on the pieces' streams, destroyed on every way out
struct by_key_events {
  std::vector<hipEvent_t> ev;
  by_key_events() = default;
  by_key_events(const by_key_events &) = delete;
  by_key_events &operator=(const by_key_events &) = delete;
  ~by_key_events() {
    for (auto &e : ev) (void)hipEventDestroy(e);
  }
  void record(hipStream_t st) {
    hipEvent_t e;
    hip_check(hipEventCreateWithFlags(&e, hipEventDisableTiming), "hipEventCreate");
    ev.push_back(e);
    hip_check(hipEventRecord(e, st), "hipEventRecord");
  }
  // what is enqueued on st from here on runs behind everything recorded
  void wait_on(hipStream_t st) {
    for (auto &e : ev) hip_check(hipStreamWaitEvent(st, e, 0), "hipStreamWaitEvent");
  }
};

template <typename V> struct by_key_const_accessor {
  V v;
  __device__ __forceinline__ V operator()(std::size_t) const { return v; }
};
// the kernel's ACC: double for float values under the library's own functors, the value type otherwise
template <typename V, typename Op>
using by_key_acc_t = std::conditional_t<std::is_floating_point_v<V> && (op_code<Op>() >= 0), double, V>;
// op on ACC
template <typename A, typename Op> struct by_key_op {
  Op op;
  __device__ __forceinline__ A operator()(const A &a, const A &b) const { return static_cast<A>(op(a, b)); }
};
template <typename Eq> struct by_key_eq {
  Eq eq;
  template <typename K> __device__ __forceinline__ bool operator()(const K &a, const K &b) const {
    return static_cast<bool>(eq(a, b));
  }
};

template <typename S, typename K> constexpr bool by_key_span_of() {
  if constexpr (is_device_span<S>) return std::is_same_v<std::remove_const_t<typename S::value_type>, K>;
  else return false;
}

// reduce: keys, values -> kout, vout.  lengths: keys -> kout, vout (values
// unused, every element counts 1 in vout's type).  unique: keys -> kout
// (values and vout unused).  Returns the number of runs.
template <by_key_mode M, typename KR, typename VR, typename KO, typename VO, typename Eq, typename Op>
std::size_t by_key(const char *what, KR &&keys, VR &&values, KO &&kout, VO &&vout, Eq eq_, Op op_) {
  using namespace dr_segreduce;
  constexpr bool HASV = M != by_key_mode::unique;
  auto ksegs = lib::ranges::segments(keys);
  auto vsegs = lib::ranges::segments(values);
  auto kosegs = lib::ranges::segments(kout);
  auto vosegs = lib::ranges::segments(vout);
  using KSeg = std::remove_cvref_t<decltype(ksegs[0])>;
  using VSeg = std::remove_cvref_t<decltype(vsegs[0])>;
  using K = typename decltype(value_type_of_segment<KSeg>())::type;
  using VIn = typename decltype(value_type_of_segment<VSeg>())::type;
  using VOut = std::remove_cv_t<std::ranges::range_value_t<VO>>;
  using V = std::conditional_t<M == by_key_mode::reduce, VIn, std::conditional_t<HASV, VOut, sr_none>>;
  using A = std::conditional_t<HASV, by_key_acc_t<V, Op>, sr_none>;
  static_assert(sr_elem_type<K>, "shp: by-key algorithms take trivially copyable keys of 4 or 8 bytes");
  static_assert(!HASV || sr_elem_type<V>, "shp: by-key algorithms take trivially copyable values of 4 or 8 bytes");
  static_assert(std::is_same_v<std::remove_cv_t<std::ranges::range_value_t<KO>>, K>,
                "shp: the key output's value type must be the key input's");
  static_assert(!HASV || std::is_same_v<VOut, V>, "shp: the value output's value type must be the value input's");
  static_assert(std::is_trivially_copyable_v<Eq> && std::is_trivially_copyable_v<Op>,
                "shp: key_equal and op are passed to the device by value");
  const by_key_eq<Eq> eq{eq_};
  const by_key_op<A, Op> op{op_};

  const std::size_t P = ksegs.size();
  if constexpr (M == by_key_mode::reduce) {
    if (static_cast<std::size_t>(std::ranges::size(keys)) != static_cast<std::size_t>(std::ranges::size(values)))
      throw std::invalid_argument(std::string(what) + ": keys and values differ in size");
    check_segmented_alike(what, ksegs, vsegs);
  }
  check_piece_sizes(what, ksegs);

  // per non-empty piece: [keys of the runs | values of the runs | state]
  enum { TK, TV, STATE };
  std::vector<scratch_layout<3>> lay(P);
  std::vector<std::size_t> rank(P);
  for (std::size_t k = 0; k < P; k++) {
    const std::size_t n = ksegs[k].size();
    rank[k] = ksegs[k].rank();
    if (n) lay[k] = {n * sizeof(K), HASV ? n * sizeof(V) : 0, sr_state_bytes_max<K, V>(n)};
  }
  const std::vector<char *> base = carve_scratch(rank, lay);

  using Edge = by_key_edge<K, V, A>;
  pinned<Edge> edge(P);
  pinned<unsigned> err(1);
  err[0] = 0;
  by_key_events events;
  long first = -1;
  for (std::size_t k = 0; k < P; k++) {
    edge[k].count = 0;
    const std::size_t n = ksegs[k].size();
    if (!n) continue;
    const std::size_t rk = ksegs[k].rank();
    hipStream_t st = stream(rk);
    K *tk = lay[k].template at<K>(base[k], TK);
    V *tv = lay[k].template at<V>(base[k], TV);
    const sr_args a{lay[k].at(base[k], STATE), &edge[k].count, err.data()};
    if constexpr (M == by_key_mode::unique) {
      if constexpr (by_key_span_of<KSeg, K>())
        hip_check(sr_launch_unique<K>(st, static_cast<const K *>(ksegs[k].data()), n, tk, eq, a), "unique_copy launch");
      else
        hip_check((sr_launch<K, sr_none, sr_none, false, false>(st, accessor_of(ksegs[k]), (const sr_none *)nullptr, n, tk,
                                                                (sr_none *)nullptr, eq, sr_no_op{}, a)),
                  "unique_copy launch");
    } else {
      auto launch = [&](auto vin, auto vin_is_span) {
        if constexpr (by_key_span_of<KSeg, K>()) {
          const K *kp = static_cast<const K *>(ksegs[k].data());
          if constexpr (decltype(vin_is_span)::value)
            hip_check((sr_launch_spans<K, V, A>(st, kp, vin, n, tk, tv, eq, op, a)), "reduce_by_key launch");
          else
            hip_check((sr_launch_keys_span<K, V, A>(st, kp, vin, n, tk, tv, eq, op, a)), "reduce_by_key launch");
        } else {
          if constexpr (decltype(vin_is_span)::value)
            hip_check((sr_launch<K, V, A, false, true>(st, accessor_of(ksegs[k]), sr_ptr_accessor<V>{vin}, n, tk, tv, eq, op, a)),
                      "reduce_by_key launch");
          else
            hip_check((sr_launch<K, V, A, false, true>(st, accessor_of(ksegs[k]), vin, n, tk, tv, eq, op, a)),
                      "reduce_by_key launch");
        }
      };
      if constexpr (M == by_key_mode::lengths) launch(by_key_const_accessor<V>{V(1)}, std::false_type{});
      else if constexpr (by_key_span_of<VSeg, V>()) launch(static_cast<const V *>(vsegs[k].data()), std::true_type{});
      else launch(accessor_of(vsegs[k]), std::false_type{});
    }
    auto kacc = accessor_of(ksegs[k]);
    hipLaunchKernelGGL((by_key_edge_kernel<K, V, A, HASV, decltype(kacc)>), dim3(1), dim3(1), 0, st, kacc, n,
                       static_cast<const char *>(a.state), &edge[k]);
    hip_check(hipGetLastError(), "by-key edge launch");
    if (first < 0) {
      first = (long)k;
    } else if (rk != ksegs[first].rank()) {
      events.record(st);
    }
  }
  if (first < 0) return 0;
  {
    const std::size_t rk = ksegs[first].rank();
    events.wait_on(stream(rk));
    hipLaunchKernelGGL((by_key_stitch_kernel<K, V, A, HASV, by_key_eq<Eq>, by_key_op<A, Op>>), dim3(1), dim3(1), 0, stream(rk),
                       edge.data(), P, eq, op);
    hip_check(hipGetLastError(), "by-key stitch launch");
    sync(rk); // the one wait: the stitch ran behind every piece
  }
  select_check(err[0]);

  std::size_t total = 0;
  for (std::size_t k = 0; k < P; k++) total += static_cast<std::size_t>(edge[k].count) - edge[k].joined;
  if (total > static_cast<std::size_t>(std::ranges::size(kout)) || (HASV && total > static_cast<std::size_t>(std::ranges::size(vout))))
    throw std::out_of_range(std::string(what) + ": " + std::to_string(total) + " runs, the outputs hold " +
                            std::to_string(std::ranges::size(kout)) +
                            (HASV ? " and " + std::to_string(std::ranges::size(vout)) : std::string()));

  // the pieces' runs, in order, into the outputs' segments
  out_cursor<decltype(kosegs)> kcur{&kosegs};
  out_cursor<decltype(vosegs)> vcur{&vosegs};
  for (std::size_t k = 0; k < P; k++) {
    if (!edge[k].count) continue;
    const std::size_t rk = ksegs[k].rank(), j = edge[k].joined, c = static_cast<std::size_t>(edge[k].count) - j;
    if (!c) continue;
    kcur.emit(rk, lay[k].template at<const K>(base[k], TK) + j, c);
    if constexpr (HASV) {
      vcur.emit(rk, lay[k].template at<const V>(base[k], TV) + j, c);
      if (edge[k].has_edge) // on this piece's last run
        check(drhip_memcpy_h2d(static_cast<int>(rk), vcur.last(), &edge[k].edge_val, sizeof(V)), "drhip_memcpy_h2d");
    }
  }
  select_sync(ksegs);
  return total;
}

} // namespace detail

// Returns {begin(keys_out) + runs, begin(values_out) + runs}.
template <typename ExecutionPolicy, lib::distributed_range KR, lib::distributed_range VR,
          lib::distributed_contiguous_range KO, lib::distributed_contiguous_range VO, typename KeyEqual = std::equal_to<>,
          typename Op = std::plus<>>
auto reduce_by_key(ExecutionPolicy &&, KR &&keys, VR &&values, KO &&keys_out, VO &&values_out, KeyEqual key_equal = KeyEqual{},
                   Op op = Op{}) {
  const std::size_t runs = detail::by_key<detail::by_key_mode::reduce>("shp::reduce_by_key", keys, values, keys_out, values_out,
                                                                      key_equal, op);
  return std::pair(std::ranges::begin(keys_out) + static_cast<std::ranges::range_difference_t<KO>>(runs),
                   std::ranges::begin(values_out) + static_cast<std::ranges::range_difference_t<VO>>(runs));
}

// counts_out[r] = the length of run r, in counts_out's value type (a 4- or 8-byte integer)
template <typename ExecutionPolicy, lib::distributed_range KR, lib::distributed_contiguous_range KO,
          lib::distributed_contiguous_range CO, typename KeyEqual = std::equal_to<>>
auto run_length_encode(ExecutionPolicy &&, KR &&keys, KO &&keys_out, CO &&counts_out, KeyEqual key_equal = KeyEqual{}) {
  static_assert(std::is_integral_v<std::ranges::range_value_t<CO>>, "shp::run_length_encode: counts are integers");
  const std::size_t runs = detail::by_key<detail::by_key_mode::lengths>("shp::run_length_encode", keys, keys, keys_out, counts_out,
                                                                       key_equal, std::plus<>{});
  return std::pair(std::ranges::begin(keys_out) + static_cast<std::ranges::range_difference_t<KO>>(runs),
                   std::ranges::begin(counts_out) + static_cast<std::ranges::range_difference_t<CO>>(runs));
}

// Returns begin(out) + the number of runs.
template <typename ExecutionPolicy, lib::distributed_range R, lib::distributed_contiguous_range O,
          typename KeyEqual = std::equal_to<>>
auto unique_copy(ExecutionPolicy &&, R &&in, O &&out, KeyEqual key_equal = KeyEqual{}) {
  const std::size_t runs =
      detail::by_key<detail::by_key_mode::unique>("shp::unique_copy", in, in, out, out, key_equal, dr_segreduce::sr_no_op{});
  return std::ranges::begin(out) + static_cast<std::ranges::range_difference_t<O>>(runs);
}

// iterator forms: an output starts at its iterator and has room for the runs
// (at most last - first are written)
template <typename ExecutionPolicy, lib::distributed_iterator KIter, lib::distributed_iterator VIter,
          lib::distributed_iterator KOut, lib::distributed_iterator VOut, typename KeyEqual = std::equal_to<>,
          typename Op = std::plus<>>
std::pair<KOut, VOut> reduce_by_key(ExecutionPolicy &&policy, KIter kfirst, KIter klast, VIter vfirst, KOut keys_out,
                                    VOut values_out, KeyEqual key_equal = KeyEqual{}, Op op = Op{}) {
  const std::size_t n = static_cast<std::size_t>(klast - kfirst);
  return shp::reduce_by_key(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(kfirst, klast),
                            std::ranges::subrange(vfirst, vfirst + static_cast<std::ptrdiff_t>(n)),
                            detail::out_from(keys_out, n), detail::out_from(values_out, n), key_equal, op);
}
template <typename ExecutionPolicy, lib::distributed_iterator KIter, lib::distributed_iterator KOut,
          lib::distributed_iterator COut, typename KeyEqual = std::equal_to<>>
std::pair<KOut, COut> run_length_encode(ExecutionPolicy &&policy, KIter first, KIter last, KOut keys_out, COut counts_out,
                                        KeyEqual key_equal = KeyEqual{}) {
  const std::size_t n = static_cast<std::size_t>(last - first);
  return shp::run_length_encode(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last),
                                detail::out_from(keys_out, n), detail::out_from(counts_out, n), key_equal);
}
template <typename ExecutionPolicy, lib::distributed_iterator Iter, lib::distributed_iterator OutputIter,
          typename KeyEqual = std::equal_to<>>
OutputIter unique_copy(ExecutionPolicy &&policy, Iter first, Iter last, OutputIter d_first, KeyEqual key_equal = KeyEqual{}) {
  return shp::unique_copy(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last),
                          detail::out_from(d_first, static_cast<std::size_t>(last - first)), key_equal);
}

} // namespace shp

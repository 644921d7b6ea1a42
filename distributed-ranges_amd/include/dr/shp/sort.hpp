// dr/shp/sort.hpp -- shp::sort over a distributed range.
//
// The reference has no sort.  Semantics are
// std::ranges::sort: ascending under std::less, in place, the result keeps
// the range's segmentation.  Algorithm (single process, P segments):
//   1. every segment sorts locally (drhip_sort, LSD radix, in parallel) and
//      takes regular samples (drhip_sort_sample);
//   2. exact splitting (csrc/split.hip): from the samples, a value bracket
//      per segment boundary g_k = sum of the sizes of segments < k and each
//      segment's slice of sorted keys that holds it; from those slices the
//      key v_k of global rank g_k, with keys equal to v_k split in segment
//      order, so every destination gets exactly its segment's size -- two
//      small host exchanges instead of a device round trip per bisection
//      step (the same code dr_dist.exact_splits runs over two allgathers);
//   3. every (source, destination) piece moves with one device-to-device
//      copy (xGMI peer copy across GPUs) into a per-destination buffer;
//   4. every destination merges its P sorted runs straight into its segment
//      (drhip_merge_runs_to).
// All device scratch comes from the cached per-segment pool
// (detail::carve_scratch, runtime.hpp).  With P == 1 only step 1's sort runs.
// shp::sort_by_key (at the end of this file) takes the same four steps with a
// value carried beside every key, and the comparator tier (detail::
// sort_general) with its own local sort, splitting and merge.  What the three
// share is written once: the sample plan and the run offsets in dr/details/
// split_plan.hpp, and in detail below the non-empty parts (nonempty_parts),
// the two host gathers of step 2 (gather_samples, gather_windows) and step 3
// (move_pieces); each tier keeps its own sort, split and merge calls.
#pragma once

#include <cstring>
#include <functional>
#include <initializer_list>
#include <string>

#include "algorithms.hpp"
#include "merge_sort.hpp"
#include "select.hpp"
#include "../details/split_plan.hpp"

namespace shp {

namespace detail {

template <typename T> struct key_bits;
template <> struct key_bits<std::uint32_t> {
  using U = std::uint32_t;
  static U in(std::uint32_t x) { return x; }
  static std::uint32_t out(U u) { return u; }
};
template <> struct key_bits<std::int32_t> {
  using U = std::uint32_t;
  static U in(std::int32_t x) { return static_cast<U>(x) ^ 0x80000000u; }
  static std::int32_t out(U u) { return static_cast<std::int32_t>(u ^ 0x80000000u); }
};
template <> struct key_bits<float> {
  using U = std::uint32_t;
  static U in(float x) {
    U u;
    std::memcpy(&u, &x, 4);
    return u ^ ((u & 0x80000000u) ? 0xFFFFFFFFu : 0x80000000u);
  }
  static float out(U u) {
    u ^= (u & 0x80000000u) ? 0x80000000u : 0xFFFFFFFFu;
    float x;
    std::memcpy(&x, &u, 4);
    return x;
  }
};
template <> struct key_bits<std::uint64_t> {
  using U = std::uint64_t;
  static U in(std::uint64_t x) { return x; }
  static std::uint64_t out(U u) { return u; }
};
template <> struct key_bits<std::int64_t> {
  using U = std::uint64_t;
  static U in(std::int64_t x) { return static_cast<U>(x) ^ 0x8000000000000000ull; }
  static std::int64_t out(U u) { return static_cast<std::int64_t>(u ^ 0x8000000000000000ull); }
};
template <> struct key_bits<double> {
  using U = std::uint64_t;
  static U in(double x) {
    U u;
    std::memcpy(&u, &x, 8);
    return u ^ ((u & 0x8000000000000000ull) ? ~0ull : 0x8000000000000000ull);
  }
  static double out(U u) {
    u ^= (u & 0x8000000000000000ull) ? 0x8000000000000000ull : ~0ull;
    double x;
    std::memcpy(&x, &u, 8);
    return x;
  }
};

// Per-segment scratch of one sort call, from the cached per-rank device
// scratch (runtime.hpp device_scratch: grown once, reused by later calls,
// released by finalize) -- the sort allocates nothing per call once warm.
// Per segment of the radix tiers: [radix workspace | n-key exchange buffer |
// n-value exchange buffer | merge workspace | regular samples of the keys].
// Everything after the workspace serves the exchange between segments (P > 1);
// shp::sort carries no values (vb == 0).
enum { SORT_WS, SORT_BUF, SORT_VBUF, SORT_MWS, SORT_SMP };
using sort_layout = scratch_layout<5>;
template <typename T>
sort_layout radix_sort_layout(std::size_t wsb, std::size_t mwsb, std::size_t n, std::size_t vb, std::size_t nsamples,
                              std::size_t P) {
  if (P == 1) return {wsb, 0, 0, 0, 0};
  return {wsb, n * sizeof(T), n * vb, mwsb, nsamples * sizeof(T)};
}

// The non-empty segments of a range, their sizes and ranks, and the plan of
// every segment's regular samples (dr_plan::plan_samples).
template <typename T> struct sort_parts {
  std::vector<device_span<T>> parts;
  std::vector<std::uint64_t> n, stride, ns;
  std::vector<std::size_t> rank;
  std::size_t size() const { return parts.size(); }
  const device_span<T> &operator[](std::size_t k) const { return parts[k]; }
};
template <typename T, typename Segs> sort_parts<T> nonempty_parts(Segs &&segs) {
  sort_parts<T> z;
  for (auto &&s : segs) {
    if (!s.size()) continue;
    const dr_plan::sample_plan sp = dr_plan::plan_samples(s.size());
    z.parts.push_back(s);
    z.n.push_back(s.size());
    z.stride.push_back(sp.stride);
    z.ns.push_back(sp.ns);
    z.rank.push_back(s.rank());
  }
  return z;
}

// Step 1b: the ns[k] samples at smp[k] (device memory of part k) to the host,
// part after part; hs has room for the sum of ns.
template <typename T> void gather_samples(const sort_parts<T> &z, const std::vector<T *> &smp, T *hs) {
  for (std::size_t k = 0; k < z.size(); hs += z.ns[k], k++)
    check(drhip_memcpy_d2h(static_cast<int>(z.rank[k]), hs, smp[k], z.ns[k] * sizeof(T)), "sort samples d2h");
  for (std::size_t k = 0; k < z.size(); k++) sync(z.rank[k]);
}

// Step 2b: the windows of the split (win[2 (s nb + k) + {0, 1}] = the slice of
// part s that holds boundary k's bracket) to the host, in (part, boundary)
// order; hw has room for window_total(win).
inline std::size_t window_total(const std::vector<std::uint64_t> &win) {
  std::size_t t = 0;
  for (std::size_t i = 0; i < win.size(); i += 2) t += win[i + 1] - win[i];
  return t;
}
template <typename T> void gather_windows(const sort_parts<T> &z, const std::vector<std::uint64_t> &win, T *hw) {
  const std::size_t nb = z.size() - 1;
  for (std::size_t s = 0; s < z.size(); s++)
    for (std::size_t k = 0; k < nb; k++) {
      const std::size_t a = win[2 * (s * nb + k)], b = win[2 * (s * nb + k) + 1];
      if (b > a)
        check(drhip_memcpy_d2h(static_cast<int>(z.rank[s]), hw, z[s].data() + a, (b - a) * sizeof(T)),
              "sort slices d2h");
      hw += b - a;
    }
  for (std::size_t s = 0; s < z.size(); s++) sync(z.rank[s]);
}

// the boundary ranks of the split: g[k] = the sizes of the segments <= k
inline std::vector<std::uint64_t> boundary_ranks(const std::vector<std::uint64_t> &n) {
  std::vector<std::uint64_t> g(n.size() - 1);
  for (std::size_t k = 0, acc = 0; k < g.size(); k++) g[k] = acc += n[k];
  return g;
}

// Steps 1b-2 of the radix tiers, on keys alone (shared by shp::sort and
// shp::sort_by_key): the regular samples of every locally sorted segment
// come to the host, then the exact splitting at the segment boundaries
// (csrc/split.hip): value brackets from the samples, then each boundary key
// on the slices of every sorted segment that hold its bracket.  Needs P > 1.
// Returns split[s * P + k] = the number of segment s's keys that go to
// destinations <= k; keys equal to a boundary key are given out in segment
// order, which is what keeps sort_by_key stable across segments.
template <typename T> std::vector<std::uint64_t> exact_splits(const sort_parts<T> &z, const std::vector<T *> &smp) {
  using KB = key_bits<T>;
  const std::size_t P = z.size(), nb = P - 1;
  auto bits_of = [](const T *h, std::size_t count) {
    std::vector<std::uint64_t> bits(count);
    for (std::size_t i = 0; i < count; i++) bits[i] = static_cast<std::uint64_t>(KB::in(h[i]));
    return bits;
  };
  std::size_t tot_smp = 0;
  for (auto v : z.ns) tot_smp += v;
  pinned<T> hs(tot_smp);
  gather_samples(z, smp, hs.data());
  const std::vector<std::uint64_t> g = boundary_ranks(z.n);
  std::vector<std::uint64_t> lo(nb), hi(nb), win(2 * P * nb), split(P * (nb + 1));
  check(drhip_split_windows(static_cast<int>(P), z.n.data(), z.stride.data(), z.ns.data(),
                            bits_of(hs.data(), tot_smp).data(), static_cast<int>(nb), g.data(), lo.data(), hi.data(),
                            win.data()),
        "drhip_split_windows");
  const std::size_t tot_win = window_total(win);
  pinned<T> hw(tot_win);
  gather_windows(z, win, hw.data());
  check(drhip_split_exact(static_cast<int>(P), z.n.data(), static_cast<int>(nb), g.data(), lo.data(), hi.data(),
                          win.data(), bits_of(hw.data(), tot_win).data(), split.data()),
        "drhip_split_exact");
  return split;
}

// One lane of step 3: src[s] is source s's data, dst[k] destination k's
// exchange buffer, elements of `elem` bytes.  sort_by_key moves a key lane and
// a value lane by the same split indices.
struct sort_lane {
  std::vector<const char *> src;
  std::vector<char *> dst;
  std::size_t elem;
  const char *what;
};
template <typename T>
sort_lane make_lane(const std::vector<device_span<T>> &parts, const std::vector<T *> &bufs, const char *what) {
  sort_lane l{{}, {}, sizeof(T), what};
  for (std::size_t k = 0; k < parts.size(); k++) {
    l.src.push_back(reinterpret_cast<const char *>(parts[k].data()));
    l.dst.push_back(reinterpret_cast<char *>(bufs[k]));
  }
  return l;
}

// Step 3: every (source s, destination k) piece, source s's range
// [split[s][k-1], split[s][k]), moves with one device-to-device copy per lane
// (xGMI peer copy across GPUs) to its run offset in destination k's buffer, the
// runs in source order.  Returns every destination's run offsets for the
// merge; waits for the copies (they read the segments the merge writes).
inline std::vector<std::vector<std::size_t>> move_pieces(const char *who, const std::vector<std::size_t> &rank,
                                                          const std::vector<std::uint64_t> &n,
                                                          const std::vector<std::uint64_t> &split,
                                                          std::initializer_list<sort_lane> lanes) {
  const int P = static_cast<int>(n.size());
  std::vector<std::vector<std::size_t>> offs(P);
  for (int k = 0; k < P; k++) {
    dr_plan::run_plan r = dr_plan::plan_runs(split.data(), P, P, k);
    for (int s = 0; s < P; s++) {
      const std::size_t a = r.from[s], b = a + (r.offs[s + 1] - r.offs[s]); // source s's range
      if (b > a)
        for (const sort_lane &l : lanes)
          check(drhip_memcpy_d2d(static_cast<int>(rank[k]), l.dst[k] + r.offs[s] * l.elem, l.src[s] + a * l.elem,
                                 (b - a) * l.elem),
                l.what);
    }
    if (r.offs[P] != n[k]) throw std::runtime_error(std::string(who) + ": splitting did not balance");
    offs[k] = std::move(r.offs);
  }
  sync_all();
  return offs;
}

} // namespace detail

namespace detail {
template <typename T, typename Comp> void sort_general(auto &segs, Comp comp);
}

// std::ranges::sort(r): ascending under std::less.  int32/uint32/int64/
// uint64/float/double keys take the LSD radix path of libdrhip below; any
// other trivially-copyable T the general merge tier (merge_sort.hpp).
template <typename ExecutionPolicy, typename R>
  requires lib::distributed_contiguous_range<R>
void sort(ExecutionPolicy &&, R &&r) {
  using T = std::remove_cv_t<std::ranges::range_value_t<R>>;
  auto segs = lib::ranges::segments(r);
  if constexpr (!detail::abi_type<T>) {
    detail::sort_general<T>(segs, std::less<>{});
    return;
  } else {
  const auto z = detail::nonempty_parts<T>(segs);
  const std::size_t P = z.size();
  if (P == 0) return;
  const int dt = detail::dtype_code<T>();
  std::vector<std::size_t> wsb(P), mwsb(P, 0);
  std::vector<detail::sort_layout> lay(P);
  for (std::size_t k = 0; k < P; k++) {
    const int rk = static_cast<int>(z.rank[k]);
    detail::check(drhip_sort_workspace(rk, dt, z.n[k], &wsb[k]), "drhip_sort_workspace");
    if (P > 1)
      detail::check(drhip_merge_workspace(rk, dt, z.n[k], static_cast<int>(P), &mwsb[k]), "drhip_merge_workspace");
    lay[k] = detail::radix_sort_layout<T>(wsb[k], mwsb[k], z.n[k], 0, z.ns[k], P);
  }
  const std::vector<char *> base = detail::carve_scratch(z.rank, lay);
  std::vector<T *> buf(P), smp(P);
  for (std::size_t k = 0; k < P; k++) {
    buf[k] = lay[k].template at<T>(base[k], detail::SORT_BUF);
    smp[k] = lay[k].template at<T>(base[k], detail::SORT_SMP);
  }

  // 1. local sorts (every segment in flight), then the regular samples
  for (std::size_t k = 0; k < P; k++) {
    const int rk = static_cast<int>(z.rank[k]);
    if (z.n[k] > 1)
      detail::check(drhip_sort(rk, dt, z[k].data(), z.n[k], lay[k].at(base[k], detail::SORT_WS), wsb[k]), "drhip_sort");
    if (P > 1) detail::check(drhip_sort_sample(rk, dt, z[k].data(), z.n[k], z.stride[k], smp[k]), "drhip_sort_sample");
  }
  if (P == 1) {
    sync(z.rank[0]);
    return;
  }
  // 2. exact splitting at the segment boundaries
  const std::vector<std::uint64_t> split = detail::exact_splits<T>(z, smp);
  // 3. move pieces
  const auto offs =
      detail::move_pieces("shp::sort", z.rank, z.n, split, {detail::make_lane(z.parts, buf, "sort piece copy")});
  // 4. destination merge of the P sorted runs straight into the segment
  //    (drhip_merge_runs_to: ceil(log2 P) merge-path passes instead of a
  //    second radix sort, the last pass writing the segment -- no copy back)
  for (std::size_t k = 0; k < P; k++)
    detail::check(drhip_merge_runs_to(static_cast<int>(z.rank[k]), dt, buf[k], z[k].data(), z.n[k], offs[k].data(),
                                      static_cast<int>(P), lay[k].at(base[k], detail::SORT_MWS), mwsb[k]),
                  "drhip_merge_runs_to");
  sync_all();
  }
}

namespace detail {

// An order-reversing involution of the key's bits: ~x for integers (for
// two's complement ~x = -1 - x), the sign bit for IEEE floats (-x).  std::
// greater sorts as std::less on flipped keys, flipped back: two elementwise
// passes around the ascending radix sort (8 B/key each).
template <typename T> struct flip_order {
  __host__ __device__ void operator()(T &x) const {
    if constexpr (std::is_same_v<T, float>)
      x = __builtin_bit_cast(float, __builtin_bit_cast(std::uint32_t, x) ^ 0x80000000u);
    else if constexpr (std::is_same_v<T, double>)
      x = __builtin_bit_cast(double, __builtin_bit_cast(std::uint64_t, x) ^ 0x8000000000000000ull);
    else
      x = static_cast<T>(~x);
  }
};

template <typename C, typename T>
constexpr bool is_less_v = std::is_same_v<C, std::less<>> || std::is_same_v<C, std::less<T>> ||
                           std::is_same_v<C, std::ranges::less>;
template <typename C, typename T>
constexpr bool is_greater_v = std::is_same_v<C, std::greater<>> || std::is_same_v<C, std::greater<T>> ||
                              std::is_same_v<C, std::ranges::greater>;

} // namespace detail

namespace detail {

// The general tier (dr/shp/merge_sort.hpp): any trivially-copyable T, any
// strict weak ordering `comp` callable on host and device.  Stable: the
// result is std::stable_sort's over the whole range (equivalent elements keep
// their order -- segment order, then index order within a segment).
//   1. every segment: stable local merge sort, then its regular samples;
//   2. exact splitting under comp (dr_plan::split_windows_cmp /
//      split_exact_cmp, the general form of csrc/split.hip): windows from the
//      samples, then the key of every boundary rank from the windows, with
//      equivalent keys given out in segment order;
//   3. every (source, destination) piece moves with one device-to-device copy;
//   4. every destination merges its P runs pairwise (ceil(log2 P) rounds of
//      merge_kernel, the earlier run first on ties) into its segment.
template <typename T, typename Comp> void sort_general(auto &segs, Comp comp) {
  static_assert(std::is_trivially_copyable_v<T>, "shp::sort: the element type must be trivially copyable");
  static_assert(sizeof(T) <= 256, "shp::sort: elements above 256 bytes are not supported");
  const auto z = nonempty_parts<T>(segs);
  const std::size_t P = z.size();
  if (P == 0) return;
  const std::vector<std::uint64_t> &n = z.n;
  // per segment: [local-sort scratch (doubles as the piece buffer) | samples]
  enum { BUF, SMP };
  std::vector<scratch_layout<2>> lay(P);
  for (std::size_t k = 0; k < P; k++) lay[k] = {msort::scratch_bytes<T>(n[k]), P > 1 ? z.ns[k] * sizeof(T) : 0};
  const std::vector<char *> base = carve_scratch(z.rank, lay);
  std::vector<T *> buf(P), smp(P);
  for (std::size_t k = 0; k < P; k++) {
    buf[k] = lay[k].template at<T>(base[k], BUF);
    smp[k] = lay[k].template at<T>(base[k], SMP);
  }
  auto st = [&](std::size_t k) {
    hip_check(hipSetDevice(device_list().at(z.rank[k])), "hipSetDevice");
    return stream(z.rank[k]);
  };
  // 1. local sorts and samples
  for (std::size_t k = 0; k < P; k++) {
    hipStream_t s = st(k);
    msort::local_sort(z[k].data(), n[k], base[k], comp, s);
    if (P > 1)
      hipLaunchKernelGGL((msort::gather_samples_kernel<T>), dim3(msort::blocks_of(z.ns[k], 256)), dim3(256), 0, s,
                         z[k].data(), z.stride[k], z.ns[k], smp[k]);
    hip_check(hipGetLastError(), "shp::sort launch");
  }
  if (P == 1) {
    sync(z.rank[0]);
    return;
  }
  // 2. exact splitting under comp
  const std::size_t nb = P - 1;
  std::size_t tot_smp = 0;
  for (auto v : z.ns) tot_smp += v;
  std::vector<T> hs(tot_smp);
  gather_samples(z, smp, hs.data());
  const std::vector<std::uint64_t> g = boundary_ranks(n);
  std::vector<std::uint64_t> win(2 * P * nb), split(P * (nb + 1));
  if (const char *why = dr_plan::split_windows_cmp(static_cast<int>(P), n.data(), z.stride.data(), z.ns.data(),
                                                   hs.data(), static_cast<int>(nb), g.data(), comp, win.data()))
    throw std::runtime_error(std::string("shp::sort: ") + why);
  std::vector<T> hw(window_total(win));
  gather_windows(z, win, hw.data());
  if (const char *why = dr_plan::split_exact_cmp(static_cast<int>(P), n.data(), static_cast<int>(nb), g.data(),
                                                 win.data(), hw.data(), comp, split.data()))
    throw std::runtime_error(std::string("shp::sort: ") + why);
  // 3. pieces into every destination's buffer, in source order
  const auto offs = move_pieces("shp::sort", z.rank, n, split, {make_lane(z.parts, buf, "sort piece copy")});
  // 4. pairwise run merges, the last round into the segment: with R rounds
  //    and two buffers, the runs start in the segment when R is even
  std::size_t R = 0;
  while ((std::size_t(1) << R) < P) R++;
  for (std::size_t k = 0; k < P; k++) {
    hipStream_t s = st(k);
    T *src = buf[k], *dst = z[k].data();
    if (R % 2 == 0) {
      hip_check(hipMemcpyAsync(dst, src, n[k] * sizeof(T), hipMemcpyDeviceToDevice, s), "sort run copy");
      std::swap(src, dst);
    }
    // the tile splits: where the local sort kept its own, past the piece buffer
    std::vector<std::size_t> run = offs[k];
    auto *part = reinterpret_cast<std::size_t *>(base[k] + align_up(n[k] * sizeof(T)));
    while (run.size() > 2) {
      std::vector<std::size_t> next{0};
      for (std::size_t r = 0; r + 1 < run.size(); r += 2) {
        const std::size_t a = run[r], m = run[r + 1], e = r + 2 < run.size() ? run[r + 2] : m;
        if (e > a) {
          if (e > m && m > a)
            msort::merge_pass<T>(src + a, dst + a, msort::pass_geom{e - a, m - a, true}, part, comp, s);
          else
            hip_check(hipMemcpyAsync(dst + a, src + a, (e - a) * sizeof(T), hipMemcpyDeviceToDevice, s), "sort run copy");
        }
        next.push_back(e);
      }
      run.swap(next);
      std::swap(src, dst);
      hip_check(hipGetLastError(), "shp::sort merge launch");
    }
  }
  sync_all();
}

} // namespace detail

// std::ranges::sort(r, comp) for comp in {std::less, std::greater} (any of
// their spellings).  Descending keys: equal keys are indistinguishable, so
// the result is bit-identical to any correct descending sort (for floats,
// as with std::less: inputs without NaN, and -0.0 / +0.0 compare equal).
// Any other comparator or element type: the stable general tier.
template <typename ExecutionPolicy, typename R, typename Compare>
  requires lib::distributed_contiguous_range<R>
void sort(ExecutionPolicy &&policy, R &&r, Compare comp) {
  using C = std::remove_cvref_t<Compare>;
  using T = std::remove_cv_t<std::ranges::range_value_t<R>>;
  if constexpr (detail::abi_type<T> && detail::is_less_v<C, T>) {
    shp::sort(std::forward<ExecutionPolicy>(policy), std::forward<R>(r));
  } else if constexpr (detail::abi_type<T> && detail::is_greater_v<C, T>) {
    shp::for_each(policy, r, detail::flip_order<T>{});
    shp::sort(policy, r);
    shp::for_each(policy, r, detail::flip_order<T>{});
  } else {
    auto segs = lib::ranges::segments(r);
    detail::sort_general<T>(segs, comp);
  }
}

// std::ranges::stable_sort(r[, comp]): equivalent elements keep their order.
// Integer keys under std::less / std::greater are indistinguishable when
// equivalent, so they keep the radix path; everything else (floats included:
// -0.0 and +0.0 are equivalent but not identical) takes the general tier.
template <typename ExecutionPolicy, typename R, typename Compare = std::ranges::less>
  requires lib::distributed_contiguous_range<R>
void stable_sort(ExecutionPolicy &&policy, R &&r, Compare comp = {}) {
  using C = std::remove_cvref_t<Compare>;
  using T = std::remove_cv_t<std::ranges::range_value_t<R>>;
  if constexpr (detail::abi_type<T> && std::is_integral_v<T> && (detail::is_less_v<C, T> || detail::is_greater_v<C, T>)) {
    shp::sort(std::forward<ExecutionPolicy>(policy), std::forward<R>(r), comp);
  } else {
    auto segs = lib::ranges::segments(r);
    detail::sort_general<T>(segs, comp);
  }
}

template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename Compare = std::ranges::less>
void stable_sort(ExecutionPolicy &&policy, Iter first, Iter last, Compare comp = {}) {
  shp::stable_sort(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), comp);
}

template <typename ExecutionPolicy, lib::distributed_iterator Iter>
void sort(ExecutionPolicy &&policy, Iter first, Iter last) {
  shp::sort(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last));
}

template <typename ExecutionPolicy, lib::distributed_iterator Iter, typename Compare>
void sort(ExecutionPolicy &&policy, Iter first, Iter last, Compare comp) {
  shp::sort(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(first, last), comp);
}

// sort_by_key(keys, values[, comp]): std::stable_sort of the (key, value)
// pairs by key over the whole range -- equal keys keep segment order, then
// index order within a segment.  Keys are any of the six ABI key types,
// values any trivially copyable type of 4 or 8 bytes (moved as bits), comp
// std::less or std::greater (any spelling).  Both ranges keep their
// segmentation, which must agree segment by segment.  The steps are
// shp::sort's with the values carried along:
//   1. every segment: drhip_sort_pairs (stable LSD radix) + key samples;
//   2. exact splitting on the keys alone (detail::exact_splits; ties go out
//      in segment order);
//   3. every (source, destination) piece: two device-to-device copies, keys
//      and values, by the same split indices;
//   4. every destination: drhip_merge_pairs_runs_to (the earlier run first
//      on ties) straight into the key segment and the value segment.
// std::greater sorts flipped keys ascending and flips them back
// (detail::flip_order reverses the order and keeps equality, so the stable
// ascending sort of the flipped keys IS the stable descending sort).
template <typename ExecutionPolicy, typename KR, typename VR, typename Compare = std::ranges::less>
  requires lib::distributed_contiguous_range<KR> && lib::distributed_contiguous_range<VR>
void sort_by_key(ExecutionPolicy &&policy, KR &&keys, VR &&values, Compare comp = {}) {
  using C = std::remove_cvref_t<Compare>;
  using T = std::remove_cv_t<std::ranges::range_value_t<KR>>;
  using V = std::remove_cv_t<std::ranges::range_value_t<VR>>;
  static_assert(detail::abi_type<T>,
                "shp::sort_by_key: keys must be int32/uint32/int64/uint64/float/double; for other records use "
                "shp::sort on a struct with a comparator");
  static_assert(std::is_trivially_copyable_v<V> && (sizeof(V) == 4 || sizeof(V) == 8),
                "shp::sort_by_key: values must be trivially copyable and 4 or 8 bytes (sort an index and gather "
                "for anything else)");
  static_assert(detail::is_less_v<C, T> || detail::is_greater_v<C, T>,
                "shp::sort_by_key: the comparator must be std::less or std::greater; for any other order pack key "
                "and value into a struct and call shp::sort(range, comp)");
  if constexpr (detail::is_greater_v<C, T>) {
    shp::for_each(policy, keys, detail::flip_order<T>{});
    shp::sort_by_key(policy, keys, values);
    shp::for_each(policy, keys, detail::flip_order<T>{});
    return;
  } else {
  constexpr std::size_t vb = sizeof(V);
  if (static_cast<std::size_t>(std::ranges::size(keys)) != static_cast<std::size_t>(std::ranges::size(values)))
    throw std::invalid_argument("shp::sort_by_key: keys and values differ in size");
  const auto z = detail::nonempty_parts<T>(lib::ranges::segments(keys));
  std::vector<device_span<V>> vparts;
  for (auto &&s : lib::ranges::segments(values))
    if (s.size()) vparts.push_back(s);
  detail::check_segmented_alike("shp::sort_by_key", z.parts, vparts);
  const std::size_t P = z.size();
  if (P == 0) return;
  const int dt = detail::dtype_code<T>();
  std::vector<std::size_t> wsb(P), mwsb(P, 0);
  std::vector<detail::sort_layout> lay(P);
  for (std::size_t k = 0; k < P; k++) {
    const int rk = static_cast<int>(z.rank[k]);
    detail::check(drhip_sort_pairs_workspace(rk, dt, vb, z.n[k], &wsb[k]), "drhip_sort_pairs_workspace");
    if (P > 1)
      detail::check(drhip_merge_pairs_workspace(rk, dt, vb, z.n[k], static_cast<int>(P), &mwsb[k]),
                    "drhip_merge_pairs_workspace");
    lay[k] = detail::radix_sort_layout<T>(wsb[k], mwsb[k], z.n[k], vb, z.ns[k], P);
  }
  const std::vector<char *> base = detail::carve_scratch(z.rank, lay);
  std::vector<T *> buf(P), smp(P);
  std::vector<V *> vbuf(P);
  for (std::size_t k = 0; k < P; k++) {
    buf[k] = lay[k].template at<T>(base[k], detail::SORT_BUF);
    vbuf[k] = lay[k].template at<V>(base[k], detail::SORT_VBUF);
    smp[k] = lay[k].template at<T>(base[k], detail::SORT_SMP);
  }
  // 1. local stable sorts of the pairs, then the regular key samples
  for (std::size_t k = 0; k < P; k++) {
    const int rk = static_cast<int>(z.rank[k]);
    if (z.n[k] > 1)
      detail::check(drhip_sort_pairs(rk, dt, z[k].data(), vparts[k].data(), vb, z.n[k],
                                     lay[k].at(base[k], detail::SORT_WS), wsb[k]),
                    "drhip_sort_pairs");
    if (P > 1) detail::check(drhip_sort_sample(rk, dt, z[k].data(), z.n[k], z.stride[k], smp[k]), "drhip_sort_sample");
  }
  if (P == 1) {
    sync(z.rank[0]);
    return;
  }
  // 2. exact splitting on the keys alone
  const std::vector<std::uint64_t> split = detail::exact_splits<T>(z, smp);
  // 3. pieces, keys and values by the same indices, in source order
  const auto offs = detail::move_pieces("shp::sort_by_key", z.rank, z.n, split,
                                        {detail::make_lane(z.parts, buf, "sort_by_key key piece copy"),
                                         detail::make_lane(vparts, vbuf, "sort_by_key value piece copy")});
  // 4. stable merge of the P runs straight into the key and value segments
  for (std::size_t k = 0; k < P; k++)
    detail::check(drhip_merge_pairs_runs_to(static_cast<int>(z.rank[k]), dt, vb, buf[k], vbuf[k], z[k].data(),
                                            vparts[k].data(), z.n[k], offs[k].data(), static_cast<int>(P),
                                            lay[k].at(base[k], detail::SORT_MWS), mwsb[k]),
                  "drhip_merge_pairs_runs_to");
  sync_all();
  }
}

template <typename ExecutionPolicy, lib::distributed_iterator KIter, lib::distributed_iterator VIter,
          typename Compare = std::ranges::less>
void sort_by_key(ExecutionPolicy &&policy, KIter keys_first, KIter keys_last, VIter values_first, Compare comp = {}) {
  shp::sort_by_key(std::forward<ExecutionPolicy>(policy), std::ranges::subrange(keys_first, keys_last),
                   std::ranges::subrange(values_first, values_first + (keys_last - keys_first)), comp);
}

} // namespace shp

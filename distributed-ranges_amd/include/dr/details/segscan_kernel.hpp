// segscan_kernel.hpp -- inclusive_scan_by_key / exclusive_scan_by_key for
// gfx950: every element receives the fold, in input order, of the values of
// its own run of consecutive equal keys up to itself (inclusive) or up to its
// predecessor, seeded with init (exclusive; a run's first element gets init).
// One template, included by the library (csrc/segscan.hip) and by the header
// layer (dr/shp/scan_by_key.hpp: any key equality and any associative op,
// instantiated in the user's translation unit).  C++17, no dependency beyond
// the HIP runtime and segreduce_kernel.hpp, whose tile shape, loads, head
// flags and in-tile segmented fold are reused unchanged.
//
// Tile = 256 threads x 8 slots x E elements, as segreduce_kernel.hpp: 8192
// elements for aligned 4-byte keys with 4-byte values, 4096 when either is 8
// bytes, 2048 in the element-load (accessor) form.
//
// One kernel, one workgroup per tile:
//   1. the tile index comes from an atomic counter in start order, so every
//      predecessor of a tile is already running (forward progress);
//   2. loads and head flags as the reduce: head[i] = (i == 0) ||
//      !eq(key[i-1], key[i]), the predecessor from the neighbour lane (DPP),
//      lane 0 of a wave reads keys[i-1] from the input, which nobody writes;
//   3. segmented inclusive fold inside the tile: thread-serial over a slot,
//      sr_wave_segscan across the wave, wave aggregates through LDS (every
//      wave scans the 32 aggregates for itself), the carry from piece to piece;
//   4. the tile's summary is {has_head, open}: open = the ACC fold of the
//      tile's last run (of the whole tile when it has no head).  The lifted
//      operator (a, b) -> b.has_head ? b : {a.has_head, op(a.open, b.open)} is
//      associative and not commutative.  A tile WITH a head publishes its
//      summary as final (INCL) at once: what it hands on does not depend on
//      its predecessors.  A head-less tile publishes AGG, looks back and
//      publishes INCL = op(carry, open).  Only a tile whose element 0 is not a
//      head looks back at all, for the carry of its leading elements, and the
//      look-back ends at the nearest predecessor that published INCL -- the
//      nearest tile with a head, or a head-less one that has finished its own
//      look-back.  Random keys: chains of length 1.  All keys equal: the plain
//      decoupled look-back scan;
//   5. wave 0 hands the carry over in LDS; every thread walks its elements
//      again with its in-tile carry, folds the tile's carry into the elements
//      before the tile's first head and stores.  Exclusive (compile-time): a
//      head gets init, any other element op(init, fold of its run before it).
//      No identity element is assumed anywhere;
//   6. stores: 16 bytes per slot (8 where the value is the narrower type) when
//      the tile is full and the output 16-byte aligned, element stores
//      otherwise.  sizeof K + 2 sizeof V bytes move per element.
// vals_out == vals_in is safe: a tile has loaded all it needs before it
// stores, and nobody reads another tile's values.
//
// Hand-off between workgroups (MI355X_MICROARCH "Valid forms", R2: the value
// IS the flag), the form of select_kernel.hpp and of dr/shp/scan.hpp's small
// values: per tile one granule on its own 128-byte line, one 8-byte word per
// 32 bits of ACC, {tag:32 | payload:32}, tag = status (none / aggregate /
// inclusive) | has_head << 2.  Every word is written by ONE agent-scope atomic
// store and read by ONE agent-scope atomic load; a two-word value is accepted
// when both words carry the same tag (a tile's value is fixed per tag, so
// words of two publications never pass for one).  Spins are bounded by
// select's limit and report through the error word.
//
// State = [256-byte head | one 128-byte granule per tile], zeroed by the
// caller on the stream before every launch (a memset node under capture, so a
// replay recomputes everything).  The head holds the tile counter (word 0)
// and what a caller that joins launches needs:
//   kSsFirstBreak (uint32): 0xFFFFFFFF - i for the smallest i > 0 with
//     !eq(k[i-1], k[i]); still 0 when there is none -- ss_first_break()
//     decodes it to i, or n;
//   kSsLastAcc (ACC): the inclusive fold of the launch's last run, unrounded,
//     also for an exclusive scan.
// Elements past n of a partial last tile count as heads for the fold (they cut
// the chain behind the last valid element) and are never stored.
#pragma once

#include "segreduce_kernel.hpp"

namespace dr_segscan {

using dr_segreduce::kSrSlots;
using dr_segreduce::sr_elem_type;
using dr_segreduce::sr_elems;
using dr_segreduce::sr_ptr_accessor;
using dr_segreduce::sr_tile;
using dr_segreduce::sr_tiles;
using dr_select::kSelHeadBytes;
using dr_select::kSelStride;
using dr_select::kSelThreads;
using dr_select::kSelWaves;

constexpr std::size_t kSsFirstBreak = 128, kSsLastAcc = 136; // in the 256-byte head
enum : unsigned { SS_NONE = 0, SS_AGG = 1, SS_INCL = 2, SS_STATUS = 3, SS_HEAD = 4 };

template <typename A> constexpr int ss_words = (int)(sizeof(A) / 4);

// bytes of state a launch of `ntiles` tiles uses, all of which the caller zeroes
inline std::size_t ss_state_bytes(std::size_t ntiles) { return kSelHeadBytes + ntiles * kSelStride; }
// the most a launch over n elements can need (the accessor form's tile count)
template <typename K, typename V> inline std::size_t ss_state_bytes_max(std::size_t n) {
  return ss_state_bytes(sr_tiles<K, V, false>(n));
}

struct ss_args {
  char *state;   // ss_state_bytes(ntiles), zeroed on the stream before the launch
  unsigned *err; // device-visible error word (dr_select::SEL_ERR_*)
};

// the first-break index a finished launch over n elements left in its state
__host__ __device__ inline std::size_t ss_first_break(const char *state, std::size_t n) {
  const unsigned w = *reinterpret_cast<const unsigned *>(state + kSsFirstBreak);
  return w ? (std::size_t)(0xFFFFFFFFu - w) : n;
}

template <typename A> __device__ __forceinline__ void ss_publish(char *state, long t, unsigned tag, const A &x) {
  unsigned w[ss_words<A>];
  __builtin_memcpy(w, &x, sizeof(A));
  std::uint64_t *g = dr_select::sel_word(state, t);
#pragma unroll
  for (int i = 0; i < ss_words<A>; i++)
    __hip_atomic_store(g + i, ((std::uint64_t)tag << 32) | w[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
// the tag of tile t's granule and its value; SS_NONE while the words are those of two publications
template <typename A> __device__ __forceinline__ unsigned ss_read(char *state, long t, A &x) {
  std::uint64_t *g = dr_select::sel_word(state, t);
  std::uint64_t r[ss_words<A>];
#pragma unroll
  for (int i = 0; i < ss_words<A>; i++) r[i] = __hip_atomic_load(g + i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  const unsigned tag = (unsigned)(r[0] >> 32);
  unsigned w[ss_words<A>];
  bool same = true;
#pragma unroll
  for (int i = 0; i < ss_words<A>; i++) {
    w[i] = (unsigned)r[i];
    same &= (unsigned)(r[i] >> 32) == tag;
  }
  __builtin_memcpy(&x, w, sizeof(A));
  return same ? tag : (unsigned)SS_NONE;
}

template <typename A> __device__ __forceinline__ A ss_shfl_xor(const A &x, int m) {
  unsigned w[ss_words<A>];
  __builtin_memcpy(w, &x, sizeof(A));
#pragma unroll
  for (int i = 0; i < ss_words<A>; i++) w[i] = (unsigned)__shfl_xor((int)w[i], m, 64);
  A r;
  __builtin_memcpy(&r, w, sizeof(A));
  return r;
}

// Wave 0 of a tile whose element 0 is not a head (so tile > 0): the fold of
// the run that is open when the tile begins, over the predecessors back to the
// nearest one that published INCL.  64 granules per step, folded in tile order
// by an ordered butterfly (higher lane = earlier tile on the left).  Tile 0
// always has a head, so the chain ends there at the latest.
template <typename A, typename Op> __device__ inline A ss_lookback(char *state, long tile, int lane, const Op &op, unsigned *err) {
  A acc{};
  bool has = false;
  long pred = tile - 1;
  unsigned spins = 0;
  while (true) {
    const long idx = pred - lane;
    A v{};
    unsigned st = SS_INCL; // before tile 0: nothing to wait for
    const bool valid = idx >= 0;
    if (valid) st = ss_read(state, idx, v) & SS_STATUS;
    const std::uint64_t incl = __ballot(st == SS_INCL);
    const int k = incl ? __builtin_ctzll(incl) : 64;
    const std::uint64_t upto = k >= 63 ? ~0ull : ((2ull << k) - 1ull); // lanes 0..k
    if (__ballot(st == SS_NONE) & upto) {
      if (++spins > dr_select::kSelSpinLimit) {
        if (lane == 0) __hip_atomic_fetch_or(err, dr_select::SEL_ERR_SPIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return acc;
      }
      __builtin_amdgcn_s_sleep(1);
      continue;
    }
    bool ok = valid && lane <= k;
#pragma unroll
    for (int m = 1; m < 64; m <<= 1) {
      const A pv = ss_shfl_xor(v, m);
      const bool pok = __shfl_xor((int)ok, m, 64) != 0;
      if (lane & m) { // this lane holds the earlier tiles
        if (ok && pok) v = op(v, pv);
        else if (pok) v = pv;
      } else {
        if (ok && pok) v = op(pv, v);
        else if (pok) v = pv;
      }
      ok = ok || pok;
    }
    if (ok) {
      acc = has ? op(v, acc) : v;
      has = true;
    }
    if (k < 64) break;
    pred -= 64;
  }
  return acc;
}

template <typename K, typename V, typename A, int E, int U, bool EXCL, typename KIn, typename VIn, typename Eq, typename Op>
__global__ __launch_bounds__(kSelThreads) void segscan_kernel(KIn kin, VIn vin, std::size_t n, V *out, bool vec_out, A init, Eq eq,
                                                              Op op, ss_args a) {
  using namespace dr_select;
  using namespace dr_segreduce;
  constexpr int NT = kSelThreads, NW = kSelWaves, NP = U * NW;
  constexpr std::size_t TILE = (std::size_t)NT * U * E;
  static_assert(NP <= 64, "one wave scans the piece aggregates");
  static_assert(U * E <= 64, "one flag bit per element of a thread");
  static_assert(sr_elem_type<K> && sr_elem_type<V>, "keys and values are 4 or 8 bytes, trivially copyable");
  static_assert(std::is_trivially_copyable<A>::value && (sizeof(A) == 4 || sizeof(A) == 8), "ACC is 4 or 8 bytes");
  __shared__ unsigned s_aggf[NP];
  __shared__ __attribute__((aligned(8))) unsigned char s_agg_raw[NP * sizeof(A)];
  __shared__ __attribute__((aligned(8))) unsigned char s_carry_raw[sizeof(A)];
  __shared__ unsigned s_tile, s_fh, s_lead;
  A *s_agg = reinterpret_cast<A *>(s_agg_raw);
  A *s_carry = reinterpret_cast<A *>(s_carry_raw);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const std::size_t ntiles = (n + TILE - 1) / TILE;

  if (tid == 0) {
    s_tile = atomicAdd(reinterpret_cast<unsigned *>(a.state), 1u);
    s_fh = ~0u;
  }
  __syncthreads();
  const std::size_t tile = s_tile;
  if (tile >= ntiles) { // a counter that did not start at 0: report, touch nothing
    if (tid == 0) __hip_atomic_fetch_or(a.err, SEL_ERR_CLAIM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    return;
  }
  const std::size_t base = tile * TILE;
  const bool full = base + TILE <= n;
  const unsigned rem = full ? (unsigned)TILE : (unsigned)(n - base);

  // ---- loads
  K k[U][E];
  V v[U][E];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    sr_load_slot<K, E>(kin, base + li, full, li, rem, k[u]);
  }
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    sr_load_slot<V, E>(vin, base + li, full, li, rem, v[u]);
  }
  // the predecessors only lane 0 of a wave cannot get from its neighbour
  K pk0[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    pk0[u] = k[u][0];
    if (lane == 0 && li < rem && base + li > 0) pk0[u] = sr_load_one<K>(kin, base + li - 1);
  }

  // ---- head flags, the values' slot and wave folds
  std::uint64_t hm = 0; // bit u * E + j: element (u, j) starts a fold (a run's head, or it lies past n)
  A ie[U];              // the wave's fold up to and including the lane below, per slot
  unsigned pbm = 0;     // bit u: a lower lane of this wave has a head in slot u
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    K prev = sr_shift_up1(k[u][E - 1]);
    if (lane == 0) prev = pk0[u];
    unsigned hb = 0, vb = 0; // heads and valid elements of this slot
#pragma unroll
    for (int j = 0; j < E; j++) {
      const bool valid = li + j < rem;
      const bool first = base + li + j == 0;
      const bool h = valid && (first || !eq(j ? k[u][j - 1] : prev, k[u][j]));
      hb |= (unsigned)h << j;
      vb |= (unsigned)valid << j;
    }
    asm volatile("" : "+v"(hb)); // the flags stay in a VGPR, not in E lane masks (select_kernel.hpp)
    const unsigned sb = hb | (~vb & ((1u << E) - 1u));
    hm |= (std::uint64_t)sb << (u * E);
    // the launch's first break: the lowest head of the piece, element 0 of the input apart
    const unsigned fb = base + li == 0 ? (hb & ~1u) : hb;
    const std::uint64_t rb = __ballot(fb != 0);
    if (fb != 0 && !(rb & ((1ull << lane) - 1ull))) atomicMin(&s_fh, li + (unsigned)__builtin_ctz(fb));
    A t = static_cast<A>(v[u][0]);
#pragma unroll
    for (int j = 1; j < E; j++) t = ((sb >> j) & 1u) ? static_cast<A>(v[u][j]) : op(t, static_cast<A>(v[u][j]));
    const std::uint64_t b = __ballot(sb != 0);
    const A incl = sr_wave_segscan(t, lane, sr_head_lane(b, lane), op);
    ie[u] = sr_shift_up1(incl);
    pbm |= (unsigned)((b & ((1ull << lane) - 1ull)) != 0) << u;
    if (lane == 63) {
      s_agg[u * NW + wid] = incl;
      s_aggf[u * NW + wid] = b != 0;
    }
  }
  if (tid == 0) s_lead = !(hm & 1ull); // the tile's leading elements continue a run of its predecessors
  __syncthreads();

  // ---- every wave: the segmented scan of the NP wave folds: pin[p] = the fold that is open at the end of piece p
  const bool pf = lane < NP ? s_aggf[lane] != 0 : true;
  const std::uint64_t pfb = __ballot(pf);
  const std::uint64_t ph = NP < 64 ? pfb & ((1ull << (NP & 63)) - 1ull) : pfb; // the pieces with a head
  const A pin = sr_wave_segscan(s_agg[lane < NP ? lane : 0], lane, sr_head_lane(pfb, lane), op);
  const bool lead = s_lead != 0; // block-uniform

  // ---- wave 0: publish, look back for the carry, publish
  if (wid == 0) {
    const A topen = sr_readlane(pin, NP - 1);
    if (lane == 0) ss_publish(a.state, (long)tile, ph ? (SS_INCL | SS_HEAD) : SS_AGG, topen);
    if (lead) {
      const A c = ss_lookback<A>(a.state, (long)tile, lane, op, a.err);
      if (lane == 0) {
        if (!ph) ss_publish(a.state, (long)tile, SS_INCL, op(c, topen));
        *s_carry = c;
      }
    }
    if (lane == 0 && s_fh != ~0u) {
      unsigned *w = reinterpret_cast<unsigned *>(a.state + kSsFirstBreak);
      const unsigned enc = 0xFFFFFFFFu - (unsigned)(base + s_fh); // n < 2^32: never 0
      if (__hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < enc)
        __hip_atomic_fetch_max(w, enc, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
  }
  A carry{};
  if (lead) {
    __syncthreads();
    carry = *s_carry;
  }

  // ---- the walk: every element's fold, the tile's carry into the elements before the first head, stores
  asm volatile("" : "+v"(hm));
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    const int p = u * NW + wid;
    // everything of the open run that lies before this slot in the tile
    A acc = ie[u];
    bool has = true;
    if (p > 0) {
      const A pc = sr_readlane(pin, p - 1);
      if (lane == 0) acc = pc;
      else if (!((pbm >> u) & 1u)) acc = op(pc, acc);
    } else if (lane == 0) {
      has = false;
    }
    if (lead && !(ph & ((1ull << p) - 1ull)) && !((pbm >> u) & 1u)) { // no head before this slot in the tile
      acc = has ? op(carry, acc) : carry;
      has = true;
    }
#pragma unroll
    for (int j = 0; j < E; j++) {
      const A x = static_cast<A>(v[u][j]);
      const bool h = ((hm >> (u * E + j)) & 1ull) || !has;
      if constexpr (EXCL) v[u][j] = static_cast<V>(h ? init : op(init, acc));
      acc = h ? x : op(acc, x);
      has = true;
      if constexpr (!EXCL) v[u][j] = static_cast<V>(acc);
      if (li + j == rem - 1 && tile == ntiles - 1) *reinterpret_cast<A *>(a.state + kSsLastAcc) = acc;
    }
    bool stored = false;
    if constexpr (E > 1) {
      if (full && vec_out) {
        if constexpr (E * sizeof(V) == 16) {
          sel_u32x4 w;
          __builtin_memcpy(&w, &v[u][0], 16);
          *reinterpret_cast<sel_u32x4 *>(out + base + li) = w;
        } else {
          static_assert(E * sizeof(V) == 8, "a slot of the narrower type is 8 bytes");
          unsigned long long w;
          __builtin_memcpy(&w, &v[u][0], 8);
          *reinterpret_cast<unsigned long long *>(out + base + li) = w;
        }
        stored = true;
      }
    }
    if (!stored) {
#pragma unroll
      for (int j = 0; j < E; j++)
        if (li + j < rem) out[base + li + j] = v[u][j];
    }
  }
}

// ------------------------------------------------------------------ host
// Enqueue one scan by key of n > 0 elements on `st`.  a.state: ss_state_bytes
// of the form's tile count; this function zeroes it.  init is read only by the
// exclusive form.
template <typename K, typename V, typename A, bool VEC, bool EXCL, int U = kSrSlots, typename KIn, typename VIn, typename Eq,
          typename Op>
inline hipError_t ss_launch(hipStream_t st, KIn kin, VIn vin, std::size_t n, V *out, A init, Eq eq, Op op, ss_args a) {
  constexpr int E = sr_elems<K, V, VEC>();
  const std::size_t ntiles = sr_tiles<K, V, VEC, U>(n);
  hipError_t e = hipMemsetAsync(a.state, 0, ss_state_bytes(ntiles), st);
  if (e != hipSuccess) return e;
  const bool vec_out = reinterpret_cast<std::uintptr_t>(out) % 16 == 0;
  hipLaunchKernelGGL((segscan_kernel<K, V, A, E, U, EXCL, KIn, VIn, Eq, Op>), dim3((unsigned)ntiles), dim3(kSelThreads), 0, st, kin,
                     vin, n, out, vec_out, init, eq, op, a);
  return hipGetLastError();
}

// contiguous keys and values: the 16-byte form when both spans are 16-byte aligned
template <typename K, typename V, typename A, bool EXCL, typename Eq, typename Op>
inline hipError_t ss_launch_spans(hipStream_t st, const K *kin, const V *vin, std::size_t n, V *out, A init, Eq eq, Op op, ss_args a) {
  if (dr_segreduce::sr_aligned16(kin) && dr_segreduce::sr_aligned16(vin))
    return ss_launch<K, V, A, true, EXCL>(st, kin, vin, n, out, init, eq, op, a);
  return ss_launch<K, V, A, false, EXCL>(st, sr_ptr_accessor<K>{kin}, sr_ptr_accessor<V>{vin}, n, out, init, eq, op, a);
}
// contiguous keys, values from an accessor (a transform view)
template <typename K, typename V, typename A, bool EXCL, typename VIn, typename Eq, typename Op>
inline hipError_t ss_launch_keys_span(hipStream_t st, const K *kin, VIn vin, std::size_t n, V *out, A init, Eq eq, Op op, ss_args a) {
  if (dr_segreduce::sr_aligned16(kin)) return ss_launch<K, V, A, true, EXCL>(st, kin, vin, n, out, init, eq, op, a);
  return ss_launch<K, V, A, false, EXCL>(st, sr_ptr_accessor<K>{kin}, vin, n, out, init, eq, op, a);
}

} // namespace dr_segscan

// select_kernel.hpp -- single-pass order-preserving selection (copy_if /
// count_if) for gfx950.  One template, included by the library
// (csrc/select.hip: the C-ABI's comparison and flag predicates) and by the
// header layer (dr/shp/select.hpp: any device callable, instantiated in the
// user's translation unit).  C++17, no dependency beyond the HIP runtime.
//
// Tile = 256 threads x U slots x V elements.  VEC: the input is a
// 16-byte-aligned contiguous span of T, V = 16 / sizeof(T) consecutive
// elements per slot, one 16-byte nontemporal load each, U = 16: 64 KiB of
// elements (16384 4-byte, 8192 8-byte); otherwise the input is an accessor
// (in(i)), V = 1, coalesced element loads, U <= 16 (4096 elements).  Element li of a tile sits in slot
// u = li / (256 V), thread (li / V) % 256, position j = li % V.
//   1. the tile index comes from an atomic counter in start order, so every
//      predecessor of a tile is already running (forward progress);
//   2. loads, the predicate per element (never on elements past n), one flag
//      bit per element in a 64-bit mask per thread;
//   3. in-tile ranks: per slot V ballots; mbcnt gives the flagged elements of
//      the lower lanes, popcount the wave's total, which goes to LDS; after
//      one barrier every wave scans the U x 4 wave totals (in element order)
//      for itself, in registers: piece prefixes and the tile's count;
//   4. wave 0 publishes the count, looks back over 64 predecessor tiles per
//      step and publishes its inclusive prefix; the last tile writes the
//      total (uint64) to a device-visible word;
//   5. SEL_STAGED: meanwhile every wave scatters its survivors into LDS at
//      their tile-local ranks (32 KiB of LDS: a VEC tile with more than half
//      its elements selected takes a second pass); after the second barrier
//      the survivors leave as one contiguous run out[excl, excl + count):
//      16-byte stores between a head and a tail of single elements.  SEL_DIRECT: after the
//      barrier every lane stores its survivors itself at excl + rank (each
//      wave instruction writes one contiguous run).  DESIGN.md "Selection"
//      has the measurement that chose between them.
// Nothing is written at or past out[total].
// Inter-workgroup hand-off (MI355X_MICROARCH "Valid forms", R2: the value IS
// the flag): one self-validating 8-byte word per tile, {status:32 |
// count:32}, written by ONE agent-scope atomic store and read by ONE
// agent-scope atomic load, one word per 128-byte line.  Only this word
// crosses workgroups -- no payload is handed over, so there is no
// release/acquire pair to get wrong.  Spins are bounded and report through
// the error word.  Counts are 32-bit: one launch takes n < 2^32.
// SEL_COUNT: the same loads and flags, no ranks, no look-back, no stores: a
// contiguous run of tiles per block, one 64-bit atomic add per block of
// {blocks done:24 | count:40}; the block that finds every other block done
// writes the total.
// State (tile counter, count word, status words) lives in `state`, zeroed by
// the caller on the stream before every launch (a memset node in a captured
// graph), so a replay recomputes everything.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace dr_select {

constexpr int kSelThreads = 256;
constexpr int kSelWaves = kSelThreads / 64;
constexpr std::size_t kSelTileBytes = 65536;    // VEC form
constexpr std::size_t kSelAccTileBytes = 32768; // accessor form
constexpr std::size_t kSelStageBytes = 32768;   // SEL_STAGED: survivors staged in LDS per pass
constexpr std::size_t kSelHeadBytes = 256; // word 0: tile counter; byte 64: SEL_COUNT's 64-bit word
constexpr std::size_t kSelCountWord = 64;
constexpr std::size_t kSelStride = 128;    // one status word per 128-byte line
constexpr unsigned kSelSpinLimit = 1u << 22;

enum : int { SEL_STAGED = 0, SEL_DIRECT = 1, SEL_COUNT = 2 };
// The store variant the library and the header layer ship.
#ifndef DR_SELECT_MODE
#define DR_SELECT_MODE 0
#endif
constexpr int kSelMode = DR_SELECT_MODE;
enum : unsigned { SEL_NONE = 0, SEL_AGG = 1, SEL_INCL = 2 };
enum : unsigned { SEL_ERR_SPIN = 1, SEL_ERR_CLAIM = 2 };

template <typename T> constexpr bool sel_vec_type = std::is_trivially_copyable<T>::value &&
                                                   (sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16);
// Slots per thread.  VEC: 16 slots of 16 bytes, a 64 KiB tile (16384 4-byte,
// 8192 8-byte elements) -- DESIGN.md "Selection": with 32 KiB tiles the claim
// and the look-back, paid once per tile, held the kernel at 2.4 TB/s.
// Accessor form: 32 KiB of elements, at most 16 slots (4096 elements up to
// 8-byte T; with 32 slots the ballot and branch masks overflow the SGPR file).
template <typename T, bool VEC> constexpr int sel_slots() {
  if (VEC) return (int)(kSelTileBytes / 16 / kSelThreads);
  constexpr std::size_t u = kSelAccTileBytes / sizeof(T) / kSelThreads;
  return u < 1 ? 1 : u > 16 ? 16 : (int)u;
}
template <typename T, bool VEC> constexpr std::size_t sel_tile() {
  return (std::size_t)kSelThreads * sel_slots<T, VEC>() * (VEC ? 16 / sizeof(T) : 1);
}
template <typename T, bool VEC> inline std::size_t sel_tiles(std::size_t n) {
  return (n + sel_tile<T, VEC>() - 1) / sel_tile<T, VEC>();
}
// bytes of state one launch over n elements of T uses at most (the accessor
// form's tile count), which the caller zeroes
template <typename T> inline std::size_t sel_state_bytes(std::size_t n) {
  return kSelHeadBytes + sel_tiles<T, false>(n) * kSelStride;
}

struct sel_args {
  char *state;               // sel_state_bytes, zeroed on the stream before the launch
  unsigned long long *total; // device-visible; receives the number selected
  unsigned *err;             // device-visible error word (SEL_ERR_*)
};

// contiguous input that is not 16-byte aligned, as an accessor
template <typename T> struct sel_ptr_accessor {
  const T *p;
  __device__ __forceinline__ T operator()(std::size_t i) const { return p[i]; }
};

typedef unsigned int sel_u32x4 __attribute__((ext_vector_type(4)));

template <int CTRL, int ROW_MASK> __device__ __forceinline__ unsigned sel_dpp(unsigned x) {
  // lanes without a source receive 0
  return (unsigned)__builtin_amdgcn_update_dpp(0, (int)x, CTRL, ROW_MASK, 0xf, false);
}
// inclusive +-scan across the 64 lanes (row_shr 1/2/4/8, row_bcast 15/31)
__device__ __forceinline__ unsigned sel_wave_scan(unsigned x) {
  x += sel_dpp<0x111, 0xf>(x);
  x += sel_dpp<0x112, 0xf>(x);
  x += sel_dpp<0x114, 0xf>(x);
  x += sel_dpp<0x118, 0xf>(x);
  x += sel_dpp<0x142, 0xa>(x);
  x += sel_dpp<0x143, 0xc>(x);
  return x;
}
__device__ __forceinline__ unsigned sel_wave_sum(unsigned x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) x += (unsigned)__shfl_xor((int)x, m, 64);
  return x;
}

__device__ __forceinline__ std::uint64_t *sel_word(char *state, long t) {
  return reinterpret_cast<std::uint64_t *>(state + kSelHeadBytes + (std::size_t)t * kSelStride);
}
__device__ __forceinline__ void sel_publish(char *state, long t, unsigned status, unsigned count) {
  __hip_atomic_store(sel_word(state, t), ((std::uint64_t)status << 32) | count, __ATOMIC_RELAXED,
                     __HIP_MEMORY_SCOPE_AGENT);
}

// Wave 0: the number selected in every tile before `tile`.
__device__ inline unsigned sel_lookback(char *state, long tile, int lane, unsigned *err) {
  unsigned excl = 0, spins = 0;
  long pred = tile - 1;
  while (true) {
    const long idx = pred - lane;
    unsigned val = 0, st = SEL_INCL; // tiles before 0: an inclusive 0
    if (idx >= 0) {
      const std::uint64_t w = __hip_atomic_load(sel_word(state, idx), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      val = (unsigned)w;
      st = (unsigned)(w >> 32);
    }
    // the nearest INCL, and whether any nearer word is still unset
    const std::uint64_t incl = __ballot(st == SEL_INCL);
    const std::uint64_t none = __ballot(st == SEL_NONE);
    const int k = incl ? __builtin_ctzll(incl) : 64;
    const std::uint64_t upto = k >= 63 ? ~0ull : ((2ull << k) - 1ull); // lanes 0..k
    if (none & upto) {
      if (++spins > kSelSpinLimit) {
        if (lane == 0) __hip_atomic_fetch_or(err, SEL_ERR_SPIN, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return excl;
      }
      __builtin_amdgcn_s_sleep(1);
      asm volatile("" ::: "memory"); // re-read every word next pass
      continue;
    }
    excl += sel_wave_sum(lane <= k ? val : 0u);
    if (k < 64) break;
    pred -= 64;
  }
  return excl;
}

// The tile's loads and flags: v holds the elements, the result has bit
// u * V + j set when element (u, j) exists and passes pred(value, index).
template <typename T, int V, int U, bool VEC, typename In, typename Pred>
__device__ __forceinline__ std::uint64_t sel_load(const In &in, std::size_t n, std::size_t base, int tid, const Pred &pred,
                                             T (&v)[U][V]) {
  constexpr int NT = kSelThreads;
  constexpr std::size_t TILE = (std::size_t)NT * U * V;
  static_assert(U * V <= 64, "one flag bit per element of a thread");
  const bool full = base + TILE <= n;
  const unsigned rem = full ? (unsigned)TILE : (unsigned)(n - base);
  std::uint64_t fm = 0;
  if constexpr (VEC) {
    const T *src = in + base;
    if (full) {
#pragma unroll
      for (int u = 0; u < U; u++) {
        const sel_u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const sel_u32x4 *>(src) + u * NT + tid);
        __builtin_memcpy(&v[u][0], &w, 16);
      }
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int j = 0; j < V; j++) {
          const unsigned li = ((unsigned)u * NT + tid) * V + j;
          if (pred(v[u][j], base + li)) fm |= 1ull << (u * V + j);
        }
    } else {
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int j = 0; j < V; j++) {
          const unsigned li = ((unsigned)u * NT + tid) * V + j;
          if (li < rem) {
            v[u][j] = src[li];
            if (pred(v[u][j], base + li)) fm |= 1ull << (u * V + j);
          }
        }
    }
  } else {
    static_assert(V == 1, "accessor form: one element per slot");
#pragma unroll
    for (int u = 0; u < U; u++) {
      const unsigned li = (unsigned)u * NT + tid;
      if (li < rem) {
        v[u][0] = static_cast<T>(in(base + li));
        if (pred(v[u][0], base + li)) fm |= 1ull << u;
      }
    }
  }
  return fm;
}

template <typename T, int V, int U, bool VEC, int MODE, typename In, typename Pred>
__global__ __launch_bounds__(kSelThreads) void select_kernel(In in, T *out, std::size_t n, Pred pred, sel_args a) {
  constexpr int NT = kSelThreads, NW = kSelWaves, NP = U * NW, NC = (NP + 63) / 64;
  constexpr std::size_t TILE = (std::size_t)NT * U * V;
  static_assert(std::is_trivially_copyable<T>::value, "selection moves elements as bits");
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const std::size_t ntiles = (n + TILE - 1) / TILE;

  if constexpr (MODE == SEL_COUNT) {
    __shared__ unsigned s_red[NW];
    unsigned c = 0;
    // block b counts the contiguous tiles [b * per, (b + 1) * per), as the
    // library's reduce walks its input
    const std::size_t per = (ntiles + gridDim.x - 1) / gridDim.x;
    const std::size_t t0 = blockIdx.x * per, t1 = t0 + per < ntiles ? t0 + per : ntiles;
    for (std::size_t tile = t0; tile < t1; tile++) {
      T v[U][V];
      c += (unsigned)__popcll(sel_load<T, V, U, VEC>(in, n, tile * TILE, tid, pred, v));
    }
    c = sel_wave_sum(c);
    if (lane == 0) s_red[wid] = c;
    __syncthreads();
    if (tid == 0) {
      unsigned long long sum = 0;
#pragma unroll
      for (int w = 0; w < NW; w++) sum += s_red[w];
      // one word carries the blocks done and the count, so the block that
      // sees every other block done also sees every other block's count
      const unsigned long long old =
          __hip_atomic_fetch_add(reinterpret_cast<unsigned long long *>(a.state + kSelCountWord), (1ull << 40) | sum,
                                 __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if ((old >> 40) == gridDim.x - 1) *a.total = (old & ((1ull << 40) - 1)) + sum;
    }
    return;
  } else {
    __shared__ unsigned s_wt[NP];
    __shared__ unsigned s_tile, s_excl;
    // SEL_STAGED: room for CAP survivors per pass
    constexpr unsigned CAP = TILE * sizeof(T) <= kSelStageBytes ? (unsigned)TILE : (unsigned)(kSelStageBytes / sizeof(T));
    constexpr bool STAGED = MODE == SEL_STAGED;
    constexpr std::size_t STAGE = STAGED ? (std::size_t)CAP * sizeof(T) : 16;
    __shared__ __attribute__((aligned(16))) unsigned char s_stage_raw[STAGE];
    T *stage = reinterpret_cast<T *>(s_stage_raw);

    if (tid == 0) s_tile = atomicAdd(reinterpret_cast<unsigned *>(a.state), 1u);
    __syncthreads();
    const std::size_t tile = s_tile;
    if (tile >= ntiles) { // a counter that did not start at 0: report, touch nothing
      if (tid == 0) __hip_atomic_fetch_or(a.err, SEL_ERR_CLAIM, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
      return;
    }
    T v[U][V];
    std::uint64_t fm = sel_load<T, V, U, VEC>(in, n, tile * TILE, tid, pred, v);
    // The flags live in these two VGPRs and nowhere else: without the opaque
    // copies (here and before the stores) the compiler keeps every element's
    // predicate as a lane mask in an SGPR pair from the load to the stores,
    // 128 SGPRs for a VEC tile, and spills them.
    asm volatile("" : "+v"(fm));

    // ---- ranks inside the wave, per slot; wave totals to LDS
    unsigned lp[U]; // flagged elements of the lower lanes in slot u
#pragma unroll
    for (int u = 0; u < U; u++) {
      unsigned p = 0, wt = 0;
#pragma unroll
      for (int j = 0; j < V; j++) {
        const std::uint64_t b = __ballot((int)((fm >> (u * V + j)) & 1ull));
        p = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, p));
        wt += (unsigned)__builtin_popcountll(b);
      }
      // the rank is formed here, not where it is used: sunk past the barrier,
      // the mbcnt pairs keep all U x V ballots alive in SGPR pairs (spills)
      asm volatile("" : "+v"(p));
      lp[u] = p;
      if (lane == 0) s_wt[u * NW + wid] = wt;
    }
    __syncthreads();

    // ---- every wave: exclusive scan of the NP wave totals in element order
    //      (piece u * NW + w), in registers; the tile's count
    unsigned ex[NC], agg = 0;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const int idx = c * 64 + lane;
      const unsigned pt = idx < NP ? s_wt[idx] : 0u;
      const unsigned incl = sel_wave_scan(pt);
      ex[c] = agg + incl - pt;
      agg += (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
    }
    // lp[u] becomes the tile-local rank of the thread's first survivor in slot u
#pragma unroll
    for (int u = 0; u < U; u++)
      lp[u] += (unsigned)__builtin_amdgcn_readlane((int)ex[(u * NW) >> 6], (u * NW + wid) & 63);

    // ---- wave 0: publish, look back, publish
    if (wid == 0) {
      unsigned excl = 0;
      if (tile == 0) {
        if (lane == 0) sel_publish(a.state, 0, SEL_INCL, agg);
      } else {
        if (lane == 0) sel_publish(a.state, (long)tile, SEL_AGG, agg);
        excl = sel_lookback(a.state, (long)tile, lane, a.err);
        if (lane == 0) sel_publish(a.state, (long)tile, SEL_INCL, excl + agg);
      }
      if (lane == 0) {
        s_excl = excl;
        if (tile == ntiles - 1) *a.total = (unsigned long long)excl + agg;
      }
    }

    asm volatile("" : "+v"(fm));
    if constexpr (STAGED) {
      // Survivors to LDS at their tile-local ranks, CAP of them per pass (one
      // pass up to half a VEC tile selected); the other waves make the first
      // pass while wave 0 looks back.  After the barrier the pass's survivors
      // leave as one contiguous run.
      const unsigned cnt = agg; // block-uniform
      for (unsigned off = 0; off < cnt; off += CAP) {
        if (off) __syncthreads(); // the pass before has been copied out
        std::uint64_t f = fm;
        asm volatile("" : "+v"(f)); // per pass: or the flag tests are hoisted out of the loop as lane masks
#pragma unroll
        for (int u = 0; u < U; u++) {
          unsigned r = lp[u] - off; // wraps for ranks of earlier passes
#pragma unroll
          for (int j = 0; j < V; j++)
            if ((f >> (u * V + j)) & 1ull) {
              if (r < CAP) stage[r] = v[u][j];
              r++;
            }
        }
        __syncthreads();
        T *dst = out + s_excl + off;
        const unsigned m = cnt - off < CAP ? cnt - off : CAP;
        constexpr int SV = sel_vec_type<T> ? 16 / sizeof(T) : 1;
        const std::uintptr_t ad = reinterpret_cast<std::uintptr_t>(dst);
        bool vec_out = false;
        if constexpr (SV > 1) vec_out = ad % sizeof(T) == 0;
        if constexpr (SV > 1) {
          if (vec_out) {
            // head up to the first 16-byte boundary, whole 16-byte stores, tail
            unsigned head = (unsigned)(((16 - (ad & 15)) & 15) / sizeof(T));
            if (head > m) head = m;
            if ((unsigned)tid < head) dst[tid] = stage[tid];
            const unsigned nvec = (m - head) / SV;
            for (unsigned k = tid; k < nvec; k += NT) {
              T t[SV];
#pragma unroll
              for (int j = 0; j < SV; j++) t[j] = stage[head + k * SV + j];
              sel_u32x4 w;
              __builtin_memcpy(&w, t, 16);
              *reinterpret_cast<sel_u32x4 *>(dst + head + k * SV) = w;
            }
            const unsigned t0 = head + nvec * SV;
            if (t0 + tid < m) dst[t0 + tid] = stage[t0 + tid];
          }
        }
        if (!vec_out)
          for (unsigned k = tid; k < m; k += NT) dst[k] = stage[k];
      }
    } else {
      __syncthreads();
      T *dst = out + s_excl;
#pragma unroll
      for (int u = 0; u < U; u++) {
        unsigned r = lp[u];
#pragma unroll
        for (int j = 0; j < V; j++)
          if ((fm >> (u * V + j)) & 1ull) dst[r++] = v[u][j];
      }
    }
  }
}

template <int = 0> __global__ void sel_write_total(unsigned long long *total, unsigned long long v) { *total = v; }

// ------------------------------------------------------------------ host
// Enqueue one selection (MODE SEL_STAGED / SEL_DIRECT) or count (SEL_COUNT)
// of n > 0 elements on `st`.  a.state must have been zeroed on `st` over
// sel_state_bytes<T>(n) bytes (SEL_COUNT: kSelHeadBytes suffice).  grid_cap:
// SEL_COUNT's grid limit (blocks), ignored otherwise.
template <typename T, int MODE, typename In, typename Pred>
inline hipError_t sel_launch_accessor(hipStream_t st, In in, T *out, std::size_t n, Pred pred, sel_args a,
                                      unsigned grid_cap) {
  constexpr int U = sel_slots<T, false>();
  const std::size_t ntiles = sel_tiles<T, false>(n);
  const unsigned grid = MODE == SEL_COUNT && ntiles > grid_cap ? grid_cap : (unsigned)ntiles;
  hipLaunchKernelGGL((select_kernel<T, 1, U, false, MODE, In, Pred>), dim3(grid), dim3(kSelThreads), 0, st, in, out, n,
                     pred, a);
  return hipGetLastError();
}
// contiguous input: the 16-byte form when `in` is 16-byte aligned and T is 4, 8 or 16 bytes
template <typename T, int MODE, typename Pred>
inline hipError_t sel_launch_span(hipStream_t st, const T *in, T *out, std::size_t n, Pred pred, sel_args a,
                                  unsigned grid_cap) {
  if constexpr (sel_vec_type<T>) {
    if (reinterpret_cast<std::uintptr_t>(in) % 16 == 0) {
      constexpr int V = 16 / sizeof(T), U = sel_slots<T, true>();
      const std::size_t ntiles = sel_tiles<T, true>(n);
      const unsigned grid = MODE == SEL_COUNT && ntiles > grid_cap ? grid_cap : (unsigned)ntiles;
      hipLaunchKernelGGL((select_kernel<T, V, U, true, MODE, const T *, Pred>), dim3(grid), dim3(kSelThreads), 0, st,
                         in, out, n, pred, a);
      return hipGetLastError();
    }
  }
  return sel_launch_accessor<T, MODE>(st, sel_ptr_accessor<T>{in}, out, n, pred, a, grid_cap);
}

} // namespace dr_select

// segreduce_kernel.hpp -- reduce_by_key / run_length_encode / unique_copy for
// gfx950: every maximal run of consecutive equal keys becomes one output key
// (the run's FIRST key) and one output value (the fold of the run's values in
// input order).  One template, included by the library (csrc/segreduce.hip)
// and by the header layer (dr/shp/reduce_by_key.hpp: any key equality and any
// associative op, instantiated in the user's translation unit).  C++17, no
// dependency beyond the HIP runtime and select_kernel.hpp, whose tile claim,
// status word and look-back are reused unchanged.
//
// Tile = 256 threads x 8 slots x E elements.  VEC: keys and values are
// 16-byte-aligned contiguous spans, E = 16 / max(sizeof K, sizeof V)
// consecutive elements per slot (the wider type takes one 16-byte nontemporal
// load per slot, the narrower one 8 bytes): 8192 elements for 4-byte keys
// with 4-byte values, 4096 otherwise.  Accessor form: E = 1, element loads,
// any alignment, 2048 elements.  Element li of a tile sits in slot
// u = li / (256 E), thread (li / E) % 256, position j = li % E; the 4 waves
// of slot u are pieces 4u .. 4u + 3 in element order.
//
// Main kernel, one workgroup per tile:
//   1. the tile index comes from an atomic counter in start order;
//   2. loads; head[i] = (i == 0) || !eq(key[i-1], key[i]).  The predecessor
//      of a thread's first element of a slot is its neighbour lane's last
//      (DPP); lane 0 of a wave loads it from the input (keys[i-1], which
//      nobody writes), and so does the tile's first element;
//   3. heads are ranked as select ranks survivors (ballots, mbcnt, wave totals
//      through LDS); wave 0 publishes the tile's head count, looks back and
//      publishes the inclusive count.  ONLY this 32-bit count crosses
//      workgroups inside the kernel -- values never ride the look-back;
//   4. segmented inclusive fold of the values: thread-serial over a slot's E
//      elements, a DPP wave scan that stops at the nearest head (known from
//      the ballot), wave aggregates through LDS (every wave scans the 32
//      aggregates for itself), the carry handed from piece to piece;
//   5. every thread walks its elements again with its carry: at a head of
//      tile-local rank r > 0 the finished run's fold goes to LDS slot r - 1,
//      the key to LDS slot r; both leave as contiguous runs
//      vals_out[excl, excl + count - 1) and keys_out[excl, excl + count);
//   6. the two open ends go to the tile's record in the state: lead = the fold
//      of the elements before the tile's first head (a head-less tile is all
//      lead), trail = the fold of the tile's last run;
//   7. the last tile writes the run count (uint64) to a device-visible word.
// Fix-up kernel, same stream, after the main kernel (the kernel boundary is
// the ordering): one workgroup makes a segmented scan over the tile records,
// 1024 at a time, and writes, for every tile t with a head, the value of the
// run that was open when t began (trail of the previous head tile, the leads
// of the head-less tiles between, t's own lead) to vals_out[excl_t - 1], and
// the last run's to vals_out[total - 1].  Each output slot has one writer, no
// atomics on values, input order kept: the op need not commute.
// HASV = false compiles values, records and fix-up out (unique_copy).
// Invalid elements of a partial last tile count as heads for the fold only
// (they cut the chain behind the last valid element) and never for the ranks.
// The fix-up also leaves the folds of the launch's first and last run in ACC
// in the state's head (kSrFirstAcc, kSrLastAcc): the header layer joins runs
// across segments from these, so such a run is rounded once too.
// State = [select's head and status words | one 32-byte record per tile],
// the head and status words zeroed by the caller on the stream before every
// launch (a memset node under capture, so a replay recomputes everything).
#pragma once

#include "select_kernel.hpp"

namespace dr_segreduce {

using dr_select::kSelHeadBytes;
using dr_select::kSelStride;
using dr_select::kSelThreads;
using dr_select::kSelWaves;

constexpr int kSrSlots = 8;
constexpr int kSrFixThreads = 1024;
constexpr std::size_t kSrRecordBytes = 32; // {flags:4 | pad:4 | lead:8 | trail:8 | pad:8}
// in select's 256-byte head: the folds of the launch's first and last run in ACC,
// before the rounding to the value type (what a caller that joins launches carries on)
constexpr std::size_t kSrFirstAcc = 128, kSrLastAcc = 136;
enum : unsigned { SR_HAS_HEAD = 1, SR_HAS_LEAD = 2 };

struct sr_none {}; // the value type of a keys-only launch

template <typename T> constexpr bool sr_elem_type = std::is_trivially_copyable<T>::value && (sizeof(T) == 4 || sizeof(T) == 8);
template <typename K, typename V> constexpr std::size_t sr_wide() {
  if (std::is_same<V, sr_none>::value) return sizeof(K);
  return sizeof(K) > sizeof(V) ? sizeof(K) : sizeof(V);
}
// elements per slot
template <typename K, typename V, bool VEC> constexpr int sr_elems() { return VEC ? (int)(16 / sr_wide<K, V>()) : 1; }
template <typename K, typename V, bool VEC, int U = kSrSlots> constexpr std::size_t sr_tile() {
  return (std::size_t)kSelThreads * U * sr_elems<K, V, VEC>();
}
template <typename K, typename V, bool VEC, int U = kSrSlots> inline std::size_t sr_tiles(std::size_t n) {
  return (n + sr_tile<K, V, VEC, U>() - 1) / sr_tile<K, V, VEC, U>();
}
// bytes the caller zeroes for a launch of `ntiles` tiles (a multiple of 16), and
// the whole state (the records follow the status words)
inline std::size_t sr_zero_bytes(std::size_t ntiles) { return kSelHeadBytes + ntiles * kSelStride; }
inline std::size_t sr_state_bytes(std::size_t ntiles) { return sr_zero_bytes(ntiles) + ntiles * kSrRecordBytes; }
// the most state a launch over n elements can need (the accessor form's tile count)
template <typename K, typename V> inline std::size_t sr_state_bytes_max(std::size_t n) {
  return sr_state_bytes(sr_tiles<K, V, false>(n));
}

struct sr_args {
  char *state;               // sr_state_bytes(ntiles); the first sr_zero_bytes zeroed on the stream
  unsigned long long *total; // device-visible; receives the number of runs
  unsigned *err;             // device-visible error word (dr_select::SEL_ERR_*)
};

template <typename T> struct sr_ptr_accessor {
  const T *p;
  __device__ __forceinline__ T operator()(std::size_t i) const { return p[i]; }
};
// run_length_encode's value stream: 1 per element, nothing read
struct sr_one_accessor {
  __device__ __forceinline__ unsigned long long operator()(std::size_t) const { return 1ull; }
};

// ---- DPP on any 4- or 8-byte trivially copyable type; a lane without a
// source keeps its own value (the callers test the lane index themselves)
template <int CTRL, int ROW_MASK, typename T> __device__ __forceinline__ T sr_dpp(const T &x) {
  static_assert(sizeof(T) == 4 || sizeof(T) == 8, "DPP moves 4- or 8-byte values");
  T r;
  if constexpr (sizeof(T) == 8) {
    unsigned w[2];
    __builtin_memcpy(w, &x, 8);
    w[0] = (unsigned)__builtin_amdgcn_update_dpp((int)w[0], (int)w[0], CTRL, ROW_MASK, 0xf, false);
    w[1] = (unsigned)__builtin_amdgcn_update_dpp((int)w[1], (int)w[1], CTRL, ROW_MASK, 0xf, false);
    __builtin_memcpy(&r, w, 8);
  } else {
    int w;
    __builtin_memcpy(&w, &x, 4);
    w = __builtin_amdgcn_update_dpp(w, w, CTRL, ROW_MASK, 0xf, false);
    __builtin_memcpy(&r, &w, 4);
  }
  return r;
}
// lane i receives lane i - 1's value (lane 0 keeps its own)
template <typename T> __device__ __forceinline__ T sr_shift_up1(const T &x) { return sr_dpp<0x138, 0xf>(x); }
// the value of lane `src` (wave-uniform)
template <typename T> __device__ __forceinline__ T sr_readlane(const T &x, int src) {
  T r;
  if constexpr (sizeof(T) == 8) {
    unsigned w[2];
    __builtin_memcpy(w, &x, 8);
    w[0] = (unsigned)__builtin_amdgcn_readlane((int)w[0], src);
    w[1] = (unsigned)__builtin_amdgcn_readlane((int)w[1], src);
    __builtin_memcpy(&r, w, 8);
  } else {
    int w;
    __builtin_memcpy(&w, &x, 4);
    w = __builtin_amdgcn_readlane(w, src);
    __builtin_memcpy(&r, &w, 4);
  }
  return r;
}

// the lane of the nearest head at or before `lane` in the ballot b, or 0
__device__ __forceinline__ int sr_head_lane(std::uint64_t b, int lane) {
  const std::uint64_t m = b & ((2ull << lane) - 1ull); // lane 63: 2 << 63 wraps to 0, the mask to all ones
  return m ? 63 - __builtin_clzll(m) : 0;
}

// Inclusive segmented scan across the 64 lanes: lane L receives the fold, in
// lane order, of x over [hl, L], hl = sr_head_lane (a wave without a head
// before L folds from lane 0).  Row shifts 1, 2, 4, 8, then row_bcast 15 / 31
// as the unsegmented scans of this library; a lane takes a step's source only
// when the source exists and lies at or behind its head.  Every lane of the
// wave must call this.
template <typename A, typename Op> __device__ __forceinline__ A sr_wave_segscan(A x, int lane, int hl, const Op &op) {
  const int rl = lane & 15;
  A s = sr_dpp<0x111, 0xf>(x);
  if (rl >= 1 && lane - 1 >= hl) x = op(s, x);
  s = sr_dpp<0x112, 0xf>(x);
  if (rl >= 2 && lane - 2 >= hl) x = op(s, x);
  s = sr_dpp<0x114, 0xf>(x);
  if (rl >= 4 && lane - 4 >= hl) x = op(s, x);
  s = sr_dpp<0x118, 0xf>(x);
  if (rl >= 8 && lane - 8 >= hl) x = op(s, x);
  s = sr_dpp<0x142, 0xa>(x); // lane 15 of row r - 1 to row r, r = 1, 3
  if ((lane & 16) && hl < (lane & ~15)) x = op(s, x);
  s = sr_dpp<0x143, 0xc>(x); // lane 31 to rows 2 and 3
  if (lane >= 32 && hl < 32) x = op(s, x);
  return x;
}

__device__ __forceinline__ char *sr_record(char *state, std::size_t ntiles, std::size_t t) {
  return state + kSelHeadBytes + ntiles * kSelStride + t * kSrRecordBytes;
}

// m elements of LDS to dst as one contiguous run: 16-byte stores between a
// head and a tail of single elements when dst is element-aligned
template <typename T> __device__ __forceinline__ void sr_copy_out(T *dst, const T *stage, unsigned m, int tid) {
  constexpr int NT = kSelThreads, SV = 16 / sizeof(T);
  const std::uintptr_t ad = reinterpret_cast<std::uintptr_t>(dst);
  if (ad % sizeof(T) == 0) {
    unsigned head = (unsigned)(((16 - (ad & 15)) & 15) / sizeof(T));
    if (head > m) head = m;
    if ((unsigned)tid < head) dst[tid] = stage[tid];
    const unsigned nvec = (m - head) / SV;
    for (unsigned k = tid; k < nvec; k += NT) {
      T t[SV];
#pragma unroll
      for (int j = 0; j < SV; j++) t[j] = stage[head + k * SV + j];
      dr_select::sel_u32x4 w;
      __builtin_memcpy(&w, t, 16);
      *reinterpret_cast<dr_select::sel_u32x4 *>(dst + head + k * SV) = w;
    }
    const unsigned t0 = head + nvec * SV;
    if (t0 + tid < m) dst[t0 + tid] = stage[t0 + tid];
  } else {
    for (unsigned k = tid; k < m; k += NT) dst[k] = stage[k];
  }
}

// E consecutive elements of a slot: one 16- or 8-byte nontemporal load from a
// pointer (full VEC tiles), element loads otherwise
template <typename T, int E, typename In>
__device__ __forceinline__ void sr_load_slot(const In &in, std::size_t g, bool full, unsigned li, unsigned rem, T (&x)[E]) {
  if constexpr (std::is_pointer<In>::value && E > 1) {
    if (full) {
      if constexpr (E * sizeof(T) == 16) {
        const dr_select::sel_u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const dr_select::sel_u32x4 *>(in + g));
        __builtin_memcpy(&x[0], &w, 16);
      } else {
        static_assert(E * sizeof(T) == 8, "a slot of the narrower type is 8 bytes");
        const unsigned long long w = __builtin_nontemporal_load(reinterpret_cast<const unsigned long long *>(in + g));
        __builtin_memcpy(&x[0], &w, 8);
      }
      return;
    }
  }
#pragma unroll
  for (int j = 0; j < E; j++) {
    if (li + j < rem) {
      if constexpr (std::is_pointer<In>::value) x[j] = in[g + j];
      else x[j] = static_cast<T>(in(g + j));
    } else {
      x[j] = T{};
    }
  }
}
template <typename T, typename In> __device__ __forceinline__ T sr_load_one(const In &in, std::size_t g) {
  if constexpr (std::is_pointer<In>::value) return in[g];
  else return static_cast<T>(in(g));
}

// what the stage holds when it is not the output type (run_length_encode: 4-byte counts in the tile, uint64 out)
template <typename T, typename S> __device__ __forceinline__ void sr_copy_out_as(T *dst, const S *stage, unsigned m, int tid) {
  if constexpr (std::is_same<T, S>::value) sr_copy_out(dst, stage, m, tid);
  else
    for (unsigned k = tid; k < m; k += kSelThreads) dst[k] = static_cast<T>(stage[k]);
}

// S: the type a finished run's fold is staged as -- V, or a narrower type that holds every in-launch result and
// is widened to V at the stores; the tile shape follows K and S.
template <typename K, typename V, typename A, typename S, int E, int U, bool HASV, typename KIn, typename VIn, typename Eq,
          typename Op>
__global__ __launch_bounds__(kSelThreads) void segreduce_kernel(KIn kin, VIn vin, std::size_t n, K *keys_out, V *vals_out,
                                                                Eq eq, Op op, sr_args a) {
  using namespace dr_select;
  constexpr int NT = kSelThreads, NW = kSelWaves, NP = U * NW;
  constexpr std::size_t TILE = (std::size_t)NT * U * E;
  static_assert(NP <= 64, "one wave scans the piece aggregates");
  static_assert(sr_elem_type<K>, "keys are 4 or 8 bytes, trivially copyable");
  constexpr std::size_t SB = HASV ? (sizeof(K) > sizeof(S) ? sizeof(K) : sizeof(S)) : sizeof(K);
  static_assert(std::is_same<S, V>::value || !std::is_pointer<VIn>::value, "a narrower stage type: values come from an accessor");
  __shared__ __attribute__((aligned(16))) unsigned char s_stage_raw[TILE * SB];
  __shared__ unsigned s_wt[NP];
  __shared__ unsigned s_aggf[HASV ? NP : 1];
  __shared__ __attribute__((aligned(8))) unsigned char s_agg_raw[(HASV ? NP : 1) * sizeof(A)];
  __shared__ unsigned s_tile, s_excl;
  A *s_agg = reinterpret_cast<A *>(s_agg_raw);

  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  const std::size_t ntiles = (n + TILE - 1) / TILE;

  if (tid == 0) s_tile = atomicAdd(reinterpret_cast<unsigned *>(a.state), 1u);
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
  V v[HASV ? U : 1][HASV ? E : 1];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    sr_load_slot<K, E>(kin, base + li, full, li, rem, k[u]);
  }
  if constexpr (HASV) {
#pragma unroll
    for (int u = 0; u < U; u++) {
      const unsigned li = ((unsigned)u * NT + tid) * E;
      sr_load_slot<V, E>(vin, base + li, full, li, rem, v[u]);
    }
  }
  // the predecessors only lane 0 of a wave cannot get from its neighbour
  K pk0[U];
#pragma unroll
  for (int u = 0; u < U; u++) {
    const unsigned li = ((unsigned)u * NT + tid) * E;
    pk0[u] = k[u][0];
    if (lane == 0 && li < rem && base + li > 0) pk0[u] = sr_load_one<K>(kin, base + li - 1);
  }

  // ---- head flags, ranks inside the wave, the values' slot and wave folds
  std::uint64_t hm = 0; // bit u * E + j: element (u, j) starts a run
  unsigned lp[U];       // heads of the lower lanes in slot u, later the tile-local rank of the thread's first
  A ie[HASV ? U : 1];   // the wave's fold up to and including the lane below, per slot
  unsigned pbm = 0;     // bit u: a lower lane of this wave has a (fold) head in slot u
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
    hm |= (std::uint64_t)hb << (u * E);
    unsigned p = 0, wt = 0;
#pragma unroll
    for (int j = 0; j < E; j++) {
      const std::uint64_t b = __ballot((int)((hb >> j) & 1u));
      p = __builtin_amdgcn_mbcnt_hi((unsigned)(b >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)b, p));
      wt += (unsigned)__builtin_popcountll(b);
    }
    asm volatile("" : "+v"(p));
    lp[u] = p;
    if (lane == 0) s_wt[u * NW + wid] = wt;
    if constexpr (HASV) {
      const unsigned sb = hb | (~vb & ((1u << E) - 1u)); // fold heads: the heads and what lies past n
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
  }
  __syncthreads();

  // ---- every wave: exclusive scan of the NP wave totals in element order
  unsigned agg;
  {
    const unsigned pt = lane < NP ? s_wt[lane] : 0u;
    const unsigned incl = sel_wave_scan(pt);
    const unsigned ex = incl - pt;
    agg = (unsigned)__builtin_amdgcn_readlane((int)incl, 63);
#pragma unroll
    for (int u = 0; u < U; u++) lp[u] += (unsigned)__builtin_amdgcn_readlane((int)ex, u * NW + wid);
  }
  // ---- and the segmented scan of the NP wave folds: pin[p] = the fold that is open at the end of piece p
  A pin{};
  if constexpr (HASV) {
    const bool pf = lane < NP ? s_aggf[lane] != 0 : true;
    const A px = s_agg[lane < NP ? lane : 0];
    pin = sr_wave_segscan(px, lane, sr_head_lane(__ballot(pf), lane), op);
  }

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

  asm volatile("" : "+v"(hm));
  if constexpr (HASV) {
    // ---- the walk: every finished run's fold to LDS at its rank, the open ends to the record
    S *stage = reinterpret_cast<S *>(s_stage_raw);
    char *rec = sr_record(a.state, ntiles, tile);
    if (tid == 0)
      *reinterpret_cast<unsigned *>(rec) = (agg ? SR_HAS_HEAD : 0u) | ((hm & 1ull) ? 0u : SR_HAS_LEAD);
#pragma unroll
    for (int u = 0; u < U; u++) {
      const unsigned li = ((unsigned)u * NT + tid) * E;
      const int p = u * NW + wid;
      // the carry: everything of the open run that lies before this slot in the tile
      A acc = ie[u];
      bool has = true;
      if (p > 0) {
        const A pc = sr_readlane(pin, p - 1);
        if (lane == 0) acc = pc;
        else if (!((pbm >> u) & 1u)) acc = op(pc, acc);
      } else if (lane == 0) {
        has = false;
      }
      unsigned r = lp[u];
#pragma unroll
      for (int j = 0; j < E; j++) {
        if ((hm >> (u * E + j)) & 1ull) {
          if (r) {
            stage[r - 1] = static_cast<S>(acc);
            if (r == 1 && tile == 0) *reinterpret_cast<A *>(a.state + kSrFirstAcc) = acc; // the launch's first run
          } else if (has) {
            *reinterpret_cast<A *>(rec + 8) = acc; // the lead
          }
          r++;
          acc = static_cast<A>(v[u][j]);
          has = true;
        } else { // what lies past n comes after the trail has been written
          acc = has ? op(acc, static_cast<A>(v[u][j])) : static_cast<A>(v[u][j]);
          has = true;
        }
        if (li + j == rem - 1) *reinterpret_cast<A *>(rec + (agg ? 16 : 8)) = acc; // the trail; a head-less tile is all lead
      }
    }
    __syncthreads();
    if (agg > 1) sr_copy_out_as(vals_out + s_excl, stage, agg - 1, tid);
    __syncthreads(); // the stage is reused for the keys
  }
  {
    K *stage = reinterpret_cast<K *>(s_stage_raw);
#pragma unroll
    for (int u = 0; u < U; u++) {
      unsigned r = lp[u];
#pragma unroll
      for (int j = 0; j < E; j++)
        if ((hm >> (u * E + j)) & 1ull) stage[r++] = k[u][j];
    }
    __syncthreads();
    if (agg) sr_copy_out(keys_out + s_excl, stage, agg, tid);
  }
}

// The fold of the tile records.  One workgroup; chunk c holds tiles
// [1024 c, 1024 c + 1024), one per thread.  A tile's item is (head =
// has_head, value = has_head ? trail : lead); the exclusive segmented scan at
// tile t is the run that is open when t begins.
template <typename V, typename A, typename Op>
__global__ __launch_bounds__(kSrFixThreads) void segreduce_fixup(char *state, std::size_t ntiles, V *vals_out, Op op) {
  constexpr int NT = kSrFixThreads, NW = NT / 64;
  __shared__ __attribute__((aligned(8))) unsigned char s_raw[2][(NW + 1) * sizeof(A)];
  __shared__ unsigned s_f[2][NW];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wid = __builtin_amdgcn_readfirstlane(tid >> 6);
  int it = 0;
  for (std::size_t c = 0; c < ntiles; c += NT, it ^= 1) {
    A *s_a = reinterpret_cast<A *>(s_raw[it]);           // wave folds of this chunk; s_a[NW]: the carry INTO this chunk
    A *s_next = reinterpret_cast<A *>(s_raw[it ^ 1]);
    const std::size_t t = c + tid;
    const bool valid = t < ntiles;
    unsigned fl = SR_HAS_HEAD; // past the end: a head, so nothing behind depends on it
    A val{}, lead{};
    if (valid) {
      const char *rec = sr_record(state, ntiles, t);
      fl = *reinterpret_cast<const unsigned *>(rec);
      if (fl & SR_HAS_LEAD) lead = *reinterpret_cast<const A *>(rec + 8);
      val = (fl & SR_HAS_HEAD) ? *reinterpret_cast<const A *>(rec + 16) : lead;
    }
    const bool hf = (fl & SR_HAS_HEAD) != 0;
    const std::uint64_t b = __ballot(hf);
    const A incl = sr_wave_segscan(val, lane, sr_head_lane(b, lane), op);
    const A ie = sr_shift_up1(incl);
    const bool pb = (b & ((1ull << lane) - 1ull)) != 0;
    if (lane == 63) {
      s_a[wid] = incl;
      s_f[it][wid] = b != 0;
    }
    __syncthreads();
    // the run open at the start of this wave: the chunk's carry and the waves before
    const bool wf = lane < NW ? s_f[it][lane] != 0 : true;
    const std::uint64_t wb = __ballot(wf);
    const A win = sr_wave_segscan(s_a[lane < NW ? lane : 0], lane, sr_head_lane(wb, lane), op);
    A wc = s_a[NW];
    bool has = c > 0;
    if (wid > 0) {
      const A pw = sr_readlane(win, wid - 1);
      const bool cut = (wb & ((1ull << wid) - 1ull)) != 0;
      wc = (has && !cut) ? op(wc, pw) : pw;
      has = true;
    }
    // ... and at the start of this tile
    A ex = wc;
    if (lane > 0) {
      ex = (has && !pb) ? op(wc, ie) : ie;
      has = true;
    }
    const A inc = (hf || !has) ? val : op(ex, val);
    if (valid) {
      if (hf && t > 0 && has) {
        const unsigned excl = (unsigned)*dr_select::sel_word(state, (long)t - 1); // the inclusive count of t - 1
        if (excl) {
          const A r = (fl & SR_HAS_LEAD) ? op(ex, lead) : ex;
          vals_out[excl - 1] = static_cast<V>(r);
          if (excl == 1) *reinterpret_cast<A *>(state + kSrFirstAcc) = r;
        }
      }
      if (t == ntiles - 1) {
        const unsigned total = (unsigned)*dr_select::sel_word(state, (long)t);
        if (total) {
          vals_out[total - 1] = static_cast<V>(inc);
          *reinterpret_cast<A *>(state + kSrLastAcc) = inc;
          if (total == 1) *reinterpret_cast<A *>(state + kSrFirstAcc) = inc;
        }
      }
    }
    if (tid == NT - 1) s_next[NW] = inc; // read after the next chunk's barrier
  }
}

// ------------------------------------------------------------------ host
// Enqueue one reduce_by_key of n > 0 elements on `st`.  a.state: sr_state_bytes
// of the form's tile count; this function zeroes what must be zero.  HASV =
// false: keys only (vin, vals_out and op unused, no fix-up).  U: slots per
// thread, the shipped kSrSlots unless a measurement asks for another shape.
template <typename K, typename V, typename A, bool VEC, bool HASV, int U = kSrSlots, typename S = V, typename KIn,
          typename VIn, typename Eq, typename Op>
inline hipError_t sr_launch(hipStream_t st, KIn kin, VIn vin, std::size_t n, K *keys_out, V *vals_out, Eq eq, Op op, sr_args a) {
  constexpr int E = sr_elems<K, S, VEC>();
  const std::size_t ntiles = sr_tiles<K, S, VEC, U>(n);
  hipError_t e = hipMemsetAsync(a.state, 0, sr_zero_bytes(ntiles), st);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL((segreduce_kernel<K, V, A, S, E, U, HASV, KIn, VIn, Eq, Op>), dim3((unsigned)ntiles), dim3(kSelThreads), 0, st, kin,
                     vin, n, keys_out, vals_out, eq, op, a);
  e = hipGetLastError();
  if (e != hipSuccess) return e;
  if constexpr (HASV) {
    hipLaunchKernelGGL((segreduce_fixup<V, A, Op>), dim3(1), dim3(kSrFixThreads), 0, st, a.state, ntiles, vals_out, op);
    e = hipGetLastError();
  }
  return e;
}

template <typename T> inline bool sr_aligned16(const T *p) { return reinterpret_cast<std::uintptr_t>(p) % 16 == 0; }

// contiguous keys and values: the 16-byte form when both spans are 16-byte aligned
template <typename K, typename V, typename A, typename Eq, typename Op>
inline hipError_t sr_launch_spans(hipStream_t st, const K *kin, const V *vin, std::size_t n, K *keys_out, V *vals_out, Eq eq, Op op,
                                  sr_args a) {
  if (sr_aligned16(kin) && sr_aligned16(vin))
    return sr_launch<K, V, A, true, true>(st, kin, vin, n, keys_out, vals_out, eq, op, a);
  return sr_launch<K, V, A, false, true>(st, sr_ptr_accessor<K>{kin}, sr_ptr_accessor<V>{vin}, n, keys_out, vals_out, eq, op, a);
}
// contiguous keys, values from an accessor (run_length_encode's constant 1, a transform view)
template <typename K, typename V, typename A, typename S = V, typename VIn, typename Eq, typename Op>
inline hipError_t sr_launch_keys_span(hipStream_t st, const K *kin, VIn vin, std::size_t n, K *keys_out, V *vals_out, Eq eq, Op op,
                                      sr_args a) {
  if (sr_aligned16(kin)) return sr_launch<K, V, A, true, true, kSrSlots, S>(st, kin, vin, n, keys_out, vals_out, eq, op, a);
  return sr_launch<K, V, A, false, true, kSrSlots, S>(st, sr_ptr_accessor<K>{kin}, vin, n, keys_out, vals_out, eq, op, a);
}
struct sr_no_op {
  __device__ __forceinline__ sr_none operator()(sr_none, sr_none) const { return {}; }
};
// keys only
template <typename K, typename Eq>
inline hipError_t sr_launch_unique(hipStream_t st, const K *kin, std::size_t n, K *keys_out, Eq eq, sr_args a) {
  if (sr_aligned16(kin))
    return sr_launch<K, sr_none, sr_none, true, false>(st, kin, (const sr_none *)nullptr, n, keys_out, (sr_none *)nullptr, eq,
                                                       sr_no_op{}, a);
  return sr_launch<K, sr_none, sr_none, false, false>(st, sr_ptr_accessor<K>{kin}, (const sr_none *)nullptr, n, keys_out,
                                                      (sr_none *)nullptr, eq, sr_no_op{}, a);
}

} // namespace dr_segreduce

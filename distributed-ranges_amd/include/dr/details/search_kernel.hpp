// search_kernel.hpp -- the algorithms that answer a question about a range
// with a position, for gfx950: first match (find_if, adjacent_find /
// is_sorted_until, mismatch) and arg-extremum (min / max / minmax_element).
// One template, included by the library (csrc/search.hip: the C-ABI's
// comparisons) and by the header layer (dr/shp/search.hpp: any device
// callable, instantiated in the user's translation unit).  C++17, no
// dependency beyond the HIP runtime.
//
// Tile = 256 threads x U slots x V elements, the loads of select_kernel.hpp.
// VEC: every input is a 16-byte-aligned contiguous span of T, V = 16 /
// sizeof(T) consecutive elements per slot, one 16-byte nontemporal load each,
// 64 KiB of elements per tile shared among the inputs (U = 16 with one input,
// 8 with two); otherwise the inputs are accessors (in(i)), V = 1, coalesced
// element loads, 32 KiB per tile, U <= 16.  A wave owns a contiguous run of
// the tile (U x 64 x V elements; every wave instruction still reads one
// contiguous stretch): element li sits in wave li / (U 64 V), slot
// (li / (64 V)) % U, lane (li / V) % 64, position li % V (srch_li).  Only
// whole tiles take this unrolled form; the last, partial tile of an input is
// walked by a rolled loop, 256 elements at a time (kept in the unrolled body,
// its guarded element loads set every kernel's register count and spilled
// lane masks).  Block b visits the tiles b,
// b + grid, b + 2 grid, ...: ascending, and the tiles in flight at any time
// are neighbours.  One launch takes n < 2^32.
//
// (a) search_first_kernel: the least i with pred(x[i], i) (SRCH_UNARY), with
//     pred(x[i], x[i+1]) for i < n - 1 (SRCH_ADJACENT) or with pred(a[i],
//     b[i]) (SRCH_TWO).  The result is ONE 64-bit word in `state`, all-ones
//     before the launch; a wave that finds matches in its part of a tile
//     folds them to their least index and does one agent-scope atomic min
//     into the word.  A wave stops at the first tile whose first index is
//     above a value it has read from the word (one relaxed agent-scope load
//     per tile, issued a tile ahead so that it never stalls the loads), and
//     after a hit of its own.  The word only ever decreases and only to
//     indices that match, so a tile is skipped only when a match below it is
//     recorded: the word ends as the exact minimum whatever the order and the
//     timing of the blocks.  No barrier, no spin, no look-back, no wait on
//     another workgroup; only the atomic word crosses workgroups.
//     SRCH_ADJACENT: the pair (i, i + 1) belongs to the tile of i.  The right
//     neighbour of a thread's last element in a slot is the next lane's first
//     (a DPP wave shift); for lane 63 it is lane 0's first element of the next
//     slot (a broadcast), and behind the wave's last slot the one element the
//     wave loads past its run, so the last pair of a wave and of a tile is
//     seen, the pair that straddles two tiles included.
//     srch_first_finish (one thread, the next launch on the stream) turns the
//     word into the caller's answer: `none` when it is still all-ones, else
//     word + add.  It is a launch of its own because the answer may live in
//     pinned host memory, where an atomic min does not belong.
// (b) search_extremum_kernel: under a strict weak order less(a, b), the first
//     least element (SRCH_MIN), the first greatest (SRCH_MAX), or the first
//     least and the LAST greatest in one pass (SRCH_MINMAX, the rule of
//     std::minmax_element).  A thread keeps {value, index} per end, seeded
//     with its own first element, and visits its elements in ascending index
//     order with one strict comparison each: less(x, cur) replaces the
//     minimum, less(cur, x) the first maximum, !less(x, cur) the last
//     maximum.  Every fold after that (64 lanes by shuffles, 4 waves through
//     LDS, the blocks' candidates in search_extremum_finish) goes through
//     srch_displaces, which compares the indices when neither value is less:
//     a candidate of a higher lane, a later tile or a later block never
//     displaces an equal earlier one (for the last maximum: a later one
//     always does).  Across blocks: every block writes its candidates to
//     `state` and search_extremum_finish, ONE block launched behind it on the
//     stream, folds them and writes the indices -- the kernel boundary is the
//     hand-off, nothing crosses workgroups inside a launch.  The finish can
//     also store the winners' values (srch_ext_args::value), which is how the
//     header layer gathers the pieces' winners.
// State lives in caller-provided device memory.  (a): kSrchHeadBytes, set to
// all-ones by hipMemsetAsync on the stream before every launch (a memset node
// in a captured graph), by the enqueue functions below.  (b): every word of
// srch_ext_state_bytes that a launch reads has been written by the launch
// before it on the stream, so there is nothing to clear and a replay
// recomputes everything.  No tile is claimed from a counter, so there is no
// error word.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace dr_search {

constexpr int kSrchThreads = 256;
constexpr int kSrchWaves = kSrchThreads / 64;
constexpr std::size_t kSrchTileBytes = 65536;    // VEC form, all inputs together
constexpr std::size_t kSrchAccTileBytes = 32768; // accessor form, all inputs together
constexpr std::size_t kSrchHeadBytes = 16;       // (a): the result word, padded to a 16-byte memset
constexpr unsigned long long kSrchNone = ~0ull;  // the result word before any hit
constexpr unsigned kSrchNoIndex = ~0u;           // (b): a candidate that holds no element

enum : int { SRCH_UNARY = 0, SRCH_ADJACENT = 1, SRCH_TWO = 2 };
enum : int { SRCH_MIN = 0, SRCH_MAX = 1, SRCH_MINMAX = 2 };
// the tie rule of a candidate (srch_displaces)
enum : int { SRCH_FIRST_LEAST = 0, SRCH_FIRST_GREATEST = 1, SRCH_LAST_GREATEST = 2 };

template <typename T> constexpr bool srch_vec_type = std::is_trivially_copyable<T>::value &&
                                                    (sizeof(T) == 4 || sizeof(T) == 8 || sizeof(T) == 16);
// Slots per thread with NIN inputs.
template <typename T, bool VEC, int NIN> constexpr int srch_slots() {
  if (VEC) return (int)(kSrchTileBytes / NIN / 16 / kSrchThreads);
  constexpr std::size_t u = kSrchAccTileBytes / NIN / sizeof(T) / kSrchThreads;
  return u < 1 ? 1 : u > 16 ? 16 : (int)u;
}
template <typename T, bool VEC, int NIN> constexpr std::size_t srch_tile() {
  return (std::size_t)kSrchThreads * srch_slots<T, VEC, NIN>() * (VEC ? 16 / sizeof(T) : 1);
}

// contiguous input that is not 16-byte aligned, as an accessor
template <typename T> struct srch_ptr_accessor {
  const T *p;
  __device__ __forceinline__ T operator()(std::size_t i) const { return p[i]; }
};

typedef unsigned int srch_u32x4 __attribute__((ext_vector_type(4)));

// x as 32-bit words (the last one padded), and back
template <typename T> struct srch_words {
  static constexpr int W = (int)((sizeof(T) + 3) / 4);
  unsigned w[W];
  __device__ __forceinline__ explicit srch_words(const T &x) {
#pragma unroll
    for (int k = 0; k < W; k++) w[k] = 0;
    __builtin_memcpy(w, &x, sizeof(T));
  }
  __device__ __forceinline__ T value() const {
    T r;
    __builtin_memcpy(&r, w, sizeof(T));
    return r;
  }
};
template <typename T> __device__ __forceinline__ T srch_shfl_xor(const T &x, int m) {
  srch_words<T> s(x);
#pragma unroll
  for (int k = 0; k < srch_words<T>::W; k++) s.w[k] = (unsigned)__shfl_xor((int)s.w[k], m, 64);
  return s.value();
}
// lane i receives lane i + 1's x (wave_shl:1); lane 63 keeps its own
template <typename T> __device__ __forceinline__ T srch_next_lane(const T &x) {
  srch_words<T> s(x);
#pragma unroll
  for (int k = 0; k < srch_words<T>::W; k++)
    s.w[k] = (unsigned)__builtin_amdgcn_update_dpp((int)s.w[k], (int)s.w[k], 0x130, 0xf, 0xf, false);
  return s.value();
}
__device__ __forceinline__ unsigned srch_wave_min(unsigned x) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const unsigned y = (unsigned)__shfl_xor((int)x, m, 64);
    x = y < x ? y : x;
  }
  return x;
}

// x as the compiler must take it here, in VGPRs: between two volatile statements nothing that uses x moves.
// The tile loops pin a slot's elements behind the slot before, so the predicates are evaluated slot by slot;
// left to itself the compiler compares all of a tile's elements first and keeps a lane mask per element in
// an SGPR pair (128 SGPRs for a tile of 4-byte elements), which spills.
template <typename T> __device__ __forceinline__ void srch_pin(T &x) {
  srch_words<T> s(x);
#pragma unroll
  for (int k = 0; k < srch_words<T>::W; k++) asm volatile("" : "+v"(s.w[k]));
  x = s.value();
}
// lane 0's x in every lane
template <typename T> __device__ __forceinline__ T srch_first_lane(const T &x) {
  srch_words<T> s(x);
#pragma unroll
  for (int k = 0; k < srch_words<T>::W; k++) s.w[k] = (unsigned)__builtin_amdgcn_readfirstlane((int)s.w[k]);
  return s.value();
}
// the tile-local index of position j in slot u of thread tid
template <int V, int U> __device__ __forceinline__ unsigned srch_li(int tid, int u, int j) {
  return ((((unsigned)tid >> 6) * U + u) * 64 + ((unsigned)tid & 63)) * V + j;
}

template <typename T, bool VEC, typename In> __device__ __forceinline__ T srch_elem(const In &in, std::size_t i) {
  if constexpr (VEC) return in[i];
  else return static_cast<T>(in(i));
}

// The loads of a whole tile: v[u][j] = element base + srch_li(tid, u, j).
template <typename T, int V, int U, bool VEC, typename In>
__device__ __forceinline__ void srch_load(const In &in, std::size_t base, int tid, T (&v)[U][V]) {
  if constexpr (VEC) {
    const T *src = in + base;
#pragma unroll
    for (int u = 0; u < U; u++) {
      const srch_u32x4 w =
          __builtin_nontemporal_load(reinterpret_cast<const srch_u32x4 *>(src) + srch_li<1, U>(tid, u, 0));
      __builtin_memcpy(&v[u][0], &w, 16);
    }
  } else {
    static_assert(V == 1, "accessor form: one element per slot");
#pragma unroll
    for (int u = 0; u < U; u++) v[u][0] = static_cast<T>(in(base + srch_li<1, U>(tid, u, 0)));
  }
}

// ------------------------------------------------------------ (a) first match

template <typename T, int V, int U, bool VEC, int KIND, typename In, typename In2, typename Pred>
__global__ __launch_bounds__(kSrchThreads) void search_first_kernel(In in, In2 in2, std::size_t n, Pred pred,
                                                                    unsigned long long *word) {
  constexpr int NT = kSrchThreads;
  constexpr std::size_t TILE = (std::size_t)NT * U * V;
  static_assert(std::is_trivially_copyable<T>::value, "elements are read as bits");
  const int tid = threadIdx.x, lane = tid & 63;
  // the positions that can match: a pair needs its right element
  const std::size_t m = KIND == SRCH_ADJACENT ? n - 1 : n;
  const std::size_t ntiles = (m + TILE - 1) / TILE;

  unsigned long long seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  for (std::size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const std::size_t base = tile * TILE;
    // wave-uniform: every lane loaded the same word with the same instruction
    const unsigned long long lim = ((unsigned long long)__builtin_amdgcn_readfirstlane((int)(seen >> 32)) << 32) |
                                   (unsigned)__builtin_amdgcn_readfirstlane((int)seen);
    if (lim < base) break; // a match below this tile, and below every later tile of this block, is recorded
    unsigned best = ~0u; // the thread's least matching position, tile-local
    if (base + TILE <= m) {
      // a whole tile of positions (SRCH_ADJACENT: the element behind it exists too)
      T v[U][V];
      srch_load<T, V, U, VEC>(in, base, tid, v);
      [[maybe_unused]] T v2[KIND == SRCH_TWO ? U : 1][V];
      if constexpr (KIND == SRCH_TWO) srch_load<T, V, U, VEC>(in2, base, tid, v2);
      [[maybe_unused]] T tail = v[0][0]; // SRCH_ADJACENT: the element behind the wave's run (wave-uniform)
      if constexpr (KIND == SRCH_ADJACENT) tail = srch_elem<T, VEC>(in, base + (std::size_t)((tid >> 6) + 1) * U * 64 * V);
      // for the next tile, behind this tile's loads
      seen = __hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
      for (int u = 0; u < U; u++) {
#pragma unroll
        for (int j = 0; j < V; j++) {
          srch_pin(v[u][j]);
          if constexpr (KIND == SRCH_TWO) srch_pin(v2[u][j]);
        }
        T nb = v[u][0]; // SRCH_ADJACENT: the element after the thread's last of this slot
        if constexpr (KIND == SRCH_ADJACENT) {
          nb = srch_next_lane(v[u][0]);
          const T behind = u + 1 < U ? srch_first_lane(v[u + 1 < U ? u + 1 : u][0]) : tail;
          if (lane == 63) nb = behind;
        }
#pragma unroll
        for (int j = 0; j < V; j++) {
          const unsigned li = srch_li<V, U>(tid, u, j);
          bool hit;
          if constexpr (KIND == SRCH_UNARY) hit = pred(v[u][j], base + li);
          else if constexpr (KIND == SRCH_TWO) hit = pred(v[u][j], v2[u][j]);
          else hit = pred(v[u][j], j + 1 < V ? v[u][(j + 1) % V] : nb);
          if (hit && li < best) best = li;
        }
        asm volatile("" : "+v"(best)); // the slot is done before the next one is pinned
      }
    } else {
      // the last, partial tile: position by position, 256 at a time
      const unsigned rem = (unsigned)(m - base);
#pragma unroll 1
      for (unsigned li = tid; li < rem; li += NT) {
        const T x = srch_elem<T, VEC>(in, base + li);
        bool hit;
        if constexpr (KIND == SRCH_UNARY) hit = pred(x, base + li);
        else if constexpr (KIND == SRCH_TWO) hit = pred(x, srch_elem<T, VEC>(in2, base + li));
        else hit = pred(x, srch_elem<T, VEC>(in, base + li + 1));
        if (hit && li < best) best = li;
      }
    }
    if (__ballot(best != ~0u)) {
      best = srch_wave_min(best);
      if (lane == 0) __hip_atomic_fetch_min(word, (unsigned long long)(base + best), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      break; // every later tile of this block lies above the hit
    }
  }
}

template <int = 0>
__global__ void srch_first_finish(const unsigned long long *word, unsigned long long none, unsigned long long add,
                                  unsigned long long *index) {
  const unsigned long long w = *word;
  *index = w == kSrchNone ? none : w + add;
}
// index[0, count) = v
template <int = 0> __global__ void srch_put(unsigned long long *index, int count, unsigned long long v) {
  if ((int)threadIdx.x < count) index[threadIdx.x] = v;
}

// --------------------------------------------------------- (b) arg-extremum

// Does candidate b displace candidate a?  Strict comparisons of the values;
// when neither is less the indices decide.
template <int RULE, typename T, typename Less>
__device__ __forceinline__ bool srch_displaces(const T &bv, unsigned bi, const T &av, unsigned ai, const Less &less) {
  if (bi == kSrchNoIndex) return false;
  if (ai == kSrchNoIndex) return true;
  if constexpr (RULE == SRCH_FIRST_LEAST) return less(bv, av) || (!less(av, bv) && bi < ai);
  else if constexpr (RULE == SRCH_FIRST_GREATEST) return less(av, bv) || (!less(bv, av) && bi < ai);
  else return less(av, bv) || (!less(bv, av) && bi > ai);
}
// x at index xi, above the index of cur
template <int RULE, typename T, typename Less>
__device__ __forceinline__ void srch_visit(const T &x, unsigned xi, T &cur, unsigned &ci, const Less &less) {
  bool t;
  if constexpr (RULE == SRCH_FIRST_LEAST) t = less(x, cur);
  else if constexpr (RULE == SRCH_FIRST_GREATEST) t = less(cur, x);
  else t = !less(x, cur);
  if (t) {
    cur = x;
    ci = xi;
  }
}

constexpr std::size_t srch_align16(std::size_t b) { return (b + 15) & ~std::size_t(15); }
// (b)'s state for a grid limit of `cap` blocks: per end `cap` values and `cap` indices
template <typename T> constexpr std::size_t srch_ext_state_bytes(unsigned cap) {
  return 2 * (srch_align16(cap * sizeof(T)) + srch_align16(cap * sizeof(unsigned)));
}
template <typename T> __device__ __forceinline__ char *srch_part_vals(char *state, unsigned cap, int e) {
  return state + e * (srch_align16(cap * sizeof(T)) + srch_align16(cap * sizeof(unsigned)));
}
template <typename T> __device__ __forceinline__ unsigned *srch_part_idx(char *state, unsigned cap, int e) {
  return reinterpret_cast<unsigned *>(srch_part_vals<T>(state, cap, e) + srch_align16(cap * sizeof(T)));
}

// The block's candidate of one end, in thread 0: 64 lanes by shuffles, the
// waves through LDS (s_val: kSrchWaves values as bytes, s_idx: kSrchWaves).
template <int RULE, typename T, typename Less>
__device__ __forceinline__ void srch_block_fold(T &v, unsigned &i, const Less &less, unsigned char *s_val, unsigned *s_idx) {
  const int tid = threadIdx.x;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    const T bv = srch_shfl_xor(v, m);
    const unsigned bi = (unsigned)__shfl_xor((int)i, m, 64);
    if (srch_displaces<RULE>(bv, bi, v, i, less)) {
      v = bv;
      i = bi;
    }
  }
  if ((tid & 63) == 0) {
    __builtin_memcpy(s_val + (tid >> 6) * sizeof(T), &v, sizeof(T));
    s_idx[tid >> 6] = i;
  }
  __syncthreads();
  if (tid == 0) {
#pragma unroll
    for (int w = 1; w < kSrchWaves; w++) {
      T bv;
      __builtin_memcpy(&bv, s_val + w * sizeof(T), sizeof(T));
      const unsigned bi = s_idx[w];
      if (srch_displaces<RULE>(bv, bi, v, i, less)) {
        v = bv;
        i = bi;
      }
    }
  }
}

template <int MODE> constexpr int srch_rule_a = MODE == SRCH_MAX ? SRCH_FIRST_GREATEST : SRCH_FIRST_LEAST;

template <typename T, int V, int U, bool VEC, int MODE, typename In, typename Less>
__global__ __launch_bounds__(kSrchThreads) void search_extremum_kernel(In in, std::size_t n, Less less, char *state,
                                                                       unsigned cap) {
  constexpr int NT = kSrchThreads;
  constexpr std::size_t TILE = (std::size_t)NT * U * V;
  constexpr int RA = srch_rule_a<MODE>, RB = SRCH_LAST_GREATEST;
  constexpr bool TWO = MODE == SRCH_MINMAX;
  static_assert(std::is_trivially_copyable<T>::value, "elements are read as bits");
  __shared__ __attribute__((aligned(16))) unsigned char s_val[2][kSrchWaves * sizeof(T)];
  __shared__ unsigned s_idx[2][kSrchWaves];
  const int tid = threadIdx.x;
  const std::size_t ntiles = (n + TILE - 1) / TILE;

  // the thread's lowest index seeds its candidates; a thread without it has no element at all
  const std::size_t base0 = blockIdx.x * TILE;
  const std::size_t first = base0 + (base0 + TILE <= n ? srch_li<V, U>(tid, 0, 0) : (unsigned)tid);
  T av, bv;
  unsigned ai = kSrchNoIndex, bi = kSrchNoIndex;
  if (first < n) {
    av = bv = srch_elem<T, VEC>(in, first);
    ai = bi = (unsigned)first;
  }
  for (std::size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const std::size_t base = tile * TILE;
    if (base + TILE <= n) {
      T v[U][V];
      srch_load<T, V, U, VEC>(in, base, tid, v);
#pragma unroll
      for (int u = 0; u < U; u++)
#pragma unroll
        for (int j = 0; j < V; j++) {
          const unsigned li = srch_li<V, U>(tid, u, j);
          srch_visit<RA>(v[u][j], (unsigned)(base + li), av, ai, less);
          if constexpr (TWO) srch_visit<RB>(v[u][j], (unsigned)(base + li), bv, bi, less);
        }
    } else {
      // the last, partial tile: element by element, 256 at a time
      const unsigned rem = (unsigned)(n - base);
#pragma unroll 1
      for (unsigned li = tid; li < rem; li += NT) {
        const T x = srch_elem<T, VEC>(in, base + li);
        srch_visit<RA>(x, (unsigned)(base + li), av, ai, less);
        if constexpr (TWO) srch_visit<RB>(x, (unsigned)(base + li), bv, bi, less);
      }
    }
  }
  srch_block_fold<RA>(av, ai, less, s_val[0], s_idx[0]);
  if constexpr (TWO) srch_block_fold<RB>(bv, bi, less, s_val[1], s_idx[1]);
  if (tid == 0) {
    __builtin_memcpy(srch_part_vals<T>(state, cap, 0) + blockIdx.x * sizeof(T), &av, sizeof(T));
    srch_part_idx<T>(state, cap, 0)[blockIdx.x] = ai;
    if constexpr (TWO) {
      __builtin_memcpy(srch_part_vals<T>(state, cap, 1) + blockIdx.x * sizeof(T), &bv, sizeof(T));
      srch_part_idx<T>(state, cap, 1)[blockIdx.x] = bi;
    }
  }
}

// One block: folds the `grid` block candidates of the launch before it;
// index[0] (and index[1], MINMAX's maximum) = the winners' indices, *value0 (and *value1) = their values
// where the pointer is not null.
template <typename T, int MODE, typename Less>
__global__ __launch_bounds__(kSrchThreads) void search_extremum_finish(char *state, unsigned cap, unsigned grid, Less less,
                                                                       unsigned long long *index, T *value0, T *value1) {
  constexpr int RA = srch_rule_a<MODE>, RB = SRCH_LAST_GREATEST;
  constexpr bool TWO = MODE == SRCH_MINMAX;
  __shared__ __attribute__((aligned(16))) unsigned char s_val[2][kSrchWaves * sizeof(T)];
  __shared__ unsigned s_idx[2][kSrchWaves];
  const int tid = threadIdx.x;
  T cv[2];
  unsigned ci[2] = {kSrchNoIndex, kSrchNoIndex};
#pragma unroll
  for (int e = 0; e < (TWO ? 2 : 1); e++) {
    const char *pv = srch_part_vals<T>(state, cap, e);
    const unsigned *pi = srch_part_idx<T>(state, cap, e);
    for (unsigned g = tid; g < grid; g += kSrchThreads) {
      T bv;
      __builtin_memcpy(&bv, pv + (std::size_t)g * sizeof(T), sizeof(T));
      const unsigned bi = pi[g];
      const bool t = e == 0 ? srch_displaces<RA>(bv, bi, cv[e], ci[e], less) : srch_displaces<RB>(bv, bi, cv[e], ci[e], less);
      if (t) {
        cv[e] = bv;
        ci[e] = bi;
      }
    }
  }
  srch_block_fold<RA>(cv[0], ci[0], less, s_val[0], s_idx[0]);
  if constexpr (TWO) srch_block_fold<RB>(cv[1], ci[1], less, s_val[1], s_idx[1]);
  if (tid == 0) {
    index[0] = ci[0];
    if (value0) *value0 = cv[0];
    if constexpr (TWO) {
      index[1] = ci[1];
      if (value1) *value1 = cv[1];
    }
  }
}

// ------------------------------------------------------------------ host
// The enqueue functions put everything one call needs on `st`: the state
// clear, the kernel and its finish.

struct srch_first_args {
  char *state;                   // device memory, kSrchHeadBytes
  unsigned long long *index;     // device-visible; receives the answer
  unsigned long long none;       // the answer without a match
  unsigned long long add;        // added to a match's position (is_sorted_until: 1)
  unsigned grid_cap;             // grid limit, blocks
};
struct srch_ext_args {
  char *state;               // device memory, srch_ext_state_bytes<T>(grid_cap)
  unsigned long long *index; // device-visible; receives one index (MINMAX: two)
  unsigned grid_cap;
  void *value[2] = {nullptr, nullptr}; // device-visible or null; receive the winners' values (T)
};

template <typename T, int KIND, int V, int U, bool VEC, typename In, typename In2, typename Pred>
inline hipError_t srch_first_enqueue(hipStream_t st, In in, In2 in2, std::size_t n, Pred pred, const srch_first_args &a) {
  constexpr std::size_t TILE = (std::size_t)kSrchThreads * U * V;
  const std::size_t m = KIND == SRCH_ADJACENT ? (n ? n - 1 : 0) : n;
  if (m == 0) { // nothing can match: the answer alone
    hipLaunchKernelGGL(srch_put<0>, dim3(1), dim3(64), 0, st, a.index, 1, a.none);
    return hipGetLastError();
  }
  unsigned long long *word = reinterpret_cast<unsigned long long *>(a.state);
  if (hipError_t e = hipMemsetAsync(a.state, 0xFF, kSrchHeadBytes, st); e != hipSuccess) return e;
  const std::size_t ntiles = (m + TILE - 1) / TILE;
  const unsigned grid = ntiles > a.grid_cap ? a.grid_cap : (unsigned)ntiles;
  hipLaunchKernelGGL((search_first_kernel<T, V, U, VEC, KIND, In, In2, Pred>), dim3(grid), dim3(kSrchThreads), 0, st, in,
                     in2, n, pred, word);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL(srch_first_finish<0>, dim3(1), dim3(1), 0, st, (const unsigned long long *)word, a.none, a.add,
                     a.index);
  return hipGetLastError();
}
// accessor inputs (in2 is read by SRCH_TWO only; pass `in` again otherwise)
template <typename T, int KIND, typename In, typename In2, typename Pred>
inline hipError_t srch_first_accessor(hipStream_t st, In in, In2 in2, std::size_t n, Pred pred, const srch_first_args &a) {
  constexpr int NIN = KIND == SRCH_TWO ? 2 : 1;
  return srch_first_enqueue<T, KIND, 1, srch_slots<T, false, NIN>(), false>(st, in, in2, n, pred, a);
}
// contiguous inputs: the 16-byte form when every input is 16-byte aligned and T is 4, 8 or 16 bytes
template <typename T, int KIND, typename Pred>
inline hipError_t srch_first_span(hipStream_t st, const T *in, const T *in2, std::size_t n, Pred pred,
                                  const srch_first_args &a) {
  constexpr int NIN = KIND == SRCH_TWO ? 2 : 1;
  if (KIND != SRCH_TWO) in2 = in;
  if constexpr (srch_vec_type<T>) {
    if ((reinterpret_cast<std::uintptr_t>(in) | reinterpret_cast<std::uintptr_t>(in2)) % 16 == 0)
      return srch_first_enqueue<T, KIND, 16 / sizeof(T), srch_slots<T, true, NIN>(), true>(st, in, in2, n, pred, a);
  }
  return srch_first_accessor<T, KIND>(st, srch_ptr_accessor<T>{in}, srch_ptr_accessor<T>{in2}, n, pred, a);
}

template <typename T, int MODE, int V, int U, bool VEC, typename In, typename Less>
inline hipError_t srch_extremum_enqueue(hipStream_t st, In in, std::size_t n, Less less, const srch_ext_args &a) {
  constexpr std::size_t TILE = (std::size_t)kSrchThreads * U * V;
  if (n == 0) { // std: end(), which is 0
    hipLaunchKernelGGL(srch_put<0>, dim3(1), dim3(64), 0, st, a.index, MODE == SRCH_MINMAX ? 2 : 1, 0ull);
    return hipGetLastError();
  }
  const std::size_t ntiles = (n + TILE - 1) / TILE;
  const unsigned grid = ntiles > a.grid_cap ? a.grid_cap : (unsigned)ntiles;
  hipLaunchKernelGGL((search_extremum_kernel<T, V, U, VEC, MODE, In, Less>), dim3(grid), dim3(kSrchThreads), 0, st, in, n,
                     less, a.state, a.grid_cap);
  if (hipError_t e = hipGetLastError(); e != hipSuccess) return e;
  hipLaunchKernelGGL((search_extremum_finish<T, MODE, Less>), dim3(1), dim3(kSrchThreads), 0, st, a.state, a.grid_cap, grid,
                     less, a.index, static_cast<T *>(a.value[0]), static_cast<T *>(a.value[1]));
  return hipGetLastError();
}
template <typename T, int MODE, typename In, typename Less>
inline hipError_t srch_extremum_accessor(hipStream_t st, In in, std::size_t n, Less less, const srch_ext_args &a) {
  return srch_extremum_enqueue<T, MODE, 1, srch_slots<T, false, 1>(), false>(st, in, n, less, a);
}
template <typename T, int MODE, typename Less>
inline hipError_t srch_extremum_span(hipStream_t st, const T *in, std::size_t n, Less less, const srch_ext_args &a) {
  if constexpr (srch_vec_type<T>) {
    if (reinterpret_cast<std::uintptr_t>(in) % 16 == 0)
      return srch_extremum_enqueue<T, MODE, 16 / sizeof(T), srch_slots<T, true, 1>(), true>(st, in, n, less, a);
  }
  return srch_extremum_accessor<T, MODE>(st, srch_ptr_accessor<T>{in}, n, less, a);
}

} // namespace dr_search

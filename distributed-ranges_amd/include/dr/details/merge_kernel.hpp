// merge_kernel.hpp -- the stable merge of two sorted sequences, for gfx950:
// std::merge(A, B, comp), optionally carrying one value per key (merge_by_key).
// One template, included by the library (csrc/merge.hip: the C-ABI's six
// dtypes under <, values of 4 or 8 bytes) and by the header layer
// (dr/shp/merge.hpp: any trivially copyable element and value, any device
// callable, instantiated in the user's translation unit).  C++17, no
// dependency beyond the HIP runtime.
//
// Contract.  A (na elements) and B (nb elements) are callables g -> element
// over 64-bit global indices (mg_ptr, or dr_bsearch's bs_one / bs_table: a
// virtual concatenation of pieces), each sorted under comp.  Output element d
// of the na + nb diagonals is element d of std::merge(A, B, comp): on ties A's
// element comes first and each input keeps its own order (the lower-bound
// form of the merge path).  A launch receives a window [d0, d1) of the
// diagonals and the destination of that window, so every piece of a segmented
// output is one launch over the same A and B.
//
// The merge path.  split(d) = the number of A's elements among the first d
// outputs = the least i in [max(0, d - nb), min(d, na)] for which
// comp(B[d - 1 - i], A[i]) holds (or the interval's end).  mg_split finds it
// with the 64 lanes of one wave: the interval is cut into at most 64 chunks,
// every lane probes the last index of its chunk, the count of lanes whose
// probe lies left of the split (one ballot) names the chunk that holds it --
// 64-ary instead of binary, 5 dependent rounds of global loads for 2^28
// elements instead of 28.  Every round shrinks the interval strictly and every
// probe index lies inside it, so whatever the data (unsorted, NaNs) the loop
// ends, the split is in range and no read leaves A[0, na) or B[0, nb).
//
// The kernel.  Workgroups of 256 threads; a tile is mg_tile<T, V>() outputs
// (256 x 8 for elements of up to 8 bytes, fewer items per thread above, and
// never more than fits the LDS budget).  Workgroups are persistent over a
// CONTIGUOUS run of tiles: wave 0 searches the split of the run's first
// diagonal once (global indices, 64-bit) and then, per tile, only the end
// split -- which lies at most one tile beyond the start split, so that search
// is 2 rounds over the very elements the tile is about to stream -- and the
// end split is the next tile's start.  Per tile (everything 32-bit from here):
//   1. A's piece then B's piece go to padded LDS (one pad element per 8), all
//      of a thread's loads issued before its first LDS store; values likewise,
//      in the same staged order;
//   2. every thread takes its diagonal's split in LDS (binary, 32-bit) and
//      merges its items serially into registers, the two heads held in
//      registers (one LDS read per output); for each output it keeps the
//      staged rank it took (A's rank, or la + B's rank) and, with values,
//      fetches the value at that rank from LDS;
//   3. keys (and values) go back through LDS in output order and leave as
//      coalesced nontemporal stores: 16 bytes per lane for whole tiles when
//      the elements are 4 or 8 bytes wide and the destination is 16-byte
//      aligned (VEC), element stores otherwise.
// Staging loads through mg_ptr are nontemporal (each element is read once);
// the split probes are ordinary loads and warm the lines the staging reads.
//
// No state: the kernel reads A and B (and their values) and writes exactly
// out[0, d1 - d0), each element once -- no workspace, no partition array, no
// counters, no word that crosses workgroups.  A captured launch replays as is.
// Unsorted inputs or NaNs give unspecified output values, within those bounds.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace dr_merge {

constexpr int kMgThreads = 256;
// outputs per tile, by element width (256 threads x 8 items; DESIGN.md "Merge" records the sweep)
constexpr unsigned kMgTile4 = 2048; // elements of up to 4 bytes
constexpr unsigned kMgTile8 = 2048; // elements of 8 bytes
constexpr std::size_t kMgLdsBytes = 24576; // wider elements and values: what a tile's keys, and its values, may take
constexpr std::size_t kMgMaxElem = 4096;   // the widest element or value

struct mg_none {}; // no values
template <typename V> constexpr bool mg_has = !std::is_same<V, mg_none>::value;

template <typename T, typename V = mg_none, unsigned T4 = kMgTile4, unsigned T8 = kMgTile8> constexpr unsigned mg_tile() {
  const std::size_t ipt = sizeof(T) <= 4 ? T4 / kMgThreads : sizeof(T) <= 8 ? T8 / kMgThreads : sizeof(T) <= 16 ? 4
                          : sizeof(T) <= 32 ? 2 : 1;
  std::size_t t = ipt * kMgThreads;
  if (sizeof(T) > 8 && t * sizeof(T) > kMgLdsBytes) t = kMgLdsBytes / sizeof(T);
  if (mg_has<V> && t * sizeof(V) > kMgLdsBytes) t = kMgLdsBytes / sizeof(V);
  return (unsigned)t;
}
constexpr unsigned kMgPad = 8; // one pad element after every 8
__host__ __device__ constexpr unsigned mg_padded(unsigned e) { return e + e / kMgPad; }

struct mg_less {
  template <typename A, typename B> __device__ __forceinline__ bool operator()(const A &a, const B &b) const { return a < b; }
};

// contiguous elements: ordinary loads for the probes, nontemporal ones for the staging
template <typename T> struct mg_ptr {
  const T *p;
  __device__ __forceinline__ T operator()(std::size_t g) const { return p[g]; }
  __device__ __forceinline__ T stream(std::size_t g) const {
    if constexpr (std::is_arithmetic<T>::value) return __builtin_nontemporal_load(p + g);
    else return p[g];
  }
};
template <typename X> constexpr bool mg_is_ptr = false;
template <typename T> constexpr bool mg_is_ptr<mg_ptr<T>> = true;
template <typename T, typename F> __device__ __forceinline__ T mg_stream(const F &f, std::size_t g) {
  if constexpr (mg_is_ptr<F>) return f.stream(g);
  else return static_cast<T>(f(g));
}
// the accessor of absent values
struct mg_no_values {
  __device__ __forceinline__ mg_none operator()(std::size_t) const { return {}; }
};

typedef unsigned int mg_u32x4 __attribute__((ext_vector_type(4)));
using mg_idx = unsigned long long;

// split(diag) in [lo, hi], by the 64 lanes of one wave (all active; lo and hi wave-uniform).  Probes stay in
// A[lo, hi) and B[diag - hi, diag - lo): the caller's interval keeps those inside the inputs.
template <typename T, typename FA, typename FB, typename Comp>
__device__ inline mg_idx mg_split(const FA &A, const FB &B, mg_idx diag, mg_idx lo, mg_idx hi, const Comp &comp, unsigned lane) {
  while (lo < hi) {
    const mg_idx stride = (hi - lo + 63) / 64; // chunk `lane` = [lo + lane * stride, ...) cut at hi
    const mg_idx first = lo + lane * stride;
    const bool valid = first < hi;
    mg_idx m = first + (stride - 1); // the chunk's last index
    if (!valid || m > hi - 1) m = hi - 1;
    const T a = static_cast<T>(A((std::size_t)m));
    const T b = static_cast<T>(B((std::size_t)(diag - 1 - m)));
    const bool left = valid && !static_cast<bool>(comp(b, a)); // the split lies beyond m
    const unsigned c = (unsigned)__popcll(__ballot(left));
    const mg_idx nlo = lo + c * stride; // the chunk that holds the split
    if (nlo >= hi) {
      lo = hi;
    } else {
      mg_idx nhi = nlo + (stride - 1);
      if (nhi > hi - 1) nhi = hi - 1;
      lo = nlo;
      hi = nhi;
    }
  }
  return lo;
}

// A tile in LDS, indexed through the padding.
template <typename T> struct mg_lds {
  unsigned char *raw;
  __device__ __forceinline__ T get(unsigned j) const {
    T x;
    __builtin_memcpy(&x, raw + (std::size_t)(j + j / kMgPad) * sizeof(T), sizeof(T));
    return x;
  }
  __device__ __forceinline__ void put(unsigned j, const T &x) const {
    __builtin_memcpy(raw + (std::size_t)(j + j / kMgPad) * sizeof(T), &x, sizeof(T));
  }
};

// cnt elements of the tile in LDS to dst, coalesced
template <typename T, bool VEC, unsigned TILE>
__device__ __forceinline__ void mg_store_tile(const mg_lds<T> &s, T *dst, unsigned cnt, unsigned tid) {
  constexpr unsigned NT = kMgThreads, N = (TILE + NT - 1) / NT;
  if constexpr (VEC) {
    if (cnt == TILE) {
      constexpr unsigned PER = 16 / sizeof(T), NV = TILE / PER;
#pragma unroll
      for (unsigned q = 0; q < (NV + NT - 1) / NT; q++) {
        const unsigned v = q * NT + tid;
        if (NV % NT == 0 || v < NV) {
          T x[PER];
#pragma unroll
          for (unsigned e = 0; e < PER; e++) x[e] = s.get(v * PER + e);
          mg_u32x4 w;
          __builtin_memcpy(&w, x, 16);
          __builtin_nontemporal_store(w, reinterpret_cast<mg_u32x4 *>(dst) + v);
        }
      }
      return;
    }
  }
#pragma unroll
  for (unsigned k = 0; k < N; k++) {
    const unsigned e = k * NT + tid;
    if (e < cnt) {
      if constexpr (std::is_arithmetic<T>::value) __builtin_nontemporal_store(s.get(e), dst + e);
      else dst[e] = s.get(e);
    }
  }
}

// ------------------------------------------------------------ the kernel
// d0 < d1 <= na + nb; `per` tiles per workgroup.  out (and vout) point at output d0.
template <typename T, typename V, bool VEC, unsigned TILE, typename FA, typename FB, typename VA, typename VB, typename Comp>
__global__ __launch_bounds__(kMgThreads) void merge_kernel(FA A, mg_idx na, FB B, mg_idx nb, VA va, VB vb, mg_idx d0, mg_idx d1,
                                                           T *out, V *vout, Comp comp, unsigned per) {
  constexpr unsigned NT = kMgThreads, N = (TILE + NT - 1) / NT;
  constexpr bool VALS = mg_has<V>;
  static_assert(std::is_trivially_copyable<T>::value && std::is_trivially_copyable<V>::value, "elements move as bits");
  static_assert(TILE >= 1 && TILE <= NT * 64, "a tile is indexed with 32 bits");
  static_assert(!VEC || ((sizeof(T) == 4 || sizeof(T) == 8) && (TILE * sizeof(T)) % 16 == 0), "16-byte stores: 4- and 8-byte keys");
  static_assert(!VEC || !VALS || ((sizeof(V) == 4 || sizeof(V) == 8) && (TILE * sizeof(V)) % 16 == 0),
                "16-byte stores: 4- and 8-byte values");
  __shared__ __attribute__((aligned(16))) unsigned char s_keys[(std::size_t)mg_padded(TILE) * sizeof(T)];
  __shared__ __attribute__((aligned(16))) unsigned char s_vals[VALS ? (std::size_t)mg_padded(TILE) * sizeof(V) : 16];
  __shared__ mg_idx s_split;
  const mg_lds<T> sk{s_keys};
  const mg_lds<V> sv{s_vals};
  const unsigned tid = threadIdx.x;

  const mg_idx ntiles = (d1 - d0 + TILE - 1) / TILE;
  const mg_idx t0 = (mg_idx)blockIdx.x * per;
  mg_idx t1 = t0 + per;
  if (t1 > ntiles) t1 = ntiles;
  if (t0 >= t1) return; // uniform: before any barrier

  // the split of the run's first diagonal
  mg_idx i0 = 0;
  if (tid < 64) {
    const mg_idx d = d0 + t0 * TILE;
    const mg_idx r = mg_split<T>(A, B, d, d > nb ? d - nb : 0, d < na ? d : na, comp, tid);
    if (tid == 0) s_split = r;
  }
  __syncthreads();
  i0 = s_split;
  __syncthreads();

  for (mg_idx t = t0; t < t1; t++) {
    const mg_idx ds = d0 + t * TILE;                            // the tile's first diagonal
    const unsigned cnt = (unsigned)(d1 - ds < TILE ? d1 - ds : TILE); // its outputs, >= 1
    const mg_idx de = ds + cnt, j0 = ds - i0;
    if (tid < 64) {
      // the end split lies in [i0, i0 + cnt]: B's share of the tile is not negative, nor is A's.  i0 is a
      // split of ds, so ds - nb <= i0 <= min(ds, na) and with it lo <= hi, whatever the data
      mg_idx lo = de > nb ? de - nb : 0, hi = i0 + cnt;
      if (lo < i0) lo = i0;
      if (hi > na) hi = na;
      const mg_idx r = mg_split<T>(A, B, de, lo, hi, comp, tid);
      if (tid == 0) s_split = r;
    }
    __syncthreads(); // (also: the last tile's stores have read the LDS)
    const mg_idx i1 = s_split;
    const unsigned la = (unsigned)(i1 - i0), lb = cnt - la; // la <= cnt

    // 1. staged element e: A's piece, then B's
    {
      T r[N];
      V w[N];
#pragma unroll
      for (unsigned k = 0; k < N; k++) {
        const unsigned e = k * NT + tid;
        if (e < la) {
          r[k] = mg_stream<T>(A, (std::size_t)(i0 + e));
          if constexpr (VALS) w[k] = mg_stream<V>(va, (std::size_t)(i0 + e));
        } else if (e < cnt) {
          r[k] = mg_stream<T>(B, (std::size_t)(j0 + (e - la)));
          if constexpr (VALS) w[k] = mg_stream<V>(vb, (std::size_t)(j0 + (e - la)));
        }
      }
#pragma unroll
      for (unsigned k = 0; k < N; k++) {
        const unsigned e = k * NT + tid;
        if (e < cnt) {
          sk.put(e, r[k]);
          if constexpr (VALS) sv.put(e, w[k]);
        }
      }
    }
    __syncthreads();

    // 2. the thread's diagonal in the tile, its split, its N outputs
    const unsigned diag = tid * N < cnt ? tid * N : cnt;
    unsigned ai, bi; // staged indices of the two heads: A's in [0, la], B's in [la, cnt]
    {
      unsigned lo = diag > lb ? diag - lb : 0, hi = diag < la ? diag : la;
      while (lo < hi) {
        const unsigned mid = (lo + hi) / 2;
        if (!static_cast<bool>(comp(sk.get(la + diag - 1 - mid), sk.get(mid)))) lo = mid + 1;
        else hi = mid;
      }
      ai = lo;
      bi = la + (diag - lo);
    }
    const unsigned last = cnt - 1;
    T y[N];
    V z[N];
    {
      T ka = sk.get(ai < last ? ai : last), kb = sk.get(bi < last ? bi : last);
#pragma unroll
      for (unsigned k = 0; k < N; k++) {
        const bool take_b = bi < cnt && (ai >= la || static_cast<bool>(comp(kb, ka)));
        unsigned rank; // the staged element this output is; past the tile's end: a clamped re-read, never stored
        if (take_b) {
          y[k] = kb;
          rank = bi++;
          kb = sk.get(bi < last ? bi : last);
        } else {
          y[k] = ka;
          rank = ai++;
          ka = sk.get(ai < last ? ai : last);
        }
        if constexpr (VALS) z[k] = sv.get(rank < last ? rank : last);
      }
    }
    __syncthreads();
    // 3. back through LDS in output order, out coalesced
#pragma unroll
    for (unsigned k = 0; k < N; k++)
      if (diag + k < cnt && tid * N + k < TILE) {
        sk.put(diag + k, y[k]);
        if constexpr (VALS) sv.put(diag + k, z[k]);
      }
    __syncthreads();
    mg_store_tile<T, VEC, TILE>(sk, out + (ds - d0), cnt, tid);
    if constexpr (VALS) mg_store_tile<V, VEC, TILE>(sv, vout + (ds - d0), cnt, tid);
    i0 = i1;
  }
}

// ------------------------------------------------------------------ host

// The window [d0, d1) of merge(A, B) to out (its values to vout) on `st`; at most grid_cap workgroups.
// d0 == d1: nothing.  16-byte stores when the element widths allow them and out (and vout) are 16-byte aligned.
template <typename T, typename V = mg_none, unsigned T4 = kMgTile4, unsigned T8 = kMgTile8, typename FA, typename FB,
          typename VA, typename VB, typename Comp>
inline hipError_t mg_enqueue(hipStream_t st, FA A, std::size_t na, FB B, std::size_t nb, VA va, VB vb, std::size_t d0,
                             std::size_t d1, T *out, V *vout, Comp comp, unsigned grid_cap) {
  static_assert(sizeof(T) <= kMgMaxElem && sizeof(V) <= kMgMaxElem, "merge: elements and values of at most 4 KiB");
  if (d1 <= d0) return hipSuccess;
  constexpr unsigned TILE = mg_tile<T, V, T4, T8>();
  const mg_idx ntiles = ((mg_idx)(d1 - d0) + TILE - 1) / TILE;
  const mg_idx cap = grid_cap ? grid_cap : 1;
  const mg_idx per = (ntiles + cap - 1) / cap;
  const unsigned grid = (unsigned)((ntiles + per - 1) / per);
  auto go = [&](auto vec) {
    constexpr bool VEC = decltype(vec)::value;
    hipLaunchKernelGGL((merge_kernel<T, V, VEC, TILE, FA, FB, VA, VB, Comp>), dim3(grid), dim3(kMgThreads), 0, st, A,
                       (mg_idx)na, B, (mg_idx)nb, va, vb, (mg_idx)d0, (mg_idx)d1, out, vout, comp, (unsigned)per);
    return hipGetLastError();
  };
  constexpr bool key_vec = (sizeof(T) == 4 || sizeof(T) == 8) && (TILE * sizeof(T)) % 16 == 0;
  constexpr bool val_vec = !mg_has<V> || ((sizeof(V) == 4 || sizeof(V) == 8) && (TILE * sizeof(V)) % 16 == 0);
  if constexpr (key_vec && val_vec) {
    const bool al = reinterpret_cast<std::uintptr_t>(out) % 16 == 0 &&
                    (!mg_has<V> || reinterpret_cast<std::uintptr_t>(vout) % 16 == 0);
    if (al) return go(std::true_type{});
  }
  return go(std::false_type{});
}

} // namespace dr_merge

// bsearch_kernel.hpp -- the searches of a sorted (partitioned) range, for
// gfx950: lower_bound, upper_bound, binary_search, equal_range and
// partition_point of a batch of m needles in a haystack of n elements.  One
// template, included by the library (csrc/bsearch.hip: the C-ABI's six
// dtypes under <) and by the header layer (dr/shp/sorted_search.hpp: any
// device callable, instantiated in the user's translation unit).  C++17, no
// dependency beyond the HIP runtime.
//
// All of them are ONE search: the least p in [0, n] for which
// order.right(h[p], needle, i) is false, where right is true on a prefix of
// the haystack (bs_lower: comp(h, v); bs_upper: !comp(v, h); bs_equal_range:
// the former for needle 0 and the latter for needle 1; bs_partition: pred(h)).
// BS_FOUND stores order.hit(h[p], v) && p < n instead of p (binary_search).
//
// The search.  L = the bit width of n, so 2^L > n.  pos starts at 0 and for
// step = 2^(L-1), ..., 2, 1:
//     idx = pos + step - 1;   x = h[min(idx, n - 1)];
//     pos += (idx < n && right(x)) ? step : 0
// -- L probes whatever the data, the trip count derived from n alone and so
// uniform across the wave; the body is a clamped load and a select, no branch.
// Every element below pos has right == true and pos never passes n (a probe
// at idx >= n is never taken), so pos ends in [0, n] and no read leaves
// h[0, n) even when the haystack is not partitioned or holds NaNs; the result
// is then unspecified but in range.  Before a level of step s, pos is a
// multiple of 2s and at most 2^L - 2s: idx and pos stay below 2^L, so 32-bit
// positions serve every n < 2^32 (Idx = unsigned), 64-bit ones anything larger.
//
// Staged levels.  The top t = log2 S levels probe the same S - 1 addresses
// for every needle: idx = k * stride - 1, k = 1 .. S - 1, stride = 2^(L - t).
// A workgroup first copies those elements to LDS (sample k - 1 =
// h[min(k * stride - 1, n - 1)]), one barrier, and every search then takes
// its first t levels from LDS -- the very probes of the loop above, so the
// staged and the direct search return the same position bit for bit -- and
// only the remaining L - t = about ceil(log2(n / S)) levels from global
// memory.  With L <= t the whole haystack is in LDS (stride 1) and no probe
// goes to global memory.  S (bs_stage<T>()) is a compile-time power of two per
// element width; DESIGN.md "Sorted search" records the sweep.  Workgroups are
// persistent: the grid is at most grid_cap (2 x CUs) and block b takes the
// needle tiles b, b + grid, ..., so the staging is paid once per workgroup.
// A launch with fewer needles than S (the scalar forms: m = 1 or 2) skips the
// staging and the barrier and takes every level from global memory.
//
// A tile is 256 threads x 4 needles; a thread owns 4 CONSECUTIVE needles (one
// 16-byte load for 4-byte needles, two for 8-byte ones, when the needles are
// a 16-byte-aligned span: NVEC) and runs its 4 searches interleaved, level by
// level, so 4 independent probes are in flight per thread.  The 4 results
// leave as 16-byte stores when the output is 16-byte aligned (OVEC: two
// stores for 8-byte positions, one for 4-byte ones; the 4 flags of BS_FOUND
// as one 4-byte store).  The ragged last group of a piece and unaligned
// needles or outputs take element loads and stores.
//
// The haystack is a callable g -> h[g] over the global index: bs_one (one
// accessor) or bs_table, the virtual concatenation of P non-empty pieces
// {accessor, first global index} held in device memory: piece(g) = the
// greatest k with first[k] <= g, found by a fixed-trip search of the table.
// So one search over a segmented haystack returns the global position
// directly, whatever runs of equal elements span the seams.
//
// No state: the kernel reads the haystack and the needles and writes the
// output, nothing else -- no workspace, no counters, no word that crosses
// workgroups, no wait, no spin.  A captured launch replays as is.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <type_traits>

namespace dr_bsearch {

constexpr int kBsThreads = 256;
constexpr int kBsPer = 4;                          // searches per thread
constexpr std::size_t kBsTile = kBsThreads * kBsPer; // needles per tile
// S, the staged samples: per element width, from the sweep in DESIGN.md "Sorted search"
constexpr unsigned kBsStage4 = 8192; // elements of up to 4 bytes
constexpr unsigned kBsStage8 = 8192; // elements of 8 bytes
constexpr std::size_t kBsStageBytes = 65536; // wider elements: the largest power of two that fits, at least 64
constexpr std::size_t kBsMaxLds = 65536;     // a workgroup's static LDS; beyond it (elements above 1 KiB) nothing is staged
template <typename T> constexpr unsigned bs_stage() {
  if (sizeof(T) <= 4) return kBsStage4;
  if (sizeof(T) <= 8) return kBsStage8;
  unsigned s = 64;
  while (2 * s * sizeof(T) <= kBsStageBytes) s *= 2;
  return s;
}

enum : int { BS_POS = 0, BS_FOUND = 1 };

// ------------------------------------------------------------ the orders
template <typename Comp> struct bs_lower {
  Comp c;
  template <typename T, typename N> __device__ __forceinline__ bool right(const T &h, const N &v, std::size_t) const {
    return static_cast<bool>(c(h, v));
  }
  // binary_search: the element at the lower bound is not above the needle
  template <typename T, typename N> __device__ __forceinline__ bool hit(const T &h, const N &v) const {
    return !static_cast<bool>(c(v, h));
  }
};
template <typename Comp> struct bs_upper {
  Comp c;
  template <typename T, typename N> __device__ __forceinline__ bool right(const T &h, const N &v, std::size_t) const {
    return !static_cast<bool>(c(v, h));
  }
};
// needle 0: the lower bound, needle 1: the upper bound (both of one value)
template <typename Comp> struct bs_equal_range {
  Comp c;
  template <typename T, typename N> __device__ __forceinline__ bool right(const T &h, const N &v, std::size_t i) const {
    return i == 0 ? static_cast<bool>(c(h, v)) : !static_cast<bool>(c(v, h));
  }
};
template <typename Pred> struct bs_partition {
  Pred p;
  template <typename T, typename N> __device__ __forceinline__ bool right(const T &h, const N &, std::size_t) const {
    return static_cast<bool>(p(h));
  }
};
struct bs_less {
  template <typename A, typename B> __device__ __forceinline__ bool operator()(const A &a, const B &b) const { return a < b; }
};

// ----------------------------------------------------------- the needles
// contiguous and 16-byte aligned: 16-byte loads
template <typename N> struct bs_span {
  const N *p;
  using value_type = N;
  __device__ __forceinline__ N operator()(std::size_t i) const { return p[i]; }
};
// contiguous, any alignment
template <typename N> struct bs_ptr {
  const N *p;
  using value_type = N;
  __device__ __forceinline__ N operator()(std::size_t i) const { return p[i]; }
};
// one value, held in the kernel arguments
template <typename N> struct bs_const {
  N v;
  using value_type = N;
  __device__ __forceinline__ N operator()(std::size_t) const { return v; }
};
// any accessor in(i)
template <typename N, typename Acc> struct bs_acc {
  Acc a;
  using value_type = N;
  __device__ __forceinline__ N operator()(std::size_t i) const { return static_cast<N>(a(i)); }
};
template <typename X> constexpr bool bs_is_span = false;
template <typename N> constexpr bool bs_is_span<bs_span<N>> = true;

// ---------------------------------------------------------- the haystack
template <typename T, typename Acc> struct bs_one {
  Acc a;
  __device__ __forceinline__ T operator()(std::size_t g) const { return static_cast<T>(a(g)); }
};
template <typename Acc> struct bs_piece {
  Acc a;
  unsigned long long first; // the global index of the piece's element 0
};
// P >= 1 non-empty pieces in device-visible memory, `first` ascending from 0; top = the greatest power of two
// below P (0 when P == 1)
template <typename T, typename Acc> struct bs_table {
  const bs_piece<Acc> *p;
  unsigned P, top;
  __device__ __forceinline__ T operator()(std::size_t g) const {
    unsigned k = 0;
    for (unsigned s = top; s; s >>= 1) {
      const unsigned c = k + s;
      const bool ok = c < P && p[c < P ? c : P - 1].first <= g;
      k += ok ? s : 0;
    }
    return static_cast<T>(p[k].a(g - p[k].first));
  }
};
inline unsigned bs_table_top(unsigned P) {
  unsigned s = 0;
  for (unsigned q = 1; q < P; q *= 2) s = q;
  return s;
}

typedef unsigned int bs_u32x4 __attribute__((ext_vector_type(4)));

template <typename Idx> __device__ __forceinline__ int bs_width(Idx n) {
  if constexpr (sizeof(Idx) == 8) return 64 - __clzll((long long)n);
  else return 32 - __clz((int)n);
}

// ------------------------------------------------------------ the kernel
// n >= 1, m >= 1.  staged != 0: the top levels from LDS.
template <typename T, typename Idx, int S, bool NVEC, bool OVEC, int MODE, typename Hay, typename Needles, typename Order,
          typename Out>
__global__ __launch_bounds__(kBsThreads) void bsearch_kernel(Hay hay, Idx n, Needles nd, std::size_t m, Order ord, Out *out,
                                                             unsigned staged) {
  using N = typename Needles::value_type;
  constexpr int NT = kBsThreads, PER = kBsPer;
  constexpr int LOGS = __builtin_ctz((unsigned)S);
  static_assert((S & (S - 1)) == 0 && S >= 2, "S is a power of two");
  static_assert(std::is_trivially_copyable<T>::value && std::is_trivially_copyable<N>::value, "elements are read as bits");
  static_assert(!NVEC || sizeof(N) == 4 || sizeof(N) == 8, "16-byte needle loads: 4- and 8-byte needles");
  static_assert(!OVEC || sizeof(Out) == 1 || sizeof(Out) == 4 || sizeof(Out) == 8, "vector stores: 1-, 4- and 8-byte outputs");
  // elements so wide that S of them exceed a workgroup's LDS are searched in global memory alone
  constexpr bool FITS = (std::size_t)S * sizeof(T) <= kBsMaxLds;
  __shared__ __attribute__((aligned(16))) unsigned char s_raw[FITS ? (std::size_t)S * sizeof(T) : 16];
  const int tid = threadIdx.x;
  if (!FITS) staged = 0;

  const int L = bs_width<Idx>(n);          // 2^L > n >= 2^(L-1)
  const int t = staged ? (L < LOGS ? L : LOGS) : 0; // levels taken from LDS
  const int sh = L - t;                    // log2 of the sample stride; the levels left for global memory
  if (staged) {
    const unsigned ns = (1u << t) - 1; // samples
    for (unsigned k = tid + 1; k <= ns; k += NT) {
      const Idx idx = ((Idx)k << sh) - 1;
      const T x = hay((std::size_t)(idx < n ? idx : n - 1));
      __builtin_memcpy(s_raw + (std::size_t)(k - 1) * sizeof(T), &x, sizeof(T));
    }
    __syncthreads();
  }

  const std::size_t ntiles = (m + kBsTile - 1) / kBsTile;
  for (std::size_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const std::size_t b = tile * kBsTile + (std::size_t)tid * PER; // the thread's first needle
    if (b >= m) continue; // the ragged last tile (no barrier below)
    const bool whole = b + PER <= m;
    N v[PER];
    if constexpr (NVEC) {
      if (whole) {
#pragma unroll
        for (int q = 0; q < (int)(PER * sizeof(N) / 16); q++) {
          const bs_u32x4 w = __builtin_nontemporal_load(reinterpret_cast<const bs_u32x4 *>(nd.p + b) + q);
          __builtin_memcpy(reinterpret_cast<unsigned char *>(v) + 16 * q, &w, 16);
        }
      } else {
#pragma unroll
        for (int j = 0; j < PER; j++) v[j] = nd(b + j < m ? b + j : m - 1);
      }
    } else {
#pragma unroll
      for (int j = 0; j < PER; j++) v[j] = nd(b + j < m ? b + j : m - 1);
    }

    Idx pos[PER];
#pragma unroll
    for (int j = 0; j < PER; j++) pos[j] = 0;
    if (staged) {
      unsigned pu[PER]; // pos in units of the stride
#pragma unroll
      for (int j = 0; j < PER; j++) pu[j] = 0;
      for (unsigned su = t ? 1u << (t - 1) : 0; su; su >>= 1) {
        T x[PER];
#pragma unroll
        for (int j = 0; j < PER; j++)
          __builtin_memcpy(&x[j], s_raw + (std::size_t)(pu[j] + su - 1) * sizeof(T), sizeof(T));
#pragma unroll
        for (int j = 0; j < PER; j++) {
          const Idx idx = ((Idx)(pu[j] + su) << sh) - 1;
          const bool take = idx < n && ord.right(x[j], v[j], b + j);
          pu[j] += take ? su : 0;
        }
      }
#pragma unroll
      for (int j = 0; j < PER; j++) pos[j] = (Idx)pu[j] << sh;
    }
    for (Idx step = sh ? (Idx)1 << (sh - 1) : 0; step; step >>= 1) {
      T x[PER];
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const Idx idx = pos[j] + (step - 1);
        x[j] = hay((std::size_t)(idx < n ? idx : n - 1));
      }
#pragma unroll
      for (int j = 0; j < PER; j++) {
        const Idx idx = pos[j] + (step - 1);
        const bool take = idx < n && ord.right(x[j], v[j], b + j);
        pos[j] += take ? step : 0;
      }
    }

    Out r[PER];
    if constexpr (MODE == BS_FOUND) {
      T x[PER];
#pragma unroll
      for (int j = 0; j < PER; j++) x[j] = hay((std::size_t)(pos[j] < n ? pos[j] : n - 1));
#pragma unroll
      for (int j = 0; j < PER; j++) r[j] = (Out)(pos[j] < n && ord.hit(x[j], v[j]));
    } else {
#pragma unroll
      for (int j = 0; j < PER; j++) r[j] = (Out)pos[j];
    }
    bool stored = false;
    if constexpr (OVEC) {
      if (whole) {
        if constexpr (sizeof(Out) == 1) {
          unsigned w;
          __builtin_memcpy(&w, r, 4);
          *reinterpret_cast<unsigned *>(out + b) = w;
        } else {
#pragma unroll
          for (int q = 0; q < (int)(PER * sizeof(Out) / 16); q++) {
            bs_u32x4 w;
            __builtin_memcpy(&w, reinterpret_cast<const unsigned char *>(r) + 16 * q, 16);
            *(reinterpret_cast<bs_u32x4 *>(out + b) + q) = w;
          }
        }
        stored = true;
      }
    }
    if (!stored) {
#pragma unroll
      for (int j = 0; j < PER; j++)
        if (b + j < m) out[b + j] = r[j];
    }
  }
}

// ------------------------------------------------------------------ host

template <typename T, typename Idx, int S, bool NVEC, bool OVEC, int MODE, typename Hay, typename Needles, typename Order,
          typename Out>
inline hipError_t bs_launch(hipStream_t st, Hay hay, std::size_t n, Needles nd, std::size_t m, Order ord, Out *out,
                            unsigned grid_cap) {
  const std::size_t ntiles = (m + kBsTile - 1) / kBsTile;
  const unsigned grid = ntiles > grid_cap ? grid_cap : (unsigned)ntiles;
  hipLaunchKernelGGL((bsearch_kernel<T, Idx, S, NVEC, OVEC, MODE, Hay, Needles, Order, Out>), dim3(grid), dim3(kBsThreads), 0,
                     st, hay, (Idx)n, nd, m, ord, out, (unsigned)(m >= (std::size_t)S));
  return hipGetLastError();
}

// Everything one search of m needles needs, on `st`.  m == 0: nothing.  n == 0: m zeros.  Needles that are a
// bs_span<N> must be a contiguous span; they are read with 16-byte loads when 16-byte aligned (and N is 4 or
// 8 bytes wide) and as a bs_ptr<N> otherwise.  WIDE (the header layer): outputs and needles choose their vector
// forms separately and n >= 2^32 takes 64-bit positions; otherwise (the C-ABI, a quarter of the kernels) both
// vector forms or neither, and the caller has refused n >= 2^32.
template <typename T, int MODE, int S = (int)bs_stage<T>(), bool WIDE = true, typename Hay, typename Needles, typename Order,
          typename Out>
inline hipError_t bs_enqueue(hipStream_t st, Hay hay, std::size_t n, Needles nd, std::size_t m, Order ord, Out *out,
                             unsigned grid_cap) {
  using N = typename Needles::value_type;
  if (m == 0) return hipSuccess;
  if (n == 0) return hipMemsetAsync(out, 0, m * sizeof(Out), st);
  constexpr bool out_vec_type = sizeof(Out) == 1 || sizeof(Out) == 4 || sizeof(Out) == 8;
  const bool oal = out_vec_type && reinterpret_cast<std::uintptr_t>(out) % 16 == 0;
  auto go = [&](auto needles, auto nvec, auto ovec) {
    constexpr bool NV = decltype(nvec)::value, OV = decltype(ovec)::value;
    using Nd = decltype(needles);
    if constexpr (WIDE) {
      if (n >= (std::size_t(1) << 32))
        return bs_launch<T, unsigned long long, S, NV, OV, MODE, Hay, Nd, Order, Out>(st, hay, n, needles, m, ord, out,
                                                                                      grid_cap);
    }
    return bs_launch<T, unsigned, S, NV, OV, MODE, Hay, Nd, Order, Out>(st, hay, n, needles, m, ord, out, grid_cap);
  };
  if constexpr (bs_is_span<Needles>) {
    constexpr bool needle_vec_type = sizeof(N) == 4 || sizeof(N) == 8;
    const bool nal = needle_vec_type && reinterpret_cast<std::uintptr_t>(nd.p) % 16 == 0;
    if constexpr (needle_vec_type && out_vec_type) {
      if (nal && oal) return go(nd, std::true_type{}, std::true_type{});
    }
    if constexpr (WIDE) {
      if constexpr (needle_vec_type) {
        if (nal) return go(nd, std::true_type{}, std::false_type{});
      }
      if constexpr (out_vec_type) {
        if (oal) return go(bs_ptr<N>{nd.p}, std::false_type{}, std::true_type{});
      }
    }
    return go(bs_ptr<N>{nd.p}, std::false_type{}, std::false_type{});
  } else {
    if constexpr (out_vec_type) {
      if (oal) return go(nd, std::false_type{}, std::true_type{});
    }
    return go(nd, std::false_type{}, std::false_type{});
  }
}

} // namespace dr_bsearch

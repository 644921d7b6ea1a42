// select.hip -- C-ABI entries of the single-pass selection
// (kernel: include/dr/details/select_kernel.hpp): drhip_count_if,
// drhip_copy_if, drhip_copy_flagged.
#include "common.hpp"

#include "../include/dr/details/select_kernel.hpp"

namespace drhip {

using namespace dr_select;

struct FlagPred {
  const uint8_t *f;
  __device__ __forceinline__ bool operator()(const uint32_t &, size_t i) const { return f[i] != 0; }
  __device__ __forceinline__ bool operator()(const uint64_t &, size_t i) const { return f[i] != 0; }
};

static bool overlaps(const void *a, size_t ab, const void *b, size_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bb && b0 < a0 + ab;
}

// SEL_COUNT grid: blocks per CU (the reduce's grid, csrc/reduce.hip)
constexpr int kSelCountBlocksPerCU = 2;

// One selection or count of n elements on seg's stream; n == 0 writes 0.
template <typename T, int MODE, typename Pred>
static int launch_select(Segment *s, int seg, const T *in, T *out, size_t n, Pred pred, uint64_t *count) {
  DRHIP_CHECK_HIP(hipSetDevice(s->device));
  if (n == 0) {
    hipLaunchKernelGGL(sel_write_total<0>, dim3(1), dim3(1), 0, s->stream, (unsigned long long *)count, 0ull);
    DRHIP_CHECK_LAUNCH();
    return DRHIP_OK;
  }
  // status words in the segment's workspace, re-zeroed before every launch
  const size_t bytes = MODE == SEL_COUNT ? kSelHeadBytes : sel_state_bytes<T>(n);
  if (int rc = ensure_workspace(seg, bytes)) return rc;
  DRHIP_CHECK_HIP(hipMemsetAsync(s->ws, 0, bytes, s->stream));
  sel_args a{(char *)s->ws, (unsigned long long *)count, s->err};
  DRHIP_CHECK_HIP((sel_launch_span<T, MODE>(s->stream, in, out, n, pred, a, grid_cap(s, kSelCountBlocksPerCU))));
  return DRHIP_OK;
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_count_if(int seg, int dtype, int cmp, const void *x, size_t n, const void *scalar_host, uint64_t *count) {
  if (dtype_size(dtype) == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_count_if: unsupported dtype");
  if (cmp < DRHIP_LT || cmp > DRHIP_NE) return set_error(DRHIP_ERR_BAD_ARG, "drhip_count_if: unknown cmp");
  if (!count || !scalar_host || (n > 0 && !x)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_count_if: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_count_if: n must be below 2^32");
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    T sc;
    memcpy(&sc, scalar_host, sizeof(T));
    return dispatch_cmp(cmp, "drhip_count_if: unknown cmp", [&](auto c) {
      return launch_select<T, SEL_COUNT>(s, seg, (const T *)x, (T *)nullptr, n, CmpPred<T, decltype(c)::value>{sc},
                                         count);
    });
  });
}

int drhip_copy_if(int seg, int dtype, int cmp, const void *in, void *out, size_t n, const void *scalar_host,
                  uint64_t *count) {
  const size_t es = dtype_size(dtype);
  if (es == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_if: unsupported dtype");
  if (cmp < DRHIP_LT || cmp > DRHIP_NE) return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_if: unknown cmp");
  if (!count || !scalar_host || (n > 0 && (!in || !out)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_if: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_if: n must be below 2^32");
  if (n > 0 && overlaps(in, n * es, out, n * es))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_if: out overlaps in");
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    T sc;
    memcpy(&sc, scalar_host, sizeof(T));
    return dispatch_cmp(cmp, "drhip_copy_if: unknown cmp", [&](auto c) {
      return launch_select<T, kSelMode>(s, seg, (const T *)in, (T *)out, n, CmpPred<T, decltype(c)::value>{sc}, count);
    });
  });
}

int drhip_copy_flagged(int seg, size_t elem_bytes, const void *in, const uint8_t *flags, void *out, size_t n,
                       uint64_t *count) {
  if (elem_bytes != 4 && elem_bytes != 8)
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_flagged: elem_bytes must be 4 or 8");
  if (!count || (n > 0 && (!in || !out || !flags)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_flagged: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_flagged: n must be below 2^32");
  if (n > 0 && (overlaps(in, n * elem_bytes, out, n * elem_bytes) || overlaps(flags, n, out, n * elem_bytes)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_copy_flagged: out overlaps in or flags");
  DRHIP_GET_SEG(s, seg);
  if (elem_bytes == 4)
    return launch_select<uint32_t, kSelMode>(s, seg, (const uint32_t *)in, (uint32_t *)out, n, FlagPred{flags}, count);
  return launch_select<uint64_t, kSelMode>(s, seg, (const uint64_t *)in, (uint64_t *)out, n, FlagPred{flags}, count);
}

} // extern "C"

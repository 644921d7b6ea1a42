// search.hip -- C-ABI entries of the searches that return a position
// (kernels: include/dr/details/search_kernel.hpp): drhip_find_if,
// drhip_is_sorted_until, drhip_mismatch, drhip_min_element,
// drhip_max_element, drhip_minmax_element.
#include "common.hpp"

#include <string>

#include "../include/dr/details/search_kernel.hpp"

namespace drhip {

using namespace dr_search;

// x[i + 1] < x[i]: the pair that ends a sorted prefix
struct DescentPred {
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const { return b < a; }
};
struct DifferPred {
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const { return a != b; }
};
struct LessOp {
  template <typename T> __device__ __forceinline__ bool operator()(const T &a, const T &b) const { return a < b; }
};

// the grid of the reduce and of count_if (csrc/reduce.hip, csrc/select.hip)
constexpr int kSrchBlocksPerCU = 2;

// One first-match search of n elements on seg's stream; *index = the match + add, or n.
template <typename T, int KIND, typename Pred>
static int launch_first(Segment *s, int seg, const T *a, const T *b, size_t n, Pred pred, size_t add, uint64_t *index) {
  DRHIP_CHECK_HIP(hipSetDevice(s->device));
  if (n > 0)
    if (int rc = ensure_workspace(seg, kSrchHeadBytes)) return rc;
  const srch_first_args args{(char *)s->ws, (unsigned long long *)index, n, add, grid_cap(s, kSrchBlocksPerCU)};
  DRHIP_CHECK_HIP((srch_first_span<T, KIND>(s->stream, a, b, n, pred, args)));
  return DRHIP_OK;
}

template <int MODE> static int launch_extremum(const char *fn, int seg, int dtype, const void *x, size_t n, uint64_t *index) {
  const std::string name(fn);
  if (dtype_size(dtype) == 0) return set_error(DRHIP_ERR_BAD_ARG, (name + ": unsupported dtype").c_str());
  if (!index || (n > 0 && !x)) return set_error(DRHIP_ERR_BAD_ARG, (name + ": null pointer").c_str());
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, (name + ": n must be below 2^32").c_str());
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    DRHIP_CHECK_HIP(hipSetDevice(s->device));
    const unsigned cap = grid_cap(s, kSrchBlocksPerCU);
    if (n > 0)
      if (int rc = ensure_workspace(seg, srch_ext_state_bytes<T>(cap))) return rc;
    const srch_ext_args args{(char *)s->ws, (unsigned long long *)index, cap};
    DRHIP_CHECK_HIP((srch_extremum_span<T, MODE>(s->stream, (const T *)x, n, LessOp{}, args)));
    return (int)DRHIP_OK;
  });
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_find_if(int seg, int dtype, int cmp, const void *x, size_t n, const void *scalar_host, uint64_t *index) {
  if (dtype_size(dtype) == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_find_if: unsupported dtype");
  if (cmp < DRHIP_LT || cmp > DRHIP_NE) return set_error(DRHIP_ERR_BAD_ARG, "drhip_find_if: unknown cmp");
  if (!index || !scalar_host || (n > 0 && !x)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_find_if: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_find_if: n must be below 2^32");
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    T sc;
    memcpy(&sc, scalar_host, sizeof(T));
    return dispatch_cmp(cmp, "drhip_find_if: unknown cmp", [&](auto c) {
      return launch_first<T, SRCH_UNARY>(s, seg, (const T *)x, (const T *)nullptr, n, CmpPred<T, decltype(c)::value>{sc},
                                         0, index);
    });
  });
}

int drhip_is_sorted_until(int seg, int dtype, const void *x, size_t n, uint64_t *index) {
  if (dtype_size(dtype) == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_is_sorted_until: unsupported dtype");
  if (!index || (n > 0 && !x)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_is_sorted_until: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_is_sorted_until: n must be below 2^32");
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    // the pair (i, i + 1) with x[i + 1] < x[i] answers i + 1
    return launch_first<T, SRCH_ADJACENT>(s, seg, (const T *)x, (const T *)nullptr, n, DescentPred{}, 1, index);
  });
}

int drhip_mismatch(int seg, int dtype, const void *a, const void *b, size_t n, uint64_t *index) {
  if (dtype_size(dtype) == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_mismatch: unsupported dtype");
  if (!index || (n > 0 && (!a || !b))) return set_error(DRHIP_ERR_BAD_ARG, "drhip_mismatch: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_mismatch: n must be below 2^32");
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    return launch_first<T, SRCH_TWO>(s, seg, (const T *)a, (const T *)b, n, DifferPred{}, 0, index);
  });
}

int drhip_min_element(int seg, int dtype, const void *x, size_t n, uint64_t *index) {
  return launch_extremum<SRCH_MIN>("drhip_min_element", seg, dtype, x, n, index);
}
int drhip_max_element(int seg, int dtype, const void *x, size_t n, uint64_t *index) {
  return launch_extremum<SRCH_MAX>("drhip_max_element", seg, dtype, x, n, index);
}
int drhip_minmax_element(int seg, int dtype, const void *x, size_t n, uint64_t *idx2) {
  return launch_extremum<SRCH_MINMAX>("drhip_minmax_element", seg, dtype, x, n, idx2);
}

} // extern "C"

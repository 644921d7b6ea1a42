// bsearch.hip -- C-ABI entries of the searches of a sorted range (kernel:
// include/dr/details/bsearch_kernel.hpp): drhip_lower_bound,
// drhip_upper_bound, drhip_binary_search.
#include "common.hpp"

#include <string>

#include "../include/dr/details/bsearch_kernel.hpp"

namespace drhip {

using namespace dr_bsearch;

// the grid of the reduce, of count_if and of the searches (csrc/search.hip)
constexpr int kBsBlocksPerCU = 2;

static bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

// UPPER: the order of upper_bound; MODE: positions (Out = uint64_t) or flags (Out = uint8_t)
template <bool UPPER, int MODE, typename Out>
static int sorted_search(const char *fn, int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m,
                         Out *out) {
  const std::string name(fn);
  const size_t es = dtype_size(dtype);
  if (es == 0) return set_error(DRHIP_ERR_BAD_ARG, (name + ": unsupported dtype").c_str());
  if ((n > 0 && !hay) || (m > 0 && (!needles || !out))) return set_error(DRHIP_ERR_BAD_ARG, (name + ": null pointer").c_str());
  if (n >= (size_t(1) << 32) || m >= (size_t(1) << 32))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": n and m must be below 2^32").c_str());
  if (overlap(out, m * sizeof(Out), hay, n * es) || overlap(out, m * sizeof(Out), needles, m * es))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": the output overlaps an input").c_str());
  if (m == 0) return DRHIP_OK;
  DRHIP_GET_SEG(s, seg);
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    DRHIP_CHECK_HIP(hipSetDevice(s->device));
    const bs_one<T, bs_ptr<T>> h{bs_ptr<T>{(const T *)hay}};
    const bs_span<T> nd{(const T *)needles};
    const unsigned cap = grid_cap(s, kBsBlocksPerCU);
    if constexpr (UPPER)
      DRHIP_CHECK_HIP((bs_enqueue<T, MODE, (int)bs_stage<T>(), false>(s->stream, h, n, nd, m, bs_upper<bs_less>{}, out, cap)));
    else
      DRHIP_CHECK_HIP((bs_enqueue<T, MODE, (int)bs_stage<T>(), false>(s->stream, h, n, nd, m, bs_lower<bs_less>{}, out, cap)));
    return (int)DRHIP_OK;
  });
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_lower_bound(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint64_t *pos) {
  return sorted_search<false, BS_POS>("drhip_lower_bound", seg, dtype, hay, n, needles, m, pos);
}
int drhip_upper_bound(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint64_t *pos) {
  return sorted_search<true, BS_POS>("drhip_upper_bound", seg, dtype, hay, n, needles, m, pos);
}
int drhip_binary_search(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint8_t *found) {
  return sorted_search<false, BS_FOUND>("drhip_binary_search", seg, dtype, hay, n, needles, m, found);
}

} // extern "C"

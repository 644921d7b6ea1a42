// merge.hip -- C-ABI entries of the stable merge of two sorted ranges (kernel:
// include/dr/details/merge_kernel.hpp): drhip_merge, drhip_merge_pairs.
#include "common.hpp"

#include <string>

#include "../include/dr/details/merge_kernel.hpp"

static_assert(DRHIP_MERGE_TILE(4) == dr_merge::kMgTile4 && DRHIP_MERGE_TILE(8) == dr_merge::kMgTile8,
              "DRHIP_MERGE_TILE is the kernel's tile");

namespace drhip {

using namespace dr_merge;

// persistent workgroups over contiguous runs of tiles: as many as a CU holds (8 x 4 waves)
constexpr int kMgBlocksPerCU = 8;

static bool overlap(const void *a, size_t abytes, const void *b, size_t bbytes) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return abytes && bbytes && a0 < b0 + bbytes && b0 < a0 + abytes;
}

// pairs: every key carries a value of val_bytes
static int merge_entry(const char *fn, bool pairs, int seg, int dtype, const void *a, const void *av, size_t na, const void *b,
                       const void *bv, size_t nb, size_t val_bytes, void *out, void *vout) {
  const std::string name(fn);
  const size_t es = dtype_size(dtype);
  if (es == 0) return set_error(DRHIP_ERR_BAD_ARG, (name + ": unsupported dtype").c_str());
  if (pairs && val_bytes != 4 && val_bytes != 8)
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": val_bytes must be 4 or 8").c_str());
  if ((na > 0 && (!a || (pairs && !av))) || (nb > 0 && (!b || (pairs && !bv))) ||
      (na + nb > 0 && (!out || (pairs && !vout))))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": null pointer").c_str());
  const size_t lim = size_t(1) << 32;
  if (na >= lim || nb >= lim || na + nb >= lim)
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": na + nb must be below 2^32").c_str());
  const size_t n = na + nb;
  const void *in[4] = {a, b, av, bv};
  const size_t inb[4] = {na * es, nb * es, pairs ? na * val_bytes : 0, pairs ? nb * val_bytes : 0};
  for (int k = 0; k < 4; k++)
    if (overlap(out, n * es, in[k], inb[k]) || (pairs && overlap(vout, n * val_bytes, in[k], inb[k])))
      return set_error(DRHIP_ERR_BAD_ARG, (name + ": an output overlaps an input").c_str());
  if (pairs && overlap(out, n * es, vout, n * val_bytes))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": the outputs overlap each other").c_str());
  if (n == 0) return DRHIP_OK;
  DRHIP_GET_SEG(s, seg);
  DRHIP_CHECK_HIP(hipSetDevice(s->device));
  if (na == 0 || nb == 0) { // a copy of the other input
    DRHIP_CHECK_HIP(hipMemcpyAsync(out, na ? a : b, n * es, hipMemcpyDeviceToDevice, s->stream));
    if (pairs) DRHIP_CHECK_HIP(hipMemcpyAsync(vout, na ? av : bv, n * val_bytes, hipMemcpyDeviceToDevice, s->stream));
    return DRHIP_OK;
  }
  return dispatch_dtype(dtype, [&](auto tag) {
    using T = decltype(tag);
    const mg_ptr<T> A{(const T *)a}, B{(const T *)b};
    const unsigned cap = grid_cap(s, kMgBlocksPerCU);
    if (!pairs) {
      DRHIP_CHECK_HIP((mg_enqueue<T>(s->stream, A, na, B, nb, mg_no_values{}, mg_no_values{}, 0, n, (T *)out, (mg_none *)nullptr,
                                     mg_less{}, cap)));
    } else if (val_bytes == 4) {
      using V = uint32_t;
      DRHIP_CHECK_HIP((mg_enqueue<T, V>(s->stream, A, na, B, nb, mg_ptr<V>{(const V *)av}, mg_ptr<V>{(const V *)bv}, 0, n,
                                        (T *)out, (V *)vout, mg_less{}, cap)));
    } else {
      using V = uint64_t;
      DRHIP_CHECK_HIP((mg_enqueue<T, V>(s->stream, A, na, B, nb, mg_ptr<V>{(const V *)av}, mg_ptr<V>{(const V *)bv}, 0, n,
                                        (T *)out, (V *)vout, mg_less{}, cap)));
    }
    return (int)DRHIP_OK;
  });
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_merge(int seg, int dtype, const void *a, size_t na, const void *b, size_t nb, void *out) {
  return merge_entry("drhip_merge", false, seg, dtype, a, nullptr, na, b, nullptr, nb, 0, out, nullptr);
}
int drhip_merge_pairs(int seg, int kdtype, const void *a_keys, const void *a_vals, size_t na, const void *b_keys,
                      const void *b_vals, size_t nb, size_t val_bytes, void *out_keys, void *out_vals) {
  return merge_entry("drhip_merge_pairs", true, seg, kdtype, a_keys, a_vals, na, b_keys, b_vals, nb, val_bytes, out_keys,
                     out_vals);
}

} // extern "C"

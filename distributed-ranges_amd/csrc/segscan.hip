// segscan.hip -- C-ABI entries of the by-key scans
// (kernel: include/dr/details/segscan_kernel.hpp): drhip_inclusive_scan_by_key,
// drhip_exclusive_scan_by_key.
#include "bykey.hpp"

#include <string>

#include "../include/dr/details/segscan_kernel.hpp"

namespace drhip {

using namespace dr_segscan;

// Both entries: the argument checks (before the segment is looked up), then
// one launch.  init_host: the exclusive form's init in the value dtype, or
// null for the identity of op.
template <bool EXCL>
static int scan_by_key(const char *fn, int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                       const void *init_host, void *vals_out) {
  const std::string name(fn);
  const size_t ks = dtype_size(kdtype), vs = dtype_size(vdtype);
  if (ks == 0 || vs == 0) return set_error(DRHIP_ERR_BAD_ARG, (name + ": unsupported dtype").c_str());
  if (op < DRHIP_PLUS || op > DRHIP_MAX) return set_error(DRHIP_ERR_BAD_ARG, (name + ": unknown op").c_str());
  if (n > 0 && (!keys_in || !vals_in || !vals_out)) return set_error(DRHIP_ERR_BAD_ARG, (name + ": null pointer").c_str());
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, (name + ": n must be below 2^32").c_str());
  if (n > 0 && overlaps(vals_out, n * vs, keys_in, n * ks))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": vals_out overlaps keys_in").c_str());
  if (n > 0 && vals_out != vals_in && overlaps(vals_out, n * vs, vals_in, n * vs))
    return set_error(DRHIP_ERR_BAD_ARG, (name + ": vals_out overlaps vals_in without being vals_in").c_str());
  DRHIP_GET_SEG(s, seg);
  if (n == 0) return DRHIP_OK;
  return dispatch_key_class(kdtype, [&](auto ktag) {
    using K = decltype(ktag);
    return dispatch_dtype(vdtype, [&](auto vtag) {
      using T = decltype(vtag);
      return dispatch_op(op, [&](auto o) {
        constexpr int OP = decltype(o)::value;
        using C = val_class<OP, T>;
        using V = typename C::V;
        using A = typename C::A;
        A init = Op<OP, A>::identity();
        if (EXCL && init_host) {
          V x;
          memcpy(&x, init_host, sizeof(V));
          init = static_cast<A>(x);
        }
        DRHIP_CHECK_HIP(hipSetDevice(s->device));
        if (int rc = ensure_workspace(seg, ss_state_bytes_max<K, V>(n))) return rc;
        const ss_args a{(char *)s->ws, s->err};
        DRHIP_CHECK_HIP((ss_launch_spans<K, V, A, EXCL>(s->stream, (const K *)keys_in, (const V *)vals_in, n, (V *)vals_out, init,
                                                        KeyEq<K>{}, FoldOp<OP, A>{}, a)));
        return (int)DRHIP_OK;
      });
    });
  });
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_inclusive_scan_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                                void *vals_out) {
  return scan_by_key<false>("drhip_inclusive_scan_by_key", seg, kdtype, vdtype, op, keys_in, vals_in, n, nullptr, vals_out);
}

int drhip_exclusive_scan_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                                const void *init_host, void *vals_out) {
  return scan_by_key<true>("drhip_exclusive_scan_by_key", seg, kdtype, vdtype, op, keys_in, vals_in, n, init_host, vals_out);
}

} // extern "C"

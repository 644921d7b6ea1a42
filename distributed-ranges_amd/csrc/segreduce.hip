// segreduce.hip -- C-ABI entries of the by-key reduction
// (kernel: include/dr/details/segreduce_kernel.hpp): drhip_reduce_by_key,
// drhip_run_length_encode, drhip_unique_copy.
#include "bykey.hpp"

#include "../include/dr/details/segreduce_kernel.hpp"

namespace drhip {

using namespace dr_segreduce;

static int write_zero(Segment *s, uint64_t *num_runs) {
  DRHIP_CHECK_HIP(hipSetDevice(s->device));
  hipLaunchKernelGGL(dr_select::sel_write_total<0>, dim3(1), dim3(1), 0, s->stream, (unsigned long long *)num_runs, 0ull);
  DRHIP_CHECK_LAUNCH();
  return DRHIP_OK;
}

// the segment's workspace as the launch's state (the caller's n > 0)
template <typename K, typename V> static int state_of(Segment *s, int seg, size_t n, uint64_t *num_runs, sr_args *a) {
  DRHIP_CHECK_HIP(hipSetDevice(s->device));
  if (int rc = ensure_workspace(seg, sr_state_bytes_max<K, V>(n))) return rc;
  *a = sr_args{(char *)s->ws, (unsigned long long *)num_runs, s->err};
  return DRHIP_OK;
}

} // namespace drhip

using namespace drhip;

extern "C" {

int drhip_reduce_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                        void *keys_out, void *vals_out, uint64_t *num_runs) {
  const size_t ks = dtype_size(kdtype), vs = dtype_size(vdtype);
  if (ks == 0 || vs == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_reduce_by_key: unsupported dtype");
  if (op < DRHIP_PLUS || op > DRHIP_MAX) return set_error(DRHIP_ERR_BAD_ARG, "drhip_reduce_by_key: unknown op");
  if (!num_runs || (n > 0 && (!keys_in || !vals_in || !keys_out || !vals_out)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_reduce_by_key: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_reduce_by_key: n must be below 2^32");
  if (n > 0 && (overlaps(keys_out, n * ks, keys_in, n * ks) || overlaps(keys_out, n * ks, vals_in, n * vs) ||
                overlaps(vals_out, n * vs, keys_in, n * ks) || overlaps(vals_out, n * vs, vals_in, n * vs)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_reduce_by_key: an output overlaps an input");
  DRHIP_GET_SEG(s, seg);
  if (n == 0) return write_zero(s, num_runs);
  return dispatch_key_class(kdtype, [&](auto ktag) {
    using K = decltype(ktag);
    return dispatch_dtype(vdtype, [&](auto vtag) {
      return dispatch_op(op, [&](auto o) {
        constexpr int OP = decltype(o)::value;
        using C = val_class<OP, decltype(vtag)>;
        using V = typename C::V;
        using A = typename C::A;
        sr_args a;
        if (int rc = state_of<K, V>(s, seg, n, num_runs, &a)) return rc;
        DRHIP_CHECK_HIP((sr_launch_spans<K, V, A>(s->stream, (const K *)keys_in, (const V *)vals_in, n, (K *)keys_out,
                                                  (V *)vals_out, KeyEq<K>{}, FoldOp<OP, A>{}, a)));
        return (int)DRHIP_OK;
      });
    });
  });
}

int drhip_run_length_encode(int seg, int kdtype, const void *keys_in, size_t n, void *keys_out, uint64_t *counts_out,
                            uint64_t *num_runs) {
  const size_t ks = dtype_size(kdtype);
  if (ks == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_run_length_encode: unsupported dtype");
  if (!num_runs || (n > 0 && (!keys_in || !keys_out || !counts_out)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_run_length_encode: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_run_length_encode: n must be below 2^32");
  if (n > 0 && (overlaps(keys_out, n * ks, keys_in, n * ks) || overlaps(counts_out, n * 8, keys_in, n * ks)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_run_length_encode: an output overlaps the input");
  DRHIP_GET_SEG(s, seg);
  if (n == 0) return write_zero(s, num_runs);
  return dispatch_key_class(kdtype, [&](auto ktag) {
    using K = decltype(ktag);
    using V = unsigned long long;
    // n < 2^32, so every count of a launch fits 4 bytes: the fold, the stage and the tile shape (8192 elements
    // for 4-byte keys) are those of a 4-byte value, widened to uint64 at the stores
    using A = uint32_t;
    sr_args a;
    if (int rc = state_of<K, V>(s, seg, n, num_runs, &a)) return rc;
    DRHIP_CHECK_HIP((sr_launch_keys_span<K, V, A, A>(s->stream, (const K *)keys_in, sr_one_accessor{}, n, (K *)keys_out,
                                                  (V *)counts_out, KeyEq<K>{}, FoldOp<DRHIP_PLUS, A>{}, a)));
    return (int)DRHIP_OK;
  });
}

int drhip_unique_copy(int seg, int kdtype, const void *keys_in, size_t n, void *keys_out, uint64_t *num_runs) {
  const size_t ks = dtype_size(kdtype);
  if (ks == 0) return set_error(DRHIP_ERR_BAD_ARG, "drhip_unique_copy: unsupported dtype");
  if (!num_runs || (n > 0 && (!keys_in || !keys_out)))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_unique_copy: null pointer");
  if (n >= (size_t(1) << 32)) return set_error(DRHIP_ERR_BAD_ARG, "drhip_unique_copy: n must be below 2^32");
  if (n > 0 && overlaps(keys_out, n * ks, keys_in, n * ks))
    return set_error(DRHIP_ERR_BAD_ARG, "drhip_unique_copy: the output overlaps the input");
  DRHIP_GET_SEG(s, seg);
  if (n == 0) return write_zero(s, num_runs);
  return dispatch_key_class(kdtype, [&](auto ktag) {
    using K = decltype(ktag);
    sr_args a;
    if (int rc = state_of<K, sr_none>(s, seg, n, num_runs, &a)) return rc;
    DRHIP_CHECK_HIP((sr_launch_unique<K>(s->stream, (const K *)keys_in, n, (K *)keys_out, KeyEq<K>{}, a)));
    return (int)DRHIP_OK;
  });
}

} // extern "C"

// bykey.hpp -- what the C-ABI entries of the by-key algorithms share
// (segreduce.hip, segscan.hip): the key classes, the fold in ACC and the
// overlap test of the argument checks.
#pragma once

#include "common.hpp"

namespace drhip {

// Keys are instantiated by class, not by dtype: integers compare as bits,
// floats with the IEEE == (-0.0 == +0.0, a NaN equals nothing).
template <typename K> struct KeyEq {
  __device__ __forceinline__ bool operator()(const K &a, const K &b) const { return a == b; }
};
template <typename F> static int dispatch_key_class(int kdtype, F &&f) {
  switch (kdtype) {
  case DRHIP_I32: case DRHIP_U32: return f(uint32_t{});
  case DRHIP_I64: case DRHIP_U64: return f(uint64_t{});
  case DRHIP_F32: return f(float{});
  case DRHIP_F64: return f(double{});
  default: return set_error(DRHIP_ERR_BAD_ARG, "unsupported key dtype");
  }
}

// The fold runs in ACC inside the tile too (double for F32 / F64, the wrapping
// unsigned type for integer + and *), and the output is rounded once.
template <int OP, typename A> struct FoldOp {
  __device__ __forceinline__ A operator()(A a, A b) const { return Op<OP, A>::apply(a, b); }
};
// value class of (op, dtype): integers of one size share + and *, not min / max
template <int OP, typename T> struct val_class {
  using V = T;
  using A = T;
};
template <int OP> struct val_class<OP, float> {
  using V = float;
  using A = double;
};
template <> struct val_class<DRHIP_PLUS, int32_t> : val_class<DRHIP_PLUS, uint32_t> {};
template <> struct val_class<DRHIP_MUL, int32_t> : val_class<DRHIP_MUL, uint32_t> {};
template <> struct val_class<DRHIP_PLUS, int64_t> : val_class<DRHIP_PLUS, uint64_t> {};
template <> struct val_class<DRHIP_MUL, int64_t> : val_class<DRHIP_MUL, uint64_t> {};

static inline bool overlaps(const void *a, size_t ab, const void *b, size_t bb) {
  const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
  return a0 < b0 + bb && b0 < a0 + ab;
}

} // namespace drhip

// The depthwise 3x3 stencil of the MDTA qkv_dwconv (KDLAE_model.py:120), one output value.
//
// The operation order is part of the numerics contract: the Gram sweeps (mdta.hip) and the dwconv-
// prologue attention-output kernel (attn_out_dw.hip) must give the same bits for a channel of a pixel.
// a = bias, then the taps row-major (t = 3 r + dx) as explicit fused multiply-adds; out-of-image taps
// are zero values, never skipped.
#pragma once
#include <hip/hip_runtime.h>

namespace kdlae {

// one stencil row: the three taps of a row, left to right, onto the running value
__device__ __forceinline__ float dw3_row(float a, float x0, float x1, float x2, float w0, float w1, float w2) {
  a = fmaf(x0, w0, a);
  a = fmaf(x1, w1, a);
  return fmaf(x2, w2, a);
}

// tap(r, dx): the input at row offset r - 1, column offset dx - 1; w[3 r + dx]
template <class Tap>
__device__ __forceinline__ float dw3x3(float bias, const float (&w)[9], Tap&& tap) {
  float a = bias;
#pragma unroll
  for (int r = 0; r < 3; ++r) a = dw3_row(a, tap(r, 0), tap(r, 1), tap(r, 2), w[3 * r], w[3 * r + 1], w[3 * r + 2]);
  return a;
}

}  // namespace kdlae

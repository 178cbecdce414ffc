// NIQE (Train/basicsr/metrics/niqe.py:10-205) up to the per-block moments its AGGD fits need, over a cropped
// window of a stored [B, C, Hs, Ws] tensor.  The host finishes (metrics.finish_niqe): 10 fits per block and
// scale against a 9801-entry table, a 36 x 36 covariance and a pseudo-inverse are not GPU work.
//
//   niqe_prepare_kernel<MODE>  one thread per pixel of the cropped image (a multiple of 96 on each axis):
//                              tensor2img's quantisation (mode 1), / 255, the BT.601 Y row over (B, G, R) in
//                              fp64 for C = 3, * 255, in the reference's operation order -> y1 [B][H'][W'].
//   niqe_half_kernel           the 2 x 2 mean that stands for cv2.resize(.., INTER_LINEAR) at one half
//                              -> y2 [B][H'/2][W'/2].
//   niqe_block_kernel<BS>      grid (blocks, B), 256 threads, one workgroup per 96 x 96 (scale 1) or 48 x 48
//                              (scale 2) block, blockIdx.x in the reference's order (idx_w outer).  In strips of
//                              16 rows: the strip with a halo of 3 to LDS (source indices clamped to the edge of
//                              the scale's image: mode='nearest'), then per pixel mu and E[x^2] over the 49 taps
//                              in scipy's order (flipped window, row-major; fp64 multiply, fp64 add, one rounding
//                              to fp32 at the end), the field f = (x - mu) / (sqrt|E - mu^2| + 1) in correctly
//                              rounded fp32 -> LDS (BS x BS floats) and, when asked for, HBM.  Then the five maps
//                              (f and its fp32 products with itself rolled by (0,1), (1,0), (1,1), (1,-1) inside
//                              the block) are reduced from LDS: per map n_neg, n_pos, sum x^2 over x < 0, over
//                              x > 0 and sum |x| in fp64, thread (pixels tid, tid + 256, ...) -> wave (xor
//                              butterfly) -> block (LDS, waves in index order).  No atomics: equal inputs give
//                              equal bits.
//
// LDS per block at BS = 96: 22 * 102 * 4 + 96 * 96 * 4 + 800 = 46640 B (three blocks per CU).  Traffic: the image
// is read once per scale (plus the halo, 13 % at 96, 27 % at 48); per pixel 49 * 4 fp64 operations, so the
// kernel is bound by the fp64 pipe, not by HBM.  Nothing is contracted: every rounding is the reference's, so
// the arithmetic is written with plain operators under `fp contract(off)` (the __fmul_rn family are header
// functions compiled with the default contraction, which fuses them again once they are inlined, and
// __fsqrt_rn is the 1-ulp native square root; "/" and sqrtf are correctly rounded in HIP).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "runtime.h"

namespace kdlae {
namespace niqe {

constexpr int kThreads = 256;
constexpr int kHalo = kNiqeTaps / 2;
constexpr int kStrip = 16;  // rows of the field formed between two barriers
constexpr int kVals = 25;   // 5 maps x (n_neg, n_pos, s_neg, s_pos, s_abs)

template <int MODE>
__device__ __forceinline__ float quant(float v) {  // tensor2img's uint8 route, as in metrics.hip / ssim.hip
  if (MODE == 0) return v;
  return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void niqe_prepare_kernel(const float* __restrict__ x, int C, int Hs, int Ws,
                                                                int crop, int Hc, int Wc, float* __restrict__ y1) {
#pragma clang fp contract(off)
  const long long n = (long long)Hc * Wc;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int r = (int)(i / Wc), c = (int)(i - (long long)r * Wc);
  const long long plane = (long long)Hs * Ws;
  const float* __restrict__ p = x + (long long)blockIdx.y * C * plane + (long long)(crop + r) * Ws + (crop + c);
  float y;
  if (C == 3) {
    // to_y_channel -> bgr2ycbcr(y_only): np.dot over (B, G, R) and the offset in fp64, / 255., then fp32
    const double R = (double)(quant<MODE>(p[0]) / 255.0f);
    const double G = (double)(quant<MODE>(p[plane]) / 255.0f);
    const double B = (double)(quant<MODE>(p[2 * plane]) / 255.0f);
    const double pb = B * 24.966, pg = G * 128.553, pr = R * 65.481;
    const double d = (((pb + pg) + pr) + 16.0) / 255.0;
    y = (float)d;
  } else {
    y = quant<MODE>(p[0]) / 255.0f;
  }
  y1[(long long)blockIdx.y * n + i] = y * 255.0f;
}

__global__ __launch_bounds__(kThreads) void niqe_half_kernel(const float* __restrict__ y1, int Hc, int Wc,
                                                             float* __restrict__ y2) {
#pragma clang fp contract(off)
  const int H2 = Hc / 2, W2 = Wc / 2;
  const long long n = (long long)H2 * W2;
  const long long i = (long long)blockIdx.x * kThreads + threadIdx.x;
  if (i >= n) return;
  const int r = (int)(i / W2), c = (int)(i - (long long)r * W2);
  const float* __restrict__ p = y1 + (long long)blockIdx.y * Hc * Wc + (long long)(2 * r) * Wc + 2 * c;
  const float a = p[0] / 255.0f, b = p[1] / 255.0f, d = p[Wc] / 255.0f, e = p[Wc + 1] / 255.0f;
  const float top = (a + b) * 0.5f, bot = (d + e) * 0.5f;
  const float v = (top + bot) * 0.5f;
  y2[(long long)blockIdx.y * n + i] = v * 255.0f;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma clang fp contract(off)
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}

template <int BS>
__global__ __launch_bounds__(kThreads) void niqe_block_kernel(const float* __restrict__ y, int Hc, int Wc, int nbh,
                                                              NiqeWindow win, double* __restrict__ out,
                                                              long long out_img_stride, float* __restrict__ field) {
#pragma clang fp contract(off)
  constexpr int kInW = BS + 2 * kHalo, kInH = kStrip + 2 * kHalo;
  static_assert(BS % kStrip == 0 && (kStrip * BS) % kThreads == 0 && (BS * BS) % kThreads == 0, "strip shape");
  __shared__ float s_in[kInH][kInW];
  __shared__ float s_f[BS * BS];
  __shared__ double s_red[kThreads / 64][kVals];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int k = blockIdx.x, bx = k / nbh, by = k - bx * nbh;
  const int y0 = by * BS, x0 = bx * BS;
  const long long img_off = (long long)blockIdx.y * Hc * Wc;
  const float* __restrict__ img = y + img_off;

  for (int s = 0; s < BS; s += kStrip) {
    for (int i = tid; i < kInH * kInW; i += kThreads) {
      const int r = i / kInW, c = i - r * kInW;
      const int sy = min(max(y0 + s + r - kHalo, 0), Hc - 1), sx = min(max(x0 + c - kHalo, 0), Wc - 1);
      s_in[r][c] = img[(long long)sy * Wc + sx];
    }
    __syncthreads();
    for (int i = tid; i < kStrip * BS; i += kThreads) {
      const int r = i / BS, c = i - r * BS;
      double m = 0.0, e = 0.0;
#pragma unroll
      for (int a = 0; a < kNiqeTaps; ++a) {
#pragma unroll
        for (int b = 0; b < kNiqeTaps; ++b) {
          const float v = s_in[r + a][c + b];
          const double w = win.w[a * kNiqeTaps + b];
          const float sq = v * v;  // np.square(img) is fp32
          const double tm = w * (double)v, te = w * (double)sq;
          m = m + tm;
          e = e + te;
        }
      }
      const float mu = (float)m, ex = (float)e;
      const float mu2 = mu * mu;
      const float sigma = sqrtf(fabsf(ex - mu2));
      const float f = (s_in[r + kHalo][c + kHalo] - mu) / (sigma + 1.0f);
      s_f[(s + r) * BS + c] = f;
      if (field) field[img_off + (long long)(y0 + s + r) * Wc + (x0 + c)] = f;
    }
    __syncthreads();  // the next strip's staging overwrites s_in; the last one publishes s_f
  }

  double acc[kVals];
#pragma unroll
  for (int t = 0; t < kVals; ++t) acc[t] = 0.0;
  for (int i = tid; i < BS * BS; i += kThreads) {
    const int r = i / BS, c = i - r * BS;
    const int rm = r == 0 ? BS - 1 : r - 1, cm = c == 0 ? BS - 1 : c - 1, cp = c == BS - 1 ? 0 : c + 1;
    const float f0 = s_f[i];
    // np.roll(block, (s0, s1))[r][c] = block[r - s0][c - s1], wrapped inside the block
    const float v[5] = {f0, f0 * s_f[r * BS + cm], f0 * s_f[rm * BS + c], f0 * s_f[rm * BS + cm],
                        f0 * s_f[rm * BS + cp]};
#pragma unroll
    for (int mp = 0; mp < 5; ++mp) {
      const double d = (double)v[mp];
      const double d2 = d * d;  // exact: the square of a float has 48 bits
      if (v[mp] < 0.f) {
        acc[5 * mp] += 1.0;
        acc[5 * mp + 2] += d2;
      } else if (v[mp] > 0.f) {  // zeros belong to neither side
        acc[5 * mp + 1] += 1.0;
        acc[5 * mp + 3] += d2;
      }
      acc[5 * mp + 4] += fabs(d);
    }
  }
#pragma unroll
  for (int t = 0; t < kVals; ++t) {
    const double v = wave_sum_f64(acc[t]);
    if (lane == 0) s_red[wv][t] = v;
  }
  __syncthreads();
  if (tid < kVals)
    out[(long long)blockIdx.y * out_img_stride + (long long)k * kVals + tid] =
        ((s_red[0][tid] + s_red[1][tid]) + s_red[2][tid]) + s_red[3][tid];
}

// floats of y1 and y2 for B images whose window is h x w before the crop
inline int64_t scratch_floats(int64_t B, int64_t h, int64_t w) {
  const int64_t n = (h / kNiqeBlock * kNiqeBlock) * (w / kNiqeBlock * kNiqeBlock);
  return B * (n + n / 4);
}

}  // namespace niqe
}  // namespace kdlae

using namespace kdlae;

extern "C" {

int64_t kdlae_metric_niqe_scratch_bytes(int B, int h, int w) {
  if (B < 1 || h < 1 || w < 1) return 0;
  return (niqe::scratch_floats(B, h, w) * (int64_t)sizeof(float) + 255) / 256 * 256 + 256;
}

int kdlae_metric_niqe(const float* x, int B, int C, int Hs, int Ws, int h, int w, int crop_border, int mode,
                      int convert, const double* window49, double* out, float* field_s1, float* field_s2,
                      void* scratch, int64_t scratch_bytes, void* stream) {
  if (!x || !window49 || !out || !scratch) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_niqe: null argument");
  if (mode != 0 && mode != 1) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_niqe: mode must be 0 (float) or 1 (uint8)");
  if (convert != 0)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_niqe: convert must be 0 (Y of MATLAB YCbCr); 'gray' is cv2's conversion");
  if (C != 1 && C != 3)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: C must be 1 (taken as it is) or 3 (RGB -> Y), got " + std::to_string(C));
  if (B < 1 || B > 65535 || h < 1 || w < 1 || h > Hs || w > Ws)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: need 1 <= B <= 65535 and a window 1 <= h <= Hs, 1 <= w <= Ws");
  if (crop_border < 0 || 2ll * crop_border >= h || 2ll * crop_border >= w)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: crop_border leaves no pixel of the " + std::to_string(h) + "x" +
                                        std::to_string(w) + " window");
  const int hh = h - 2 * crop_border, ww = w - 2 * crop_border;
  if (hh < kNiqeBlock || ww < kNiqeBlock)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: needs at least one 96 x 96 block after the crop, got " +
                                        std::to_string(hh) + "x" + std::to_string(ww));
  const int nbh = hh / kNiqeBlock, nbw = ww / kNiqeBlock, Hc = nbh * kNiqeBlock, Wc = nbw * kNiqeBlock;
  const long long nblk = (long long)nbh * nbw, n1 = (long long)Hc * Wc;
  const int64_t need = niqe::scratch_floats(B, hh, ww) * (int64_t)sizeof(float);
  if (scratch_bytes < need || ((uintptr_t)scratch & 3))
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: scratch of " + std::to_string(scratch_bytes) + " bytes, need " +
                                        std::to_string(need) + " (4-byte aligned)");
  if (ceil_div(n1, niqe::kThreads) > 0x7fffffffll || nblk > 0x7fffffffll)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_niqe: image too large");
  hipStream_t s = (hipStream_t)stream;

  NiqeWindow win;  // scipy's convolve walks the flipped window
  for (int t = 0; t < kNiqeTaps * kNiqeTaps; ++t) win.w[t] = window49[kNiqeTaps * kNiqeTaps - 1 - t];
  float* y1 = (float*)scratch;
  float* y2 = y1 + (long long)B * n1;
  const long long img_stride = 2 * nblk * niqe::kVals;

  const dim3 block(niqe::kThreads);
  const dim3 g1((unsigned)ceil_div(n1, niqe::kThreads), B), g2((unsigned)ceil_div(n1 / 4, niqe::kThreads), B);
  if (mode == 0)
    hipLaunchKernelGGL(niqe::niqe_prepare_kernel<0>, g1, block, 0, s, x, C, Hs, Ws, crop_border, Hc, Wc, y1);
  else
    hipLaunchKernelGGL(niqe::niqe_prepare_kernel<1>, g1, block, 0, s, x, C, Hs, Ws, crop_border, Hc, Wc, y1);
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) {
    hipLaunchKernelGGL(niqe::niqe_half_kernel, g2, block, 0, s, y1, Hc, Wc, y2);
    e = hipGetLastError();
  }
  const dim3 gb((unsigned)nblk, B);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(niqe::niqe_block_kernel<kNiqeBlock>, gb, block, 0, s, y1, Hc, Wc, nbh, win, out, img_stride,
                       field_s1);
    e = hipGetLastError();
  }
  if (e == hipSuccess) {
    hipLaunchKernelGGL(niqe::niqe_block_kernel<kNiqeBlock / 2>, gb, block, 0, s, y2, Hc / 2, Wc / 2, nbh, win,
                       out + nblk * niqe::kVals, img_stride, field_s2);
    e = hipGetLastError();
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

}  // extern "C"

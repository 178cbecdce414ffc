// Validation metric kernels: SSIM per image over a cropped window of a stored [B, C, Hs, Ws] tensor, in fp64
// and in a fixed order.  Two flavours of the same five windowed moments (mu1, mu2, E[x^2], E[y^2], E[xy], the
// 11 taps of a sigma 1.5 Gaussian on each axis) and the same map:
//
//   variant 0  calculate_ssim -> _ssim_3d (Train/basicsr/metrics/psnr_ssim.py:146-197,240-318): the 11^3
//              Conv3d over the (H, W, C) volume with replicate padding.  Along H and W that is the 11-tap
//              filter with indices clamped to the compared window; along C it is a C x C matrix (the taps
//              that clamp onto one channel added up), computed by the host and passed by value.
//   variant 1  Train/utils.py:31-78 (= _ssim, psnr_ssim.py:73-114): per channel, valid positions only
//              (the [5:-5, 5:-5] cut), L = 255.
//
// The filter and the channel matrix are linear and commute, so the kernel filters each stored channel's
// five product fields in space and applies the matrix last, in registers:
//
//   stage 1  ssim_partial_kernel  grid (nblk, B), 256 threads = one 16 x 16 tile of map positions.  A block
//            takes tiles blockIdx.x, + nblk, ... of its image.  Per tile and stored channel: both operands'
//            26 x 26 patch (tile + halo of 5, source indices clamped to the window; quantised in mode 1)
//            to LDS as fp32 -> horizontal pass, five fp64 fields of 26 x 16, to LDS -> vertical pass, one
//            position per thread -> acc[c][field] += M[c][channel] * value (variant 0) or the map at once
//            (variant 1).  Then the map with the L = 1 and the L = 255 constants (the host picks by the
//            maximum, so nothing synchronises), lane -> wave (xor butterfly) -> block (LDS, waves in index
//            order): one (sum L=1, sum L=255, max) triple per block.
//   stage 2  ssim_final_kernel    grid (B): one wave adds the nblk triples, lane l taking l, l + 64, ...
//
// LDS per block: 2 * 26 * 26 * 4 + 5 * 26 * 16 * 8 + 80 = 22128 B, which alone would let seven blocks share a
// CU's 160 KiB; the 100 (variant 0) / 112 (variant 1) VGPRs allow 4 waves per SIMD, so four blocks per CU.
// No atomics, so the bits depend only on the shape.  Every global read is of a clamped index inside the
// compared window: nothing outside it is touched, whatever the storage around it holds.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "runtime.h"

namespace kdlae {
namespace ssim {

constexpr int kThreads = 256;
constexpr int kTile = 16;  // map positions per tile side: kTile * kTile == kThreads
constexpr int kHalo = 5, kTaps = 2 * kHalo + 1;
constexpr int kIn = kTile + 2 * kHalo;  // staged patch side
constexpr int kMaxC = 4;                // channels variant 0 mixes (acc[kMaxC][5] lives in registers)
constexpr int kMaxPart = 16384;         // triples the scratch holds: blocks of one launch, all images
constexpr int kPartStride = 4;          // doubles per triple (padded)

struct Coef {
  double g[kTaps];          // the normalised taps
  double m[kMaxC][kMaxC];   // variant 0: m[c][c'] = sum of g[t] over clamp(c + t - 5, 0, C - 1) == c'
};

template <int MODE>
__device__ __forceinline__ float quant(float v) {  // tensor2img's uint8 route, as in metrics.hip
  if (MODE == 0) return v;
  return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

// One map entry.  No contraction: with equal operands the numerator and the denominator must be the same
// sequence of roundings (2 p == p + p exactly), so that the quotient is exactly 1.
__device__ __forceinline__ double map_entry(double mu1, double mu2, double e11, double e22, double e12, double c1,
                                            double c2) {
#pragma clang fp contract(off)
  const double m11 = mu1 * mu1, m22 = mu2 * mu2, m12 = mu1 * mu2;
  const double s11 = e11 - m11, s22 = e22 - m22, s12 = e12 - m12;
  const double num = (2.0 * m12 + c1) * (2.0 * s12 + c2);
  const double den = (m11 + m22 + c1) * (s11 + s22 + c2);
  return num / den;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

template <int MODE, int VARIANT>
__global__ __launch_bounds__(kThreads) void ssim_partial_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ gt, int b0, int C, int Hs,
                                                                int Ws, int Hg, int Wg, int hh, int ww, int crop,
                                                                int tiles_x, long long ntiles, Coef cf, double c1_1,
                                                                double c2_1, double c1_255, double c2_255,
                                                                double* __restrict__ part) {
  __shared__ float sa[kIn][kIn], sb[kIn][kIn];
  __shared__ double hp[5][kIn][kTile];
  __shared__ double sh_s[2][kThreads / 64];
  __shared__ float sh_m[kThreads / 64];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int tx = tid & (kTile - 1), ty = tid / kTile;
  const long long img = (long long)b0 + blockIdx.y;
  const long long plane = (long long)Hs * Ws, plane_g = (long long)Hg * Wg;
  // map extent; a staged patch starts kHalo before the tile (variant 0) or at it (variant 1)
  const int map_h = VARIANT == 0 ? hh : hh - 2 * kHalo, map_w = VARIANT == 0 ? ww : ww - 2 * kHalo;
  const int shift = VARIANT == 0 ? kHalo : 0;
  double s1 = 0.0, s255 = 0.0;
  float mx = -INFINITY;
  for (long long tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int y0 = (int)(tile / tiles_x) * kTile, x0 = (int)(tile % tiles_x) * kTile;
    const bool live = y0 + ty < map_h && x0 + tx < map_w;
    double acc[kMaxC][5];
#pragma unroll
    for (int c = 0; c < kMaxC; ++c)
#pragma unroll
      for (int f = 0; f < 5; ++f) acc[c][f] = 0.0;
    for (int cp = 0; cp < C; ++cp) {
      const float* __restrict__ pa = pred + ((img * C + cp) * plane + (long long)crop * Ws + crop);
      const float* __restrict__ pb = gt + ((img * C + cp) * plane_g + (long long)crop * Wg + crop);
      for (int i = tid; i < kIn * kIn; i += kThreads) {
        const int r = i / kIn, c = i - r * kIn;
        const int sy = min(max(y0 + r - shift, 0), hh - 1), sx = min(max(x0 + c - shift, 0), ww - 1);
        const float a = quant<MODE>(pa[(long long)sy * Ws + sx]);
        const float b = quant<MODE>(pb[(long long)sy * Wg + sx]);
        sa[r][c] = a;
        sb[r][c] = b;
        mx = fmaxf(mx, a);
      }
      __syncthreads();
      for (int i = tid; i < kIn * kTile; i += kThreads) {
        const int r = i / kTile, x = i & (kTile - 1);
        double h0 = 0.0, h1 = 0.0, h2 = 0.0, h3 = 0.0, h4 = 0.0;
#pragma unroll
        for (int t = 0; t < kTaps; ++t) {
          const double a = (double)sa[r][x + t], b = (double)sb[r][x + t], g = cf.g[t];
          h0 = fma(g, a, h0);
          h1 = fma(g, b, h1);
          h2 = fma(g, a * a, h2);  // the products of two floats are exact in fp64
          h3 = fma(g, b * b, h3);
          h4 = fma(g, a * b, h4);
        }
        hp[0][r][x] = h0;
        hp[1][r][x] = h1;
        hp[2][r][x] = h2;
        hp[3][r][x] = h3;
        hp[4][r][x] = h4;
      }
      __syncthreads();
      double v[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
      for (int t = 0; t < kTaps; ++t) {
        const double g = cf.g[t];
#pragma unroll
        for (int f = 0; f < 5; ++f) v[f] = fma(g, hp[f][ty + t][tx], v[f]);
      }
      if (VARIANT == 0) {
#pragma unroll
        for (int c = 0; c < kMaxC; ++c) {
          if (c < C) {
            const double m = cf.m[c][cp];
#pragma unroll
            for (int f = 0; f < 5; ++f) acc[c][f] = fma(m, v[f], acc[c][f]);
          }
        }
      } else if (live) {
        s255 += map_entry(v[0], v[1], v[2], v[3], v[4], c1_255, c2_255);
      }
      // the next channel's staging writes sa / sb, which nobody reads past the barrier above; its
      // horizontal pass writes hp only after the barrier that follows the staging
    }
    if (VARIANT == 0 && live) {
#pragma unroll
      for (int c = 0; c < kMaxC; ++c) {
        if (c < C) {
          s1 += map_entry(acc[c][0], acc[c][1], acc[c][2], acc[c][3], acc[c][4], c1_1, c2_1);
          s255 += map_entry(acc[c][0], acc[c][1], acc[c][2], acc[c][3], acc[c][4], c1_255, c2_255);
        }
      }
    }
  }
  s1 = wave_sum_f64(s1);
  s255 = wave_sum_f64(s255);
  mx = wave_max_f32(mx);
  if (lane == 0) {
    sh_s[0][wv] = s1;
    sh_s[1][wv] = s255;
    sh_m[wv] = mx;
  }
  __syncthreads();
  if (tid == 0) {
    const long long slot = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    part[kPartStride * slot] = ((sh_s[0][0] + sh_s[0][1]) + sh_s[0][2]) + sh_s[0][3];
    part[kPartStride * slot + 1] = ((sh_s[1][0] + sh_s[1][1]) + sh_s[1][2]) + sh_s[1][3];
    part[kPartStride * slot + 2] = (double)fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
  }
}

__global__ __launch_bounds__(64) void ssim_final_kernel(const double* __restrict__ part, int nblk, int b0, double n,
                                                        double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double* __restrict__ p = part + (long long)kPartStride * blockIdx.x * nblk;
  double s1 = 0.0, s255 = 0.0, mx = -INFINITY;
  for (int j = lane; j < nblk; j += 64) {
    s1 += p[kPartStride * j];
    s255 += p[kPartStride * j + 1];
    mx = fmax(mx, p[kPartStride * j + 2]);
  }
  s1 = wave_sum_f64(s1);
  s255 = wave_sum_f64(s255);
  for (int m = 32; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m, 64));
  if (lane == 0) {
    double* o = out + 4ll * (b0 + blockIdx.x);
    o[0] = s1;
    o[1] = s255;
    o[2] = mx;
    o[3] = n;
  }
}

}  // namespace ssim
}  // namespace kdlae

using namespace kdlae;

extern "C" {

int64_t kdlae_metric_ssim_scratch_bytes(void) {
  return (int64_t)ssim::kMaxPart * ssim::kPartStride * sizeof(double);
}

int kdlae_metric_ssim(const float* pred, const float* gt, int B, int C, int Hs, int Ws, int Hg, int Wg, int h, int w,
                      int crop_border, int mode, int variant, double* out, void* scratch, void* stream) {
  if (!pred || !gt || !out || !scratch) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_ssim: null argument");
  if (mode != 0 && mode != 1) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_ssim: mode must be 0 (float) or 1 (uint8)");
  if (variant != 0 && variant != 1)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_ssim: variant must be 0 (basicsr, replicate 3-D window) or 1 (valid)");
  if (B < 1 || C < 1 || h < 1 || w < 1 || h > Hs || w > Ws || h > Hg || w > Wg)
    return fail(KDLAE_EINVAL_SHAPE,
                "kdlae_metric_ssim: need B, C >= 1 and a valid window 1 <= h <= min(Hs, Hg), 1 <= w <= min(Ws, Wg)");
  if (crop_border < 0 || 2ll * crop_border >= h || 2ll * crop_border >= w)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_ssim: crop_border leaves no pixel of the " + std::to_string(h) + "x" +
                                        std::to_string(w) + " window");
  const int hh = h - 2 * crop_border, ww = w - 2 * crop_border;
  if (variant == 1 && (hh < ssim::kTaps || ww < ssim::kTaps))
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_ssim: variant 1 (valid positions) needs at least 11 x 11 pixels after "
                                    "the crop, got " + std::to_string(hh) + "x" + std::to_string(ww));
  if (variant == 0 && C > ssim::kMaxC)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_ssim: variant 0 mixes 1 <= C <= 4 channels, got C = " + std::to_string(C));
  hipStream_t s = (hipStream_t)stream;

  ssim::Coef cf = {};
  double sum = 0.0;
  for (int t = 0; t < ssim::kTaps; ++t) {
    const double d = t - ssim::kHalo;
    cf.g[t] = std::exp(-(d * d) / (2.0 * 1.5 * 1.5));
    sum += cf.g[t];
  }
  for (int t = 0; t < ssim::kTaps; ++t) cf.g[t] /= sum;
  if (variant == 0)
    for (int c = 0; c < C; ++c)
      for (int t = 0; t < ssim::kTaps; ++t) cf.m[c][std::min(std::max(c + t - ssim::kHalo, 0), C - 1)] += cf.g[t];
  const double c1_1 = (0.01 * 1.0) * (0.01 * 1.0), c2_1 = (0.03 * 1.0) * (0.03 * 1.0);
  const double c1_255 = (0.01 * 255.0) * (0.01 * 255.0), c2_255 = (0.03 * 255.0) * (0.03 * 255.0);

  const int map_h = variant == 0 ? hh : hh - 2 * ssim::kHalo, map_w = variant == 0 ? ww : ww - 2 * ssim::kHalo;
  const int tiles_x = (int)ceil_div(map_w, ssim::kTile);
  const long long ntiles = (long long)tiles_x * ceil_div(map_h, ssim::kTile);
  const double n = (double)C * (double)map_h * (double)map_w;
  double* part = (double*)scratch;
  // one block per tile while the scratch holds a triple for each; past that a block walks several tiles,
  // and a batch larger than the scratch holds triples goes out in several launches
  for (int b0 = 0; b0 < B; b0 += ssim::kMaxPart) {
    const int nb = std::min(B - b0, ssim::kMaxPart);
    const int nblk = (int)std::max(1ll, std::min(ntiles, (long long)(ssim::kMaxPart / nb)));
    const dim3 grid(nblk, nb), block(ssim::kThreads);
#define KDLAE_SSIM_LAUNCH(M, V)                                                                                      \
  hipLaunchKernelGGL((ssim::ssim_partial_kernel<M, V>), grid, block, 0, s, pred, gt, b0, C, Hs, Ws, Hg, Wg, hh, ww, \
                     crop_border, tiles_x, ntiles, cf, c1_1, c2_1, c1_255, c2_255, part)
    if (mode == 0 && variant == 0)
      KDLAE_SSIM_LAUNCH(0, 0);
    else if (mode == 1 && variant == 0)
      KDLAE_SSIM_LAUNCH(1, 0);
    else if (mode == 0)
      KDLAE_SSIM_LAUNCH(0, 1);
    else
      KDLAE_SSIM_LAUNCH(1, 1);
#undef KDLAE_SSIM_LAUNCH
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(ssim::ssim_final_kernel, dim3(nb), dim3(64), 0, s, part, nblk, b0, n, out);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  }
  return KDLAE_OK;
}

}  // extern "C"

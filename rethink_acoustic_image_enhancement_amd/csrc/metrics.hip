// Validation metric kernels: the two reductions calculate_psnr (Train/basicsr/metrics/psnr_ssim.py:53-70)
// needs per image, over a cropped window of a stored [B, C, Hs, Ws] tensor, in fp64 and in a fixed order.
//
//   stage 1  psnr_partial_kernel  grid (nblk, B): block j of image b takes rows j, j + nblk, ... of the
//            C * (h - 2 crop) window rows in groups of four (one row per wave, the 64 lanes across the row);
//            lane -> wave (xor butterfly) -> block (LDS, waves in index order) gives one (sse, max) pair.
//   stage 2  psnr_final_kernel    grid (B): one wave adds the nblk pairs, lane l taking l, l + 64, ...
//
// No atomics anywhere, so the bits depend only on the shape and on the operands' 16-byte alignment.  The
// float -> double difference is exact; what the reference's astype(np.float64) computes differs from this
// only in the order of the fp64 additions.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "runtime.h"

namespace kdlae {
namespace metric {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 4096;  // (sse, max) pairs the scratch holds: blocks of one launch, all images

// tensor2img's uint8 route (Train/basicsr/utils/img_util.py:67-68,91-94): clamp to [0, 1] in fp32, * 255 in
// fp32, np.round (half to even).  The value stays a float holding an integer 0..255.
template <int MODE>
__device__ __forceinline__ float quant(float v) {
  if (MODE == 0) return v;
  return rintf(fminf(fmaxf(v, 0.f), 1.f) * 255.0f);
}

template <int MODE>
__device__ __forceinline__ void take(float p, float g, double& sse, float& mx) {
  p = quant<MODE>(p);
  g = quant<MODE>(g);
  const double d = (double)p - (double)g;
  sse = fma(d, d, sse);
  mx = fmaxf(mx, p);
}

__device__ __forceinline__ double wave_sum_f64(double v) {
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max_f32(float v) {
  for (int m = 32; m >= 1; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void psnr_partial_kernel(const float* __restrict__ pred,
                                                                const float* __restrict__ gt, int b0, int C, int Hs,
                                                                int Ws, int Hg, int Wg, int hh, int ww, int crop,
                                                                double* __restrict__ part) {
  __shared__ double sh_s[kThreads / 64];
  __shared__ float sh_m[kThreads / 64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const long long img = (long long)b0 + blockIdx.y;
  const long long rows = (long long)C * hh;  // window rows of one image
  const long long plane = (long long)Hs * Ws, plane_g = (long long)Hg * Wg;
  double sse = 0.0;
  float mx = -INFINITY;
  for (long long r = (long long)blockIdx.x * (kThreads / 64) + wv; r < rows;
       r += (long long)gridDim.x * (kThreads / 64)) {
    const long long c = r / hh, y = r - c * hh;
    const long long off = (img * C + c) * plane + (y + crop) * (long long)Ws + crop;
    const float* __restrict__ p = pred + off;
    const float* __restrict__ g = gt + ((img * C + c) * plane_g + (y + crop) * (long long)Wg + crop);
    const unsigned mp = (unsigned)((uintptr_t)p & 15), mg = (unsigned)((uintptr_t)g & 15);
    if (mp == mg) {
      // head to the next 16-byte boundary, float4 body, tail
      int head = (int)(((16u - mp) & 15u) >> 2);
      if (head > ww) head = ww;
      const int nvec = (ww - head) >> 2;
      const int tail0 = head + (nvec << 2);
      if (lane < head) take<MODE>(p[lane], g[lane], sse, mx);
      const float4* __restrict__ p4 = reinterpret_cast<const float4*>(p + head);
      const float4* __restrict__ g4 = reinterpret_cast<const float4*>(g + head);
      for (int j = lane; j < nvec; j += 64) {
        const float4 a = p4[j], b = g4[j];
        take<MODE>(a.x, b.x, sse, mx);
        take<MODE>(a.y, b.y, sse, mx);
        take<MODE>(a.z, b.z, sse, mx);
        take<MODE>(a.w, b.w, sse, mx);
      }
      if (lane < ww - tail0) take<MODE>(p[tail0 + lane], g[tail0 + lane], sse, mx);
    } else {
      // the operands sit at different offsets within 16 bytes: no common float4 grid, element loads
      for (int x = lane; x < ww; x += 64) take<MODE>(p[x], g[x], sse, mx);
    }
  }
  sse = wave_sum_f64(sse);
  mx = wave_max_f32(mx);
  if (lane == 0) {
    sh_s[wv] = sse;
    sh_m[wv] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    const long long slot = (long long)blockIdx.y * gridDim.x + blockIdx.x;
    part[2 * slot] = ((sh_s[0] + sh_s[1]) + sh_s[2]) + sh_s[3];
    part[2 * slot + 1] = (double)fmaxf(fmaxf(sh_m[0], sh_m[1]), fmaxf(sh_m[2], sh_m[3]));
  }
}

__global__ __launch_bounds__(64) void psnr_final_kernel(const double* __restrict__ part, int nblk, int b0,
                                                        double* __restrict__ out) {
  const int lane = threadIdx.x;
  const double* __restrict__ p = part + 2ll * blockIdx.x * nblk;
  double sse = 0.0, mx = -INFINITY;
  for (int j = lane; j < nblk; j += 64) {
    sse += p[2 * j];
    mx = fmax(mx, p[2 * j + 1]);
  }
  sse = wave_sum_f64(sse);
  for (int m = 32; m >= 1; m >>= 1) mx = fmax(mx, __shfl_xor(mx, m, 64));
  if (lane == 0) {
    out[2ll * (b0 + blockIdx.x)] = sse;
    out[2ll * (b0 + blockIdx.x) + 1] = mx;
  }
}

}  // namespace metric
}  // namespace kdlae

using namespace kdlae;

extern "C" {

int64_t kdlae_metric_scratch_bytes(void) { return (int64_t)metric::kMaxBlocks * 2 * sizeof(double); }

int kdlae_metric_psnr(const float* pred, const float* gt, int B, int C, int Hs, int Ws, int Hg, int Wg, int h, int w,
                      int crop_border, int mode, double* out, void* scratch, void* stream) {
  if (!pred || !gt || !out || !scratch) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_psnr: null argument");
  if (mode != 0 && mode != 1) return fail(KDLAE_EINVAL_CONFIG, "kdlae_metric_psnr: mode must be 0 (float) or 1 (uint8)");
  if (B < 1 || C < 1 || h < 1 || w < 1 || h > Hs || w > Ws || h > Hg || w > Wg)
    return fail(KDLAE_EINVAL_SHAPE,
                "kdlae_metric_psnr: need B, C >= 1 and a valid window 1 <= h <= min(Hs, Hg), 1 <= w <= min(Ws, Wg)");
  if (crop_border < 0 || 2ll * crop_border >= h || 2ll * crop_border >= w)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_metric_psnr: crop_border leaves no pixel of the " + std::to_string(h) + "x" +
                                        std::to_string(w) + " window");
  hipStream_t s = (hipStream_t)stream;
  const int hh = h - 2 * crop_border, ww = w - 2 * crop_border;
  const long long rows = (long long)C * hh;
  double* part = (double*)scratch;
  // every block sums at least two rows per wave when there are that many; all images of one launch share
  // the scratch, so a batch larger than it holds pairs goes out in several launches
  for (int b0 = 0; b0 < B; b0 += metric::kMaxBlocks) {
    const int nb = std::min(B - b0, metric::kMaxBlocks);
    const int nblk = (int)std::max(1ll, std::min(ceil_div(rows, 8), (long long)(metric::kMaxBlocks / nb)));
    const dim3 grid(nblk, nb);
    if (mode == 0)
      hipLaunchKernelGGL(metric::psnr_partial_kernel<0>, grid, dim3(metric::kThreads), 0, s, pred, gt, b0, C, Hs, Ws, Hg, Wg,
                         hh, ww, crop_border, part);
    else
      hipLaunchKernelGGL(metric::psnr_partial_kernel<1>, grid, dim3(metric::kThreads), 0, s, pred, gt, b0, C, Hs, Ws, Hg, Wg,
                         hh, ww, crop_border, part);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) {
      hipLaunchKernelGGL(metric::psnr_final_kernel, dim3(nb), dim3(64), 0, s, part, nblk, b0, out);
      e = hipGetLastError();
    }
    if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  }
  return KDLAE_OK;
}

}  // extern "C"

// Rate sweep kernels (kdlae_t_forward_rates, kdlae_rate_select): both move bytes and compute nothing.
//
//   rate_fanout_kernel  the `output` conv's B NHWC-4 images -> R B NHWC-4 images whose channel `ch` holds the
//                       denoise rate of (r, b): what small_out(..., extra = rate) leaves for output_param in
//                       kdlae_t_forward, for every rate at once.  One float4 load and one float4 store per
//                       output pixel, consecutive lanes on consecutive pixels; R B H W passes 2^31 at the
//                       workload's sizes, so every index is 64-bit.
//   rate_select_kernel  grid (nblk, B): every block scans the R scores of its image in index order (so ties
//                       go to the lowest r with no reduction to order), block (0, b) writes the index, and the
//                       blocks of image b copy the chosen candidate.  No atomics.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "runtime.h"

namespace kdlae {

__global__ __launch_bounds__(256) void rate_fanout_kernel(const float4* __restrict__ src,
                                                          const float* __restrict__ rates, int is_map, int ch, int B,
                                                          long long HW, long long total, float4* __restrict__ dst) {
  for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += (long long)gridDim.x * 256) {
    const long long rb = i / HW, p = i - rb * HW;
    const long long b = rb % B;
    float4 v = src[b * HW + p];
    const float rate = is_map ? rates[i] : rates[rb];
    if (ch == 0) v.x = rate;
    else if (ch == 1) v.y = rate;
    else if (ch == 2) v.z = rate;
    else v.w = rate;
    dst[i] = v;
  }
}

hipError_t launch_rate_fanout(const float* src, const float* rates, int is_map, int ch, int B, int R, long long HW,
                              float* dst, hipStream_t s) {
  if (ch < 0 || ch > 3 || B < 1 || R < 1 || HW < 1 || !al16(src) || !al16(dst)) return hipErrorInvalidValue;
  const long long total = (long long)R * B * HW;
  const long long blocks = std::min<long long>(ceil_div(total, 256), 256LL * 32);
  hipLaunchKernelGGL(rate_fanout_kernel, dim3((unsigned)blocks), dim3(256), 0, s,
                     reinterpret_cast<const float4*>(src), rates, is_map, ch, B, HW, total,
                     reinterpret_cast<float4*>(dst));
  return hipGetLastError();
}

__global__ __launch_bounds__(256) void rate_select_kernel(const float* __restrict__ scores, int R, int B, int mode,
                                                          const float* __restrict__ target,
                                                          const float* __restrict__ hq, long long per_image,
                                                          int32_t* __restrict__ index_out,
                                                          float* __restrict__ hq_out) {
  const int b = blockIdx.y;
  // every thread scans the same R scores (broadcast loads): the first strictly better key wins
  const float t = mode == 0 ? target[b] : 0.f;
  int best = -1;
  float bk = 0.f;
  for (int r = 0; r < R; ++r) {
    const float sc = scores[(long long)r * B + b];
    const float k = mode == 0 ? fabsf(sc - t) : (mode == 1 ? -sc : sc);
    if (k != k) continue;  // NaN: never chosen
    if (best < 0 || k < bk) {
      best = r;
      bk = k;
    }
  }
  if (best < 0) best = 0;
  if (blockIdx.x == 0 && threadIdx.x == 0) index_out[b] = best;
  const float* __restrict__ s = hq + ((long long)best * B + b) * per_image;
  float* __restrict__ d = hq_out + (long long)b * per_image;
  const long long tid = blockIdx.x * 256LL + threadIdx.x, nth = (long long)gridDim.x * 256;
  const unsigned ms = (unsigned)((uintptr_t)s & 15), md = (unsigned)((uintptr_t)d & 15);
  if (ms == md) {
    // head to the next 16-byte boundary, float4 body, tail
    long long head = ((16u - ms) & 15u) >> 2;
    if (head > per_image) head = per_image;
    const long long nvec = (per_image - head) >> 2, tail0 = head + (nvec << 2);
    if (tid < head) d[tid] = s[tid];
    const float4* __restrict__ s4 = reinterpret_cast<const float4*>(s + head);
    float4* __restrict__ d4 = reinterpret_cast<float4*>(d + head);
    for (long long j = tid; j < nvec; j += nth) d4[j] = s4[j];
    if (tid < per_image - tail0) d[tail0 + tid] = s[tail0 + tid];
  } else {
    // source and destination sit at different offsets within 16 bytes: no common float4 grid
    for (long long j = tid; j < per_image; j += nth) d[j] = s[j];
  }
}

}  // namespace kdlae

using namespace kdlae;

extern "C" int kdlae_rate_select(const float* scores, int R, int B, int mode, const float* target, const float* hq,
                                 int64_t per_image, int32_t* index_out, float* hq_out, void* stream) {
  if (!scores || !hq || !index_out || !hq_out) return fail(KDLAE_EINVAL_CONFIG, "kdlae_rate_select: null argument");
  if (mode < 0 || mode > 2)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_rate_select: mode must be 0 (closest to target), 1 (max) or 2 (min)");
  if (mode == 0 && !target) return fail(KDLAE_EINVAL_CONFIG, "kdlae_rate_select: mode 0 needs a target per image");
  if (R < 1 || B < 1 || per_image < 1 || B > 65535)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_rate_select: need R >= 1, 1 <= B <= 65535 and per_image >= 1");
  // 4 float4 per thread and pass; the grid covers one image's copy, every image takes grid.y
  const long long nblk = std::max(1LL, std::min(ceil_div(per_image, 4 * 256 * 4), 64LL));
  hipLaunchKernelGGL(rate_select_kernel, dim3((unsigned)nblk, (unsigned)B), dim3(256), 0, (hipStream_t)stream, scores,
                     R, B, mode, target, hq, (long long)per_image, index_out, hq_out);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

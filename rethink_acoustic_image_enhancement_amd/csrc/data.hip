// Dataset sample transforms of the two training datasets (Train/basicsr/data/paired_image_dataset.py:160-294,
// 902-982) on device buffers: what runs per sample between image decode and the batch.
//
//   data_sample_kernel  one launch for a table of items (grid.y = item).  An item reads one source image (u8 or
//                       fp32, any element strides) through a virtual canvas (centre zero pad, then a bottom/right
//                       reflect pad), a window, one of the eight dihedral index maps and an optional channel
//                       reversal, and writes one fp32 CHW slot: u8 -> v / 255, optional Gaussian noise in fp64
//                       with the clip to [0, 1], optional (x - mean) / std.
//   data_count_kernel   per sample the number of elements == 0 and == 1 (integer adds only).
//   data_finish_kernel  in place per sample: x + nudge when the counts say so, then the optional normalisation.
//
// Plain streaming kernels as prepare_kernel (augment.hip) is: no LDS, 64-bit element indices, grid-stride
// loops.  The arithmetic the reference does in two steps is kept in two steps (explicitly rounded adds,
// multiplies and divides), so nothing is contracted into an FMA.  Noise normals come from the caller's fp64 array
// or from Philox4x32-10 (philox.h): key = seed, counter = (e / 2, call + item), e the linear index of the
// pre-dihedral window element (i, j, c) in [h, w, C]; an even e takes words 0, 1 of its block and an odd e words
// 2, 3; u1 = ((w0 >> 8) + 1) * 2^-24, u2 = (w1 >> 8) * 2^-24, z = sqrtf(-2 logf(u1)) * cosf(2 pi u2).
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox.h"
#include "runtime.h"

namespace kdlae {
namespace data {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // per launch, shared by the items of a table
constexpr int kMaxItems = 65535;  // grid.y

enum Pad { kPadNone = 0, kPadReflect101 = 1, kPadSymmetric = 2 };
enum Noise { kNoiseOff = 0, kNoiseArray = 1, kNoisePhilox = 2 };

// canvas coordinate p >= 0 of an axis whose first n entries exist -> the entry it mirrors
__device__ __forceinline__ int fold(int p, int n, int mode) {
  if (p < n) return p;
  if (mode == kPadSymmetric) {
    const int m = p % (2 * n);
    return m < n ? m : 2 * n - 1 - m;
  }
  if (n == 1) return 0;
  const int per = 2 * n - 2, m = p % per;
  return m < n ? m : per - m;
}

// the reference's condition on the counts of exact zeros and ones: max(c0, c1) / n > thr in fp64
__device__ __forceinline__ bool counts_say(const int32_t* c, long long n, double thr) {
  const int32_t m = c[0] > c[1] ? c[0] : c[1];
  return __ddiv_rn((double)m, (double)n) > thr;
}

__global__ __launch_bounds__(kThreads) void data_sample_kernel(const kdlae_data_item* items, unsigned k0, unsigned k1,
                                                               unsigned long long call) {
  const kdlae_data_item& it = items[blockIdx.y];
  const int h = it.h, w = it.w, C = it.C;
  const long long n = (long long)C * h * w;
  const bool tr = it.dihedral & 4, fr = it.dihedral & 2, fc = it.dihedral & 1;
  const int ho = tr ? w : h, wo = tr ? h : w;
  const int cy = (it.Hc - it.Hs) / 2, cx = (it.Wc - it.Ws) / 2;
  const bool noisy = it.noise != kNoiseOff && (!it.counts || counts_say(it.counts, it.count_n, it.count_thr));
  const unsigned long long cl = call + blockIdx.y;
  for (long long o = (long long)blockIdx.x * kThreads + threadIdx.x; o < n; o += (long long)gridDim.x * kThreads) {
    // o -> (co, io, jo) of dst [C, ho, wo] -> window (i, j), source channel c
    const long long r = o / wo;
    const int jo = (int)(o - r * wo);
    const int co = (int)(r / ho);
    const int io = (int)(r - (long long)co * ho);
    const int a = tr ? jo : io, b = tr ? io : jo;
    const int i = fr ? h - 1 - a : a, j = fc ? w - 1 - b : b;
    const int c = it.reverse_c ? C - 1 - co : co;
    const int ys = fold(it.top + i, it.Hc, it.pad_mode) - cy, xs = fold(it.left + j, it.Wc, it.pad_mode) - cx;
    float x = 0.f;
    if (ys >= 0 && ys < it.Hs && xs >= 0 && xs < it.Ws) {
      const long long off = ys * it.sy + xs * it.sx + c * it.sc;
      x = it.src_u8 ? __fdiv_rn((float)static_cast<const uint8_t*>(it.src)[off], 255.0f)
                    : static_cast<const float*>(it.src)[off];
    }
    if (noisy) {
      const unsigned long long e = ((unsigned long long)i * w + j) * C + c;
      double z;
      if (it.noise == kNoiseArray) {
        z = it.z[e];
      } else {
        const unsigned long long q = e >> 1;
        const uint4 p = philox4x32_10(make_uint4((unsigned)q, (unsigned)(q >> 32), (unsigned)cl, (unsigned)(cl >> 32)),
                                      k0, k1);
        const unsigned w0 = e & 1 ? p.z : p.x, w1 = e & 1 ? p.w : p.y;
        const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(w1 >> 8) * 0x1p-24f;
        z = (double)(sqrtf(-2.0f * logf(u1)) * cosf(6.28318530717958647692f * u2));
      }
      const double v = __dadd_rn((double)x, __dadd_rn(it.loc, __ddiv_rn(__dmul_rn(it.scale, z), it.div)));
      x = (float)fmin(fmax(v, 0.0), 1.0);
    }
    if (it.mean) x = __fsub_rn(x, it.mean[co]);
    if (it.std) x = __fdiv_rn(x, it.std[co]);
    it.dst[o] = x;
  }
}

// grid (blocks, B): every wave adds its two sums to the sample's pair
__global__ __launch_bounds__(kThreads) void data_count_kernel(const float* x, long long n, int32_t* counts) {
  const float* p = x + (long long)blockIdx.y * n;
  int c0 = 0, c1 = 0;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < n; e += (long long)gridDim.x * kThreads) {
    const float v = p[e];
    c0 += v == 0.0f;
    c1 += v == 1.0f;
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) {
    c0 += __shfl_down(c0, d);
    c1 += __shfl_down(c1, d);
  }
  if ((threadIdx.x & 63) == 0) {
    if (c0) atomicAdd(counts + 2 * blockIdx.y, c0);
    if (c1) atomicAdd(counts + 2 * blockIdx.y + 1, c1);
  }
}

__global__ __launch_bounds__(kThreads) void data_finish_kernel(float* x, long long total, int C, long long hw,
                                                               const int32_t* counts, double thr, float nudge,
                                                               const float* mean, const float* std) {
  const long long per = (long long)C * hw;
  for (long long e = (long long)blockIdx.x * kThreads + threadIdx.x; e < total; e += (long long)gridDim.x * kThreads) {
    const long long b = e / per;
    const int c = (int)((e - b * per) / hw);
    float v = x[e];
    if (counts_say(counts + 2 * b, per, thr)) v = __fadd_rn(v, nudge);
    if (mean) v = __fsub_rn(v, mean[c]);
    if (std) v = __fdiv_rn(v, std[c]);
    x[e] = v;
  }
}

inline int grid_for(long long n, int cap) {
  return (int)std::max(1ll, std::min(ceil_div(n, kThreads), (long long)std::max(1, cap)));
}

}  // namespace data
}  // namespace kdlae

using namespace kdlae;

extern "C" {

int kdlae_data_sample(const kdlae_data_item* items, void* table, int n_items, uint64_t seed, uint64_t call,
                      void* stream) {
  if (!items || !table) return fail(KDLAE_EINVAL_CONFIG, "kdlae_data_sample: items or table is null");
  if (n_items < 1 || n_items > data::kMaxItems)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_data_sample: n_items must be 1..65535, got " + std::to_string(n_items));
  long long n_max = 0;
  for (int k = 0; k < n_items; ++k) {
    const kdlae_data_item& g = items[k];
    const std::string what = "kdlae_data_sample: item " + std::to_string(k);
    if (!g.src || !g.dst) return fail(KDLAE_EINVAL_CONFIG, what + ": null src or dst");
    if (((uintptr_t)g.dst & 3) || (!g.src_u8 && ((uintptr_t)g.src & 3)))
      return fail(KDLAE_EINVAL_CONFIG, what + ": fp32 pointers must be 4-byte aligned");
    if (g.Hs <= 0 || g.Ws <= 0 || g.C <= 0 || g.h <= 0 || g.w <= 0)
      return fail(KDLAE_EINVAL_SHAPE, what + ": every extent must be positive");
    if (g.sy < 0 || g.sx < 0 || g.sc < 0) return fail(KDLAE_EINVAL_SHAPE, what + ": negative source stride");
    if (g.Hc < g.Hs || g.Wc < g.Ws)
      return fail(KDLAE_EINVAL_SHAPE, what + ": the centre-pad canvas " + std::to_string(g.Hc) + "x" + std::to_string(g.Wc) +
                                          " is smaller than the " + std::to_string(g.Hs) + "x" + std::to_string(g.Ws) + " source");
    if (g.pad_mode < data::kPadNone || g.pad_mode > data::kPadSymmetric)
      return fail(KDLAE_EINVAL_CONFIG, what + ": pad_mode must be 0 (none), 1 (reflect101) or 2 (symmetric)");
    if (g.Hp < g.Hc || g.Wp < g.Wc || (g.pad_mode == data::kPadNone && (g.Hp != g.Hc || g.Wp != g.Wc)))
      return fail(KDLAE_EINVAL_SHAPE, what + ": the padded canvas " + std::to_string(g.Hp) + "x" + std::to_string(g.Wp) +
                                          " must be at least " + std::to_string(g.Hc) + "x" + std::to_string(g.Wc) +
                                          ", and equal to it without a pad mode");
    if (g.top < 0 || g.left < 0 || (long long)g.top + g.h > g.Hp || (long long)g.left + g.w > g.Wp)
      return fail(KDLAE_EINVAL_SHAPE, what + ": window rows " + std::to_string(g.top) + "+" + std::to_string(g.h) +
                                          ", cols " + std::to_string(g.left) + "+" + std::to_string(g.w) + " leaves the " +
                                          std::to_string(g.Hp) + "x" + std::to_string(g.Wp) + " canvas");
    if (g.dihedral < 0 || g.dihedral > 7) return fail(KDLAE_EINVAL_CONFIG, what + ": dihedral code must be 0..7");
    if (g.noise < data::kNoiseOff || g.noise > data::kNoisePhilox)
      return fail(KDLAE_EINVAL_CONFIG, what + ": noise must be 0 (off), 1 (z array) or 2 (Philox)");
    if (g.noise == data::kNoiseArray && !g.z) return fail(KDLAE_EINVAL_CONFIG, what + ": noise from an array needs z");
    if (g.noise != data::kNoiseOff && !(g.div != 0.0)) return fail(KDLAE_EINVAL_CONFIG, what + ": noise div must not be 0");
    if (g.counts && g.count_n <= 0) return fail(KDLAE_EINVAL_SHAPE, what + ": counts need a positive count_n");
    const long long n = (long long)g.C * g.h * g.w;
    const long long span = (g.Hs - 1) * g.sy + (g.Ws - 1) * g.sx + (g.C - 1) * g.sc + 1;
    const uintptr_t s0 = (uintptr_t)g.src, s1 = s0 + (uintptr_t)span * (g.src_u8 ? 1 : 4);
    const uintptr_t d0 = (uintptr_t)g.dst, d1 = d0 + (uintptr_t)n * 4;
    if (s0 < d1 && d0 < s1) return fail(KDLAE_EINVAL_CONFIG, what + ": dst overlaps src");
    n_max = std::max(n_max, n);
  }
  HIPCHK(hipMemcpyAsync(table, items, sizeof(kdlae_data_item) * (size_t)n_items, hipMemcpyHostToDevice,
                        (hipStream_t)stream));
  const dim3 grid(data::grid_for(n_max, data::kMaxBlocks / n_items), n_items);
  hipLaunchKernelGGL(data::data_sample_kernel, grid, dim3(data::kThreads), 0, (hipStream_t)stream,
                     static_cast<const kdlae_data_item*>(table), (unsigned)seed, (unsigned)(seed >> 32),
                     (unsigned long long)call);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int kdlae_data_count(const float* x, int B, int64_t n_per_sample, int32_t* counts, void* stream) {
  if (!x || !counts) return fail(KDLAE_EINVAL_CONFIG, "kdlae_data_count: null x or counts");
  if (B <= 0 || B > data::kMaxItems || n_per_sample <= 0 || n_per_sample > INT32_MAX)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_data_count: B must be 1..65535 and n_per_sample 1..2^31-1");
  HIPCHK(zero_fill(counts, sizeof(int32_t) * 2 * (size_t)B, (hipStream_t)stream));
  const dim3 grid(data::grid_for(n_per_sample, data::kMaxBlocks / B), B);
  hipLaunchKernelGGL(data::data_count_kernel, grid, dim3(data::kThreads), 0, (hipStream_t)stream, x,
                     (long long)n_per_sample, counts);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int kdlae_data_finish(float* x, int B, int C, int64_t hw, const int32_t* counts, double thr, float nudge,
                      const float* mean, const float* std, void* stream) {
  if (!x || !counts) return fail(KDLAE_EINVAL_CONFIG, "kdlae_data_finish: null x or counts");
  if (B <= 0 || C <= 0 || hw <= 0) return fail(KDLAE_EINVAL_SHAPE, "kdlae_data_finish: every extent must be positive");
  const long long total = (long long)B * C * hw;
  hipLaunchKernelGGL(data::data_finish_kernel, dim3(data::grid_for(total, data::kMaxBlocks)), dim3(data::kThreads), 0,
                     (hipStream_t)stream, x, total, C, (long long)hw, counts, thr, nudge, mean, std);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

}  // extern "C"

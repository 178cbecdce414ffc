// Progressive-learning batch preparation (Train/basicsr/train.py:374-448) and the KDLAE-S per-frame input
// mask (Train/basicsr/data/paired_image_dataset.py:19-36,219-272) on device buffers.
//
//   prepare_kernel      one launch for up to four segments (img, denoise_rate, hq, sr): gather the sub-batch
//                       through `index`, crop one window, and replace the pixels the Bernoulli mask drops by
//                       -value.  dst[b,c,i,j] = keep ? src[index[b],c,y0+i,x0+j] : -value.
//   mask_frames_kernel  [B, F, H, W]: frame f masked with probs[f]; with `interpolate` an odd frame takes its
//                       base from 0.5f * (masked[f-1] + src[f+1]) (one fp32 add, one multiply), masked[f-1]
//                       recomputed from src and frame f-1's own mask bit, so dst is never read.
//
// Both are copies with a select: the work is split into units of four consecutive dst elements (one 16-byte
// store) where the segment's rows and dst allow it (w % 4 == 0, dst 16-byte aligned), else single elements.
// A unit's four source floats sit in one row; they are read as one float4 when that address happens to be
// 16-byte aligned (it depends on x0, Ws and the row) and as four dwords otherwise.  64-bit element indices
// throughout.  The mask bit comes from the caller's `keep` bytes or from Philox4x32-10: key = seed,
// counter = (e / 4, call), element e takes word e % 4, u = (word >> 8) * 2^-24, keep = u >= prob in fp32, so a
// vector unit needs one Philox block.  No atomics, no scratch, no synchronisation.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "philox.h"
#include "runtime.h"

namespace kdlae {
namespace augment {

constexpr int kThreads = 256;
constexpr int kMaxBlocks = 2048;  // 256 CUs x 8 blocks; larger batches grid-stride
constexpr int kMaxSegs = 4;
constexpr int kMaxFrames = 16;

enum Mode { kCopy = 0, kFill = 1, kKeepBytes = 2, kPhilox = 3 };

struct Seg {
  const float* src;
  float* dst;
  const uint8_t* keep;
  long long n;           // dst elements
  long long unit_begin;  // first work unit of this segment in the launch
  int C, Hs, Ws, h, w, y0, x0;
  int mode, vec, keep4;  // keep4: keep is 4-byte aligned (vector units read its bytes as one word)
  float prob;
  unsigned call_lo, call_hi;
};
struct PrepArgs {
  Seg seg[kMaxSegs];
  int nseg;
  long long units;
  const int* index;
  float fill;  // -value
  unsigned key0, key1;
};

struct FrameArgs {
  const float* src;
  float* dst;
  const uint8_t* keep;
  long long n, hw;
  int F, interpolate, vec, keep4;
  int mode[kMaxFrames];
  float prob[kMaxFrames];
  float fill;
  unsigned key0, key1, call_lo, call_hi;
};

__device__ __forceinline__ bool philox_keep(unsigned word, float prob) {
  return (float)(word >> 8) * 0x1p-24f >= prob;
}

// keep bits of the four elements e .. e + 3 (e % 4 == 0), bit k = element e + k
__device__ __forceinline__ unsigned keep4_bits(int mode, const uint8_t* keep, int keep4, long long e, float prob,
                                               unsigned k0, unsigned k1, unsigned call_lo, unsigned call_hi) {
  if (mode == kCopy) return 0xFu;
  if (mode == kFill) return 0u;
  if (mode == kKeepBytes) {
    if (keep4) {
      const unsigned v = *reinterpret_cast<const unsigned*>(keep + e);
      return ((v & 0xFFu) != 0) | (((v >> 8) & 0xFFu) != 0) << 1 | (((v >> 16) & 0xFFu) != 0) << 2 | ((v >> 24) != 0) << 3;
    }
    return (keep[e] != 0) | (keep[e + 1] != 0) << 1 | (keep[e + 2] != 0) << 2 | (keep[e + 3] != 0) << 3;
  }
  const unsigned long long q = (unsigned long long)e >> 2;
  const uint4 r = philox4x32_10(make_uint4((unsigned)q, (unsigned)(q >> 32), call_lo, call_hi), k0, k1);
  return philox_keep(r.x, prob) | philox_keep(r.y, prob) << 1 | philox_keep(r.z, prob) << 2 | philox_keep(r.w, prob) << 3;
}

__device__ __forceinline__ bool keep1_bit(int mode, const uint8_t* keep, long long e, float prob, unsigned k0,
                                          unsigned k1, unsigned call_lo, unsigned call_hi) {
  if (mode == kCopy) return true;
  if (mode == kFill) return false;
  if (mode == kKeepBytes) return keep[e] != 0;
  const unsigned long long q = (unsigned long long)e >> 2;
  const uint4 r = philox4x32_10(make_uint4((unsigned)q, (unsigned)(q >> 32), call_lo, call_hi), k0, k1);
  const unsigned k = (unsigned)e & 3u;
  return philox_keep(k == 0 ? r.x : k == 1 ? r.y : k == 2 ? r.z : r.w, prob);
}

// four consecutive floats at an address of any 4-byte alignment
__device__ __forceinline__ float4 load4(const float* p) {
  if (((uintptr_t)p & 15) == 0) return *reinterpret_cast<const float4*>(p);
  return make_float4(p[0], p[1], p[2], p[3]);
}

__device__ __forceinline__ float4 select4(unsigned bits, float4 v, float fill) {
  return make_float4(bits & 1u ? v.x : fill, bits & 2u ? v.y : fill, bits & 4u ? v.z : fill, bits & 8u ? v.w : fill);
}

__global__ __launch_bounds__(kThreads) void prepare_kernel(const PrepArgs a) {
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < a.units; u += (long long)gridDim.x * kThreads) {
    int s = 0;
#pragma unroll
    for (int k = 1; k < kMaxSegs; ++k)
      if (k < a.nseg && u >= a.seg[k].unit_begin) s = k;
    const Seg& g = a.seg[s];
    const long long e = (u - g.unit_begin) * (g.vec ? 4 : 1);
    // e -> (b, c, i, j) of dst [B, C, h, w]
    const long long row = e / g.w;
    const int j = (int)(e - row * g.w);
    const long long bc = row / g.h;
    const int i = (int)(row - bc * g.h);
    const long long b = bc / g.C;
    const int c = (int)(bc - b * g.C);
    const long long sb = a.index ? (long long)a.index[b] : b;
    const float* sp = g.src + ((sb * g.C + c) * g.Hs + (g.y0 + i)) * (long long)g.Ws + (g.x0 + j);
    if (g.vec) {
      const unsigned bits = keep4_bits(g.mode, g.keep, g.keep4, e, g.prob, a.key0, a.key1, g.call_lo, g.call_hi);
      float4 v = make_float4(a.fill, a.fill, a.fill, a.fill);
      if (bits) v = select4(bits, load4(sp), a.fill);
      *reinterpret_cast<float4*>(g.dst + e) = v;
    } else {
      const bool k = keep1_bit(g.mode, g.keep, e, g.prob, a.key0, a.key1, g.call_lo, g.call_hi);
      g.dst[e] = k ? *sp : a.fill;
    }
  }
}

__global__ __launch_bounds__(kThreads) void mask_frames_kernel(const FrameArgs a) {
  const long long units = a.vec ? a.n >> 2 : a.n;
  for (long long u = (long long)blockIdx.x * kThreads + threadIdx.x; u < units; u += (long long)gridDim.x * kThreads) {
    const long long e = a.vec ? u << 2 : u;
    const int f = (int)((e / a.hw) % a.F);
    const bool interp = a.interpolate && (f & 1);
    if (a.vec) {
      const unsigned bits = keep4_bits(a.mode[f], a.keep, a.keep4, e, a.prob[f], a.key0, a.key1, a.call_lo, a.call_hi);
      float4 v = make_float4(a.fill, a.fill, a.fill, a.fill);
      if (bits) {
        if (interp) {
          const unsigned pb = keep4_bits(a.mode[f - 1], a.keep, a.keep4, e - a.hw, a.prob[f - 1], a.key0, a.key1,
                                         a.call_lo, a.call_hi);
          const float4 p = pb ? select4(pb, load4(a.src + (e - a.hw)), a.fill) : v;  // v still holds the fill
          const float4 n = load4(a.src + (e + a.hw));
          v = make_float4(0.5f * (p.x + n.x), 0.5f * (p.y + n.y), 0.5f * (p.z + n.z), 0.5f * (p.w + n.w));
        } else {
          v = load4(a.src + e);
        }
        v = select4(bits, v, a.fill);
      }
      *reinterpret_cast<float4*>(a.dst + e) = v;
    } else {
      float v = a.fill;
      if (keep1_bit(a.mode[f], a.keep, e, a.prob[f], a.key0, a.key1, a.call_lo, a.call_hi)) {
        if (interp) {
          const bool pk = keep1_bit(a.mode[f - 1], a.keep, e - a.hw, a.prob[f - 1], a.key0, a.key1, a.call_lo, a.call_hi);
          v = 0.5f * ((pk ? a.src[e - a.hw] : a.fill) + a.src[e + a.hw]);
        } else {
          v = a.src[e];
        }
      }
      a.dst[e] = v;
    }
  }
}

inline int mode_of(float prob, const uint8_t* keep) {
  if (!(prob > 0.f)) return kCopy;
  if (prob >= 1.f) return kFill;
  return keep ? kKeepBytes : kPhilox;
}

inline int grid_for(long long units) { return (int)std::max(1ll, std::min(ceil_div(units, kThreads), (long long)kMaxBlocks)); }

}  // namespace augment
}  // namespace kdlae

using namespace kdlae;

extern "C" {

int kdlae_train_prepare(const kdlae_prep_seg* segs, int nseg, const int* index, int B, float value, uint64_t seed,
                        uint64_t call, void* stream) {
  if (!segs) return fail(KDLAE_EINVAL_CONFIG, "kdlae_train_prepare: segs is null");
  if (nseg < 1 || nseg > augment::kMaxSegs)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_train_prepare: nseg must be 1..4, got " + std::to_string(nseg));
  if (B <= 0) return fail(KDLAE_EINVAL_SHAPE, "kdlae_train_prepare: B must be positive");
  augment::PrepArgs a{};
  a.nseg = nseg;
  a.index = index;
  a.fill = -value;
  a.key0 = (unsigned)seed;
  a.key1 = (unsigned)(seed >> 32);
  long long units = 0;
  for (int s = 0; s < nseg; ++s) {
    const kdlae_prep_seg& g = segs[s];
    const std::string what = "kdlae_train_prepare: segment " + std::to_string(s);
    if (!g.src || !g.dst) return fail(KDLAE_EINVAL_CONFIG, what + ": null src or dst");
    if ((const void*)g.src == (const void*)g.dst) return fail(KDLAE_EINVAL_CONFIG, what + ": dst must not be src");
    if (g.B_src <= 0 || g.C <= 0 || g.Hs <= 0 || g.Ws <= 0 || g.h <= 0 || g.w <= 0)
      return fail(KDLAE_EINVAL_SHAPE, what + ": every extent must be positive");
    if (g.y0 < 0 || g.x0 < 0 || (long long)g.y0 + g.h > g.Hs || (long long)g.x0 + g.w > g.Ws)
      return fail(KDLAE_EINVAL_SHAPE, what + ": window rows " + std::to_string(g.y0) + "+" + std::to_string(g.h) +
                                          ", cols " + std::to_string(g.x0) + "+" + std::to_string(g.w) + " leaves the " +
                                          std::to_string(g.Hs) + "x" + std::to_string(g.Ws) + " source");
    if (!index && B != g.B_src)
      return fail(KDLAE_EINVAL_SHAPE, what + ": without an index B must equal B_src (" + std::to_string(B) + " vs " +
                                          std::to_string(g.B_src) + ")");
    augment::Seg& d = a.seg[s];
    d.src = g.src;
    d.dst = g.dst;
    d.keep = g.keep;
    d.n = (long long)B * g.C * g.h * g.w;
    d.C = g.C, d.Hs = g.Hs, d.Ws = g.Ws, d.h = g.h, d.w = g.w, d.y0 = g.y0, d.x0 = g.x0;
    d.mode = augment::mode_of(g.prob, g.keep);
    d.vec = (g.w % 4 == 0 && al16(g.dst)) ? 1 : 0;
    d.keep4 = ((uintptr_t)g.keep & 3) == 0;
    d.prob = g.prob;
    const uint64_t cs = call + (uint64_t)s;
    d.call_lo = (unsigned)cs;
    d.call_hi = (unsigned)(cs >> 32);
    d.unit_begin = units;
    units += d.vec ? d.n / 4 : d.n;
  }
  a.units = units;
  hipLaunchKernelGGL(augment::prepare_kernel, dim3(augment::grid_for(units)), dim3(augment::kThreads), 0,
                     (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int kdlae_train_mask_frames(const float* src, float* dst, int B, int F, int H, int W, const float* probs,
                            int interpolate, float value, const uint8_t* keep, uint64_t seed, uint64_t call,
                            void* stream) {
  if (!src || !dst || !probs) return fail(KDLAE_EINVAL_CONFIG, "kdlae_train_mask_frames: null src, dst or probs");
  if (src == dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_train_mask_frames: dst must not be src (the frame rule reads "
                                                   "unmasked neighbours)");
  if (B <= 0 || F <= 0 || H <= 0 || W <= 0)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_train_mask_frames: every extent must be positive");
  if (F > augment::kMaxFrames)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_train_mask_frames: at most 16 frames, got " + std::to_string(F));
  if (interpolate && F % 2 == 0)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_train_mask_frames: interpolation needs an odd frame count (every odd frame "
                                    "has two neighbours), got " + std::to_string(F));
  augment::FrameArgs a{};
  a.src = src;
  a.dst = dst;
  a.keep = keep;
  a.hw = (long long)H * W;
  a.n = (long long)B * F * a.hw;
  a.F = F;
  a.interpolate = interpolate ? 1 : 0;
  a.vec = (a.hw % 4 == 0 && al16(dst)) ? 1 : 0;
  a.keep4 = ((uintptr_t)keep & 3) == 0;
  for (int f = 0; f < F; ++f) {
    a.mode[f] = augment::mode_of(probs[f], keep);
    a.prob[f] = probs[f];
  }
  a.fill = -value;
  a.key0 = (unsigned)seed;
  a.key1 = (unsigned)(seed >> 32);
  a.call_lo = (unsigned)call;
  a.call_hi = (unsigned)(call >> 32);
  hipLaunchKernelGGL(augment::mask_frames_kernel, dim3(augment::grid_for(a.vec ? a.n / 4 : a.n)),
                     dim3(augment::kThreads), 0, (hipStream_t)stream, a);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

}  // extern "C"

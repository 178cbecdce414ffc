// Clip inference (kdlae_clip_plan, kdlae_clip_gather, kdlae_clip_blend, kdlae_clip_blend_u8): tile.hip's plan on
// the frame axis of a clip [B][T][H][W].  The kernels move bytes, the blends also add, divide and (u8) round.
//
//   plan               f = min(frames, T), stride = f - overlap, starts range(0, T - f, stride) + [T - f], so
//                      n = ceil((T - f) / stride) + 1 (1 when T == f) and start(i) = i < n - 1 ? i stride : T - f.
//                      No start table: both kernels derive the start.
//   clip_gather_kernel windows first .. first + count - 1 (flat index b n + i) of src [B][T][H][W] -> dense
//                      [count][f][H][W].  A window is f H W consecutive floats of the clip: one item per V of them.
//   clip_blend_kernel  gather form: one thread per V consecutive output pixels of a frame loops over the covering
//                      windows in ascending index.  Uniform (WT false): acc = 0 + o1 + o2 + ... in fp32, divided by
//                      the fp32 count: E.add_(y); W.add_(1); E.div_(W) of the host loop, bit for bit.  Weighted (WT
//                      true): tile_blend_w_kernel's rule on one axis, stated at the kernel.  No atomics.
//                      Out = float writes [B][T][H][W]; Out = uint8_t applies postprocess_u8_kernel's rule to the
//                      blended value in the same thread (clamp to [0, 1], rint(x 255)) and writes the crop
//                      [B][T][h][w].
//
// V = 4 (float4 loads; float4 or 4-byte stores) when the pointers and every row start allow it, V = 1 otherwise;
// the entries state the conditions.  The four pixels of a thread lie in one frame, so they share one cover set.
// Flat 64-bit item index with a grid-stride loop: no clip is too long or too large for the grid.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "runtime.h"

namespace kdlae {

struct ClipPlan {
  int f = 0, n = 0, stride = 0;
};

// T frames, windows of f frames `stride` apart, n of them; a frame is rows of W floats of which the output keeps
// h rows of w.  The fp32 blend sees a frame as one row: H = h = 1 and W = w = the frame's floats.
struct ClipGeo {
  int T, f, stride, n, H, W, h, w;
};

constexpr long long kClipMaxBlocks = 4096;  // tile.hip's cap: 16 blocks of 256 per CU; the loop takes the rest

__device__ __forceinline__ int clip_start(int i, int n, int stride, int last) { return i < n - 1 ? i * stride : last; }

template <int V>
__global__ __launch_bounds__(256) void clip_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          ClipGeo g, int first, long long per, long long total) {
  // per: items of one window (f H W / V)
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long q = idx / per;
    const long long r = idx - q * per;
    const int flat = first + (int)q;
    const int i = flat % g.n, b = flat / g.n;
    const int t0 = clip_start(i, g.n, g.stride, g.T - g.f);
    const long long s = ((long long)b * g.T + t0) * (per / g.f) + r;  // in items: a frame is per / f of them
    if constexpr (V == 4)
      reinterpret_cast<float4*>(dst)[idx] = reinterpret_cast<const float4*>(src)[s];
    else
      dst[idx] = src[s];
  }
}

// The blend.  Per output element at frame t, over the covering windows in ascending index (the regular ones
// lo .. hi, start i stride, and, when t >= T - f, window n - 1 at T - f), p = t - start:
//   uniform   acc = fl(acc + o);  out = acc / (float)cnt
//   weighted  w = wt[p];  E = fl(E + fl(w o));  S = fl(S + w);  out = cnt == 1 ? o : E / S
// every operation rounded on its own (no contraction), true division; a frame under exactly one window keeps that
// window's value untouched in the weighted form (fl(fl(w o) / w) is not o for every o).
template <int V, bool WT, typename Out>
__global__ __launch_bounds__(256) void clip_blend_kernel(const float* __restrict__ windows,
                                                         const float* __restrict__ wt, Out* __restrict__ dst,
                                                         ClipGeo g, long long total) {
#pragma clang fp contract(off)
  constexpr bool U8 = sizeof(Out) == 1;
  const int wq = g.w / V;
  const long long HW = (long long)g.H * g.W;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over B T h
    const int x = (int)(idx - row * wq) * V;
    const int y = (int)(row % g.h);
    const long long bt = row / g.h;
    const int t = (int)(bt % g.T), b = (int)(bt / g.T);
    const int lo = t >= g.f ? (t - g.f) / g.stride + 1 : 0;
    const int hi = min(t / g.stride, g.n - 2);
    const int last = t >= g.T - g.f;
    float E[V], S[V], o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) E[e] = 0.f, S[e] = 0.f, o[e] = 0.f;
    int cnt = 0;
    for (int ii = lo; ii <= hi + last; ++ii) {
      const int i = ii <= hi ? ii : g.n - 1;
      const int p = t - (ii <= hi ? i * g.stride : g.T - g.f);
      const float* __restrict__ s = windows + (((long long)b * g.n + i) * g.f + p) * HW + (long long)y * g.W + x;
      if constexpr (V == 4) {
        const float4 v = *reinterpret_cast<const float4*>(s);
        o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
      } else {
        o[0] = *s;
      }
      if constexpr (WT) {
        const float w = wt[p];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float wo = w * o[e];
          E[e] = E[e] + wo;
          S[e] = S[e] + w;
        }
      } else {
#pragma unroll
        for (int e = 0; e < V; ++e) E[e] = E[e] + o[e];
      }
      ++cnt;
    }
    if constexpr (WT) {
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = cnt == 1 ? o[e] : E[e] / S[e];
    } else {
      const float c = (float)cnt;
#pragma unroll
      for (int e = 0; e < V; ++e) o[e] = E[e] / c;
    }
    if constexpr (U8) {
      uint8_t q[V];
#pragma unroll
      for (int e = 0; e < V; ++e) {
        const float v = fminf(fmaxf(o[e], 0.0f), 1.0f);  // postprocess_u8_kernel's rule
        q[e] = (uint8_t)rintf(v * 255.0f);
      }
      if constexpr (V == 4)
        reinterpret_cast<uchar4*>(dst)[idx] = make_uchar4(q[0], q[1], q[2], q[3]);
      else
        dst[idx] = q[0];
    } else {
      if constexpr (V == 4)
        reinterpret_cast<float4*>(dst)[idx] = make_float4(o[0], o[1], o[2], o[3]);
      else
        dst[idx] = o[0];
    }
  }
}

// the plan's own refusals; `who` names the entry in the message
static int make_clip_plan(const char* who, int T, int frames, int overlap, ClipPlan& p) {
  const std::string w(who);
  if (T < 1 || frames < 1) return fail(KDLAE_EINVAL_CONFIG, w + ": T and frames must be positive");
  const int f = std::min(frames, T);
  if (overlap < 0 || overlap >= f)
    return fail(KDLAE_EINVAL_SHAPE, w + ": need 0 <= overlap < min(frames, T) = " + std::to_string(f));
  p.f = f;
  p.stride = f - overlap;
  p.n = (int)ceil_div(T - f, p.stride) + 1;
  return KDLAE_OK;
}

// the checks the three device entries share: sizes, the plan, the index ranges the kernels keep in an int
static int check_clip(const char* who, int B, int T, int H, int W, int frames, int overlap, ClipPlan& p) {
  const std::string w(who);
  if (B < 1 || H < 1 || W < 1) return fail(KDLAE_EINVAL_CONFIG, w + ": need B, H and W >= 1");
  TRY(make_clip_plan(who, T, frames, overlap, p));
  if ((long long)B * p.n > INT_MAX || (long long)B * T > INT_MAX || (long long)H * W > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, w + ": more than 2^31 - 1 windows, frames or pixels of a frame");
  return KDLAE_OK;
}

static unsigned clip_blocks(long long total) { return (unsigned)std::min(ceil_div(total, 256), kClipMaxBlocks); }

template <typename Out>
static int launch_clip_blend(const float* windows, const float* wt, Out* dst, const ClipGeo& g, int B, bool vec,
                             void* stream) {
  const long long elems = (long long)B * g.T * g.h * g.w;
  const long long total = vec ? elems / 4 : elems;
  const dim3 grid(clip_blocks(total)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (wt) {
    if (vec)
      hipLaunchKernelGGL((clip_blend_kernel<4, true, Out>), grid, block, 0, st, windows, wt, dst, g, total);
    else
      hipLaunchKernelGGL((clip_blend_kernel<1, true, Out>), grid, block, 0, st, windows, wt, dst, g, total);
  } else {
    if (vec)
      hipLaunchKernelGGL((clip_blend_kernel<4, false, Out>), grid, block, 0, st, windows, wt, dst, g, total);
    else
      hipLaunchKernelGGL((clip_blend_kernel<1, false, Out>), grid, block, 0, st, windows, wt, dst, g, total);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

}  // namespace kdlae

using namespace kdlae;

extern "C" int kdlae_clip_plan(int T, int frames, int overlap, int* f, int* n, int* stride) {
  if (!f || !n || !stride) return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_plan: null argument");
  ClipPlan p;
  TRY(make_clip_plan("kdlae_clip_plan", T, frames, overlap, p));
  *f = p.f, *n = p.n, *stride = p.stride;
  return KDLAE_OK;
}

extern "C" int kdlae_clip_gather(const float* src, int B, int T, int H, int W, int frames, int overlap, int first,
                                 int count, float* dst, void* stream) {
  if (!src || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_gather: null argument");
  if (count < 1 || first < 0) return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_gather: need count >= 1 and first >= 0");
  ClipPlan p;
  TRY(check_clip("kdlae_clip_gather", B, T, H, W, frames, overlap, p));
  const long long nwin = (long long)B * p.n;
  if ((long long)first + count > nwin)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_gather: first + count passes the last window (B n = " +
                                         std::to_string(nwin) + ")");
  const ClipGeo g{T, p.f, p.stride, p.n, H, W, H, W};
  const long long HW = (long long)H * W;
  // H W % 4 == 0 puts every frame, so every window start of both buffers, on 16 bytes
  const bool vec = al16(src) && al16(dst) && HW % 4 == 0;
  const long long per = p.f * HW / (vec ? 4 : 1);
  const long long total = count * per;
  if (vec)
    hipLaunchKernelGGL(clip_gather_kernel<4>, dim3(clip_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       first, per, total);
  else
    hipLaunchKernelGGL(clip_gather_kernel<1>, dim3(clip_blocks(total)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       first, per, total);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_clip_blend(const float* windows, int B, int T, int H, int W, int frames, int overlap,
                                const float* wt, float* dst, void* stream) {
  if (!windows || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_blend: null argument");
  ClipPlan p;
  TRY(check_clip("kdlae_clip_blend", B, T, H, W, frames, overlap, p));
  // a frame as one row of H W floats
  const int HW = H * W;
  const ClipGeo g{T, p.f, p.stride, p.n, 1, HW, 1, HW};
  const bool vec = al16(windows) && al16(dst) && HW % 4 == 0;
  return launch_clip_blend(windows, wt, dst, g, B, vec, stream);
}

extern "C" int kdlae_clip_blend_u8(const float* windows, int B, int T, int H, int W, int h, int w, int frames,
                                   int overlap, const float* wt, uint8_t* dst, void* stream) {
  if (!windows || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_blend_u8: null argument");
  ClipPlan p;
  TRY(check_clip("kdlae_clip_blend_u8", B, T, H, W, frames, overlap, p));
  if (h < 1 || w < 1 || h > H || w > W)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_clip_blend_u8: need 1 <= h <= H and 1 <= w <= W");
  const ClipGeo g{T, p.f, p.stride, p.n, H, W, h, w};
  // four bytes per store: the destination on 4 bytes and w % 4 == 0 put every output row there; the float4 loads
  // need the windows on 16 bytes and W % 4 == 0
  const bool vec = ((uintptr_t)dst & 3) == 0 && w % 4 == 0 && al16(windows) && W % 4 == 0;
  return launch_clip_blend(windows, wt, dst, g, B, vec, stream);
}

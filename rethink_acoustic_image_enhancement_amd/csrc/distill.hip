// Distillation labels (kdlae_distill_expand_u8, kdlae_distill_expand_f32, kdlae_distill_collapse): the data movement
// either side of a KDLAE-T (or Restormer) forward that turns a stack of gray frames [B][F][h][w] into the
// targets a KDLAE-S training step reads.  Items are the frames in flat order j = b F + f; every entry works on the
// chunk j0 .. j0 + n - 1, so the teacher runs n frames at a time.  The forward between them is untouched.
//
//   distill_expand_kernel    frame j -> img [q][3][H][W] (q = j - j0; the gray value in all three channels) and, with
//                            a rate array, rate_map [q][1][H][W] = rate[j], in one launch.  U8: the gray value is the
//                            frame's byte (cin 1) or cv2's 8-bit COLOR_BGR2GRAY of the pixel (cin 3 / 4, alpha
//                            ignored), divided by 255 by preprocess_u8_kernel's expression and reflect-padded on the
//                            bottom/right to (H, W): the bits of kdlae_preprocess_u8 on the frame replicated to
//                            [h][w][3].  F32: a bit copy of a frame that is a network input already.
//   distill_collapse_kernel  hq [q][3][Hp][Wp] -> item j of dst [B][F][h][w], cropped top-left.
//                            file: per channel postprocess_u8_kernel's clamp(x, 0, 1), rintf(x 255) and its black
//                            mask (all three bytes 0 where the source frame's gray value is 0: the lq that
//                            kdlae_postprocess_u8 sees is the replicated gray frame), then the three bytes, read as
//                            R, G, B, through the gray rule to one byte g; dst = g (u8) or (float)g / 255.0f (f32).
//                            mean: ((c0 + c1) + c2) / 3.0f, every operation rounded on its own; f32 only.
//
// Gather form: one thread per V consecutive output pixels of a row, no atomics.  V = 4 (float4 accesses of the fp32
// tensors, 4-byte stores of a u8 target) when the pointers and every row start allow it, V = 1 otherwise; the entries
// state the conditions.  A u8 source is read one byte at a time at any byte offset, but V = 4 threads left of the
// reflect padding read their 4 cin bytes as cin 32-bit words when the source sits on 4 bytes and w % 4 == 0.  Both
// paths give the same bits.  Flat 64-bit item index with a grid-stride loop.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "runtime.h"

namespace kdlae {

constexpr long long kDistillMaxBlocks = 4096;  // clip.hip's cap: 16 blocks of 256 per CU; the loop takes the rest

// Chunk j0 ..; the fp32 side has H rows of W floats per channel, the u8 / target side h rows of w pixels of cin
// bytes.  src4: the u8 source may be read as 32-bit words.  mode: kdlae_distill_collapse's.
struct DistillGeo {
  int j0, H, W, h, w, cin, src4, mode;
};

namespace {

// pipeline.hip's two rules, restated: torch's reflect index for a pad shorter than the input, and cv2's 8-bit
// COLOR_BGR2GRAY, Y = (1868 B + 9617 G + 4899 R + 2^13) >> 14
__device__ __forceinline__ int distill_reflect(int i, int n) { return i < n ? i : 2 * (n - 1) - i; }
__device__ __forceinline__ uint8_t distill_gray3(unsigned b, unsigned g, unsigned r) {
  return (uint8_t)((1868u * b + 9617u * g + 4899u * r + 8192u) >> 14);
}
__device__ __forceinline__ uint8_t distill_gray(const uint8_t* px, int cin) {
  return cin >= 3 ? distill_gray3(px[0], px[1], px[2]) : px[0];
}

// gray values of four consecutive pixels at p (on 4 bytes), read as CIN 32-bit words
template <int CIN>
__device__ __forceinline__ void distill_gray4_words(const uint8_t* p, uint8_t g[4]) {
  uint32_t wv[CIN];
#pragma unroll
  for (int k = 0; k < CIN; ++k) wv[k] = reinterpret_cast<const uint32_t*>(p)[k];
  auto byte = [&](int i) { return (wv[i >> 2] >> (8 * (i & 3))) & 255u; };
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    if constexpr (CIN == 1)
      g[e] = (uint8_t)byte(e);
    else
      g[e] = distill_gray3(byte(e * CIN), byte(e * CIN + 1), byte(e * CIN + 2));
  }
}

// gray values of V consecutive pixels of row `line` (in pixels from the source's start) from column x on; columns
// past w reflect (expand only: collapse never passes them)
template <int V>
__device__ __forceinline__ void distill_gray_row(const uint8_t* src, long long line, int x, const DistillGeo& g,
                                                 uint8_t out[V]) {
  if constexpr (V == 4) {
    if (g.src4 && x < g.w) {  // w % 4 == 0: the four pixels lie left of the padding, on 4 bytes
      const uint8_t* p = src + (line + x) * g.cin;
      if (g.cin == 1)
        distill_gray4_words<1>(p, out);
      else if (g.cin == 3)
        distill_gray4_words<3>(p, out);
      else
        distill_gray4_words<4>(p, out);
      return;
    }
  }
#pragma unroll
  for (int e = 0; e < V; ++e) out[e] = distill_gray(src + (line + distill_reflect(x + e, g.w)) * g.cin, g.cin);
}

template <int V>
__device__ __forceinline__ void distill_store(float* p, const float v[V]) {
  if constexpr (V == 4)
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  else
    *p = v[0];
}

template <int V>
__device__ __forceinline__ void distill_load(const float* p, float v[V]) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
  } else {
    v[0] = *p;
  }
}

template <int V, bool U8>
__global__ __launch_bounds__(256) void distill_expand_kernel(const void* __restrict__ frames,
                                                             const float* __restrict__ rate, float* __restrict__ img,
                                                             float* __restrict__ rate_map, DistillGeo g,
                                                             long long total) {
  const int wq = g.W / V;
  const long long HW = (long long)g.H * g.W;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over n H
    const int x = (int)(idx - row * wq) * V;
    const int y = (int)(row % g.H);
    const long long q = row / g.H, j = g.j0 + q;
    float v[V];
    if constexpr (U8) {
      uint8_t gr[V];
      const long long line = (j * g.h + distill_reflect(y, g.h)) * g.w;
      distill_gray_row<V>(static_cast<const uint8_t*>(frames), line, x, g, gr);
#pragma unroll
      for (int e = 0; e < V; ++e) v[e] = (float)gr[e] / 255.0f;  // preprocess_u8_kernel's expression
    } else {
      distill_load<V>(static_cast<const float*>(frames) + j * HW + (long long)y * g.W + x, v);
    }
    const long long at = (long long)y * g.W + x;
    float* o = img + q * 3 * HW + at;
    distill_store<V>(o, v);
    distill_store<V>(o + HW, v);
    distill_store<V>(o + 2 * HW, v);
    if (rate_map) {
      const float r = rate[j];
      float rv[V];
#pragma unroll
      for (int e = 0; e < V; ++e) rv[e] = r;
      distill_store<V>(rate_map + q * HW + at, rv);
    }
  }
}

template <int V, typename Out>
__global__ __launch_bounds__(256) void distill_collapse_kernel(const float* __restrict__ hq,
                                                               const uint8_t* __restrict__ src,
                                                               Out* __restrict__ dst, DistillGeo g, long long total) {
#pragma clang fp contract(off)
  constexpr bool U8 = sizeof(Out) == 1;
  const int wq = g.w / V;
  const long long HW = (long long)g.H * g.W;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over n h
    const int x = (int)(idx - row * wq) * V;
    const int y = (int)(row % g.h);
    const long long q = row / g.h, j = g.j0 + q;
    const float* p = hq + q * 3 * HW + (long long)y * g.W + x;
    float c0[V], c1[V], c2[V];
    distill_load<V>(p, c0);
    distill_load<V>(p + HW, c1);
    distill_load<V>(p + 2 * HW, c2);
    const long long line = (j * g.h + y) * g.w;  // the row's first pixel in dst and in src
    if constexpr (!U8) {
      if (g.mode == KDLAE_DISTILL_MEAN) {
        float m[V];
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float s01 = c0[e] + c1[e];
          const float s = s01 + c2[e];
          m[e] = s / 3.0f;
        }
        distill_store<V>(dst + line + x, m);
        continue;
      }
    }
    uint8_t gs[V] = {}, gq[V];
    if (src) distill_gray_row<V>(src, line, x, g, gs);
#pragma unroll
    for (int e = 0; e < V; ++e) {
      // postprocess_u8_kernel's rule per channel, its black mask, then the gray rule on (R, G, B) = (c0, c1, c2)
      const unsigned r = (unsigned)(uint8_t)rintf(fminf(fmaxf(c0[e], 0.0f), 1.0f) * 255.0f);
      const unsigned gg = (unsigned)(uint8_t)rintf(fminf(fmaxf(c1[e], 0.0f), 1.0f) * 255.0f);
      const unsigned b = (unsigned)(uint8_t)rintf(fminf(fmaxf(c2[e], 0.0f), 1.0f) * 255.0f);
      const bool black = src && gs[e] == 0;
      gq[e] = black ? distill_gray3(0, 0, 0) : distill_gray3(b, gg, r);
    }
    if constexpr (U8) {
      if constexpr (V == 4)
        *reinterpret_cast<uchar4*>(dst + line + x) = make_uchar4(gq[0], gq[1], gq[2], gq[3]);
      else
        dst[line + x] = gq[0];
    } else {
      float f[V];
#pragma unroll
      for (int e = 0; e < V; ++e) f[e] = (float)gq[e] / 255.0f;
      distill_store<V>(dst + line + x, f);
    }
  }
}

unsigned distill_blocks(long long total) { return (unsigned)std::min(ceil_div(total, 256), kDistillMaxBlocks); }

int distill_launched(const char* who) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string(who) + ": " + hipGetErrorString(e));
  return KDLAE_OK;
}

// the checks the three entries share: the stack, the chunk, and the index ranges the kernels keep in an int (an
// item's pixels on either side; everything else is 64-bit)
int check_distill(const char* who, int B, int F, int h, int w, int H, int W, int j0, int n) {
  const std::string s(who);
  if (B < 1 || F < 1 || h < 1 || w < 1 || H < 1 || W < 1)
    return fail(KDLAE_EINVAL_CONFIG, s + ": need B, F and every height and width >= 1");
  if ((long long)B * F > INT_MAX || (long long)h * w > INT_MAX || (long long)H * W > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, s + ": more than 2^31 - 1 frames or pixels of a frame");
  if (n < 1 || j0 < 0) return fail(KDLAE_EINVAL_CONFIG, s + ": need n >= 1 and j0 >= 0");
  if ((long long)j0 + n > (long long)B * F)
    return fail(KDLAE_EINVAL_CONFIG, s + ": j0 + n passes the last frame (B F = " + std::to_string((long long)B * F) + ")");
  return KDLAE_OK;
}

int check_rate(const char* who, const float* rate, const float* rate_map) {
  if ((rate == nullptr) != (rate_map == nullptr))
    return fail(KDLAE_EINVAL_CONFIG, std::string(who) + ": rate and rate_map come together or not at all");
  return KDLAE_OK;
}

template <bool U8>
int launch_distill_expand(const char* who, const void* frames, const float* rate, float* img, float* rate_map,
                          const DistillGeo& g, int n, bool vec, void* stream) {
  const long long total = (long long)n * g.H * (g.W / (vec ? 4 : 1));
  const dim3 grid(distill_blocks(total)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((distill_expand_kernel<4, U8>), grid, block, 0, st, frames, rate, img, rate_map, g, total);
  else
    hipLaunchKernelGGL((distill_expand_kernel<1, U8>), grid, block, 0, st, frames, rate, img, rate_map, g, total);
  return distill_launched(who);
}

template <typename Out>
int launch_distill_collapse(const char* who, const float* hq, const uint8_t* src, Out* dst, const DistillGeo& g, int n,
                            bool vec, void* stream) {
  const long long total = (long long)n * g.h * (g.w / (vec ? 4 : 1));
  const dim3 grid(distill_blocks(total)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (vec)
    hipLaunchKernelGGL((distill_collapse_kernel<4, Out>), grid, block, 0, st, hq, src, dst, g, total);
  else
    hipLaunchKernelGGL((distill_collapse_kernel<1, Out>), grid, block, 0, st, hq, src, dst, g, total);
  return distill_launched(who);
}

bool al4(const void* p) { return ((uintptr_t)p & 3) == 0; }

}  // namespace

}  // namespace kdlae

using namespace kdlae;

extern "C" int kdlae_distill_expand_u8(const uint8_t* frames, int B, int F, int h, int w, int channels, int multiple,
                                       const float* rate, int j0, int n, float* img, float* rate_map, void* stream) {
  const char* who = "kdlae_distill_expand_u8";
  if (!frames || !img) return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_expand_u8: null argument");
  TRY(check_rate(who, rate, rate_map));
  if (channels != 1 && channels != 3 && channels != 4)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_expand_u8: channels must be 1, 3 or 4");
  if (h < 1 || w < 1 || multiple < 1)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_expand_u8: need h, w and multiple >= 1");
  if ((long long)h + multiple > INT_MAX || (long long)w + multiple > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_expand_u8: the padded size passes 2^31 - 1");
  int H, W;
  kdlae_padded_size(h, w, multiple, &H, &W);
  if (H - h >= h || W - w >= w)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_expand_u8: frame smaller than its reflect padding");
  TRY(check_distill(who, B, F, h, w, H, W, j0, n));
  if (!al4(img) || !al4(rate) || !al4(rate_map))
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_expand_u8: rate, img and rate_map must sit on 4 bytes");
  // W % 4 == 0 puts every row of every channel of both outputs on 16 bytes
  const bool vec = al16(img) && al16(rate_map) && W % 4 == 0;
  // w % 4 == 0 puts the 4 cin bytes of every pixel group left of the padding on 4 bytes
  const int src4 = vec && al4(frames) && w % 4 == 0;
  const DistillGeo g{j0, H, W, h, w, channels, src4, 0};
  return launch_distill_expand<true>(who, frames, rate, img, rate_map, g, n, vec, stream);
}

extern "C" int kdlae_distill_expand_f32(const float* frames, int B, int F, int H, int W, const float* rate, int j0,
                                        int n, float* img, float* rate_map, void* stream) {
  const char* who = "kdlae_distill_expand_f32";
  if (!frames || !img) return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_expand_f32: null argument");
  TRY(check_rate(who, rate, rate_map));
  TRY(check_distill(who, B, F, H, W, H, W, j0, n));
  if (H % 8 || W % 8)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_expand_f32: H and W must be multiples of 8 (a network input)");
  if (!al4(frames) || !al4(img) || !al4(rate) || !al4(rate_map))
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_expand_f32: frames, rate, img and rate_map must sit on 4 bytes");
  const bool vec = al16(frames) && al16(img) && al16(rate_map);  // W % 8 == 0: every row on 16 bytes
  const DistillGeo g{j0, H, W, H, W, 1, 0, 0};
  return launch_distill_expand<false>(who, frames, rate, img, rate_map, g, n, vec, stream);
}

extern "C" int kdlae_distill_collapse(const float* hq, int B, int F, int Hp, int Wp, int h, int w, int j0, int n,
                                      int mode, const uint8_t* src, int src_channels, void* dst, int dst_u8,
                                      void* stream) {
  const char* who = "kdlae_distill_collapse";
  if (!hq || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_collapse: null argument");
  if (mode != KDLAE_DISTILL_FILE && mode != KDLAE_DISTILL_MEAN)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_collapse: mode must be KDLAE_DISTILL_FILE or KDLAE_DISTILL_MEAN");
  if (mode == KDLAE_DISTILL_MEAN && dst_u8)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_collapse: mode mean has no u8 output");
  if (src && src_channels != 1 && src_channels != 3 && src_channels != 4)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_distill_collapse: src_channels must be 1, 3 or 4");
  TRY(check_distill(who, B, F, h, w, Hp, Wp, j0, n));
  if (h > Hp || w > Wp) return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_collapse: need h <= Hp and w <= Wp");
  if (!al4(hq) || (!dst_u8 && !al4(dst)))
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_distill_collapse: hq and an f32 dst must sit on 4 bytes");
  if (mode == KDLAE_DISTILL_MEAN) src = nullptr;  // no mask in this mode
  // float4 loads: hq on 16 bytes and Wp % 4 == 0; w % 4 == 0 puts every output row on 16 (f32) or 4 (u8) bytes
  const bool vec = al16(hq) && Wp % 4 == 0 && w % 4 == 0 && (dst_u8 ? al4(dst) : al16(dst));
  const int cin = src ? src_channels : 1;
  const int src4 = vec && src && al4(src);
  const DistillGeo g{j0, Hp, Wp, h, w, cin, src4, mode};
  if (dst_u8) return launch_distill_collapse(who, hq, src, static_cast<uint8_t*>(dst), g, n, vec, stream);
  return launch_distill_collapse(who, hq, src, static_cast<float*>(dst), g, n, vec, stream);
}

// Tiled inference (kdlae_tile_plan, kdlae_tile_gather, kdlae_tile_blend, kdlae_tile_blend_rates): the kernels move
// bytes, the blends also add and divide.
//
//   plan                per axis of length L: t = min(tile, L), stride = t - overlap, starts
//                       range(0, L - t, stride) + [L - t], so n = ceil((L - t) / stride) + 1 (1 when L == t) and
//                       start(i) = i < n - 1 ? i stride : L - t.  No start table: both kernels derive the start.
//   tile_gather_kernel  tiles first .. first + count - 1 (flat index (b ni + i) nj + j) of src [B][C][H][W] ->
//                       dense [count][C][th][tw].  One item per V consecutive floats of a destination row.
//   tile_blend_kernel   gather form: one thread per V consecutive output pixels loops over the covering tiles in
//                       ascending flat index (i outer, j inner), acc = 0 + o1 + o2 + ... in fp32, then divides by
//                       the fp32 count: E.add_(patch); W.add_(1); E.div_(W) of the host loop, bit for bit.
//                       No atomics.  scale 2 (the sr output) is the same plan with every coordinate doubled.
//   tile_blend_rates_kernel  the same blend for the R outputs of a tiled rate sweep in one launch: dst
//                       [R][B][C][sH][sW] from the chunk-major staging kdlae_t_forward_rates leaves when it runs
//                       on the n = B ni nj tiles tile_batch at a time: chunk k (count_k = min(tile_batch,
//                       n - k tile_batch) tiles) at float k tile_batch R T, rate r / tile q inside it at
//                       (r count_k + q) T, T = C s^2 th tw.  Same cover loop, same sum order, same division, so
//                       dst[r] has the bits tile_blend_kernel gives for the r-th slice laid out [n][C][sth][stw].
//   tile_blend_w_kernel the two blends with a separable window (kdlae_tile_blend_w, kdlae_tile_blend_rates_w);
//                       stated at the kernel.
//
// V = 4 (float4 loads and stores) when both base pointers sit on 16 bytes and every tile start along x is a
// multiple of 4 floats (H, W and tile are multiples of 8, so that is a condition on the stride alone); V = 1
// otherwise (odd overlaps, offset storage).  In the V = 4 blend all tile edges are multiples of 4, so the four
// pixels of a thread share one cover set.  Flat 64-bit item index with a grid-stride loop: no image is too wide
// or too tall for the grid.
#include <hip/hip_runtime.h>

#include <climits>
#include <cstdint>

#include "runtime.h"

namespace kdlae {

struct TilePlan {
  int th = 0, tw = 0, ni = 0, nj = 0, sy = 0, sx = 0;
};

// kernel geometry, already multiplied by the blend's scale: L = image, t = tile, s = stride, n = tiles
struct TileGeo {
  int Ly, Lx, ty, tx, sy, sx, ni, nj;
};

constexpr long long kTileMaxBlocks = 4096;  // 16 blocks of 256 per CU; the loop takes the rest

__device__ __forceinline__ int tile_start(int i, int n, int stride, int last) { return i < n - 1 ? i * stride : last; }

template <int V>
__global__ __launch_bounds__(256) void tile_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                          TileGeo g, int C, int first, long long total) {
  const int twq = g.tx / V;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / twq;  // over count C th
    const int x = (int)(idx - row * twq) * V;
    const int y = (int)(row % g.ty);
    const long long kc = row / g.ty;
    const int c = (int)(kc % C);
    const int flat = first + (int)(kc / C);
    const int j = flat % g.nj, bi = flat / g.nj;
    const int i = bi % g.ni, b = bi / g.ni;
    const int y0 = tile_start(i, g.ni, g.sy, g.Ly - g.ty), x0 = tile_start(j, g.nj, g.sx, g.Lx - g.tx);
    const float* __restrict__ s = src + (((long long)b * C + c) * g.Ly + y0 + y) * g.Lx + x0 + x;
    if constexpr (V == 4)
      reinterpret_cast<float4*>(dst)[idx] = *reinterpret_cast<const float4*>(s);
    else
      dst[idx] = *s;
  }
}

// tiles covering coordinate p along one axis: the regular ones lo .. hi (start i s, i < n - 1) and, with `last`,
// tile n - 1 at L - t; ascending index is ascending start
struct Cover {
  int lo, hi, last;
};
__device__ __forceinline__ Cover tile_cover(int p, int L, int t, int s, int n) {
  Cover c;
  c.lo = p >= t ? (p - t) / s + 1 : 0;
  c.hi = min(p / s, n - 2);
  c.last = p >= L - t;
  return c;
}

template <int V>
__global__ __launch_bounds__(256) void tile_blend_kernel(const float* __restrict__ tiles, float* __restrict__ dst,
                                                         TileGeo g, int C, long long total) {
  const int wq = g.Lx / V;
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over B C Ly
    const int X = (int)(idx - row * wq) * V;
    const int Y = (int)(row % g.Ly);
    const long long bc = row / g.Ly;
    const int c = (int)(bc % C), b = (int)(bc / C);
    const Cover cy = tile_cover(Y, g.Ly, g.ty, g.sy, g.ni), cx = tile_cover(X, g.Lx, g.tx, g.sx, g.nj);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    int cnt = 0;
    for (int ii = cy.lo; ii <= cy.hi + cy.last; ++ii) {
      const int i = ii <= cy.hi ? ii : g.ni - 1;
      const int yt = Y - (ii <= cy.hi ? i * g.sy : g.Ly - g.ty);
      for (int jj = cx.lo; jj <= cx.hi + cx.last; ++jj) {
        const int j = jj <= cx.hi ? jj : g.nj - 1;
        const int xt = X - (jj <= cx.hi ? j * g.sx : g.Lx - g.tx);
        const long long flat = ((long long)b * g.ni + i) * g.nj + j;
        const float* __restrict__ t = tiles + ((flat * C + c) * g.ty + yt) * g.tx + xt;
        if constexpr (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(t);
          acc[0] += v.x;
          acc[1] += v.y;
          acc[2] += v.z;
          acc[3] += v.w;
        } else {
          acc[0] += *t;
        }
        ++cnt;
      }
    }
    const float w = (float)cnt;
    if constexpr (V == 4)
      reinterpret_cast<float4*>(dst)[idx] = make_float4(acc[0] / w, acc[1] / w, acc[2] / w, acc[3] / w);
    else
      dst[idx] = acc[0] / w;
  }
}

template <int V>
__global__ __launch_bounds__(256) void tile_blend_rates_kernel(const float* __restrict__ staged,
                                                               float* __restrict__ dst, TileGeo g, int C, int R, int B,
                                                               int tile_batch, int ntiles, long long total) {
  const int wq = g.Lx / V;
  const long long T = (long long)C * g.ty * g.tx;  // floats of one staged tile
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over R B C Ly
    const int X = (int)(idx - row * wq) * V;
    const int Y = (int)(row % g.Ly);
    const long long rbc = row / g.Ly;
    const int c = (int)(rbc % C);
    const int rb = (int)(rbc / C);
    const int b = rb % B, r = rb / B;
    const Cover cy = tile_cover(Y, g.Ly, g.ty, g.sy, g.ni), cx = tile_cover(X, g.Lx, g.tx, g.sx, g.nj);
    float acc[V];
#pragma unroll
    for (int e = 0; e < V; ++e) acc[e] = 0.f;
    int cnt = 0;
    for (int ii = cy.lo; ii <= cy.hi + cy.last; ++ii) {
      const int i = ii <= cy.hi ? ii : g.ni - 1;
      const int yt = Y - (ii <= cy.hi ? i * g.sy : g.Ly - g.ty);
      for (int jj = cx.lo; jj <= cx.hi + cx.last; ++jj) {
        const int j = jj <= cx.hi ? jj : g.nj - 1;
        const int xt = X - (jj <= cx.hi ? j * g.sx : g.Lx - g.tx);
        const int flat = (b * g.ni + i) * g.nj + j;
        const int k = flat / tile_batch, q = flat - k * tile_batch;
        const int cnt_k = min(tile_batch, ntiles - k * tile_batch);
        const long long slot = (long long)k * tile_batch * R + (long long)r * cnt_k + q;
        const float* __restrict__ t = staged + slot * T + ((long long)c * g.ty + yt) * g.tx + xt;
        if constexpr (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(t);
          acc[0] += v.x;
          acc[1] += v.y;
          acc[2] += v.z;
          acc[3] += v.w;
        } else {
          acc[0] += *t;
        }
        ++cnt;
      }
    }
    const float w = (float)cnt;
    if constexpr (V == 4)
      reinterpret_cast<float4*>(dst)[idx] = make_float4(acc[0] / w, acc[1] / w, acc[2] / w, acc[3] / w);
    else
      dst[idx] = acc[0] / w;
  }
}

// The weighted blends (kdlae_tile_blend_w, kdlae_tile_blend_rates_w): the cover loop, the tile order and the
// item layout of the two kernels above, with a separable window w = wy[yt] * wx[xt] read at the tile-local
// coordinate (tables of scale * th and scale * tw floats, every entry finite and > 0).  Per pixel, over the
// covering tiles in ascending flat index:  w = fl(wy wx);  E = fl(E + fl(w o));  S = fl(S + w);  out = E / S,
// every operation rounded on its own (no contraction), and a pixel under exactly one tile takes that tile's
// value untouched: fl(fl(w o) / w) is not o for every o, and tile interiors keep the bits of the tile.
// RATES selects the chunk-major staging of the rate sweep (tile_blend_rates_kernel's addressing).  V = 4 also
// needs wx on 16 bytes; the four pixels of a thread share the cover set and wy, each has its own wx.
template <int V, bool RATES>
__global__ __launch_bounds__(256) void tile_blend_w_kernel(const float* __restrict__ tiles,
                                                           const float* __restrict__ wy,
                                                           const float* __restrict__ wx, float* __restrict__ dst,
                                                           TileGeo g, int C, int R, int B, int tile_batch,
                                                           int ntiles, long long total) {
#pragma clang fp contract(off)
  const int wq = g.Lx / V;
  const long long T = (long long)C * g.ty * g.tx;  // floats of one tile
  for (long long idx = blockIdx.x * 256LL + threadIdx.x; idx < total; idx += (long long)gridDim.x * 256) {
    const long long row = idx / wq;  // over [R] B C Ly
    const int X = (int)(idx - row * wq) * V;
    const int Y = (int)(row % g.Ly);
    const long long rbc = row / g.Ly;
    const int c = (int)(rbc % C);
    const int rb = (int)(rbc / C);
    const int b = RATES ? rb % B : rb, r = RATES ? rb / B : 0;
    const Cover cy = tile_cover(Y, g.Ly, g.ty, g.sy, g.ni), cx = tile_cover(X, g.Lx, g.tx, g.sx, g.nj);
    float E[V], S[V], o[V];
#pragma unroll
    for (int e = 0; e < V; ++e) E[e] = 0.f, S[e] = 0.f, o[e] = 0.f;
    int cnt = 0;
    for (int ii = cy.lo; ii <= cy.hi + cy.last; ++ii) {
      const int i = ii <= cy.hi ? ii : g.ni - 1;
      const int yt = Y - (ii <= cy.hi ? i * g.sy : g.Ly - g.ty);
      const float wr = wy[yt];
      for (int jj = cx.lo; jj <= cx.hi + cx.last; ++jj) {
        const int j = jj <= cx.hi ? jj : g.nj - 1;
        const int xt = X - (jj <= cx.hi ? j * g.sx : g.Lx - g.tx);
        const int flat = (b * g.ni + i) * g.nj + j;
        long long slot = flat;
        if constexpr (RATES) {
          const int k = flat / tile_batch, q = flat - k * tile_batch;
          const int cnt_k = min(tile_batch, ntiles - k * tile_batch);
          slot = (long long)k * tile_batch * R + (long long)r * cnt_k + q;
        }
        const float* __restrict__ t = tiles + slot * T + ((long long)c * g.ty + yt) * g.tx + xt;
        float wc[V];
        if constexpr (V == 4) {
          const float4 v = *reinterpret_cast<const float4*>(t);
          const float4 u = *reinterpret_cast<const float4*>(wx + xt);
          o[0] = v.x, o[1] = v.y, o[2] = v.z, o[3] = v.w;
          wc[0] = u.x, wc[1] = u.y, wc[2] = u.z, wc[3] = u.w;
        } else {
          o[0] = *t;
          wc[0] = wx[xt];
        }
#pragma unroll
        for (int e = 0; e < V; ++e) {
          const float w = wr * wc[e];
          const float wo = w * o[e];
          E[e] = E[e] + wo;
          S[e] = S[e] + w;
        }
        ++cnt;
      }
    }
#pragma unroll
    for (int e = 0; e < V; ++e) o[e] = cnt == 1 ? o[e] : E[e] / S[e];
    if constexpr (V == 4)
      reinterpret_cast<float4*>(dst)[idx] = make_float4(o[0], o[1], o[2], o[3]);
    else
      dst[idx] = o[0];
  }
}

static int axis_tiles(int L, int t, int stride) { return L == t ? 1 : (int)ceil_div(L - t, stride) + 1; }

// the argument checks every entry shares; `who` names the entry in the message
static int make_plan(const char* who, int H, int W, int tile, int overlap, TilePlan& p) {
  const std::string w(who);
  if (H < 1 || W < 1) return fail(KDLAE_EINVAL_CONFIG, w + ": H and W must be positive");
  if (H % 8 || W % 8) return fail(KDLAE_EINVAL_SHAPE, w + ": need H % 8 == 0 and W % 8 == 0");
  if (tile < 16 || tile % 8) return fail(KDLAE_EINVAL_SHAPE, w + ": tile must be a multiple of 8, at least 16");
  if (overlap < 0 || overlap >= tile) return fail(KDLAE_EINVAL_SHAPE, w + ": need 0 <= overlap < tile");
  p.th = std::min(tile, H);
  p.tw = std::min(tile, W);
  // an axis the tile covers whole has one tile and no stride to speak of: report the tile size
  p.sy = H > p.th ? p.th - overlap : p.th;
  p.sx = W > p.tw ? p.tw - overlap : p.tw;
  p.ni = axis_tiles(H, p.th, p.sy);
  p.nj = axis_tiles(W, p.tw, p.sx);
  return KDLAE_OK;
}

static unsigned tile_blocks(long long total) { return (unsigned)std::min(ceil_div(total, 256), kTileMaxBlocks); }

}  // namespace kdlae

using namespace kdlae;

extern "C" int kdlae_tile_plan(int H, int W, int tile, int overlap, int* th, int* tw, int* ni, int* nj,
                               int* stride_y, int* stride_x) {
  if (!th || !tw || !ni || !nj || !stride_y || !stride_x)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_plan: null argument");
  TilePlan p;
  TRY(make_plan("kdlae_tile_plan", H, W, tile, overlap, p));
  *th = p.th, *tw = p.tw, *ni = p.ni, *nj = p.nj, *stride_y = p.sy, *stride_x = p.sx;
  return KDLAE_OK;
}

extern "C" int kdlae_tile_gather(const float* src, int B, int C, int H, int W, int tile, int overlap, int first,
                                 int count, float* dst, void* stream) {
  if (!src || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_gather: null argument");
  if (B < 1 || C < 1 || count < 1 || first < 0)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_gather: need B, C, count >= 1 and first >= 0");
  TilePlan p;
  TRY(make_plan("kdlae_tile_gather", H, W, tile, overlap, p));
  const long long ntiles = (long long)B * p.ni * p.nj;
  if (ntiles > INT_MAX) return fail(KDLAE_EINVAL_SHAPE, "kdlae_tile_gather: more than 2^31 - 1 tiles");
  if ((long long)first + count > ntiles)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_gather: first + count passes the last tile (B ni nj = " +
                                         std::to_string(ntiles) + ")");
  const TileGeo g{H, W, p.th, p.tw, p.sy, p.sx, p.ni, p.nj};
  const long long floats = (long long)count * C * p.th * p.tw;
  const bool vec = al16(src) && al16(dst) && (p.nj == 1 || p.sx % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(tile_gather_kernel<4>, dim3(tile_blocks(floats / 4)), dim3(256), 0, (hipStream_t)stream, src,
                       dst, g, C, first, floats / 4);
  else
    hipLaunchKernelGGL(tile_gather_kernel<1>, dim3(tile_blocks(floats)), dim3(256), 0, (hipStream_t)stream, src, dst,
                       g, C, first, floats);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_tile_blend(const float* tiles, int B, int C, int H, int W, int tile, int overlap, int scale,
                                float* dst, void* stream) {
  if (!tiles || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend: null argument");
  if (B < 1 || C < 1) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend: need B >= 1 and C >= 1");
  if (scale != 1 && scale != 2) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend: scale must be 1 or 2");
  TilePlan p;
  TRY(make_plan("kdlae_tile_blend", H, W, tile, overlap, p));
  if ((long long)B * p.ni * p.nj > INT_MAX || (long long)scale * std::max(H, W) > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE, "kdlae_tile_blend: more than 2^31 - 1 tiles or pixels along an axis");
  const int s = scale;
  const TileGeo g{s * H, s * W, s * p.th, s * p.tw, s * p.sy, s * p.sx, p.ni, p.nj};
  const long long floats = (long long)B * C * g.Ly * g.Lx;
  const bool vec = al16(tiles) && al16(dst) && (p.nj == 1 || g.sx % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(tile_blend_kernel<4>, dim3(tile_blocks(floats / 4)), dim3(256), 0, (hipStream_t)stream, tiles,
                       dst, g, C, floats / 4);
  else
    hipLaunchKernelGGL(tile_blend_kernel<1>, dim3(tile_blocks(floats)), dim3(256), 0, (hipStream_t)stream, tiles, dst,
                       g, C, floats);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_tile_blend_rates(const float* staged, int R, int B, int C, int H, int W, int tile, int overlap,
                                      int tile_batch, int scale, float* dst, void* stream) {
  if (!staged || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates: null argument");
  if (R < 1 || R > 64) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates: need 1 <= R <= 64");
  if (B < 1 || C < 1 || tile_batch < 1)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates: need B, C and tile_batch >= 1");
  if (scale != 1 && scale != 2) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates: scale must be 1 or 2");
  TilePlan p;
  TRY(make_plan("kdlae_tile_blend_rates", H, W, tile, overlap, p));
  const long long ntiles = (long long)B * p.ni * p.nj;
  if (ntiles > INT_MAX || (long long)scale * std::max(H, W) > INT_MAX || (long long)R * B * C > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE,
                "kdlae_tile_blend_rates: more than 2^31 - 1 tiles, images x channels or pixels along an axis");
  const int s = scale;
  const TileGeo g{s * H, s * W, s * p.th, s * p.tw, s * p.sy, s * p.sx, p.ni, p.nj};
  const long long floats = (long long)R * B * C * g.Ly * g.Lx;
  // a chunk larger than the sweep is one chunk of all the tiles (and keeps k tile_batch inside an int)
  const int tb = (int)std::min<long long>(tile_batch, ntiles);
  const bool vec = al16(staged) && al16(dst) && (p.nj == 1 || g.sx % 4 == 0);
  if (vec)
    hipLaunchKernelGGL(tile_blend_rates_kernel<4>, dim3(tile_blocks(floats / 4)), dim3(256), 0, (hipStream_t)stream,
                       staged, dst, g, C, R, B, tb, (int)ntiles, floats / 4);
  else
    hipLaunchKernelGGL(tile_blend_rates_kernel<1>, dim3(tile_blocks(floats)), dim3(256), 0, (hipStream_t)stream,
                       staged, dst, g, C, R, B, tb, (int)ntiles, floats);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

// both weighted entries after their checks: R = 0 marks the plain layout [B ni nj][C][s th][s tw]
static int launch_blend_w(const float* tiles, int R, int B, int C, const TileGeo& g, int nj, int tile_batch,
                          int ntiles, const float* wy, const float* wx, float* dst, void* stream) {
  const long long floats = (long long)std::max(R, 1) * B * C * g.Ly * g.Lx;
  const bool vec = al16(tiles) && al16(dst) && al16(wx) && (nj == 1 || g.sx % 4 == 0);
  const long long total = vec ? floats / 4 : floats;
  const dim3 grid(tile_blocks(total)), block(256);
  const hipStream_t st = (hipStream_t)stream;
  if (R == 0) {
    if (vec)
      hipLaunchKernelGGL((tile_blend_w_kernel<4, false>), grid, block, 0, st, tiles, wy, wx, dst, g, C, 1, B, 1,
                         ntiles, total);
    else
      hipLaunchKernelGGL((tile_blend_w_kernel<1, false>), grid, block, 0, st, tiles, wy, wx, dst, g, C, 1, B, 1,
                         ntiles, total);
  } else {
    if (vec)
      hipLaunchKernelGGL((tile_blend_w_kernel<4, true>), grid, block, 0, st, tiles, wy, wx, dst, g, C, R, B,
                         tile_batch, ntiles, total);
    else
      hipLaunchKernelGGL((tile_blend_w_kernel<1, true>), grid, block, 0, st, tiles, wy, wx, dst, g, C, R, B,
                         tile_batch, ntiles, total);
  }
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_tile_blend_w(const float* tiles, int B, int C, int H, int W, int tile, int overlap, int scale,
                                  const float* wy, const float* wx, float* dst, void* stream) {
  if (!tiles || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_w: null argument");
  if (!wy || !wx) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_w: null window table");
  if (B < 1 || C < 1) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_w: need B >= 1 and C >= 1");
  if (scale != 1 && scale != 2) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_w: scale must be 1 or 2");
  TilePlan p;
  TRY(make_plan("kdlae_tile_blend_w", H, W, tile, overlap, p));
  const long long ntiles = (long long)B * p.ni * p.nj;
  if (ntiles > INT_MAX || (long long)scale * std::max(H, W) > INT_MAX || (long long)B * C > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE,
                "kdlae_tile_blend_w: more than 2^31 - 1 tiles, images x channels or pixels along an axis");
  const int s = scale;
  const TileGeo g{s * H, s * W, s * p.th, s * p.tw, s * p.sy, s * p.sx, p.ni, p.nj};
  return launch_blend_w(tiles, 0, B, C, g, p.nj, 1, (int)ntiles, wy, wx, dst, stream);
}

extern "C" int kdlae_tile_blend_rates_w(const float* staged, int R, int B, int C, int H, int W, int tile, int overlap,
                                        int tile_batch, int scale, const float* wy, const float* wx, float* dst,
                                        void* stream) {
  if (!staged || !dst) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates_w: null argument");
  if (!wy || !wx) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates_w: null window table");
  if (R < 1 || R > 64) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates_w: need 1 <= R <= 64");
  if (B < 1 || C < 1 || tile_batch < 1)
    return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates_w: need B, C and tile_batch >= 1");
  if (scale != 1 && scale != 2) return fail(KDLAE_EINVAL_CONFIG, "kdlae_tile_blend_rates_w: scale must be 1 or 2");
  TilePlan p;
  TRY(make_plan("kdlae_tile_blend_rates_w", H, W, tile, overlap, p));
  const long long ntiles = (long long)B * p.ni * p.nj;
  if (ntiles > INT_MAX || (long long)scale * std::max(H, W) > INT_MAX || (long long)R * B * C > INT_MAX)
    return fail(KDLAE_EINVAL_SHAPE,
                "kdlae_tile_blend_rates_w: more than 2^31 - 1 tiles, images x channels or pixels along an axis");
  const int s = scale;
  const TileGeo g{s * H, s * W, s * p.th, s * p.tw, s * p.sy, s * p.sx, p.ni, p.nj};
  // a chunk larger than the sweep is one chunk of all the tiles (and keeps k tile_batch inside an int)
  const int tb = (int)std::min<long long>(tile_batch, ntiles);
  return launch_blend_w(staged, R, B, C, g, p.nj, tb, (int)ntiles, wy, wx, dst, stream);
}

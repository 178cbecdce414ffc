// Geometric self-ensemble (kdlae_ens_gather, kdlae_ens_merge; include/kdlae_ensemble.h states the rule): the
// kernels move bytes, the merge also adds and divides.
//
//   mode m in 0..7      T_m(x) = flipud^(m % 2)(rot90ccw^(m / 2)(x)) on the last two axes.  As an index map a mode
//                       is (t, fy, fx): view element (i, j) is source pixel (y, x) with
//                         t = 0 (modes 0 1 4 5, view [H][W]):  y = fy ? H-1-i : i,  x = fx ? W-1-j : j
//                         t = 1 (modes 2 3 6 7, view [W][H]):  y = fy ? H-1-j : j,  x = fx ? W-1-i : i
//                       t = (m >> 1) & 1, fy for modes {1, 4, 6, 7}, fx for modes {2, 4, 5, 7}.
//   slots               one dense block [N][C][H'][W'] per set bit of the mask, packed in ascending mode order:
//                       slot s at float s N C H W (every view has H W pixels).
//   ens_gather_kernel   a block takes a 32 x 32 tile of one source plane, reads it once (coalesced along x) and
//                       writes it into every slot: the shape-preserving slots from registers, rows and / or
//                       columns reversed; the transposing slots through a padded LDS tile, so that those
//                       writes run along the view's rows (the source's y) and are coalesced as well.
//   ens_merge_kernel    gather form, no atomics: a block owns a 32 x 32 tile of one destination plane.  Per set
//                       mode in ascending order it fetches that slot's values of its pixels (the transposing
//                       slots' tiles are read along the view's rows into LDS and consumed transposed) and every
//                       thread does acc = acc + u on its four pixels, acc starting at 0; one division by the
//                       fp32 count of modes at the end.  Every add and the divide are separate fp32 roundings.
//
// V = 4: the untransposed accesses (the source and the shape-preserving slots, the merged destination) are
// float4 when both base pointers sit on 16 bytes and W % 4 == 0; a reversed row swaps the four components.
// V = 1 otherwise.  A thread owns four pixels either way (V = 1: one column, four rows 8 apart; V = 4: four
// consecutive columns of one row); a pixel's sum order does not depend on V, so neither do its bits.
//
// LDS tile [32][33] floats: ds_read_b32 / ds_write_b32 bank a 32-lane group by dword address mod 32, so the
// transposed reads (stride 33 across the lanes) are conflict-free; two tiles alternate, one barrier per fill.
// Items (plane, tile) are a flat 64-bit index walked with a grid-stride loop under a block cap: no image is too
// large for the grid.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/kdlae_ensemble.h"
#include "runtime.h"

namespace kdlae {

constexpr int kEnsTile = 32;
// 4 blocks of 256 threads per CU on 256 CUs, 4 pixels and up to 8 loads in flight per thread; the loop takes the rest
constexpr long long kEnsMaxBlocks = 1024;
constexpr int kEnsTransposing = 0xCC;  // modes 2 3 6 7

__device__ __forceinline__ bool ens_t(int m) { return (m >> 1) & 1; }
__device__ __forceinline__ bool ens_fy(int m) { return (0xD2 >> m) & 1; }
__device__ __forceinline__ bool ens_fx(int m) { return (0xB4 >> m) & 1; }

struct EnsGeo {
  int H, W, tx;          // the untransformed plane and its tiles along x
  long long tiles;       // tiles of one plane
  long long planes;      // N C
};

// the four pixels of a thread inside its tile
template <int V>
__device__ __forceinline__ void ens_pixels(int tid, int (&ly)[4], int (&lx)[4]) {
#pragma unroll
  for (int e = 0; e < 4; ++e) {
    ly[e] = V == 4 ? tid >> 3 : (tid >> 5) + 8 * e;
    lx[e] = V == 4 ? 4 * (tid & 7) + e : tid & 31;
  }
}

template <int V>
__global__ __launch_bounds__(256) void ens_gather_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                         EnsGeo g, int mask, long long items) {
  __shared__ float lds[2][kEnsTile][kEnsTile + 1];
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  int ly[4], lx[4];
  ens_pixels<V>(tid, ly, lx);
  const int H = g.H, W = g.W;
  const long long plane = (long long)H * W, slot = g.planes * plane;
  const bool any_t = mask & kEnsTransposing;
  int p = 0;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long pl = it / g.tiles, r = it - pl * g.tiles;
    const int y0 = (int)(r / g.tx) * kEnsTile, x0 = (int)(r % g.tx) * kEnsTile;
    const float* __restrict__ sp = src + pl * plane;
    float v[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok[4];
    if constexpr (V == 4) {
      const bool in = y0 + ly[0] < H && x0 + lx[0] < W;  // W % 4 == 0: the four columns are in or out together
      if (in) {
        const float4 q = *reinterpret_cast<const float4*>(sp + (long long)(y0 + ly[0]) * W + x0 + lx[0]);
        v[0] = q.x, v[1] = q.y, v[2] = q.z, v[3] = q.w;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) ok[e] = in;
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        ok[e] = y0 + ly[e] < H && x0 + lx[e] < W;
        if (ok[e]) v[e] = sp[(long long)(y0 + ly[e]) * W + x0 + lx[e]];
      }
    }
    if (any_t) {
#pragma unroll
      for (int e = 0; e < 4; ++e) lds[p][ly[e]][lx[e]] = v[e];
      __syncthreads();
    }
    int s = 0;
    for (int m = 0; m < 8; ++m) {
      if (!((mask >> m) & 1)) continue;
      float* __restrict__ dp = dst + s * slot + pl * plane;
      ++s;
      const bool fy = ens_fy(m), fx = ens_fx(m);
      if (!ens_t(m)) {
        if constexpr (V == 4) {
          if (ok[0]) {
            const int y = y0 + ly[0], x = x0 + lx[0];
            const long long row = (long long)(fy ? H - 1 - y : y) * W;
            if (fx)
              *reinterpret_cast<float4*>(dp + row + (W - 4 - x)) = make_float4(v[3], v[2], v[1], v[0]);
            else
              *reinterpret_cast<float4*>(dp + row + x) = make_float4(v[0], v[1], v[2], v[3]);
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int y = y0 + ly[e], x = x0 + lx[e];
            if (ok[e]) dp[(long long)(fy ? H - 1 - y : y) * W + (fx ? W - 1 - x : x)] = v[e];
          }
        }
      } else {
        // view [W][H]: the lanes run along the source's y, which is the view's row direction
        const int y = y0 + tx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + ty + 8 * k;
          if (y < H && x < W)
            dp[(long long)(fx ? W - 1 - x : x) * H + (fy ? H - 1 - y : y)] = lds[p][tx][ty + 8 * k];
        }
      }
    }
    if (any_t) p ^= 1;
  }
}

template <int V>
__global__ __launch_bounds__(256) void ens_merge_kernel(const float* __restrict__ staged, float* __restrict__ dst,
                                                        EnsGeo g, int mask, float count, long long items) {
  __shared__ float lds[2][kEnsTile][kEnsTile + 1];  // [source column][source row] of the tile
  const int tid = threadIdx.x, tx = tid & 31, ty = tid >> 5;
  int ly[4], lx[4];
  ens_pixels<V>(tid, ly, lx);
  const int H = g.H, W = g.W;
  const long long plane = (long long)H * W, slot = g.planes * plane;
  int p = 0;
  for (long long it = blockIdx.x; it < items; it += gridDim.x) {
    const long long pl = it / g.tiles, r = it - pl * g.tiles;
    const int y0 = (int)(r / g.tx) * kEnsTile, x0 = (int)(r % g.tx) * kEnsTile;
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) ok[e] = y0 + ly[e] < H && x0 + lx[e] < W;
    float acc[4] = {0.f, 0.f, 0.f, 0.f};
    int s = 0;
    for (int m = 0; m < 8; ++m) {
      if (!((mask >> m) & 1)) continue;
      const float* __restrict__ up = staged + s * slot + pl * plane;
      ++s;
      const bool fy = ens_fy(m), fx = ens_fx(m);
      float u[4] = {0.f, 0.f, 0.f, 0.f};
      if (!ens_t(m)) {
        if constexpr (V == 4) {
          if (ok[0]) {
            const int y = y0 + ly[0], x = x0 + lx[0];
            const long long row = (long long)(fy ? H - 1 - y : y) * W;
            if (fx) {
              const float4 q = *reinterpret_cast<const float4*>(up + row + (W - 4 - x));
              u[0] = q.w, u[1] = q.z, u[2] = q.y, u[3] = q.x;
            } else {
              const float4 q = *reinterpret_cast<const float4*>(up + row + x);
              u[0] = q.x, u[1] = q.y, u[2] = q.z, u[3] = q.w;
            }
          }
        } else {
#pragma unroll
          for (int e = 0; e < 4; ++e) {
            const int y = y0 + ly[e], x = x0 + lx[e];
            if (ok[e]) u[e] = up[(long long)(fy ? H - 1 - y : y) * W + (fx ? W - 1 - x : x)];
          }
        }
      } else {
        // view [W][H]: read along its rows (the destination's y), consume transposed
        const int y = y0 + tx;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
          const int x = x0 + ty + 8 * k;
          lds[p][ty + 8 * k][tx] =
              y < H && x < W ? up[(long long)(fx ? W - 1 - x : x) * H + (fy ? H - 1 - y : y)] : 0.f;
        }
        __syncthreads();
#pragma unroll
        for (int e = 0; e < 4; ++e) u[e] = lds[p][lx[e]][ly[e]];
        p ^= 1;
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) acc[e] = acc[e] + u[e];
    }
    float* __restrict__ dp = dst + pl * plane;
    if constexpr (V == 4) {
      if (ok[0])
        *reinterpret_cast<float4*>(dp + (long long)(y0 + ly[0]) * W + x0 + lx[0]) =
            make_float4(acc[0] / count, acc[1] / count, acc[2] / count, acc[3] / count);
    } else {
#pragma unroll
      for (int e = 0; e < 4; ++e)
        if (ok[e]) dp[(long long)(y0 + ly[e]) * W + x0 + lx[e]] = acc[e] / count;
    }
  }
}

// the argument checks both entries share; `who` names the entry in the message
static int ens_check(const char* who, const void* src, const void* dst, int N, int C, int H, int W, int mode_mask,
                     EnsGeo& g, long long& items) {
  const std::string w(who);
  if (!src || !dst) return fail(KDLAE_EINVAL_SHAPE, w + ": null argument");
  if (N < 1 || C < 1 || H < 1 || W < 1) return fail(KDLAE_EINVAL_SHAPE, w + ": N, C, H and W must be positive");
  if (mode_mask < 1 || mode_mask > 255)
    return fail(KDLAE_EINVAL_SHAPE, w + ": mode_mask must have at least one of its low 8 bits set and no other (got " +
                                        std::to_string(mode_mask) + ")");
  g.H = H, g.W = W;
  g.tx = (int)ceil_div(W, kEnsTile);
  g.tiles = ceil_div(H, kEnsTile) * g.tx;
  g.planes = (long long)N * C;
  items = g.planes * g.tiles;
  return KDLAE_OK;
}

static unsigned ens_blocks(long long items) { return (unsigned)std::min(items, kEnsMaxBlocks); }

}  // namespace kdlae

using namespace kdlae;

extern "C" int kdlae_ens_gather(const float* src, float* dst, int N, int C, int H, int W, int mode_mask,
                                void* stream) {
  EnsGeo g;
  long long items;
  TRY(ens_check("kdlae_ens_gather", src, dst, N, C, H, W, mode_mask, g, items));
  if (al16(src) && al16(dst) && W % 4 == 0)
    hipLaunchKernelGGL(ens_gather_kernel<4>, dim3(ens_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       mode_mask, items);
  else
    hipLaunchKernelGGL(ens_gather_kernel<1>, dim3(ens_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       mode_mask, items);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_ens_merge(const float* src, float* dst, int N, int C, int H, int W, int mode_mask,
                               void* stream) {
  EnsGeo g;
  long long items;
  TRY(ens_check("kdlae_ens_merge", src, dst, N, C, H, W, mode_mask, g, items));
  const float count = (float)__builtin_popcount((unsigned)mode_mask);
  if (al16(src) && al16(dst) && W % 4 == 0)
    hipLaunchKernelGGL(ens_merge_kernel<4>, dim3(ens_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       mode_mask, count, items);
  else
    hipLaunchKernelGGL(ens_merge_kernel<1>, dim3(ens_blocks(items)), dim3(256), 0, (hipStream_t)stream, src, dst, g,
                       mode_mask, count, items);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

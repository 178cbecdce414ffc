// ASDQE training kernels (gfx950): BatchNorm2d with batch statistics (forward, running update,
// backward), the adjoint of the bilinear x2 upsample, the train-mode regressor head and the MSE loss.
//
// The BatchNorm kernels are built to be memory bound (measured rates: DESIGN.md section 9).  Threads
// of a 256-thread block are (pixel lane, channel quad) with the quads fastest, so a pixel's C channels
// are one contiguous float4 run and a thread keeps its channel quad (and that quad's mean / rstd /
// gamma / beta in registers) while it walks pixels.  Reductions: a thread's run of pixels, then the
// block's lanes in lane order through LDS, then the blocks in block order in a second kernel: a fixed
// order, no atomics.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>

#include "train_a.h"
#include "train_kernels.h"

namespace kdlae {
namespace train {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kT = 256;
constexpr float kBnEps = 1e-5f;

__device__ inline f32x4 ld4(const float* p) { return *reinterpret_cast<const f32x4*>(p); }
__device__ inline void st4(float* p, f32x4 v) { *reinterpret_cast<f32x4*>(p) = v; }
__device__ inline f32x4 splat(float v) { return f32x4{v, v, v, v}; }

// Chan's pairwise update of (count, mean, M2): a <- a (+) b
__device__ inline void chan(float& na, f32x4& ma, f32x4& qa, float nb, f32x4 mb, f32x4 qb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb; ma = mb; qa = qb;
    return;
  }
  const float n = na + nb;
  const f32x4 d = mb - ma;
  const float fb = nb / n;
  ma += d * fb;
  qa += qb + d * d * (na * fb);
  na = n;
}
__device__ inline void chan1(float& na, float& ma, float& qa, float nb, float mb, float qb) {
  if (nb == 0.f) return;
  if (na == 0.f) {
    na = nb; ma = mb; qa = qb;
    return;
  }
  const float n = na + nb, d = mb - ma, fb = nb / n;
  ma += d * fb;
  qa += qb + d * d * (na * fb);
  na = n;
}

// stage 1: block b owns pixels [b per, min(P, (b + 1) per)); pmean / pm2 [nblk][C]
__global__ __launch_bounds__(kT) void bn_stats_part_kernel(const float* __restrict__ x, int ld, int C, long long P,
                                                           long long per, float* __restrict__ pmean,
                                                           float* __restrict__ pm2) {
  __shared__ f32x4 smean[kT], sm2[kT];
  __shared__ float scnt[kT];
  const int c4n = C >> 2, lanes = kT / c4n;
  const int tid = threadIdx.x, cq = tid % c4n, pl = tid / c4n;
  const long long p0 = (long long)blockIdx.x * per, p1 = min(P, p0 + per);
  f32x4 mean = splat(0.f), m2 = splat(0.f);
  float n = 0.f;
  if (pl < lanes) {
    const float* base = x + cq * 4;
#pragma unroll 4
    for (long long p = p0 + pl; p < p1; p += lanes) {
      const f32x4 v = ld4(base + p * ld);
      n += 1.f;
      const f32x4 d = v - mean;
      mean += d * (1.f / n);
      m2 += d * (v - mean);
    }
  }
  smean[tid] = mean;
  sm2[tid] = m2;
  scnt[tid] = n;
  __syncthreads();
  if (tid < c4n) {
    for (int l = 1; l < lanes; ++l) chan(n, mean, m2, scnt[l * c4n + tid], smean[l * c4n + tid], sm2[l * c4n + tid]);
    st4(pmean + (long long)blockIdx.x * C + tid * 4, mean);
    st4(pm2 + (long long)blockIdx.x * C + tid * 4, m2);
  }
}

// stage 2: block = 16 channels x 16 segments of the stage-1 blocks; segment sums in block order, then
// the 16 segments in order.  Also nn.BatchNorm2d's running update (momentum; unbiased variance).
__global__ __launch_bounds__(kT) void bn_stats_final_kernel(const float* __restrict__ pmean,
                                                            const float* __restrict__ pm2, int nblk, long long per,
                                                            long long P, int C, float* __restrict__ mean,
                                                            float* __restrict__ rstd, float* __restrict__ rm,
                                                            float* __restrict__ rv, float momentum) {
  __shared__ float sn[16][16], sm[16][16], sq[16][16];
  const int c = threadIdx.x & 15, j = threadIdx.x >> 4;
  const int ch = blockIdx.x * 16 + c;
  float n = 0.f, m = 0.f, q = 0.f;
  if (ch < C) {
    const int b0 = (int)((long long)nblk * j / 16), b1 = (int)((long long)nblk * (j + 1) / 16);
    for (int b = b0; b < b1; ++b) {
      const long long q0 = (long long)b * per;
      const float nb = (float)(min(P, q0 + per) - q0);
      chan1(n, m, q, nb, pmean[(long long)b * C + ch], pm2[(long long)b * C + ch]);
    }
  }
  sn[j][c] = n;
  sm[j][c] = m;
  sq[j][c] = q;
  __syncthreads();
  if (j != 0 || ch >= C) return;
  for (int k = 1; k < 16; ++k) chan1(n, m, q, sn[k][c], sm[k][c], sq[k][c]);
  const float var = q / (float)P;
  mean[ch] = m;
  rstd[ch] = 1.f / sqrtf(var + kBnEps);
  if (rm) {
    const float unb = P > 1 ? q / (float)(P - 1) : var;
    rm[ch] = (1.f - momentum) * rm[ch] + momentum * m;
    rv[ch] = (1.f - momentum) * rv[ch] + momentum * unb;
  }
}

constexpr int kU = 4;  // pixels per thread per step: their loads are issued together

__global__ __launch_bounds__(kT) void bn_apply_relu_kernel(const float* __restrict__ z, int ldz,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd,
                                                           const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, int C, long long P,
                                                           float* __restrict__ y, int ldy) {
  const int c4n = C >> 2, lanes = kT / c4n;
  const int cq = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  if (pl >= lanes) return;
  const f32x4 mu = ld4(mean + cq * 4), a = ld4(rstd + cq * 4) * ld4(gamma + cq * 4), b = ld4(beta + cq * 4);
  const long long step = (long long)gridDim.x * lanes;
  for (long long p = (long long)blockIdx.x * lanes + pl; p < P; p += step * kU) {
    f32x4 v[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long q = p + u * step;
      v[u] = q < P ? ld4(z + q * ldz + cq * 4) : splat(0.f);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long q = p + u * step;
      if (q >= P) break;
      f32x4 r = (v[u] - mu) * a + b;
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = fmaxf(r[e], 0.f);
      st4(y + q * ldy + cq * 4, r);
    }
  }
}

// part[blk][2 C]: [dgamma | dbeta]
__global__ __launch_bounds__(kT) void bn_bwd_reduce_kernel(const float* __restrict__ dy, int ldd,
                                                           const float* __restrict__ y, int ldy,
                                                           const float* __restrict__ z, int ldz,
                                                           const float* __restrict__ mean,
                                                           const float* __restrict__ rstd, int C, long long P,
                                                           long long per, float* __restrict__ part) {
  __shared__ f32x4 sg[kT], sb[kT];
  const int c4n = C >> 2, lanes = kT / c4n;
  const int tid = threadIdx.x, cq = tid % c4n, pl = tid / c4n;
  const long long p0 = (long long)blockIdx.x * per, p1 = min(P, p0 + per);
  f32x4 dg = splat(0.f), db = splat(0.f);
  if (pl < lanes) {
    const f32x4 mu = ld4(mean + cq * 4), rs = ld4(rstd + cq * 4);
#pragma unroll 4
    for (long long p = p0 + pl; p < p1; p += lanes) {
      f32x4 g = ld4(dy + p * ldd + cq * 4);
      const f32x4 yy = ld4(y + p * ldy + cq * 4);
      const f32x4 xh = (ld4(z + p * ldz + cq * 4) - mu) * rs;
#pragma unroll
      for (int e = 0; e < 4; ++e) g[e] = yy[e] > 0.f ? g[e] : 0.f;
      db += g;
      dg += g * xh;
    }
  }
  sg[tid] = dg;
  sb[tid] = db;
  __syncthreads();
  if (tid < c4n) {
    for (int l = 1; l < lanes; ++l) {
      dg += sg[l * c4n + tid];
      db += sb[l * c4n + tid];
    }
    float* o = part + (long long)blockIdx.x * 2 * C;
    st4(o + tid * 4, dg);
    st4(o + C + tid * 4, db);
  }
}

// dz may alias dy (each element is read, then written, by the same thread)
__global__ __launch_bounds__(kT) void bn_bwd_dx_kernel(const float* dy, int ldd, const float* __restrict__ y, int ldy,
                                                       const float* __restrict__ z, int ldz,
                                                       const float* __restrict__ mean,
                                                       const float* __restrict__ rstd,
                                                       const float* __restrict__ gamma,
                                                       const float* __restrict__ dgamma,
                                                       const float* __restrict__ dbeta, int C, long long P,
                                                       float invP, float* dz, int lddz) {
  const int c4n = C >> 2, lanes = kT / c4n;
  const int cq = threadIdx.x % c4n, pl = threadIdx.x / c4n;
  if (pl >= lanes) return;
  const f32x4 mu = ld4(mean + cq * 4), rs = ld4(rstd + cq * 4);
  const f32x4 a = ld4(gamma + cq * 4) * rs;
  const f32x4 kb = ld4(dbeta + cq * 4) * invP, kg = ld4(dgamma + cq * 4) * invP;
  const long long step = (long long)gridDim.x * lanes;
  for (long long p = (long long)blockIdx.x * lanes + pl; p < P; p += step * kU) {
    f32x4 g[kU], yy[kU], zz[kU];
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long q = p + u * step;
      const bool ok = q < P;
      g[u] = ok ? ld4(dy + q * ldd + cq * 4) : splat(0.f);
      yy[u] = ok ? ld4(y + q * ldy + cq * 4) : splat(0.f);
      zz[u] = ok ? ld4(z + q * ldz + cq * 4) : splat(0.f);
    }
#pragma unroll
    for (int u = 0; u < kU; ++u) {
      const long long q = p + u * step;
      if (q >= P) break;
      f32x4 r = g[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) r[e] = yy[u][e] > 0.f ? r[e] : 0.f;
      const f32x4 xh = (zz[u] - mu) * rs;
      st4(dz + q * lddz + cq * 4, a * (r - kb - xh * kg));
    }
  }
}

// One thread per (low-resolution pixel, channel quad).  The high-resolution rows that can read low row
// iy are oy in [2 iy - 3, 2 iy + 4] (src = oy (h - 1) / (2h - 1), a ratio in [1/3, 1/2)); each
// candidate's source row and weights are recomputed with the forward's own float arithmetic, and the
// candidate counts with weight [y0 == iy] ly0 + [y0 + yp == iy] ly1.  Columns alike.
__global__ __launch_bounds__(kT) void upsample2x_bwd_kernel(const float* __restrict__ dout, int ldo,
                                                            float* __restrict__ din, int ldi, int C, int N, int h,
                                                            int w) {
  const int H2 = 2 * h, W2 = 2 * w, c4n = C >> 2;
  const float rh = H2 > 1 ? (float)(h - 1) / (float)(H2 - 1) : 0.f;
  const float rw = W2 > 1 ? (float)(w - 1) / (float)(W2 - 1) : 0.f;
  const long long total = (long long)N * h * w * c4n;
  for (long long idx = blockIdx.x * (long long)kT + threadIdx.x; idx < total; idx += (long long)gridDim.x * kT) {
    const int c = (int)(idx % c4n) * 4;
    long long r = idx / c4n;
    const int ix = (int)(r % w);
    r /= w;
    const int iy = (int)(r % h);
    const long long n = r / h;
    float wy[8], wx[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int oy = 2 * iy - 3 + k, ox = 2 * ix - 3 + k;
      wy[k] = 0.f;
      wx[k] = 0.f;
      if (oy >= 0 && oy < H2) {
        float sy;
        {
#pragma clang fp contract(off)
          sy = rh * (float)oy;  // rounded on its own, as upsample2x_kernel does
        }
        const int y0 = (int)sy, yp = y0 < h - 1 ? 1 : 0;
        const float l1 = sy - (float)y0, l0 = 1.f - l1;
        wy[k] = (y0 == iy ? l0 : 0.f) + (y0 + yp == iy ? l1 : 0.f);
      }
      if (ox >= 0 && ox < W2) {
        float sx;
        {
#pragma clang fp contract(off)
          sx = rw * (float)ox;
        }
        const int x0 = (int)sx, xp = x0 < w - 1 ? 1 : 0;
        const float l1 = sx - (float)x0, l0 = 1.f - l1;
        wx[k] = (x0 == ix ? l0 : 0.f) + (x0 + xp == ix ? l1 : 0.f);
      }
    }
    f32x4 acc = splat(0.f);
#pragma unroll
    for (int ky = 0; ky < 8; ++ky) {
      if (wy[ky] == 0.f) continue;
      const int oy = 2 * iy - 3 + ky;
      const float* row = dout + ((n * H2 + oy) * W2) * (long long)ldo + c;
      f32x4 racc = splat(0.f);
#pragma unroll
      for (int kx = 0; kx < 8; ++kx) {
        if (wx[kx] == 0.f) continue;
        const int ox = 2 * ix - 3 + kx;
        racc += ld4(row + (long long)ox * ldo) * wx[kx];
      }
      acc += racc * wy[ky];
    }
    st4(din + ((n * h + iy) * w + ix) * (long long)ldi + c, acc);
  }
}

__global__ __launch_bounds__(kT) void asdqe_pack_inputs_kernel(const float* __restrict__ lq,
                                                               const float* __restrict__ gt, int ci, int B, int H,
                                                               int W, int Hp, int Wp, float* __restrict__ xin) {
  const long long total = (long long)B * Hp * Wp;
  for (long long p = blockIdx.x * (long long)kT + threadIdx.x; p < total; p += (long long)gridDim.x * kT) {
    const int x = (int)(p % Wp);
    const long long r = p / Wp;
    const int y = (int)(r % Hp);
    const long long b = r / Hp;
    f32x4 a = splat(0.f), g = splat(0.f);
    if (y < H && x < W) {
      for (int c = 0; c < ci; ++c) {
        const long long i = ((b * ci + c) * H + y) * W + x;
        a[c] = lq[i];
        g[c] = gt[i];
      }
    }
    st4(xin + p * 12, a);
    st4(xin + p * 12 + 4, g);
    st4(xin + p * 12 + 8, a - g);
  }
}

__global__ __launch_bounds__(kT) void narrow_w_copy_kernel(const float* __restrict__ src, float* __restrict__ dst,
                                                           int Cout, int ci) {
  const int total = Cout * ci * 9;
  for (int i = blockIdx.x * kT + threadIdx.x; i < total; i += gridDim.x * kT) {
    const int t = i % 9, c = (i / 9) % ci, o = i / (9 * ci);
    dst[i] = src[(o * 4 + c) * 9 + t];
  }
}

__global__ __launch_bounds__(kT) void bcast_rows_kernel(const float* __restrict__ v, long long ldv, int C,
                                                        long long HW, long long P, float scale,
                                                        float* __restrict__ out, int ldo) {
  const int c4n = C >> 2;
  const long long total = P * c4n;
  for (long long i = blockIdx.x * (long long)kT + threadIdx.x; i < total; i += (long long)gridDim.x * kT) {
    const int cq = (int)(i % c4n);
    const long long p = i / c4n;
    st4(out + p * ldo + cq * 4, ld4(v + (p / HW) * ldv + cq * 4) * scale);
  }
}

__global__ __launch_bounds__(kT) void grad_commit_kernel(const float* __restrict__ g, float* __restrict__ grad,
                                                         long long n4, int accumulate) {
  for (long long i = blockIdx.x * (long long)kT + threadIdx.x; i < n4; i += (long long)gridDim.x * kT) {
    f32x4 v = ld4(g + i * 4);
    if (accumulate) v += ld4(grad + i * 4);
    st4(grad + i * 4, v);
  }
}

// ---- regressor head.  save row: [g C | f M | a1 N1 | a2 N2 | da1 N1 | da2 N2 | da3, score, 0, 0 | df M | dgap C]
struct HeadOff {
  int g, f, a1, a2, da1, da2, da3, df, dgap, total;
};
__host__ __device__ inline HeadOff head_off(int C, int M, int N1, int N2) {
  HeadOff o;
  o.g = 0;
  o.f = C;
  o.a1 = o.f + M;
  o.a2 = o.a1 + N1;
  o.da1 = o.a2 + N2;
  o.da2 = o.da1 + N1;
  o.da3 = o.da2 + N2;
  o.df = o.da3 + 4;
  o.dgap = o.df + M;
  o.total = o.dgap + C;
  return o;
}

constexpr int kHeadMax = 1024;

// one block per image; every dot product is one thread's fixed-order loop
__global__ __launch_bounds__(kT) void head_train_fwd_kernel(HeadTrain p) {
  __shared__ float g[kHeadMax], f[kHeadMax], h1[kHeadMax], h2[kHeadMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  const HeadOff o = head_off(p.C, p.M, p.N1, p.N2);
  float* sv = p.save + (long long)b * o.total;
  for (int c = tid; c < p.C; c += kT) {
    float t = 0.f;
    for (int sl = 0; sl < p.slots; ++sl) t += p.partial[((long long)b * p.slots + sl) * p.C + c];
    g[c] = t * p.inv_hw;
    sv[o.g + c] = g[c];
  }
  __syncthreads();
  for (int m = tid; m < p.M; m += kT) {
    float t = p.bo[m];
    for (int c = 0; c < p.C; ++c) t = fmaf(p.wo[m * p.C + c], g[c], t);
    f[m] = t;
    sv[o.f + m] = t;
  }
  __syncthreads();
  for (int j = tid; j < p.N1; j += kT) {
    float t = p.b1[j];
    for (int m = 0; m < p.M; ++m) t = fmaf(p.w1[j * p.M + m], f[m], t);
    sv[o.a1 + j] = t;
    h1[j] = fmaxf(t, 0.f) * (p.mask1 ? p.mask1[(long long)b * p.N1 + j] : 1.f);
  }
  __syncthreads();
  for (int k = tid; k < p.N2; k += kT) {
    float t = p.b2[k];
    for (int j = 0; j < p.N1; ++j) t = fmaf(p.w2[k * p.N1 + j], h1[j], t);
    sv[o.a2 + k] = t;
    h2[k] = fmaxf(t, 0.f) * (p.mask2 ? p.mask2[(long long)b * p.N2 + k] : 1.f);
  }
  __syncthreads();
  if (tid == 0) {
    float t = p.b3[0];
    for (int k = 0; k < p.N2; ++k) t = fmaf(p.w3[k], h2[k], t);
    const float sc = tanhf(t);
    p.score[b] = sc;
    sv[o.da3 + 1] = sc;
  }
}

// per image: the activation gradients down to dgap (the gradient of the pooled UNet features)
__global__ __launch_bounds__(kT) void head_train_bwd_act_kernel(HeadTrain p, const float* __restrict__ dscore) {
  __shared__ float da2[kHeadMax], da1[kHeadMax], df[kHeadMax];
  const int b = blockIdx.x, tid = threadIdx.x;
  const HeadOff o = head_off(p.C, p.M, p.N1, p.N2);
  float* sv = p.save + (long long)b * o.total;
  const float sc = sv[o.da3 + 1];
  const float da3 = dscore[b] * (1.f - sc * sc);
  if (tid == 0) sv[o.da3] = da3;
  for (int k = tid; k < p.N2; k += kT) {
    const float m = p.mask2 ? p.mask2[(long long)b * p.N2 + k] : 1.f;
    const float t = sv[o.a2 + k] > 0.f ? p.w3[k] * da3 * m : 0.f;
    da2[k] = t;
    sv[o.da2 + k] = t;
  }
  __syncthreads();
  for (int j = tid; j < p.N1; j += kT) {
    float t = 0.f;
    for (int k = 0; k < p.N2; ++k) t = fmaf(p.w2[k * p.N1 + j], da2[k], t);
    const float m = p.mask1 ? p.mask1[(long long)b * p.N1 + j] : 1.f;
    t = sv[o.a1 + j] > 0.f ? t * m : 0.f;
    da1[j] = t;
    sv[o.da1 + j] = t;
  }
  __syncthreads();
  for (int m = tid; m < p.M; m += kT) {
    float t = 0.f;
    for (int j = 0; j < p.N1; ++j) t = fmaf(p.w1[j * p.M + m], da1[j], t);
    df[m] = t;
    sv[o.df + m] = t;
  }
  __syncthreads();
  for (int c = tid; c < p.C; c += kT) {
    float t = 0.f;
    for (int m = 0; m < p.M; ++m) t = fmaf(p.wo[m * p.C + c], df[m], t);
    sv[o.dgap + c] = t;
  }
}

// one thread per parameter gradient: a sum over the images in image order
__global__ __launch_bounds__(kT) void head_train_bwd_w_kernel(HeadTrain p, HeadTrainGrads G) {
  const HeadOff o = head_off(p.C, p.M, p.N1, p.N2);
  const int nwo = p.M * p.C, nw1 = p.N1 * p.M, nw2 = p.N2 * p.N1;
  const int e0 = nwo, e1 = e0 + p.M, e2 = e1 + nw1, e3 = e2 + p.N1, e4 = e3 + nw2, e5 = e4 + p.N2, e6 = e5 + p.N2,
            e7 = e6 + 1;
  for (int i = blockIdx.x * kT + threadIdx.x; i < e7; i += gridDim.x * kT) {
    float t = 0.f;
    float* dst;
    if (i < e0) {  // dWo[m][c] = sum_b df[b][m] g[b][c]
      const int m = i / p.C, c = i - m * p.C;
      for (int b = 0; b < p.B; ++b) t = fmaf(p.save[(long long)b * o.total + o.df + m], p.save[(long long)b * o.total + o.g + c], t);
      dst = G.wo + i;
    } else if (i < e1) {
      const int m = i - e0;
      for (int b = 0; b < p.B; ++b) t += p.save[(long long)b * o.total + o.df + m];
      dst = G.bo + m;
    } else if (i < e2) {  // dW1[j][m] = sum_b da1[b][j] f[b][m]
      const int j = (i - e1) / p.M, m = (i - e1) - j * p.M;
      for (int b = 0; b < p.B; ++b) t = fmaf(p.save[(long long)b * o.total + o.da1 + j], p.save[(long long)b * o.total + o.f + m], t);
      dst = G.w1 + (i - e1);
    } else if (i < e3) {
      const int j = i - e2;
      for (int b = 0; b < p.B; ++b) t += p.save[(long long)b * o.total + o.da1 + j];
      dst = G.b1 + j;
    } else if (i < e4) {  // dW2[k][j] = sum_b da2[b][k] h1[b][j]
      const int k = (i - e3) / p.N1, j = (i - e3) - k * p.N1;
      for (int b = 0; b < p.B; ++b) {
        const float m = p.mask1 ? p.mask1[(long long)b * p.N1 + j] : 1.f;
        const float h1 = fmaxf(p.save[(long long)b * o.total + o.a1 + j], 0.f) * m;
        t = fmaf(p.save[(long long)b * o.total + o.da2 + k], h1, t);
      }
      dst = G.w2 + (i - e3);
    } else if (i < e5) {
      const int k = i - e4;
      for (int b = 0; b < p.B; ++b) t += p.save[(long long)b * o.total + o.da2 + k];
      dst = G.b2 + k;
    } else if (i < e6) {  // dw3[k] = sum_b da3[b] h2[b][k]
      const int k = i - e5;
      for (int b = 0; b < p.B; ++b) {
        const float m = p.mask2 ? p.mask2[(long long)b * p.N2 + k] : 1.f;
        const float h2 = fmaxf(p.save[(long long)b * o.total + o.a2 + k], 0.f) * m;
        t = fmaf(p.save[(long long)b * o.total + o.da3], h2, t);
      }
      dst = G.w3 + k;
    } else {
      for (int b = 0; b < p.B; ++b) t += p.save[(long long)b * o.total + o.da3];
      dst = G.b3;
    }
    *dst = t;
  }
}

__global__ __launch_bounds__(64) void mse_kernel(const float* __restrict__ s_, const float* __restrict__ t, int n,
                                                 float scale, float* __restrict__ ds, float* __restrict__ loss) {
  const float k = scale * 2.f / (float)n;
  for (int i = threadIdx.x; i < n; i += 64) ds[i] = k * (s_[i] - t[i]);
  if (threadIdx.x == 0) {
    float a = 0.f, m = 0.f;
    for (int i = 0; i < n; ++i) {
      const float d = s_[i] - t[i];
      a = fmaf(d, d, a);
      m += fabsf(d);
    }
    loss[0] = a / (float)n;
    loss[1] = m / (float)n;
  }
}

inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline bool view_ok(const void* p, int ld, int C) { return p && al16(p) && ld % 4 == 0 && ld >= C; }
inline bool chan_ok(int C) { return C >= 4 && C % 4 == 0 && C <= 1024; }

// stage-1 geometry of the BatchNorm reductions: >= 16 pixels per lane, at most kBnMaxBlocks blocks
void red_geom(int C, long long P, int* nblk, long long* per) {
  const int lanes = kT / (C >> 2);
  long long nb = (P + 16LL * lanes - 1) / (16LL * lanes);
  nb = std::max<long long>(1, std::min<long long>(kBnMaxBlocks, nb));
  *per = (P + nb - 1) / nb;
  *nblk = (int)((P + *per - 1) / *per);
}
unsigned ew_blocks(int C, long long P) {
  const int lanes = kT / (C >> 2);
  const long long nb = (P + (long long)lanes * kU - 1) / ((long long)lanes * kU);
  return (unsigned)std::max<long long>(1, std::min<long long>(4096, nb));
}
unsigned flat_blocks(long long total) {
  return (unsigned)std::max<long long>(1, std::min<long long>(8192, (total + kT - 1) / kT));
}

}  // namespace

hipError_t launch_bn_stats(const float* x, int ldx, int C, long long P, float* mean, float* rstd, float* rm,
                           float* rv, float momentum, float* part, hipStream_t s) {
  if (!chan_ok(C) || P < 1 || !view_ok(x, ldx, C) || !mean || !rstd || !al16(part) || !part || (rm && !rv))
    return hipErrorInvalidValue;
  int nblk;
  long long per;
  red_geom(C, P, &nblk, &per);
  float* pmean = part;
  float* pm2 = part + (long long)kBnMaxBlocks * C;
  hipLaunchKernelGGL(bn_stats_part_kernel, dim3(nblk), dim3(kT), 0, s, x, ldx, C, P, per, pmean, pm2);
  hipLaunchKernelGGL(bn_stats_final_kernel, dim3((C + 15) / 16), dim3(kT), 0, s, pmean, pm2, nblk, per, P, C, mean,
                     rstd, rm, rv, momentum);
  return hipGetLastError();
}

hipError_t launch_bn_apply_relu(const float* z, int ldz, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, int C, long long P, float* y, int ldy, hipStream_t s) {
  if (!chan_ok(C) || P < 1 || !view_ok(z, ldz, C) || !view_ok(y, ldy, C) || !al16(mean) || !al16(rstd) ||
      !al16(gamma) || !al16(beta) || !mean || !rstd || !gamma || !beta)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_apply_relu_kernel, dim3(ew_blocks(C, P)), dim3(kT), 0, s, z, ldz, mean, rstd, gamma, beta, C,
                     P, y, ldy);
  return hipGetLastError();
}

hipError_t launch_bn_bwd_reduce(const float* dy, int ldd, const float* y, int ldy, const float* z, int ldz,
                                const float* mean, const float* rstd, int C, long long P, float* dgamma,
                                float* dbeta, float* part, hipStream_t s) {
  if (!chan_ok(C) || P < 1 || !view_ok(dy, ldd, C) || !view_ok(y, ldy, C) || !view_ok(z, ldz, C) || !mean || !rstd ||
      !al16(mean) || !al16(rstd) || !dgamma || !dbeta || !part || !al16(part))
    return hipErrorInvalidValue;
  int nblk;
  long long per;
  red_geom(C, P, &nblk, &per);
  hipLaunchKernelGGL(bn_bwd_reduce_kernel, dim3(nblk), dim3(kT), 0, s, dy, ldd, y, ldy, z, ldz, mean, rstd, C, P, per,
                     part);
  hipError_t e = launch_part_reduce(part, nblk, C, 1, dgamma, 0, 1.f, s, 2 * C);
  if (e != hipSuccess) return e;
  return launch_part_reduce(part + C, nblk, C, 1, dbeta, 0, 1.f, s, 2 * C);
}

hipError_t launch_bn_bwd_dx(const float* dy, int ldd, const float* y, int ldy, const float* z, int ldz,
                            const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                            const float* dbeta, int C, long long P, float* dz, int lddz, hipStream_t s) {
  if (!chan_ok(C) || P < 1 || !view_ok(dy, ldd, C) || !view_ok(y, ldy, C) || !view_ok(z, ldz, C) ||
      !view_ok(dz, lddz, C) || !mean || !rstd || !gamma || !dgamma || !dbeta || !al16(mean) || !al16(rstd) ||
      !al16(gamma) || !al16(dgamma) || !al16(dbeta))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bn_bwd_dx_kernel, dim3(ew_blocks(C, P)), dim3(kT), 0, s, dy, ldd, y, ldy, z, ldz, mean, rstd,
                     gamma, dgamma, dbeta, C, P, 1.f / (float)P, dz, lddz);
  return hipGetLastError();
}

hipError_t launch_upsample2x_bwd(const float* dout, int ldo, float* din, int ldi, int C, int N, int h, int w,
                                 hipStream_t s) {
  if (!chan_ok(C) || N < 1 || h < 1 || w < 1 || !view_ok(dout, ldo, C) || !view_ok(din, ldi, C))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(upsample2x_bwd_kernel, dim3(flat_blocks((long long)N * h * w * (C / 4))), dim3(kT), 0, s, dout,
                     ldo, din, ldi, C, N, h, w);
  return hipGetLastError();
}

hipError_t launch_asdqe_pack_inputs(const float* lq, const float* gt, int ci, int B, int H, int W, int Hp, int Wp,
                                    float* xin, hipStream_t s) {
  if (!lq || !gt || !xin || !al16(xin) || ci < 1 || ci > 4 || B < 1 || H < 1 || W < 1 || Hp < H || Wp < W)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(asdqe_pack_inputs_kernel, dim3(flat_blocks((long long)B * Hp * Wp)), dim3(kT), 0, s, lq, gt, ci,
                     B, H, W, Hp, Wp, xin);
  return hipGetLastError();
}

hipError_t launch_narrow_w_copy(const float* src, float* dst, int Cout, int ci, hipStream_t s) {
  if (!src || !dst || Cout < 1 || ci < 1 || ci > 4) return hipErrorInvalidValue;
  hipLaunchKernelGGL(narrow_w_copy_kernel, dim3(flat_blocks((long long)Cout * ci * 9)), dim3(kT), 0, s, src, dst, Cout,
                     ci);
  return hipGetLastError();
}

hipError_t launch_bcast_rows(const float* v, long long ldv, int C, int B, long long HW, float scale, float* out,
                             int ldo, hipStream_t s) {
  if (!chan_ok(C) || B < 1 || HW < 1 || !v || !al16(v) || ldv % 4 || !view_ok(out, ldo, C))
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(bcast_rows_kernel, dim3(flat_blocks(B * HW * (C / 4))), dim3(kT), 0, s, v, ldv, C, HW, B * HW,
                     scale, out, ldo);
  return hipGetLastError();
}

hipError_t launch_grad_commit(const float* g, float* grad, long long n, int accumulate, hipStream_t s) {
  if (!g || !grad || n < 4 || n % 4 || !al16(g) || !al16(grad)) return hipErrorInvalidValue;
  hipLaunchKernelGGL(grad_commit_kernel, dim3(flat_blocks(n / 4)), dim3(kT), 0, s, g, grad, n / 4, accumulate);
  return hipGetLastError();
}

static bool head_ok(const HeadTrain& p) {
  return p.B >= 1 && p.C >= 1 && p.C <= kHeadMax && p.M >= 1 && p.M <= kHeadMax && p.N1 >= 1 && p.N1 <= kHeadMax &&
         p.N2 >= 1 && p.N2 <= kHeadMax && p.save && p.wo && p.bo && p.w1 && p.b1 && p.w2 && p.b2 && p.w3 && p.b3;
}

hipError_t launch_head_train_fwd(const HeadTrain& p, hipStream_t s) {
  if (!head_ok(p) || !p.partial || p.slots < 1 || !p.score) return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_train_fwd_kernel, dim3(p.B), dim3(kT), 0, s, p);
  return hipGetLastError();
}

hipError_t launch_head_train_bwd(const HeadTrain& p, const float* dscore, const HeadTrainGrads& g, hipStream_t s) {
  if (!head_ok(p) || !dscore || !g.wo || !g.bo || !g.w1 || !g.b1 || !g.w2 || !g.b2 || !g.w3 || !g.b3)
    return hipErrorInvalidValue;
  hipLaunchKernelGGL(head_train_bwd_act_kernel, dim3(p.B), dim3(kT), 0, s, p, dscore);
  const long long n = (long long)p.M * p.C + p.M + (long long)p.N1 * p.M + p.N1 + (long long)p.N2 * p.N1 + 2 * p.N2 + 1;
  hipLaunchKernelGGL(head_train_bwd_w_kernel, dim3(flat_blocks(n)), dim3(kT), 0, s, p, g);
  return hipGetLastError();
}

hipError_t launch_mse(const float* s_, const float* t, int n, float scale, float* ds, float* loss, hipStream_t s) {
  if (!s_ || !t || !ds || !loss || n < 1) return hipErrorInvalidValue;
  hipLaunchKernelGGL(mse_kernel, dim3(1), dim3(64), 0, s, s_, t, n, scale, ds, loss);
  return hipGetLastError();
}

}  // namespace train
}  // namespace kdlae

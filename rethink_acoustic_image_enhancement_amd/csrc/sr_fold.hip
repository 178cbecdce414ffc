// The sr head's first two convs as one: cen (3x3, Cin -> hc, padding 1, KDLAE_model.py:242) and
// upen.body.0 (3x3, hc -> 2 hc, no bias, :243) have no non-linearity between them, so their composition
// is a 5x5 conv Cin -> 2 hc on the zero-padded hq, except on the one-pixel image border: upen zero-pads
// cen's OUTPUT, so an upen tap that lands outside the image contributes nothing, where the plain 5x5
// conv would evaluate cen there from in-image pixels.  The pack program (pack.hip, pack_fold_kernel)
// therefore stores 9 weight sets, {first row, interior, last row} x {first column, interior, last
// column}, each the sum over that class's valid upen taps only, composed in float64 and rounded once.
//
// K = 25 Cin (+ 1: the bias slot) is far too small for the split-bf16 GEMMs' 32-deep steps to pay (75 of
// 96 slots used, and both operands' splits on the VALU); this is conv_small.hip's form instead, exact
// fp32 products on v_mfma_f32_16x16x4_f32 with the weights as the A operand and 16 pixels of one image
// row as B.  A block owns an 8 x 64 pixel tile: it stages the (8 + 4) x (64 + 4) x Cin input patch in
// LDS with explicit zeros outside the image, and each of its 4 waves owns a quarter of the output
// channel tiles for every pixel of the tile, so a wave's weight fragments (NTW x KS VGPRs) are loaded
// once and stay in registers while it walks the tile's 32 pixel groups.
//
// Slot k = 25 c + 5 a + b is tap (a, b) of input channel c; slot 25 Cin carries the constant 1 whose
// weight is the class's bias (cen.bias pushed through the valid upen taps), so a pixel gets its bias
// in the same product as its taps.  Border classes: a pixel group of an interior block takes the
// interior set, no per-pixel test.  A group that holds column 0 or column W - 1 runs one pass per
// column class present, the B operand zeroed for the pixels of the other classes; the row class is
// uniform along a group.  Only the weight registers are swapped between passes.
//
// Output rows are permuted by the pack (row 4 e + i of tile t = pre-shuffle channel 16 t + 4 i + e),
// so a lane's accumulator (rows 4 lq .. 4 lq + 3) is channels 4 t .. 4 t + 3 of output pixel
// (2 y + lq / 2, 2 x + lq % 2) after PixelShuffle(2): one 16-byte NHWC store per tile.
#include "kernels.h"

namespace kdlae {

namespace {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int kTR = 8, kTC = 64, kPH = kTR + 4, kPW = kTC + 4;

template <int CIN, int NTW>
__global__ __launch_bounds__(256) void sr_fold_kernel(SrFoldParams p) {
  constexpr int K = 25 * CIN, KS = sr_fold_ksteps(CIN), PP = kPH * kPW;
  __shared__ float patch[CIN * PP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int li = lane & 15, lq = lane >> 4;
  const int tx_n = (p.W + kTC - 1) / kTC, ty_n = (p.H + kTR - 1) / kTR;
  int bid = blockIdx.x;
  const int txi = bid % tx_n;
  bid /= tx_n;
  const int tyi = bid % ty_n;
  const int b = bid / ty_n;
  const int x0 = txi * kTC, y0 = tyi * kTR;
  const long long HW = (long long)p.H * p.W;
  const float* inb = p.in + (long long)b * CIN * HW;
  for (int i = tid; i < CIN * PP; i += 256) {
    const int c = i / PP, rem = i - c * PP;
    const int r = rem / kPW, x = rem - r * kPW;
    const int yy = y0 + r - 2, xx = x0 + x - 2;
    const bool ok = (unsigned)yy < (unsigned)p.H && (unsigned)xx < (unsigned)p.W;
    patch[i] = ok ? inb[c * HW + (long long)yy * p.W + xx] : 0.f;
  }
  // this lane's slot per k-step (k = 4 s + lq): offset of its tap from the window's top-left corner
  int koff[KS];
#pragma unroll
  for (int s = 0; s < KS; ++s) {
    const int k = 4 * s + lq;
    const int kk = k < K ? k : 0;  // slots past the taps have zero weights: any finite value will do
    const int c = kk / 25, t = kk - c * 25;
    koff[s] = c * PP + (t / 5) * kPW + t % 5;
  }
  const int t0 = wave * NTW;  // this wave's first output tile
  // the interior-column set of the current row class stays in registers; the first- and last-column sets
  // are read where they are used (one pixel group in four of a border block's, at most)
  float wf[NTW][KS];
  int cur = -1;
  __syncthreads();
  const int Wo = 2 * p.W;
  for (int r = 0; r < kTR; ++r) {
    const int y = y0 + r;
    if (y >= p.H) break;
    const int rc = y == 0 ? 0 : y == p.H - 1 ? 2 : 1;
    const float* wrow = p.w + ((size_t)(3 * rc) * p.ntiles + t0) * (KS * 64) + lane;  // class (rc, first column)
    const size_t wcls = (size_t)p.ntiles * (KS * 64);
    if (rc != cur) {
      cur = rc;
#pragma unroll
      for (int n = 0; n < NTW; ++n)
#pragma unroll
        for (int s = 0; s < KS; ++s) wf[n][s] = wrow[wcls + (n * KS + s) * 64];
    }
#pragma unroll 1
    for (int j = 0; j < kTC / 16; ++j) {
      const int xs = x0 + 16 * j;
      if (xs >= p.W) break;
      const int x = xs + li;
      const float* win = patch + r * kPW + 16 * j + li;  // (y - 2, x - 2)
      float bv[KS];
#pragma unroll
      for (int s = 0; s < KS; ++s) bv[s] = 4 * s + lq == K ? 1.f : win[koff[s]];
      f32x4 acc[NTW];
#pragma unroll
      for (int n = 0; n < NTW; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
      const bool has0 = xs == 0, has2 = xs + 16 >= p.W;  // the group holds column 0 / column W - 1
      const bool mid = !(has0 || has2) || (x >= 1 && x <= p.W - 2);
#pragma unroll
      for (int s = 0; s < KS; ++s) {
        const float v = mid ? bv[s] : 0.f;
#pragma unroll
        for (int n = 0; n < NTW; ++n) acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(wf[n][s], v, acc[n], 0, 0, 0);
      }
      // one more pass per border column in the group, on that column's weight set
      auto edge = [&](const float* we, bool on) {
#pragma unroll
        for (int s = 0; s < KS; ++s) {
          const float v = on ? bv[s] : 0.f;
#pragma unroll
          for (int n = 0; n < NTW; ++n)
            acc[n] = __builtin_amdgcn_mfma_f32_16x16x4f32(we[(n * KS + s) * 64], v, acc[n], 0, 0, 0);
        }
      };
      if (has0) edge(wrow, x == 0);
      if (has2) edge(wrow + 2 * wcls, x == p.W - 1);
      if (x >= p.W) continue;
      float* o = p.out + (((long long)b * 2 * p.H + 2 * y + (lq >> 1)) * Wo + 2 * x + (lq & 1)) * p.ldo + 4 * t0;
#pragma unroll
      for (int n = 0; n < NTW; ++n) *reinterpret_cast<f32x4*>(o + 4 * n) = acc[n];
    }
  }
}

template <int CIN>
void launch_ntw(const SrFoldParams& p, unsigned blocks, hipStream_t s) {
  switch (p.ntiles / 4) {
    case 1: hipLaunchKernelGGL((sr_fold_kernel<CIN, 1>), dim3(blocks), dim3(256), 0, s, p); break;
    case 2: hipLaunchKernelGGL((sr_fold_kernel<CIN, 2>), dim3(blocks), dim3(256), 0, s, p); break;
    case 3: hipLaunchKernelGGL((sr_fold_kernel<CIN, 3>), dim3(blocks), dim3(256), 0, s, p); break;
    default: hipLaunchKernelGGL((sr_fold_kernel<CIN, 4>), dim3(blocks), dim3(256), 0, s, p); break;
  }
}

}  // namespace

bool sr_fold_supported(int cin, int ntiles) {
  return cin >= 1 && cin <= 4 && ntiles >= 4 && ntiles <= 16 && ntiles % 4 == 0;
}

hipError_t launch_sr_fold(const SrFoldParams& p, hipStream_t s) {
  if (!sr_fold_supported(p.Cin, p.ntiles) || !p.in || !p.w || !p.out || p.Bn <= 0 || p.H < 8 || p.W < 8 || p.H % 8 ||
      p.W % 8 || p.ldo < 4 * p.ntiles || p.ldo % 4 || ((uintptr_t)p.out & 15))
    return hipErrorInvalidValue;
  const long long blocks = (long long)p.Bn * ((p.H + kTR - 1) / kTR) * ((p.W + kTC - 1) / kTC);
  if (blocks > 0x7fffffffLL) return hipErrorInvalidValue;
  switch (p.Cin) {
    case 1: launch_ntw<1>(p, (unsigned)blocks, s); break;
    case 2: launch_ntw<2>(p, (unsigned)blocks, s); break;
    case 3: launch_ntw<3>(p, (unsigned)blocks, s); break;
    default: launch_ntw<4>(p, (unsigned)blocks, s); break;
  }
  return hipGetLastError();
}

}  // namespace kdlae

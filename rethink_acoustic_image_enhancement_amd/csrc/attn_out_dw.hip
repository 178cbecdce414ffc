// Attention output with the depthwise 3x3 of v as its prologue, C = 48 / 96 (kernels.h AttnOutDwParams):
//   out = R + bias + M_img . dw3x3(v)
// The v-writing Gram ring stored v' = dw3x3(v) and the per-image-weight gemm_res_kernel read it back;
// here v is read once from the qkv buffer (plus a one-pixel halo) and v' lives only in LDS.
//
// Blocking: a block owns a 16-column strip x a segment of rows of one image and sweeps it row by row,
// as the Gram ring does (halo re-read 18 / 16 in x, (rows + 2) / rows in y).
//  * DMA waves (the last NDW waves): rows of v arrive by LDS-DMA into a 6-row ring, 18 pixels x
//    [C | 1 pad float4] per row; pad items and out-of-image pixels read p.zeros.  Their only VMEM ops are
//    the DMAs, PPD pieces per row each at straight-line destinations, so "row y + 2 has landed" is a
//    compile-time s_waitcnt vmcnt(PPD * rows issued after it) (lds_dma.h).
//  * compute wave g (CT of them) is k-group g of the product and output tile g.  Per row it
//    1. runs the MFMAs of row y: B operands = the split planes of v' staged by all waves in the previous
//       step, A operands = its tile's M records, resident in VGPRs; then bias + residual, one 16-byte store
//       per lane (pixel li, channels 16 g + 4 lq ..);
//    2. applies the stencil to row y + 1 for its 16 channels (lane: pixel li, channel quad lq — the float4
//       a GEMM lane of k-group g loads), splits the four values (mfma3.h split1) and stages the three
//       bf16 planes in the other staging buffer, in the B-operand order of pair g / 2, half g & 1.
//    One barrier per row.
// Numerics: v' by dw3.h's order, split1 per value, pairs ascending with mfma6's term order, (acc + bias)
// + R: the bits of the ring + gemm_res_kernel pair.
#include "kernels.h"
#include "mfma3.h"
#include "lds_dma.h"
#include "dw3.h"

namespace kdlae {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));

template <int CT>
struct AttnOutDw {
  static constexpr int C = 16 * CT;
  static constexpr int KP = (CT + 1) / 2;             // 32-deep pairs (an odd last k-group pairs with zeros)
  static constexpr int NCW = CT, NDW = 2, NW = NCW + NDW;
  static constexpr int PS4 = C / 4 + 1;               // float4 per ring pixel (pad: conflict-free column reads)
  static constexpr int PS = 4 * PS4;
  static constexpr int Items = 18 * PS4;
  static constexpr int Pieces = ((Items + 63) / 64 + NDW - 1) / NDW * NDW;  // 1 KiB DMA wave-instructions per row
  static constexpr int PPD = Pieces / NDW;            // pieces per DMA wave per row
  static constexpr int RowF4 = Pieces * 64;
  static constexpr int NSlot = 6;
  static constexpr int StageF4 = 3 * KP * 64;         // [plane][pair][lane] x 16 B
  static constexpr int WdwF4 = 11 * C / 4;            // [tap | dw bias | out bias][C / 4]
  static constexpr size_t lds_bytes = (size_t)(NSlot * RowF4 + 2 * StageF4 + WdwF4) * 16;
};

constexpr int kAttnOutDwWavesPerSimd = 4;

template <int CT>
__global__ __launch_bounds__(64 * AttnOutDw<CT>::NW, kAttnOutDwWavesPerSimd) void attn_out_dw_kernel(
    AttnOutDwParams p, int seg_rows, int nseg) {
#pragma clang fp contract(off)
  using K = AttnOutDw<CT>;
  using dma::f32x4;
  constexpr int KP = K::KP, NCW = K::NCW, NDW = K::NDW, PPD = K::PPD, PS = K::PS, PS4 = K::PS4;
  static_assert(3 * PPD < 64, "ring DMA accounting");
  extern __shared__ __attribute__((aligned(16))) dma::f32x4 aring[];
  float* ringf = reinterpret_cast<float*>(aring);
  f32x4* stg = aring + K::NSlot * K::RowF4;  // [2][3][KP][64]
  f32x4* wl = stg + 2 * K::StageF4;          // [11][C / 4]: in LDS, 44 VGPRs per lane otherwise
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int li = lane & 15, lq = lane >> 4;
  // XCD-aware block order: XCD k (blockIdx.x & 7) walks the logical range [k n / 8, (k + 1) n / 8), so
  // neighbouring strips, whose 2 halo columns overlap, are read on the same L2 at about the same time
  const int strips = p.W >> 4;
  const int nblk = (int)gridDim.x;
  const int id = nblk % 8 == 0 ? (int)(blockIdx.x & 7) * (nblk >> 3) + (int)(blockIdx.x >> 3) : (int)blockIdx.x;
  const int strip = id % strips, seg = (id / strips) % nseg, b = id / (strips * nseg);
  const int HW = p.H * p.W;
  const int xs = strip * 16;
  const int y0 = seg * seg_rows, y1 = min(y0 + seg_rows, p.H);

  // staging starts as zeros: the upper half of an odd C's last pair is never written
  for (int i = tid; i < 2 * K::StageF4; i += 64 * K::NW) stg[i] = f32x4{0.f, 0.f, 0.f, 0.f};
  for (int i = tid; i < K::WdwF4; i += 64 * K::NW) {
    const int t = i / (K::C / 4), c4 = i - t * (K::C / 4);
    const float* src = t < 9 ? p.wdw + (long long)t * p.ldw : t == 9 ? p.bdw : p.bias;
    wl[i] = src ? *reinterpret_cast<const f32x4*>(src + 4 * c4) : f32x4{0.f, 0.f, 0.f, 0.f};
  }

  if (wave >= NCW) {
    // ---------------------------------------------------------------- DMA waves
    const int drank = wave - NCW;
    unsigned colo[PPD];
#pragma unroll
    for (int j = 0; j < PPD; ++j) {
      const int it = (drank + NDW * j) * 64 + lane;
      const int px = it / PS4, r = it - (it / PS4) * PS4;
      const int xx = xs - 1 + px;
      const bool ok = it < K::Items && r < PS4 - 1 && (unsigned)xx < (unsigned)p.W;
      colo[j] = ok ? (unsigned)((xx * p.ldv + 4 * r) * 4) : ~0u;
    }
    const unsigned rowbytes = (unsigned)p.W * (unsigned)p.ldv * 4u;
    const char* Xb = reinterpret_cast<const char*>(p.v + (long long)b * HW * p.ldv);
    auto issue = [&](int yy) {
      f32x4* sl = aring + ((yy + K::NSlot) % K::NSlot) * K::RowF4;
      const bool oky = (unsigned)yy < (unsigned)p.H;
#pragma unroll
      for (int j = 0; j < PPD; ++j) {
        const void* src = (oky && colo[j] != ~0u) ? (const void*)(Xb + (unsigned)yy * rowbytes + colo[j])
                                                   : (const void*)p.zeros;
        dma::dma16(src, sl + 64 * (drank + NDW * j));
      }
    };
    // wait until only the DMAs of the `ra` youngest rows are outstanding
    auto wait_rows = [&](int ra) {
      if (ra >= 3) dma::wait_vmcnt<3 * PPD>();
      else if (ra == 2) dma::wait_vmcnt<2 * PPD>();
      else if (ra == 1) dma::wait_vmcnt<PPD>();
      else dma::wait_vmcnt<0>();
    };
    __syncthreads();
    // rows y0 - 1 .. min(y0 + 4, y1) in flight; the first stencil needs y0 - 1 .. y0 + 1
    for (int yy = y0 - 1; yy <= min(y0 + 4, y1); ++yy) issue(yy);
    wait_rows(max(0, min(y0 + 4, y1) - (y0 + 1)));
    dma::barrier_lds();
    for (int y = y0; y < y1; ++y) {
      // rows .. y + 2 landed: the younger DMAs are rows y + 3 .. min(y + 4, y1)
      if (y + 1 < y1) wait_rows(max(0, min(y + 4, y1) - (y + 2)));
      dma::barrier_lds();
      if (y + 5 <= y1) issue(y + 5);  // into the slot of row y - 1, last read by the stencil of row y
    }
    return;
  }

  // ------------------------------------------------------------------ compute waves
  const int cg = 16 * wave + 4 * lq;  // this lane's channel quad: k index of the product and output channel
  F3 wm[KP];  // M records of output tile `wave`
  {
    const f32x4* M = reinterpret_cast<const f32x4*>(p.M + (long long)b * p.m_img_stride) + (long long)wave * KP * kRec3;
#pragma unroll
    for (int G = 0; G < KP; ++G) wm[G] = load_w3(M + G * kRec3, lane);
  }
  // block-uniform image base + a 32-bit lane offset (the launcher bounds an image's R / out extent)
  const float* __restrict__ Rb = p.R + (long long)b * HW * p.ldr;
  float* __restrict__ Ob = p.out + (long long)b * HW * p.ldo;
  const int ro = (xs + li) * p.ldr + cg, oo = (xs + li) * p.ldo + cg;
  auto load_res = [&](int y) { return *reinterpret_cast<const f32x4*>(Rb + (y * p.W * p.ldr + ro)); };
  // v' of ring row r for this lane's pixel and channel quad -> split planes into staging buffer sb
  auto stencil = [&](int r, int sb) {
    // one window row (3 pixels) and its 3 taps' weights live at a time
    const f32x4 bdw = wl[9 * (K::C / 4) + (cg >> 2)];
    float a[4] = {bdw[0], bdw[1], bdw[2], bdw[3]};
#pragma unroll
    for (int rr = 0; rr < 3; ++rr) {
      const float* row = ringf + ((r - 1 + rr + K::NSlot) % K::NSlot) * K::RowF4 * 4 + li * PS + cg;
      f32x4 x[3], wt[3];
#pragma unroll
      for (int dx = 0; dx < 3; ++dx) {
        x[dx] = *reinterpret_cast<const f32x4*>(row + dx * PS);
        wt[dx] = wl[(3 * rr + dx) * (K::C / 4) + (cg >> 2)];
      }
#pragma unroll
      for (int e = 0; e < 4; ++e) a[e] = dw3_row(a[e], x[0][e], x[1][e], x[2][e], wt[0][e], wt[1][e], wt[2][e]);
    }
    bf16x4 h, m, l;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
      __bf16 hh, mm, ll;
      split1(a[e], hh, mm, ll);
      h[e] = hh;
      m[e] = mm;
      l[e] = ll;
    }
    char* dst = reinterpret_cast<char*>(stg + sb * K::StageF4 + (wave >> 1) * 64 + lane) + 8 * (wave & 1);
    *reinterpret_cast<bf16x4*>(dst) = h;
    *reinterpret_cast<bf16x4*>(dst + KP * 1024) = m;
    *reinterpret_cast<bf16x4*>(dst + 2 * KP * 1024) = l;
  };

  __syncthreads();      // staging zeroed (the DMA waves start issuing after it)
  dma::barrier_lds();   // rows y0 - 1 .. y0 + 1 landed
  stencil(y0, 0);
  int buf = 0;
  for (int y = y0; y < y1; ++y) {
    const bool st = y + 1 < y1;
    dma::barrier_lds();  // row y staged by every wave; ring rows .. y + 2 landed
    // the residual's latency hides under this row's MFMAs and the next row's stencil; it follows the
    // previous row's store on the in-order counter, which is a whole step old by the time it is needed
    const f32x4 rc = load_res(y);
    f32x4 acc = f32x4{0.f, 0.f, 0.f, 0.f};
    const f32x4* xb = stg + buf * K::StageF4 + lane;
#pragma unroll
    for (int G = 0; G < KP; ++G) {
      F3 x;
      x.h = __builtin_bit_cast(bf16x8, xb[G * 64]);
      x.m = __builtin_bit_cast(bf16x8, xb[(KP + G) * 64]);
      x.l = __builtin_bit_cast(bf16x8, xb[(2 * KP + G) * 64]);
      acc = mfma6(wm[G], x, acc);
    }
    if (st) stencil(y + 1, buf ^ 1);
    f32x4 v = acc + wl[10 * (K::C / 4) + (cg >> 2)];
    v += rc;
    *reinterpret_cast<f32x4*>(Ob + (y * p.W * p.ldo + oo)) = v;
    buf ^= 1;
  }
}

bool attn_out_dw_supported(int C, int H, int W, int ldv) {
  return (C == 48 || C == 96) && H >= 1 && W >= 16 && W % 16 == 0 && ldv >= C && ldv % 4 == 0 &&
         (unsigned long long)H * W * ldv * 4 < (1ull << 32);
}

template <int CT>
static hipError_t launch_attn_out_dw_ct(const AttnOutDwParams& p, hipStream_t s) {
  using K = AttnOutDw<CT>;
  static size_t attr[64] = {};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) dev = 0;
  if (K::lds_bytes > 64 * 1024 && K::lds_bytes > attr[dev]) {
    hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&attn_out_dw_kernel<CT>),
                                       hipFuncAttributeMaxDynamicSharedMemorySize, (int)K::lds_bytes);
    if (e != hipSuccess) return e;
    attr[dev] = K::lds_bytes;
  }
  // row segments: 64 rows from 512 rows up (y halo 66 / 64), else 32 (34 / 32); the last may be partial
  const int seg_rows = p.H >= 512 ? 64 : 32;
  const int nseg = (p.H + seg_rows - 1) / seg_rows;
  const long long grid = (long long)(p.W / 16) * nseg * p.Bn;
  if (grid > 0x7fffffffLL) return hipErrorInvalidValue;
  hipLaunchKernelGGL(attn_out_dw_kernel<CT>, dim3((unsigned)grid), dim3(64 * K::NW), K::lds_bytes, s, p, seg_rows, nseg);
  return hipGetLastError();
}

hipError_t launch_attn_out_dw(const AttnOutDwParams& p, int C, hipStream_t s) {
  if (!attn_out_dw_supported(C, p.H, p.W, p.ldv) || p.Bn < 1 || !p.v || !p.wdw || !p.M || !p.R || !p.out || !p.zeros ||
      p.ldw % 4 || p.ldr % 4 || p.ldo % 4 || p.ldr < C || p.ldo < C ||
      (long long)p.H * p.W * (p.ldr > p.ldo ? p.ldr : p.ldo) * 4 >= (1LL << 31))
    return hipErrorInvalidValue;
  return C == 48 ? launch_attn_out_dw_ct<3>(p, s) : launch_attn_out_dw_ct<6>(p, s);
}

}  // namespace kdlae

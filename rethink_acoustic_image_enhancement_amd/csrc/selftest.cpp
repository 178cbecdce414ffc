// Kernel self-test entry points (include/kdlae.h, "Kernel self-test entry points"): single launches
// of internal kernel families on caller buffers, so tests/test_kernel_variants_gpu.py can reach every
// compiled variant against a torch reference.  Not part of the drop-in boundary; nothing here is on
// a forward / training path.
//   kdlae_debug_tgemm                      the training GEMM family (rows / cols / tiled kernels)
//   kdlae_debug_gemm, _gemm_variant        the inference implicit-GEMM family
//   kdlae_debug_gram                       MDTA dwconv + Gram
//   kdlae_debug_ln                         training LayerNorm forward / backward
//   kdlae_debug_small_in                   small-input 3x3 / 3x3x3 conv
//   kdlae_debug_bn                         ASDQE training BatchNorm / upsample kernels and the step's small helpers
//                                          (input packing, narrow weight copy, row broadcast, gradient commit)
//   kdlae_debug_head_train                 ASDQE train-mode regressor head, forward and backward
//   kdlae_debug_train, _train_blocks       the KDLAE-T step's non-GEMM kernels: MDTA softmax core and its
//                                          backward, depthwise / gate family, small-side 3x3 weight gradient,
//                                          column reductions, layout kernels (tests/test_train_kernels_gpu.py)
//   kdlae_debug_train_s                    the KDLAE-S step's im2col / col2im, weight permute, ReLU mask,
//                                          max-pool backward, transposed-conv scatter, fragment packing, ReLU
//   kdlae_debug_infer                      the forward paths' kernels outside those families: fused GDFN tail,
//                                          fused feed-forward half, fused MDTA pass 1, softmax + fold, dwconv
//                                          gate, LDS-tiled convs, small-output conv, max-pool, ASDQE pool + head
//                                          (tests/test_infer_kernels_gpu.py)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>

#include "../../include/kdlae.h"
#include "runtime.h"
#include "train_a.h"
#include "train_kernels.h"
#include "train_s.h"

namespace tr = kdlae::train;
using kdlae::fail;

extern "C" int kdlae_debug_tgemm(const kdlae_debug_tgemm_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  tr::TGemm g;
  g.A = d->A; g.sam = d->sam; g.sak = d->sak; g.amode = d->amode;
  g.B = d->B; g.sbk = d->sbk; g.sbn = d->sbn; g.bmode = d->bmode;
  g.C = d->C; g.scm = d->scm; g.scn = d->scn;
  g.bias = d->bias;
  g.R = d->R; g.srm = d->srm; g.srn = d->srn;
  g.rs = d->rs;
  g.M = d->M; g.N = d->N; g.K = d->K; g.nz1 = d->nz1; g.nz2 = d->nz2;
  g.bA1 = d->bA1; g.bA2 = d->bA2; g.bB1 = d->bB1; g.bB2 = d->bB2; g.bC1 = d->bC1; g.bC2 = d->bC2;
  g.bR1 = d->bR1; g.bR2 = d->bR2; g.brs1 = d->brs1; g.brs2 = d->brs2;
  g.Bn = d->Bn; g.H = d->H; g.W = d->W; g.Cg = d->Cg; g.dil = d->dil; g.lda = d->lda; g.ldb = d->ldb;
  g.partial = d->partial;
  g.c_pad_ok = d->c_pad_ok != 0;
  g.F = d->F > 0 ? d->F : 1;
  const size_t cap = d->partial ? (size_t)d->partial_floats : 0;
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  switch (d->route) {
    case 0: e = tr::launch_tgemm(g, cap, s); break;
    case 1:
      if (!tr::tgemm_rows_eligible(g)) return fail(KDLAE_EINVAL_CONFIG, "not eligible for the row-streaming kernel");
      e = tr::launch_tgemm_rows(g, s);
      break;
    case 2:
      if (!cap || !tr::tgemm_cols_eligible(g)) return fail(KDLAE_EINVAL_CONFIG, "not eligible for the pixel kernel");
      e = tr::launch_tgemm_cols(g, cap, s);
      break;
    case 3: e = tr::launch_tgemm_tiled(g, cap, s); break;
    default: return fail(KDLAE_EINVAL_CONFIG, "route must be 0..3");
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_tgemm: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_gemm_variant(int family, int i, int* v) {
  if (!v) return 0;
  return kdlae::gemm_variant_entry(family, i, v) ? 1 : 0;
}

extern "C" int kdlae_debug_gemm(const kdlae_debug_gemm_desc* d, void* stream) {
  using kdlae::ceil_div;
  if (!d || !d->A || !d->Wp || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null descriptor or operand");
  if (d->Bn < 1 || d->F < 1 || d->H < 1 || d->W < 1 || d->ntiles < 1 || d->kgroups < 1 || d->N < 1 ||
      d->N > 16 * d->ntiles || d->NT < 1 || d->KG < 1)
    return fail(KDLAE_EINVAL_SHAPE, "bad GEMM geometry");
  if (d->ksize != 1 && d->ksize != 3) return fail(KDLAE_EINVAL_SHAPE, "ksize must be 1 or 3");
  const int kt = d->ksize == 3 ? d->kt : 1;
  if (d->ksize == 3 && ((kt != 1 && kt != 3) || d->kgroups != 9 * kt * d->cg_per_tap || d->lda < 16 * d->cg_per_tap))
    return fail(KDLAE_EINVAL_SHAPE, "implicit conv needs kgroups = 9 kt cg_per_tap and lda >= 16 cg_per_tap");
  if (d->ksize == 1 && d->lda < 16 * d->kgroups) return fail(KDLAE_EINVAL_SHAPE, "lda < K");
  if (d->out_mode == 0 && d->ldo < d->N) return fail(KDLAE_EINVAL_SHAPE, "ldo < N");
  if (d->out_mode == 1 && (d->H % 2 || d->W % 2 || d->ldo < 4 * d->N)) return fail(KDLAE_EINVAL_SHAPE, "unshuffle geometry");
  if (d->out_mode == 2 && (d->N % 4 || d->ldo < d->N / 4)) return fail(KDLAE_EINVAL_SHAPE, "shuffle geometry");
  if (d->route != 0 && d->route != 1) return fail(KDLAE_EINVAL_CONFIG, "route must be 0 or 1");
  const long long HW = (long long)d->F * d->H * d->W;
  kdlae::GemmParams p{};
  p.A = d->A;
  p.lda = d->lda;
  p.cg_per_tap = d->cg_per_tap;
  p.kgroups = d->kgroups;
  p.ksize = d->ksize;
  p.dil = d->dil > 0 ? d->dil : 1;
  // the caller hands f32 fragment order (runtime.h pack_fragments); the GEMM kernels read split
  // fragment order (mfma3.h): convert into scratch owned by this call
  hipStream_t s = (hipStream_t)stream;
  const int nimg_w = d->w_img_stride ? d->Bn : 1;
  const long long w3_img = kdlae::split3_floats(d->ntiles, d->kgroups);
  float* w3 = nullptr;
  float* m3 = nullptr;
  struct Scratch {
    float** a;
    float** b;
    hipStream_t s;
    ~Scratch() {
      (void)hipStreamSynchronize(s);
      if (*a) (void)hipFree(*a);
      if (*b) (void)hipFree(*b);
    }
  } scratch{&w3, &m3, s};
  HIPCHK(hipMalloc(&w3, (size_t)(w3_img * nimg_w) * sizeof(float)));
  HIPCHK(kdlae::launch_split3(d->Wp, w3, d->ntiles, d->kgroups, nimg_w, d->w_img_stride, w3_img, s));
  p.Wp = w3;
  p.w_img_stride = d->w_img_stride ? w3_img : 0;
  p.ntiles = d->ntiles;
  p.N = d->N;
  p.bias = d->bias;
  p.out = d->out;
  p.ldo = d->ldo;
  p.R = d->R;
  p.ldr = d->ldr;
  p.ln = d->ln;
  p.ln_C = d->ln_C;
  p.relu = d->relu;
  p.Bn = d->Bn;
  p.H = d->H;
  p.W = d->W;
  p.F = d->F;
  p.kt = kt;
  p.out_mode = d->out_mode;
  p.tiles_per_img = (int)ceil_div(HW, kdlae::kGemmRows);
  p.total_tiles = d->Bn * p.tiles_per_img;
  p.kchunks = d->group_tiles ? 1 : (int)ceil_div(d->kgroups, d->KG);
  p.group_tiles = d->group_tiles;
  if (d->Wm) {  // the per-image folded projection: kgroups x kgroups tiles per image
    const long long m3_img = kdlae::split3_floats(d->kgroups, d->kgroups);
    HIPCHK(hipMalloc(&m3, (size_t)(m3_img * d->Bn) * sizeof(float)));
    HIPCHK(kdlae::launch_split3(d->Wm, m3, d->kgroups, d->kgroups, d->Bn, d->wm_img_stride, m3_img, s));
    p.Wm = m3;
    p.wm_img_stride = m3_img;
  }
  p.bias_m = d->bias_m;
  p.out1 = d->out1;
  p.ldo1 = d->ldo1;
  if (d->ln && !d->Wm && (p.kchunks > 1 || d->kgroups * 16 != d->ln_C)) {
    if (!d->stats || d->ln_C > 512 || d->lda % 4) return fail(KDLAE_EINVAL_CONFIG, "chunked LN needs stats scratch");
    HIPCHK(kdlae::launch_ln_stats(d->A, d->lda, d->ln_C, (long long)d->Bn * HW, d->stats, s));
    p.stats = d->stats;
  }
  const int gy = d->group_tiles ? (int)ceil_div(d->ntiles, d->group_tiles) : (int)ceil_div(d->ntiles, d->NT);
  p.tiles_per_block = d->tiles_per_block > 0 ? d->tiles_per_block
                                             : kdlae::gemm_tiles_per_block(p.total_tiles, gy, d->group_tiles != 0, d->wpe);
  const int gx = (int)ceil_div(p.total_tiles, p.tiles_per_block);
  const hipError_t e = kdlae::launch_gemm_route(p, d->NT, d->KG, d->wpe, gx, d->route, s);
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_gemm: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_gram(const kdlae_debug_gram_desc* d, void* stream) {
  if (!d || d->route < 0 || d->route > 3) return fail(KDLAE_EINVAL_CONFIG, "null descriptor or route not 0..3");
  const bool no_v = d->route == 3;  // the q | k ring: v_out is neither needed nor touched
  if (!d->qkv || !d->wdw || (!no_v && !d->v_out) || !d->partial || !d->reduced) return fail(KDLAE_EINVAL_CONFIG, "null operand");
  if (d->heads < 1 || d->C % d->heads || (d->C / d->heads) % 16 || d->C / d->heads > 128 || d->Bn < 1 || d->H < 1 ||
      d->W < 1 || d->ld < 3 * d->C || (!no_v && d->ldv < d->C))
    return fail(KDLAE_EINVAL_SHAPE, "bad Gram geometry (Ch = C / heads must be 16..128, a multiple of 16)");
  kdlae::GramParams p{};
  p.qkv = d->qkv;
  p.ld = d->ld;
  p.wdw = d->wdw;
  p.bdw = d->bdw;
  p.v_out = d->v_out;
  p.ldv = d->ldv;
  p.partial = d->partial;
  p.C = d->C;
  p.heads = d->heads;
  p.Ch = d->C / d->heads;
  p.Bn = d->Bn;
  p.H = d->H;
  p.W = d->W;
  p.nslots = kdlae::nslots_for(d->H, d->W);  // the engine's slot count
  p.slot_floats = kdlae::gram_slot_floats(p.Ch);
  p.zeros = (d->route == 0 || no_v) ? d->zeros : nullptr;
  p.no_v = no_v ? 1 : 0;
  if ((long long)d->Bn * d->heads * p.nslots * p.slot_floats > d->partial_floats)
    return fail(KDLAE_EINVAL_SHAPE, "partial scratch too small");
  if (no_v && !kdlae::gram_ring_applies(p))
    return fail(KDLAE_EINVAL_SHAPE, "route 3 (no v) needs the ring kernel: zeros, W % 16 == 0, ld % 4 == 0, Ch <= 96");
  hipStream_t s = (hipStream_t)stream;
  HIPCHK(kdlae::launch_dwconv_gram_route(p, no_v ? 0 : d->route, s));
  HIPCHK(kdlae::launch_gram_reduce(p.partial, d->reduced, d->Bn, d->heads, p.nslots, p.slot_floats, s));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_ln(const kdlae_debug_ln_desc* d, void* stream) {
  if (!d || d->C < 1 || d->C > 512 || d->P < 1) return fail(KDLAE_EINVAL_SHAPE, "bad LayerNorm geometry");
  hipStream_t s = (hipStream_t)stream;
  const bool generic = d->route == 1;
  hipError_t e;
  if (d->dir == 0) {
    if (!d->x || !d->w || !d->y || !d->stats) return fail(KDLAE_EINVAL_CONFIG, "null operand");
    e = tr::launch_ln_fwd(d->x, d->ldx, d->w, d->b, d->C, d->P, d->biasfree, d->y, d->ldy, d->stats, s, generic);
  } else {
    if (!d->x || !d->w || !d->dy || !d->dx || !d->stats || !d->part || d->nblk < 1)
      return fail(KDLAE_EINVAL_CONFIG, "null operand");
    e = tr::launch_ln_bwd(d->dy, d->ldd, d->x, d->ldx, d->w, d->stats, d->C, d->P, d->biasfree, d->R, d->ldr, d->dx,
                          d->lddx, d->part, d->nblk, s, generic);
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_ln: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_small_in(const kdlae_debug_small_in_desc* d, void* stream) {
  if (!d || !d->in || !d->w || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
  if (d->Bn < 1 || d->H < 1 || d->W < 1 || d->Cin < 1 || d->Cout < 16 || d->ldo < d->Cout)
    return fail(KDLAE_EINVAL_SHAPE, "bad small-input conv geometry");
  if ((d->kt != 1 && d->kt != 3) || d->Cin * 9 * d->kt > 36 || d->Cout % 16)
    return fail(KDLAE_EINVAL_SHAPE, "small-input conv: kt 1 or 3, Cin * 9 * kt <= 36, Cout % 16 == 0");
  if (d->ldo % 4 || !kdlae::al16(d->out)) return fail(KDLAE_EINVAL_SHAPE, "small-input conv: out 16-byte aligned, ldo % 4 == 0");
  if (d->wt < 0 || (d->wt && (d->kt != 1 || d->wt < d->Cout)))
    return fail(KDLAE_EINVAL_SHAPE, "small-input conv: wt needs kt 1 and wt >= Cout");
  kdlae::SmallInParams p{};
  p.in = d->in;
  p.sb = d->sb;
  p.sc = d->sc;
  p.sy = d->sy;
  p.sx = d->sx;
  p.st = d->st;
  p.in_sub = d->in_sub;
  p.Cin = d->Cin;
  p.Cout = d->Cout;
  p.dil = d->dil > 0 ? d->dil : 1;
  p.kt = d->kt;
  p.F = d->F > 0 ? d->F : 1;
  p.w = d->w;
  p.bias = d->bias;
  p.out = d->out;
  p.ldo = d->ldo;
  p.Bn = d->Bn;
  p.H = d->H;
  p.W = d->W;
  p.vh = d->vh;
  p.vw = d->vw;
  p.relu = d->relu;
  p.wt = d->wt;
  const hipError_t e = kdlae::launch_conv_small_in(p, (hipStream_t)stream);
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_small_in: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_bn(const kdlae_debug_bn_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  hipStream_t s = (hipStream_t)stream;
  hipError_t e;
  const bool need_part = d->op == 0 || d->op == 2;
  if (need_part && (!d->part || d->part_floats < tr::bn_part_floats(d->C)))
    return fail(KDLAE_EINVAL_CONFIG, "part must hold 2048 C floats");
  switch (d->op) {
    case 0:
      e = tr::launch_bn_stats(d->x, d->ldx, d->C, d->P, d->mean, d->rstd, d->running_mean, d->running_var, d->momentum,
                              d->part, s);
      break;
    case 1:
      e = tr::launch_bn_apply_relu(d->x, d->ldx, d->mean, d->rstd, d->gamma, d->beta, d->C, d->P, d->out, d->ldo, s);
      break;
    case 2:
      e = tr::launch_bn_bwd_reduce(d->dy, d->ldd, d->y, d->ldy, d->x, d->ldx, d->mean, d->rstd, d->C, d->P, d->dgamma,
                                   d->dbeta, d->part, s);
      break;
    case 3:
      e = tr::launch_bn_bwd_dx(d->dy, d->ldd, d->y, d->ldy, d->x, d->ldx, d->mean, d->rstd, d->gamma, d->dgamma,
                               d->dbeta, d->C, d->P, d->out, d->ldo, s);
      break;
    case 4: e = tr::launch_upsample2x_bwd(d->x, d->ldx, d->out, d->ldo, d->C, d->N, d->h, d->w, s); break;
    case 5:
      if (!d->x || !d->out || d->N < 1 || d->h < 1 || d->w < 1 || d->ldx < d->C || d->ldo < d->C)
        return fail(KDLAE_EINVAL_SHAPE, "bad upsample geometry");
      if (d->C < 4 || d->C % 4 || d->ldx % 4 || d->ldo % 4 || !kdlae::al16(d->x) || !kdlae::al16(d->out))
        return fail(KDLAE_EINVAL_SHAPE, "upsample2x: C >= 4, C % 4 == 0, ldx, ldo % 4 == 0, 16-byte aligned views");
      e = kdlae::launch_upsample2x(d->x, d->ldx, d->out, d->ldo, d->C, d->N, d->h, d->w, s);
      break;
    case 6:  // x = lq, y = gt [N][C = ci][h][w] -> out = xin [N Hp Wp][12]
      if (!d->x || !d->y || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->C < 1 || d->C > 4 || d->N < 1 || d->h < 1 || d->w < 1 || d->Hp < d->h || d->Wp < d->w ||
          (long long)d->N * d->Hp * d->Wp * 12 >= (1LL << 31) || !kdlae::al16(d->out))
        return fail(KDLAE_EINVAL_SHAPE, "asdqe_pack_inputs: ci 1..4, Hp >= h, Wp >= w, out 16-byte aligned");
      e = tr::launch_asdqe_pack_inputs(d->x, d->y, d->C, d->N, d->h, d->w, d->Hp, d->Wp, d->out, s);
      break;
    case 7:  // x = src [N = Cout][4][9] -> out = dst [N][C = ci][9]
      if (!d->x || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->C < 1 || d->C > 4 || d->N < 1 || d->N > (1 << 20)) return fail(KDLAE_EINVAL_SHAPE, "narrow_w_copy: ci 1..4, Cout >= 1");
      e = tr::launch_narrow_w_copy(d->x, d->out, d->N, d->C, s);
      break;
    case 8:  // x = v rows at stride ldx, N images of P pixels -> out [N P][ldo]
      if (!d->x || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->C < 4 || d->C % 4 || d->C > 1024 || d->N < 1 || d->P < 1 || d->ldx < d->C || d->ldx % 4 || d->ldo < d->C ||
          d->ldo % 4 || !kdlae::al16(d->x) || !kdlae::al16(d->out) || (long long)d->N * d->P * d->ldo >= (1LL << 31))
        return fail(KDLAE_EINVAL_SHAPE, "bcast_rows: C % 4 == 0, C <= 1024, ldx, ldo >= C and % 4 == 0, 16-byte aligned views");
      e = tr::launch_bcast_rows(d->x, d->ldx, d->C, d->N, d->P, d->scale, d->out, d->ldo, s);
      break;
    case 9:  // x = g [P], out = grad [P]
      if (!d->x || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->P < 4 || d->P % 4 || !kdlae::al16(d->x) || !kdlae::al16(d->out))
        return fail(KDLAE_EINVAL_SHAPE, "grad_commit: n >= 4, n % 4 == 0, 16-byte aligned operands");
      e = tr::launch_grad_commit(d->x, d->out, d->P, d->accumulate ? 1 : 0, s);
      break;
    default: return fail(KDLAE_EINVAL_CONFIG, "op must be 0..9");
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_bn: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_head_train(const kdlae_debug_head_train_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  if (d->dir != 0 && d->dir != 1) return fail(KDLAE_EINVAL_CONFIG, "dir must be 0 or 1");
  if (!d->wo || !d->bo || !d->w1 || !d->b1 || !d->w2 || !d->b2 || !d->w3 || !d->b3 || !d->save)
    return fail(KDLAE_EINVAL_CONFIG, "null operand");
  auto dim_ok = [](int n) { return n >= 1 && n <= 1024; };
  if (d->B < 1 || d->B > 65535 || !dim_ok(d->C) || !dim_ok(d->M) || !dim_ok(d->N1) || !dim_ok(d->N2))
    return fail(KDLAE_EINVAL_SHAPE, "head: B >= 1, C, M, N1, N2 in 1..1024");
  if (d->save_floats < (long long)d->B * tr::head_save_floats(d->C, d->M, d->N1, d->N2))
    return fail(KDLAE_EINVAL_SHAPE, "save must hold B * head_save_floats floats");
  tr::HeadTrain p{};
  p.partial = d->partial; p.slots = d->slots; p.C = d->C; p.inv_hw = d->inv_hw;
  p.wo = d->wo; p.bo = d->bo; p.M = d->M;
  p.w1 = d->w1; p.b1 = d->b1; p.N1 = d->N1;
  p.w2 = d->w2; p.b2 = d->b2; p.N2 = d->N2;
  p.w3 = d->w3; p.b3 = d->b3;
  p.mask1 = d->mask1; p.mask2 = d->mask2;
  p.score = d->score; p.B = d->B; p.save = d->save;
  hipError_t e;
  if (d->dir == 0) {
    if (!d->partial || !d->score) return fail(KDLAE_EINVAL_CONFIG, "null operand");
    if (d->slots < 1 || d->slots > 65535) return fail(KDLAE_EINVAL_SHAPE, "head: slots >= 1");
    e = tr::launch_head_train_fwd(p, (hipStream_t)stream);
  } else {
    if (!d->dscore || !d->gwo || !d->gbo || !d->gw1 || !d->gb1 || !d->gw2 || !d->gb2 || !d->gw3 || !d->gb3)
      return fail(KDLAE_EINVAL_CONFIG, "null operand");
    const tr::HeadTrainGrads g{d->gwo, d->gbo, d->gw1, d->gb1, d->gw2, d->gb2, d->gw3, d->gb3};
    e = tr::launch_head_train_bwd(p, d->dscore, g, (hipStream_t)stream);
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_head_train: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

// ---- non-GEMM training kernels (kdlae_debug_train / kdlae_debug_train_s): argument checks first,
// so that a wrong test argument is an error code and never a device fault
namespace {

constexpr long long kMaxIdx = 1LL << 31;  // the kernels' 32-bit index math; far above any self-test shape
using kdlae::al16;
// a [pixels][ld] view of `width` used columns
inline bool view_ok(const void* p, int ld, int width, long long pixels) {
  return p && width >= 1 && ld >= width && pixels >= 1 && pixels * ld < kMaxIdx;
}

}  // namespace

extern "C" int kdlae_debug_train_blocks(int which, int64_t n, int a, int b, int64_t cap) {
  if (which == 0) {
    if (n < 1 || a < 1 || b < 1 || n * a * b >= kMaxIdx) return -1;
    return tr::dwg_blocks((int)n, a, b);
  }
  if (which == 1) {
    if (n < 1 || n >= kMaxIdx || !tr::dw3_small_ok(a, b) || cap < (int64_t)a * b * 9) return -1;
    return tr::dw3_small_blocks(n, a, b, (size_t)cap);
  }
  return -1;
}

extern "C" int kdlae_debug_train(const kdlae_debug_train_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  hipStream_t s = (hipStream_t)stream;
  const int C = d->C;
  const bool geo = d->Bn >= 1 && d->H >= 1 && d->W >= 1 && (long long)d->Bn * d->H * d->W < kMaxIdx;
  const long long px = geo ? (long long)d->Bn * d->H * d->W : 0;
  auto in_ok = [&](int i, int width, long long pixels) { return view_ok(d->in[i], d->ldi[i], width, pixels); };
  auto out_ok = [&](int i, int width, long long pixels) { return view_ok(d->out[i], d->ldo[i], width, pixels); };
  // the buffer-descriptor kernels address one image with 32-bit byte offsets below their sentinel
  auto img_ok = [&](int ld) { return (long long)d->H * d->W * ld * 4 < (1LL << 30); };
  const char* bad = "bad geometry";
  hipError_t e = hipSuccess;
  switch (d->op) {
    case 0:
    case 1: {
      if (d->heads < 1 || C < 1 || C % d->heads || C / d->heads > 128 || d->Bn < 1 || d->Bn > 65535 / d->heads)
        return fail(KDLAE_EINVAL_SHAPE, "attention: C = heads * Ch with Ch <= 128");
      const int Ch = C / d->heads;
      if (!d->in[0] || !d->in[1] || !d->w || !d->out[0]) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->op == 0) {
        e = tr::launch_attn_softmax(d->in[0], d->in[1], d->w, d->Bn, C, d->heads, d->out[0], s);
        break;
      }
      if (!d->in[2] || !d->in[3] || !d->out[1] || !d->out[2] || !d->out[3])
        return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (((size_t)Ch * Ch + 4) * sizeof(float) > 65536)
        return fail(KDLAE_EINVAL_SHAPE, "attention backward: the Ch x Ch tile must fit 64 KiB of LDS");
      e = tr::launch_attn_bwd(d->in[0], d->in[1], d->w, d->in[2], d->in[3], d->Bn, C, d->heads, d->out[0], d->out[1],
                              d->out[2], d->out[3], s);
      break;
    }
    case 2: {
      if (!geo || !d->w || !in_ok(0, C, px) || !out_ok(0, C, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
      // the tile kernel (both strides % 4 == 0) moves float4 quads
      if (d->ldi[0] % 4 == 0 && d->ldo[0] % 4 == 0 && d->ldi[0] >= (C + 3) / 4 * 4 && (!al16(d->in[0]) || !al16(d->out[0])))
        return fail(KDLAE_EINVAL_SHAPE, "dw_fwd: views with ld % 4 == 0 must be 16-byte aligned");
      e = tr::launch_dw_fwd(d->in[0], d->ldi[0], d->w, d->bias, d->flag ? 1 : 0, C, d->Bn, d->H, d->W, d->out[0],
                            d->ldo[0], s);
      break;
    }
    case 3: {
      if (!geo || !d->w || C > (1 << 20) || !in_ok(0, 2 * C, px) || !out_ok(0, C, px) || (d->out[1] && !out_ok(1, 2 * C, px)) ||
          !img_ok(std::max(d->ldi[0], std::max(d->ldo[0], d->out[1] ? d->ldo[1] : 0))))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_dwgate_fwd(d->in[0], d->ldi[0], d->w, d->bias, C, d->Bn, d->H, d->W, d->out[1],
                                d->out[1] ? d->ldo[1] : 0,
                                d->out[0], d->ldo[0], s);
      break;
    }
    case 4:
    case 5:
    case 6:
    case 16:    // ops 16-18: ops 4-6 with the weight gradient left out (the dx-only kernels); part is ignored
    case 17:
    case 18: {
      if (!geo || !d->w || C < 1 || C > (1 << 20)) return fail(KDLAE_EINVAL_SHAPE, bad);
      const bool dx_only = d->op >= 16;
      const int op = dx_only ? d->op - 12 : d->op;
      const int Ct = op == 6 ? C : 2 * C;  // channels of y / dy (and of the partial rows)
      const int nin = op == 4 ? 3 : (op == 6 && dx_only) ? 1 : 2;  // op 18 does not read in1
      // in0: dg (C) or dyd (Ct); the rest: yd / y (Ct)
      int ldmax = d->ldo[0];
      for (int i = 0; i < nin; ++i) {
        if (!in_ok(i, (i == 0 && op != 6) ? C : Ct, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
        ldmax = std::max(ldmax, d->ldi[i]);
      }
      if (!out_ok(0, Ct, px) || !img_ok(ldmax)) return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!dx_only && (!d->part || d->part_floats < (long long)tr::dwg_blocks(d->Bn, d->H, d->W) * 10 * Ct))
        return fail(KDLAE_EINVAL_SHAPE, "part must hold blocks * 10 * channels floats");
      float* part = dx_only ? nullptr : d->part;  // a null part selects the dx-only kernel
      if (op == 4)
        e = tr::launch_dwgate_bwd(d->in[0], d->ldi[0], d->in[1], d->ldi[1], d->in[2], d->ldi[2], d->w, C, d->Bn, d->H,
                                  d->W, d->out[0], d->ldo[0], part, s);
      else if (op == 5)
        e = tr::launch_dwgate_bwd_rc(d->in[0], d->ldi[0], d->in[1], d->ldi[1], d->w, d->bias, C, d->Bn, d->H, d->W,
                                     d->out[0], d->ldo[0], part, s);
      else
        e = tr::launch_dw_bwd(d->in[0], d->ldi[0], dx_only ? nullptr : d->in[1], dx_only ? 0 : d->ldi[1], d->w, C, d->Bn,
                              d->H, d->W, d->out[0], d->ldo[0], part, s);
      break;
    }
    case 7: {
      if (!tr::dw3_small_ok(C, d->C2)) return fail(KDLAE_EINVAL_SHAPE, "dw3_small: Cout == 3 or Cin in {3, 4}, wide side <= 256");
      if (!geo || !in_ok(0, d->C2, px) || !in_ok(1, C, px) || d->flag < 1 || d->flag > 64 || d->nblk < 1 || d->nblk > 65535)
        return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!d->part || d->part_floats < (long long)d->nblk * C * d->C2 * 9)
        return fail(KDLAE_EINVAL_SHAPE, "part must hold nblk * Cout * Cin * 9 floats");
      e = tr::launch_dw3_small(d->in[0], d->ldi[0], d->in[1], d->ldi[1], C, d->C2, d->Bn, d->H, d->W, d->flag, d->part,
                               d->nblk, s);
      break;
    }
    case 8: {
      if (d->nseg < 1 || d->nseg > 65535 || d->nblk < 1 || d->nblk > 65535 || d->P < 1 || d->P >= kMaxIdx ||
          !in_ok(0, C, d->P * d->nseg))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!d->part || d->part_floats < (long long)d->nseg * d->nblk * C)
        return fail(KDLAE_EINVAL_SHAPE, "part must hold nseg * nblk * ncols floats");
      e = tr::launch_colsum(d->in[0], d->ldi[0], C, d->P, d->nseg, d->flag ? 1 : 0, d->part, d->nblk, s);
      break;
    }
    case 9: {
      if (!d->in[0] || !d->out[0]) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if (d->nseg < 1 || d->nseg > 65535 || d->nblk < 1 || C < 1 || (d->pstride != 0 && d->pstride < C) ||
          (long long)d->nseg * d->nblk * std::max(d->pstride, C) >= kMaxIdx)
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_part_reduce(d->in[0], d->nblk, C, d->nseg, d->out[0], d->accumulate ? 1 : 0, d->scale, s,
                                 d->pstride);
      break;
    }
    case 10: {
      if (d->nred < 1 || d->nred > tr::kRedBatch) return fail(KDLAE_EINVAL_SHAPE, "nred must be 1..8");
      tr::RedDesc r[tr::kRedBatch];
      for (int j = 0; j < d->nred; ++j) {
        const kdlae_debug_train_red& q = d->red[j];
        if (!q.part || !q.out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
        if (q.nblk < 1 || q.ncols < 1 || q.pstride < q.ncols || (long long)q.nblk * q.pstride >= kMaxIdx)
          return fail(KDLAE_EINVAL_SHAPE, bad);
        r[j].part = q.part; r[j].out = q.out; r[j].nblk = q.nblk; r[j].ncols = q.ncols; r[j].pstride = q.pstride;
        r[j].scale = q.scale;
      }
      e = tr::launch_part_reduce_multi(r, d->nred, s);
      break;
    }
    case 11: {
      if (!geo || C < 1 || C > (1 << 20) || (d->flag != 0 && d->flag != 1)) return fail(KDLAE_EINVAL_SHAPE, bad);
      const bool un = d->flag == 0;  // H, W: the low-resolution grid
      if (!in_ok(0, un ? C : 4 * C, un ? 4 * px : px) || !out_ok(0, un ? 4 * C : C, un ? px : 4 * px))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_shuffle(d->in[0], d->ldi[0], d->out[0], d->ldo[0], C, d->Bn, d->H, d->W, d->flag, s);
      break;
    }
    case 12: {
      if (d->P < 1 || d->P >= kMaxIdx || d->zero_to < 0 || !in_ok(0, C, d->P) || !out_ok(0, std::max(C, d->zero_to), d->P))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_copy_cols(d->in[0], d->ldi[0], d->out[0], d->ldo[0], C, d->P, d->accumulate ? 1 : 0, s, d->zero_to);
      break;
    }
    case 13:
    case 14: {
      if (d->Bn < 1 || d->P < 1 || C < 1 || (long long)d->Bn * d->P >= kMaxIdx || !d->in[0] || !d->out[0])
        return fail(KDLAE_EINVAL_SHAPE, bad);
      const long long pixels = (long long)d->Bn * d->P;
      if (pixels * C >= kMaxIdx) return fail(KDLAE_EINVAL_SHAPE, bad);
      if (d->op == 13) {
        if (!out_ok(0, C, pixels)) return fail(KDLAE_EINVAL_SHAPE, bad);
        e = tr::launch_nchw_to_nhwc(d->in[0], C, d->Bn, d->P, d->out[0], d->ldo[0], d->accumulate ? 1 : 0, s);
      } else {
        if (!in_ok(0, C, pixels)) return fail(KDLAE_EINVAL_SHAPE, bad);
        e = tr::launch_nhwc_to_nchw(d->in[0], d->ldi[0], d->in[1], C, d->Bn, d->P, d->out[0], s);
      }
      break;
    }
    case 15: {
      if (!d->w || !d->out[0]) return fail(KDLAE_EINVAL_CONFIG, "null operand");
      if ((d->flag != 2 && d->flag != 3) || C < 1 || d->C2 < 1 || 9LL * C * d->C2 >= kMaxIdx)
        return fail(KDLAE_EINVAL_SHAPE, "pack_w3: mode 2 or 3, Cg, N >= 1");
      e = tr::launch_pack_w3(d->w, C, d->C2, d->flag, d->out[0], s);
      break;
    }
    case 19: {  // LayerNorm backward, dx only: in0 = dy, in1 = x, in2 = stats [P][2], in3 = R (or null), w
      if (C < 1 || C > 512 || d->P < 1 || d->P >= kMaxIdx || !d->w || !d->in[2] || !in_ok(0, C, d->P) ||
          !in_ok(1, C, d->P) || (d->in[3] && !in_ok(3, C, d->P)) || !out_ok(0, C, d->P))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      const int nblk = d->nblk >= 1 ? d->nblk : 1;
      e = tr::launch_ln_bwd(d->in[0], d->ldi[0], d->in[1], d->ldi[1], d->w, d->in[2], C, d->P, d->flag & 1, d->in[3],
                            d->in[3] ? d->ldi[3] : 0, d->out[0], d->ldo[0], nullptr, nblk, s, (d->flag & 2) != 0);
      break;
    }
    default: return fail(KDLAE_EINVAL_CONFIG, "op must be 0..19");
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_train: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

extern "C" int kdlae_debug_train_s(const kdlae_debug_train_s_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  hipStream_t s = (hipStream_t)stream;
  const int C = d->C;
  const char* bad = "bad geometry";
  if (d->op == 2) {
    if (!d->in[0] || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
    if (d->O < 1 || C < 1 || 27LL * d->O * C >= kMaxIdx || (d->dir != 0 && d->dir != 1)) return fail(KDLAE_EINVAL_SHAPE, bad);
    const hipError_t e = tr::launch_wperm(d->in[0], d->out, d->O, C, d->dir, s);
    if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_train_s: ") + hipGetErrorString(e));
    return KDLAE_OK;
  }
  if (d->op == 6) {  // in0 = w [O = cout][C = cin][27], dir = dx -> out: ceil(nout / 16) * 27 in_pad / 16 * 256 floats
    if (!d->in[0] || !d->out) return fail(KDLAE_EINVAL_CONFIG, "null operand");
    if (d->O < 1 || d->O > 4096 || C < 1 || C > 4096 || (d->dir != 0 && d->dir != 1)) return fail(KDLAE_EINVAL_SHAPE, bad);
    const hipError_t e = tr::launch_pack_conv(d->in[0], d->O, C, d->dir, d->out, s);
    if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_train_s: ") + hipGetErrorString(e));
    return KDLAE_OK;
  }
  if (d->B < 1 || d->F < 1 || d->H < 1 || d->W < 1 || C < 1 || C > (1 << 16) ||
      (long long)d->B * d->F * d->H * d->W * 27 * C >= kMaxIdx)
    return fail(KDLAE_EINVAL_SHAPE, bad);
  const long long px = (long long)d->B * d->F * d->H * d->W;
  auto in_ok = [&](int i, int width, long long pixels) { return view_ok(d->in[i], d->ldi[i], width, pixels); };
  hipError_t e = hipSuccess;
  switch (d->op) {
    case 0:
      if (!in_ok(0, C, px) || !d->out) return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_im2col3d(d->in[0], d->ldi[0], C, d->B, d->F, d->H, d->W, d->out, s);
      break;
    case 1:
      if (!d->in[0] || !view_ok(d->out, d->ldo, C, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
      if (C % 4 || d->ldo % 4 || !al16(d->out) || !al16(d->in[0]))
        return fail(KDLAE_EINVAL_SHAPE, "col2im3d: C % 4 == 0, ld % 4 == 0 and 16-byte aligned operands");
      e = tr::launch_col2im3d(d->in[0], C, d->B, d->F, d->H, d->W, d->out, d->ldo, d->accumulate ? 1 : 0, s);
      break;
    case 3:
      if (!in_ok(0, C, px) || !view_ok(d->out, d->ldo, C, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_relu_mask(d->out, d->ldo, d->in[0], d->ldi[0], C, px, s);
      break;
    case 4:  // H, W: the pooled grid
      if (!in_ok(0, C, 4 * px) || !in_ok(1, C, px) || (d->in[2] && !in_ok(2, C, 4 * px)) || !view_ok(d->out, d->ldo, C, 4 * px))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_maxpool2_bwd(d->in[0], d->ldi[0], d->in[1], d->ldi[1], d->in[2], d->ldi[2], d->out, d->ldo, C, d->B,
                                  d->F, d->H, d->W, s);
      break;
    case 5:  // H, W: the output grid
      if (d->H % 2 || d->W % 2 || !in_ok(0, 4 * C, px / 4) || !in_ok(1, C, px) || !view_ok(d->out, d->ldo, C, px))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_upshuffle_add(d->in[0], d->ldi[0], d->bias, d->in[1], d->ldi[1], d->out, d->ldo, C, d->B, d->F, d->H,
                                   d->W, s);
      break;
    case 7:  // in place on out
      if (!view_ok(d->out, d->ldo, C, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
      e = tr::launch_relu(d->out, d->ldo, C, px, s);
      break;
    default: return fail(KDLAE_EINVAL_CONFIG, "op must be 0..7");
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_train_s: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

// ---- inference kernels outside the GEMM / Gram families (kdlae_debug_infer): every launcher
// precondition is checked here, so a wrong test argument is an error code and never a device fault
namespace {

// the per-image buffer-descriptor kernels (gdfn, ffn, mdta_fused) address one image with 32-bit byte offsets
inline bool img_bytes_ok(int H, int W, int ld) { return (long long)H * W * ld * 4 < (1LL << 31); }

// device scratch owned by one self-test call: released after the stream has drained
struct SplitScratch {
  float* p[3] = {nullptr, nullptr, nullptr};
  hipStream_t s;
  explicit SplitScratch(hipStream_t st) : s(st) {}
  ~SplitScratch() {
    (void)hipStreamSynchronize(s);
    for (float* q : p)
      if (q) (void)hipFree(q);
  }
  // split records of the f32 fragment block src [ntiles][kgroups][64][4]
  hipError_t split(int i, const float* src, int ntiles, int kgroups) {
    const long long n = kdlae::split3_floats(ntiles, kgroups);
    hipError_t e = hipMalloc(&p[i], (size_t)n * sizeof(float));
    if (e != hipSuccess) return e;
    return kdlae::launch_split3(src, p[i], ntiles, kgroups, 1, 0, n, s);
  }
};

}  // namespace

extern "C" int kdlae_debug_infer(const kdlae_debug_infer_desc* d, void* stream) {
  if (!d) return fail(KDLAE_EINVAL_CONFIG, "null descriptor");
  hipStream_t s = (hipStream_t)stream;
  const int C = d->C;
  const int F = d->F > 0 ? d->F : 1;
  const bool geo = d->Bn >= 1 && d->H >= 1 && d->W >= 1 && d->F >= 0 && (long long)d->Bn * F * d->H * d->W < kMaxIdx;
  const long long px = geo ? (long long)d->Bn * F * d->H * d->W : 0;
  auto in_ok = [&](int i, int width, long long pixels) { return view_ok(d->in[i], d->ldi[i], width, pixels); };
  auto out_ok = [&](int i, int width, long long pixels) { return view_ok(d->out[i], d->ldo[i], width, pixels); };
  // float4 access: 16-byte aligned base, pixel stride a multiple of 4
  auto in4 = [&](int i) { return al16(d->in[i]) && d->ldi[i] % 4 == 0; };
  auto out4 = [&](int i) { return al16(d->out[i]) && d->ldo[i] % 4 == 0; };
  const char* bad = "bad geometry";
  const char* null_op = "null operand";
  const char* align = "float4 views: 16-byte aligned, ld % 4 == 0";
  SplitScratch sc(s);
  hipError_t e = hipSuccess;
  switch (d->op) {
    case 0: {  // fused GDFN tail
      if (!d->w[0] || !d->w[1] || !d->zeros) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!kdlae::gdfn_supported(C, d->hidS)) return fail(KDLAE_EINVAL_SHAPE, "gdfn: C in {48, 96, 192, 384}, hidS % 16 == 0, hidS <= 256 (C <= 96) / 1024");
      if (!geo || F != 1 || d->ldi[0] != 2 * d->hidS || !in_ok(0, 2 * d->hidS, px) || !out_ok(0, C, px) ||
          (d->R && (d->ldr < C || px * d->ldr >= kMaxIdx)) || !img_bytes_ok(d->H, d->W, d->ldi[0]))
        return fail(KDLAE_EINVAL_SHAPE, "gdfn: x is [P][2 hidS] exactly, out / R at least C wide");
      if (!in4(0) || !out4(0) || !al16(d->w[0]) || !al16(d->bias[0]) || (d->R && (!al16(d->R) || d->ldr % 4)))
        return fail(KDLAE_EINVAL_SHAPE, align);
      HIPCHK(sc.split(0, d->w[1], C / 16, d->hidS / 16));
      kdlae::GdfnParams p{};
      p.x = d->in[0]; p.ld = d->ldi[0]; p.hidS = d->hidS; p.dw = d->w[0]; p.Wp = sc.p[0]; p.bias = d->bias[0];
      p.R = d->R; p.ldr = d->ldr; p.out = d->out[0]; p.ldo = d->ldo[0];
      p.Bn = d->Bn; p.H = d->H; p.W = d->W; p.zeros = d->zeros;
      p.split = d->out_mode != 0;
      e = kdlae::launch_gdfn_out(p, C, s);
      break;
    }
    case 1: {  // fused feed-forward half
      if (!d->w[0] || !d->w[1] || !d->w[2]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (d->ln != 1 && d->ln != 2) return fail(KDLAE_EINVAL_CONFIG, "ln must be 1 or 2");
      if (!kdlae::ffn_fused_supported(C, d->hidS)) return fail(KDLAE_EINVAL_SHAPE, "ffn: C in {48, 96}, hidS / 16 even, 2 .. 8 (C = 48) / 16");
      if (!geo || F != 1 || !in_ok(0, C, px) || !out_ok(0, C, px) ||
          !img_bytes_ok(d->H, d->W, std::max(d->ldi[0], d->ldo[0])))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!in4(0) || !out4(0) || !al16(d->w[1]) || !al16(d->bias[0]) || !al16(d->bias[1])) return fail(KDLAE_EINVAL_SHAPE, align);
      {  // neighbouring tiles read x as halo: out must not overlap it
        const uintptr_t x0 = (uintptr_t)d->in[0], x1 = x0 + (size_t)px * d->ldi[0] * 4;
        const uintptr_t o0 = (uintptr_t)d->out[0], o1 = o0 + (size_t)px * d->ldo[0] * 4;
        if (x0 < o1 && o0 < x1) return fail(KDLAE_EINVAL_SHAPE, "ffn: out must not overlap x");
      }
      HIPCHK(sc.split(0, d->w[0], 2 * d->hidS / 16, C / 16));
      HIPCHK(sc.split(1, d->w[2], C / 16, d->hidS / 16));
      kdlae::FfnParams p{};
      p.x = d->in[0]; p.ldx = d->ldi[0]; p.out = d->out[0]; p.ldo = d->ldo[0]; p.ln = d->ln; p.hidS = d->hidS;
      p.Win = sc.p[0]; p.bias_in = d->bias[0]; p.dw = d->w[1]; p.Wout = sc.p[1]; p.bias_out = d->bias[1];
      p.Bn = d->Bn; p.H = d->H; p.W = d->W;
      e = kdlae::launch_ffn_fused(p, C, s);
      break;
    }
    case 2: {  // fused MDTA pass 1 + slot reduction
      if (!d->w[0] || !d->w[1] || !d->scratch || !d->out[1]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (d->ln != 1 && d->ln != 2) return fail(KDLAE_EINVAL_CONFIG, "ln must be 1 or 2");
      if (!geo || F != 1 || !kdlae::mdta_fused_supported(C, 1, d->H, d->W, d->nseg, d->seg_rows) ||
          (long long)d->seg_rows * (d->nseg - 1) >= d->H)
        return fail(KDLAE_EINVAL_SHAPE, "mdta_fused: C in {48, 96}, W % 16 == 0, H % 8 == 0, seg_rows % 8 == 0, nseg segments that cover H, none empty");
      if (!in_ok(0, C, px) || !out_ok(0, C, px) || !img_bytes_ok(d->H, d->W, std::max(d->ldi[0], d->ldo[0])))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!in4(0) || !out4(0) || !al16(d->w[1]) || !al16(d->bias[0]) || !al16(d->bias[1]) || !al16(d->scratch))
        return fail(KDLAE_EINVAL_SHAPE, align);
      const int nslots = (d->W / 16) * d->nseg, slot_floats = kdlae::gram_slot_floats(C);
      if ((long long)d->Bn * nslots * slot_floats > d->scratch_floats)
        return fail(KDLAE_EINVAL_SHAPE, "scratch must hold Bn * nslots * slot_floats floats");
      HIPCHK(sc.split(0, d->w[0], 3 * C / 16, C / 16));
      kdlae::MdtaFusedParams p{};
      p.x = d->in[0]; p.ldx = d->ldi[0]; p.ln = d->ln; p.Wqkv = sc.p[0]; p.bias = d->bias[0];
      p.wdw = d->w[1]; p.bdw = d->bias[1]; p.v_out = d->out[0]; p.ldv = d->ldo[0]; p.partial = d->scratch;
      p.nslots = nslots; p.slot_floats = slot_floats; p.nseg = d->nseg; p.seg_rows = d->seg_rows;
      p.Bn = d->Bn; p.H = d->H; p.W = d->W;
      e = kdlae::launch_mdta_fused(p, C, s);
      if (e == hipSuccess) e = kdlae::launch_gram_reduce(d->scratch, d->out[1], d->Bn, 1, nslots, slot_floats, s);
      break;
    }
    case 3: {  // softmax + fold
      if (!d->in[0] || !d->w[0] || !d->w[1] || !d->out[0]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (d->heads < 1 || C < 16 || C % 16 || C % d->heads || (C / d->heads) % 16 || C / d->heads > 128 || d->Bn < 1 ||
          d->Bn > 65535 || d->heads > 65535)
        return fail(KDLAE_EINVAL_SHAPE, "attn_fold: C = heads * Ch, Ch a multiple of 16, 16 .. 128");
      e = kdlae::launch_attn_fold(d->in[0], kdlae::gram_slot_floats(C / d->heads), d->w[0], d->w[1], d->out[0], d->Bn, C, d->heads, s);
      break;
    }
    case 4: {  // GDFN dwconv + gate
      if (!d->w[0]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!geo || F != 1 || d->hidS < 4 || d->hidS % 4 || d->hidS > (1 << 16) || !in_ok(0, 2 * d->hidS, px) ||
          !out_ok(0, d->hidS, px))
        return fail(KDLAE_EINVAL_SHAPE, "dwconv_gate: hidS % 4 == 0, x at least 2 hidS wide, out at least hidS");
      if (!in4(0) || !out4(0) || !al16(d->w[0]) || !al16(d->bias[0])) return fail(KDLAE_EINVAL_SHAPE, align);
      kdlae::GateParams p{};
      p.x = d->in[0]; p.ld = d->ldi[0]; p.hidS = d->hidS; p.w = d->w[0]; p.b = d->bias[0];
      p.out = d->out[0]; p.ldo = d->ldo[0]; p.Bn = d->Bn; p.H = d->H; p.W = d->W;
      e = kdlae::launch_dwconv_gate(p, s);
      break;
    }
    case 5: {  // LDS-tiled implicit-GEMM conv
      if (!d->w[0] || (d->use_wp3 && d->kt == 3 && !d->w[1])) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!kdlae::conv_lds_supported(d->kt, d->ntiles, d->cin_pad) || d->cin_pad > 1024)
        return fail(KDLAE_EINVAL_SHAPE, "conv_lds: kt 1 or 3, 2 .. 16 output tiles, cin_pad % 16 == 0");
      if (!geo || (d->kt == 1 && F != 1) || d->out_mode < 0 || d->out_mode > 2 || !in_ok(0, d->cin_pad, px))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      const int N = 16 * d->ntiles;
      bool ok;
      if (d->out_mode == 0) ok = out_ok(0, N, px);
      else if (d->out_mode == 1)
        ok = d->kt == 1 && d->H % 2 == 0 && d->W % 2 == 0 && d->nout >= 1 && d->nout <= N && out_ok(0, 4 * d->nout, px / 4);
      else
        ok = d->kt == 1 && d->nout >= 4 && d->nout % 4 == 0 && d->nout <= N && out_ok(0, d->nout / 4, 4 * px);
      if (!ok) return fail(KDLAE_EINVAL_SHAPE, "conv_lds: store geometry (mode 1: even H, W, ldo >= 4 nout; mode 2: nout % 4 == 0, ldo >= nout / 4)");
      if (!in4(0) || !out4(0) || !al16(d->w[0]) || !al16(d->bias[0])) return fail(KDLAE_EINVAL_SHAPE, align);
      const int kgroups = 9 * d->kt * (d->cin_pad / 16);
      if (d->use_wp3) {
        // kt 1: split records of w0 itself; kt 3: of the tap-pair block w1 (k-group order c * 28 + tap, kdlae_s.cpp)
        if (d->kt == 1) HIPCHK(sc.split(0, d->w[0], d->ntiles, kgroups));
        else HIPCHK(sc.split(0, d->w[1], d->ntiles, 28 * (d->cin_pad / 16)));
      }
      kdlae::ConvLdsParams p{};
      p.in = d->in[0]; p.ldi = d->ldi[0]; p.cin_pad = d->cin_pad; p.wp = d->w[0]; p.ntiles = d->ntiles; p.kgroups = kgroups;
      p.bias = d->bias[0]; p.out = d->out[0]; p.ldo = d->ldo[0]; p.Bn = d->Bn; p.F = F; p.H = d->H; p.W = d->W;
      p.kt = d->kt; p.relu = d->relu ? 1 : 0; p.wp3 = sc.p[0]; p.out_mode = d->out_mode; p.nout = d->out_mode ? d->nout : 0;
      e = kdlae::launch_conv_lds(p, s);
      break;
    }
    case 6: {  // small-output conv
      if (!d->w[0]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      const int Cout = d->C2;
      if (C < 16 || C % 16 || C > 4096 || Cout < 1 || Cout > 4 || (d->ks != 1 && d->ks != 3) || (d->wt && d->ks != 3))
        return fail(KDLAE_EINVAL_SHAPE, "conv_small_out: Cin % 16 == 0, Cout 1 .. 4, ks 1 or 3 (wt: 3)");
      if ((size_t)d->ks * d->ks * C * 16 > 65536) return fail(KDLAE_EINVAL_SHAPE, "conv_small_out: the weights must fit 64 KiB of LDS");
      if (!geo || !in_ok(0, C, px) || !in4(0) || !d->out[0]) return fail(KDLAE_EINVAL_SHAPE, bad);
      if (d->out_nchw) {
        if (px * Cout >= kMaxIdx || d->R || d->in[2]) return fail(KDLAE_EINVAL_SHAPE, "conv_small_out: NCHW takes in1 = res only");
      } else {
        if (!out_ok(0, Cout + (d->in[2] ? 1 : 0), px) || d->in[1] || (d->R && (d->ldr < Cout || px * d->ldr >= kMaxIdx)))
          return fail(KDLAE_EINVAL_SHAPE, "conv_small_out: NHWC takes R (ldr >= Cout) and in2 = extra (ldo > Cout)");
      }
      kdlae::SmallOutParams p{};
      p.in = d->in[0]; p.ld = d->ldi[0]; p.Cin = C; p.Cout = Cout; p.w = d->w[0]; p.bias = d->bias[0];
      p.Bn = d->Bn; p.H = d->H; p.W = d->W; p.F = F; p.ks = d->ks; p.out = d->out[0]; p.out_nchw = d->out_nchw ? 1 : 0;
      p.ldo = d->ldo[0]; p.res = d->in[1]; p.extra = d->in[2]; p.wt = d->wt ? 1 : 0; p.res_nhwc = d->R; p.ldr = d->ldr;
      e = kdlae::launch_conv_small_out(p, s);
      break;
    }
    case 7: {  // 16 -> 16 channel conv
      if (!d->w[0] || !d->bias[0]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!geo || (d->kt != 1 && d->kt != 3) || !in_ok(0, 16, px) || !out_ok(0, 16, px)) return fail(KDLAE_EINVAL_SHAPE, bad);
      if (!in4(0) || !out4(0) || !al16(d->w[0]) || !al16(d->bias[0])) return fail(KDLAE_EINVAL_SHAPE, align);
      kdlae::Conv3dC16Params p{};
      p.in = d->in[0]; p.ldi = d->ldi[0]; p.wp = d->w[0]; p.bias = d->bias[0]; p.out = d->out[0]; p.ldo = d->ldo[0];
      p.Bn = d->Bn; p.F = F; p.H = d->H; p.W = d->W; p.relu = d->relu ? 1 : 0; p.kt = d->kt;
      e = kdlae::launch_conv3d_c16(p, s);
      break;
    }
    case 8: {  // max-pool 2x2 (floor), Bn frames
      if (!geo || F != 1 || d->H < 2 || d->W < 2 || C < 4 || C % 4 || !in_ok(0, C, px) ||
          !out_ok(0, C, (long long)d->Bn * (d->H / 2) * (d->W / 2)))
        return fail(KDLAE_EINVAL_SHAPE, "maxpool2: C % 4 == 0, H, W >= 2");
      if (!in4(0) || !out4(0)) return fail(KDLAE_EINVAL_SHAPE, align);
      e = kdlae::launch_maxpool2(d->in[0], d->ldi[0], d->out[0], d->ldo[0], C, d->Bn, d->H, d->W, s);
      break;
    }
    case 9: {  // global average pool partials + ASDQE head
      for (int i = 0; i < 4; ++i)
        if (!d->w[i] || !d->bias[i]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!d->scratch || !d->out[0]) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (!geo || F != 1 || d->Bn > 65535 || C < 4 || C % 4 || C > 1024 || d->slots < 1 || d->slots > 65535 || d->M < 1 ||
          d->M > 1024 || d->N1 < 1 || d->N1 > 1024 || d->N2 < 1 || d->N2 > 1024 || !in_ok(0, C, px))
        return fail(KDLAE_EINVAL_SHAPE, "gap + head: C % 4 == 0, C, M, N1, N2 <= 1024, slots >= 1");
      if (!in4(0) || !al16(d->scratch)) return fail(KDLAE_EINVAL_SHAPE, align);
      if ((long long)d->Bn * d->slots * C > d->scratch_floats)
        return fail(KDLAE_EINVAL_SHAPE, "scratch must hold Bn * slots * C floats");
      const long long HW = (long long)d->H * d->W;
      e = kdlae::launch_gap_partial(d->in[0], d->ldi[0], C, d->Bn, HW, d->slots, d->scratch, s);
      if (e != hipSuccess) break;
      kdlae::HeadParams p{};
      p.partial = d->scratch; p.slots = d->slots; p.C = C; p.inv_hw = 1.0f / (float)HW;
      p.wo = d->w[0]; p.bo = d->bias[0]; p.M = d->M;
      p.w1 = d->w[1]; p.b1 = d->bias[1]; p.N1 = d->N1;
      p.w2 = d->w[2]; p.b2 = d->bias[2]; p.N2 = d->N2;
      p.w3 = d->w[3]; p.b3 = d->bias[3];
      p.score = d->out[0]; p.B = d->Bn;
      e = kdlae::launch_asdqe_head(p, s);
      break;
    }
    case 10: {  // attention output with the depthwise 3x3 of v as its prologue
      if (!d->in[0] || !d->w[0] || !d->w[1] || !d->R || !d->out[0] || !d->zeros) return fail(KDLAE_EINVAL_CONFIG, null_op);
      if (C != 48 && C != 96) return fail(KDLAE_EINVAL_SHAPE, "attn_out_dw: C in {48, 96}");
      if (d->W % 16) return fail(KDLAE_EINVAL_SHAPE, "attn_out_dw: W % 16 == 0");
      if (!in4(0) || !out4(0) || !al16(d->R) || d->ldr % 4 || !al16(d->w[0]) || !al16(d->w[1]) || !al16(d->bias[0]) ||
          !al16(d->bias[1]))
        return fail(KDLAE_EINVAL_SHAPE, align);
      if (!geo || F != 1 || !in_ok(0, C, px) || !out_ok(0, C, px) || d->ldr < C || px * d->ldr >= kMaxIdx ||
          !kdlae::attn_out_dw_supported(C, d->H, d->W, d->ldi[0]) ||
          !img_bytes_ok(d->H, d->W, std::max(d->ldr, d->ldo[0])))
        return fail(KDLAE_EINVAL_SHAPE, bad);
      {  // neighbouring strips read v as halo: out must not overlap it
        const uintptr_t v0 = (uintptr_t)d->in[0], v1 = v0 + ((size_t)(px - 1) * d->ldi[0] + C) * 4;
        const uintptr_t o0 = (uintptr_t)d->out[0], o1 = o0 + ((size_t)(px - 1) * d->ldo[0] + C) * 4;
        if (v0 < o1 && o0 < v1) return fail(KDLAE_EINVAL_SHAPE, "attn_out_dw: out must not overlap v");
      }
      kdlae::AttnOutDwParams p{};
      p.v = d->in[0]; p.ldv = d->ldi[0]; p.wdw = d->w[0] + 2 * C; p.ldw = 3 * C; p.bdw = d->bias[0] ? d->bias[0] + 2 * C : nullptr;
      p.M = d->w[1]; p.m_img_stride = kdlae::folded_proj_floats(C); p.bias = d->bias[1];
      p.R = d->R; p.ldr = d->ldr; p.out = d->out[0]; p.ldo = d->ldo[0];
      p.Bn = d->Bn; p.H = d->H; p.W = d->W; p.zeros = d->zeros;
      e = kdlae::launch_attn_out_dw(p, C, s);
      break;
    }
    default: return fail(KDLAE_EINVAL_CONFIG, "op must be 0..10");
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, std::string("kdlae_debug_infer: ") + hipGetErrorString(e));
  return KDLAE_OK;
}

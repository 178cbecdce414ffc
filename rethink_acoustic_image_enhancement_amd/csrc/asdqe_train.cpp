// ASDQE training engine: one micro-batch of Train/ASDQE.py:95-122 on DenoiseRatePredictor in train mode
// (ASDQE/ASDQE_model.py:123-171): forward with every z / y activation kept, then the hand-sequenced
// backward.
//
//   conv3x3 + bias (:24,:27)            fwd  z = im2col(x) . W^T + b                     (train GEMM, amode 1)
//                                       bwd  dW = dz^T . im2col(x) (bmode 1; the 1..4-channel first convs:
//                                            train_small.hip); dx = transposed conv (bmode 3); db = 0 exactly
//                                            (the bias feeds a BatchNorm: sum dz = 0), the key stays zero
//   BatchNorm2d, batch statistics       fwd  mean / rstd over all B H' W' pixels (the zero-padded ones
//   + ReLU (:25-26,:28-29)                   included), running update, y = relu(xhat gamma + beta)
//                                       bwd  dbeta, dgamma in one pass, then dz (bn_train.hip)
//   MaxPool2d(2) (:40)                  fwd  inference kernel; bwd first-max routing added to the skip gradient
//   bilinear x2 + cat (:53,:66)         fwd  into the concat's second half; bwd the gather adjoint
//   outc + GAP + regressor (:109,:144)  outc folded after the pool; its input's gradient is the per-image
//                                       row Wo^T df / (H' W') broadcast over the pixels
// Parameters / gradients: flat buffers in named_parameters() order, every key 16-byte aligned (the
// kdlae_tt / kdlae_st layout).  BatchNorm running statistics: a second flat buffer, per BatchNorm
// [running_mean | running_var] in state_dict order, updated in place by the forward.
#include <hip/hip_runtime.h>

#include <string>
#include <unordered_map>
#include <vector>

#include "kernels.h"
#include "param_layout.h"
#include "runtime.h"
#include "train_a.h"
#include "train_host.h"
#include "train_kernels.h"
#include "train_s.h"

using namespace kdlae;
namespace tr = kdlae::train;

struct asdqe_train_handle : TrainHandleBase {  // lay: named_parameters() order
  asdqe_config cfg{};
  int64_t nstat = 0;  // floats of the statistics buffer: every BatchNorm's running_mean | running_var
  LastForward last;
  bool has_m1 = false, has_m2 = false;  // the last forward had dropout masks
};

namespace {

constexpr size_t kPartialFloats = 8u << 20;  // split-K partials of the GEMMs
constexpr size_t kPartFloats = 2u << 20;     // reduction partials (BatchNorm, first-conv dW)
constexpr float kMomentum = 0.1f;            // nn.BatchNorm2d default (ASDQE_model.py:25,28)
constexpr int kN1 = 256, kN2 = 64;

const char* kExt[3] = {"lq_extractor", "gt_extractor", "diff_extractor"};

// one conv3x3 + BatchNorm + ReLU; offsets are bytes into the workspace
struct Layer {
  std::string cv, bn;
  int cin = 0, cout = 0, lvl = 0;
  int ext = -1;  // 0..2: an extractor's first conv (reads the images)
  size_t in = 0, z = 0, y = 0, ms = 0;
  int in_ld = 0, z_ld = 0, y_ld = 0;
  int64_t run = 0;  // offset of [running_mean | running_var] in the statistics buffer
};

struct TPlan : WsPlan {
  int Hp = 0, Wp = 0, slots = 1;
  long long P[4] = {0, 0, 0, 0};
  std::vector<Layer> L;
  size_t xin = 0, cat3 = 0, cat2 = 0, cat1 = 0, p1 = 0, p2 = 0, p3 = 0, x4 = 0, y1 = 0, y2 = 0, y3 = 0, merged = 0;
  size_t ga[4] = {0, 0, 0, 0}, gb[4] = {0, 0, 0, 0}, dcat3 = 0, dcat2 = 0, dcat1 = 0, gmerged = 0, ge1 = 0;
  size_t gap = 0, save = 0, m1 = 0, m2 = 0, wpk = 0, partial = 0, part = 0, dw4 = 0, gtmp = 0;
  long long max_elems = 0;  // the largest view (pixels x pixel stride) any kernel indexes
};

int gap_slots(long long HW) { return (int)std::max<long long>(1, std::min<long long>(256, HW / 2048)); }

TPlan make_plan(const asdqe_train_handle* h, int B, int H, int W) {
  TPlan pl;
  const int d = h->cfg.dim, m = 3 * d;
  pl.Hp = (H + d - 1) / d * d;
  pl.Wp = (W + d - 1) / d * d;
  for (int l = 0; l < 4; ++l) pl.P[l] = (long long)B * (pl.Hp >> l) * (pl.Wp >> l);
  const long long P0 = pl.P[0], P1 = pl.P[1], P2 = pl.P[2], P3 = pl.P[3];
  pl.max_elems = std::max(P0 * std::max(128, m), P2 * 512);
  int64_t run = 0;
  auto layer = [&](const std::string& p, int i, int cin, int cout, int lvl, size_t in, int in_ld, size_t z, int z_ld,
                   size_t y, int y_ld) {
    Layer L;
    L.cv = p + "." + std::to_string(i);
    L.bn = p + "." + std::to_string(i + 1);
    L.cin = cin; L.cout = cout; L.lvl = lvl;
    L.in = in; L.in_ld = in_ld; L.z = z; L.z_ld = z_ld; L.y = y; L.y_ld = y_ld;
    L.run = run;
    run += 2 * cout;
    pl.L.push_back(L);
  };
  pl.xin = pl.take(P0 * 12);
  const size_t ze1 = pl.take(P0 * m), ye1 = pl.take(P0 * m), ze2 = pl.take(P0 * m);
  pl.merged = pl.take(P0 * m);
  for (int e = 0; e < 3; ++e) {
    const std::string p = std::string(kExt[e]) + ".double_conv";
    const size_t o = (size_t)e * d * 4;
    layer(p, 0, h->cfg.in_channels, d, 0, pl.xin + (size_t)e * 16, 12, ze1 + o, m, ye1 + o, m);
    pl.L.back().ext = e;
    layer(p, 3, d, d, 0, ye1 + o, m, ze2 + o, m, pl.merged + o, m);
  }
  // a DoubleConv at level lvl whose output y lands at (yo, y_ld) (a concat half or its own buffer)
  auto dc = [&](const std::string& p, int cin, int cout, int lvl, size_t in, int in_ld, size_t yo, int y_ld) {
    const long long P = pl.P[lvl];
    const size_t za = pl.take(P * cout), ya = pl.take(P * cout), zb = pl.take(P * cout);
    layer(p, 0, cin, cout, lvl, in, in_ld, za, cout, ya, cout);
    layer(p, 3, cout, cout, lvl, ya, cout, zb, cout, yo, y_ld);
  };
  pl.cat3 = pl.take(P0 * 128);
  pl.cat2 = pl.take(P1 * 256);
  pl.cat1 = pl.take(P2 * 512);
  pl.p1 = pl.take(P1 * 64);
  pl.p2 = pl.take(P2 * 128);
  pl.p3 = pl.take(P3 * 256);
  pl.x4 = pl.take(P3 * 256);
  pl.y1 = pl.take(P2 * 128);
  pl.y2 = pl.take(P1 * 64);
  pl.y3 = pl.take(P0 * 64);
  dc("unet.inc.double_conv", m, 64, 0, pl.merged, m, pl.cat3, 128);
  dc("unet.down1.maxpool_conv.1.double_conv", 64, 128, 1, pl.p1, 64, pl.cat2, 256);
  dc("unet.down2.maxpool_conv.1.double_conv", 128, 256, 2, pl.p2, 128, pl.cat1, 512);
  dc("unet.down3.maxpool_conv.1.double_conv", 256, 256, 3, pl.p3, 256, pl.x4, 256);
  dc("unet.up1.conv.double_conv", 512, 128, 2, pl.cat1, 512, pl.y1, 128);
  dc("unet.up2.conv.double_conv", 256, 64, 1, pl.cat2, 256, pl.y2, 64);
  dc("unet.up3.conv.double_conv", 128, 64, 0, pl.cat3, 128, pl.y3, 64);
  for (auto& L : pl.L) L.ms = pl.take(2 * L.cout);  // saved mean | rstd
  // backward: two gradient buffers per level, the concat gradients, the extractors' gradients
  const int gc[4] = {64, 128, 256, 256};
  for (int l = 0; l < 4; ++l) {
    pl.ga[l] = pl.take(pl.P[l] * gc[l]);
    pl.gb[l] = pl.take(pl.P[l] * gc[l]);
  }
  pl.dcat3 = pl.take(P0 * 128);
  pl.dcat2 = pl.take(P1 * 256);
  pl.dcat1 = pl.take(P2 * 512);
  pl.gmerged = pl.take(P0 * m);
  pl.ge1 = pl.take(P0 * m);
  pl.slots = gap_slots((long long)pl.Hp * pl.Wp);
  pl.gap = pl.take((long long)B * pl.slots * 64);
  pl.save = pl.take((long long)B * tr::head_save_floats(64, m, kN1, kN2));
  pl.m1 = pl.take((long long)B * kN1);
  pl.m2 = pl.take((long long)B * kN2);
  pl.wpk = pl.take(9LL * 512 * 256);
  pl.partial = pl.take((long long)kPartialFloats);
  pl.part = pl.take((long long)kPartFloats);
  pl.dw4 = pl.take(256LL * 4 * 9);
  pl.gtmp = pl.take(h->lay.total);
  return pl;
}

// gr: the backward's own gradient buffer (workspace), committed to the caller's at the end
struct Ctx : FlatCtx {
  asdqe_train_handle* h;
  TPlan pl;
  hipStream_t s;
  int B;
};

// one of a conv layer's three GEMMs: the 3x3 weight operand (bmode 2 / 3) repacked into the fixed wpk
// buffer as a [9 Cg][N] matrix, split-K partials from the plan
int conv_gemm(Ctx& c, tr::TGemm g, bool pack) {
  if (pack) HIPCHK(tr::launch_pack_w3(g, g.N, c.buf(c.pl.wpk), c.s));
  g.partial = c.buf(c.pl.partial);
  HIPCHK(tr::launch_tgemm(g, kPartialFloats, c.s));
  return KDLAE_OK;
}

int layer_fwd(Ctx& c, const Layer& L, const float* lq, const float* gt, int H, int W, float* stats) {
  const int Hl = c.pl.Hp >> L.lvl, Wl = c.pl.Wp >> L.lvl;
  const long long P = c.pl.P[L.lvl];
  float* z = c.buf(L.z);
  if (L.ext >= 0) {  // reads the NCHW images; zero beyond H x W (pad_to_multiple)
    const int ci = L.cin;
    SmallInParams p{};
    p.in = L.ext == 1 ? gt : lq;
    p.in_sub = L.ext == 2 ? gt : nullptr;
    p.sb = (long long)ci * H * W;
    p.sc = (long long)H * W;
    p.sy = W;
    p.sx = 1;
    p.Cin = ci;
    p.Cout = L.cout;
    p.dil = 1;
    p.w = c.P(L.cv + ".weight");
    p.bias = c.P(L.cv + ".bias");
    p.out = z;
    p.ldo = L.z_ld;
    p.Bn = c.B;
    p.H = Hl;
    p.W = Wl;
    p.vh = H;
    p.vw = W;
    p.F = 1;
    p.kt = 1;
    p.relu = 0;
    HIPCHK(launch_conv_small_in(p, c.s));
  } else {
    TRY(conv_gemm(c, tr::conv3_fwd_gemm({c.buf(L.in), L.in_ld, L.cin}, c.P(L.cv + ".weight"), c.P(L.cv + ".bias"),
                                        {z, L.z_ld, L.cout}, {c.B, Hl, Wl, 1}), true));
  }
  float* ms = c.buf(L.ms);
  HIPCHK(tr::launch_bn_stats(z, L.z_ld, L.cout, P, ms, ms + L.cout, stats + L.run, stats + L.run + L.cout, kMomentum,
                             c.buf(c.pl.part), c.s));
  HIPCHK(tr::launch_bn_apply_relu(z, L.z_ld, ms, ms + L.cout, c.P(L.bn + ".weight"), c.P(L.bn + ".bias"), L.cout, P,
                                  c.buf(L.y), L.y_ld, c.s));
  return KDLAE_OK;
}

// dy (ld ldd): the gradient of the layer's output y, overwritten with dz; dx (nullable): the input's gradient
int layer_bwd(Ctx& c, const Layer& L, float* dy, int ldd, float* dx, int lddx) {
  const int Hl = c.pl.Hp >> L.lvl, Wl = c.pl.Wp >> L.lvl;
  const long long P = c.pl.P[L.lvl];
  const float* ms = c.buf(L.ms);
  float* dgam = c.G(L.bn + ".weight");
  float* dbet = c.G(L.bn + ".bias");
  HIPCHK(tr::launch_bn_bwd_reduce(dy, ldd, c.buf(L.y), L.y_ld, c.buf(L.z), L.z_ld, ms, ms + L.cout, L.cout, P, dgam,
                                  dbet, c.buf(c.pl.part), c.s));
  HIPCHK(tr::launch_bn_bwd_dx(dy, ldd, c.buf(L.y), L.y_ld, c.buf(L.z), L.z_ld, ms, ms + L.cout,
                              c.P(L.bn + ".weight"), dgam, dbet, L.cout, P, dy, ldd, c.s));
  float* gw = c.G(L.cv + ".weight");
  if (L.ext >= 0) {
    // narrow input: per-block [Cout][Cin][9] partials on the VALU; 1- and 2-channel inputs go through
    // the 4-channel instance on the zero-padded xin view
    const int ci = L.cin, cc = (ci == 3) ? 3 : 4;
    const int ncols = L.cout * cc * 9;
    const int nb = tr::dw3_small_blocks(P, cc, L.cout, kPartFloats);
    float* part = c.buf(c.pl.part);
    HIPCHK(tr::launch_dw3_small(dy, ldd, c.buf(L.in), L.in_ld, cc, L.cout, c.B, Hl, Wl, 1, part, nb, c.s));
    if (cc == ci) {
      HIPCHK(tr::launch_part_reduce(part, nb, ncols, 1, gw, 0, 1.f, c.s));
    } else {
      float* dw4 = c.buf(c.pl.dw4);
      HIPCHK(tr::launch_part_reduce(part, nb, ncols, 1, dw4, 0, 1.f, c.s));
      HIPCHK(tr::launch_narrow_w_copy(dw4, gw, L.cout, ci, c.s));
    }
    return KDLAE_OK;
  }
  const tr::ConvGeo geo{c.B, Hl, Wl, 1};
  TRY(conv_gemm(c, tr::conv3_dw_gemm({dy, ldd, L.cout}, {c.buf(L.in), L.in_ld, L.cin}, gw, geo), false));
  if (dx) TRY(conv_gemm(c, tr::conv3_dx_gemm({dy, ldd, L.cout}, c.P(L.cv + ".weight"), {dx, lddx, L.cin}, geo), true));
  return KDLAE_OK;
}

tr::HeadTrain head_params(Ctx& c, float* score) {
  const int m = 3 * c.h->cfg.dim;
  tr::HeadTrain hp{};
  hp.partial = c.buf(c.pl.gap);
  hp.slots = c.pl.slots;
  hp.C = 64;
  hp.inv_hw = 1.f / (float)((long long)c.pl.Hp * c.pl.Wp);
  hp.wo = c.P("unet.outc.conv.weight");
  hp.bo = c.P("unet.outc.conv.bias");
  hp.M = m;
  hp.w1 = c.P("regressor.2.weight");
  hp.b1 = c.P("regressor.2.bias");
  hp.N1 = kN1;
  hp.w2 = c.P("regressor.5.weight");
  hp.b2 = c.P("regressor.5.bias");
  hp.N2 = kN2;
  hp.w3 = c.P("regressor.8.weight");
  hp.b3 = c.P("regressor.8.bias");
  hp.mask1 = c.h->has_m1 ? c.buf(c.pl.m1) : nullptr;
  hp.mask2 = c.h->has_m2 ? c.buf(c.pl.m2) : nullptr;
  hp.score = score;
  hp.B = c.B;
  hp.save = c.buf(c.pl.save);
  return hp;
}

int net_fwd(Ctx& c, const float* lq, const float* gt, int H, int W, float* stats, float* score) {
  const TPlan& pl = c.pl;
  const int B = c.B, Hp = pl.Hp, Wp = pl.Wp;
  HIPCHK(tr::launch_asdqe_pack_inputs(lq, gt, c.h->cfg.in_channels, B, H, W, Hp, Wp, c.buf(pl.xin), c.s));
  auto run = [&](int i) { return layer_fwd(c, pl.L[i], lq, gt, H, W, stats); };
  for (int i = 0; i < 8; ++i) TRY(run(i));  // extractors, inc
  HIPCHK(launch_maxpool2(c.buf(pl.cat3), 128, c.buf(pl.p1), 64, 64, B, Hp, Wp, c.s));
  TRY(run(8));
  TRY(run(9));
  HIPCHK(launch_maxpool2(c.buf(pl.cat2), 256, c.buf(pl.p2), 128, 128, B, Hp / 2, Wp / 2, c.s));
  TRY(run(10));
  TRY(run(11));
  HIPCHK(launch_maxpool2(c.buf(pl.cat1), 512, c.buf(pl.p3), 256, 256, B, Hp / 4, Wp / 4, c.s));
  TRY(run(12));
  TRY(run(13));
  HIPCHK(launch_upsample2x(c.buf(pl.x4), 256, c.buf(pl.cat1) + 256, 512, 256, B, Hp / 8, Wp / 8, c.s));
  TRY(run(14));
  TRY(run(15));
  HIPCHK(launch_upsample2x(c.buf(pl.y1), 128, c.buf(pl.cat2) + 128, 256, 128, B, Hp / 4, Wp / 4, c.s));
  TRY(run(16));
  TRY(run(17));
  HIPCHK(launch_upsample2x(c.buf(pl.y2), 64, c.buf(pl.cat3) + 64, 128, 64, B, Hp / 2, Wp / 2, c.s));
  TRY(run(18));
  TRY(run(19));
  HIPCHK(launch_gap_partial(c.buf(pl.y3), 64, 64, B, (long long)Hp * Wp, pl.slots, c.buf(pl.gap), c.s));
  HIPCHK(tr::launch_head_train_fwd(head_params(c, score), c.s));
  return KDLAE_OK;
}

int net_bwd(Ctx& c, const float* dscore) {
  const TPlan& pl = c.pl;
  const int B = c.B, Hp = pl.Hp, Wp = pl.Wp, d = c.h->cfg.dim, m = 3 * d;
  const std::vector<Layer>& L = pl.L;
  tr::HeadTrain hp = head_params(c, nullptr);
  tr::HeadTrainGrads hg{c.G("unet.outc.conv.weight"), c.G("unet.outc.conv.bias"), c.G("regressor.2.weight"),
                        c.G("regressor.2.bias"),      c.G("regressor.5.weight"),  c.G("regressor.5.bias"),
                        c.G("regressor.8.weight"),    c.G("regressor.8.bias")};
  HIPCHK(tr::launch_head_train_bwd(hp, dscore, hg, c.s));
  float *a0 = c.buf(pl.ga[0]), *b0 = c.buf(pl.gb[0]), *a1 = c.buf(pl.ga[1]), *b1 = c.buf(pl.gb[1]);
  float *a2 = c.buf(pl.ga[2]), *b2 = c.buf(pl.gb[2]), *a3 = c.buf(pl.ga[3]), *b3 = c.buf(pl.gb[3]);
  float *dcat3 = c.buf(pl.dcat3), *dcat2 = c.buf(pl.dcat2), *dcat1 = c.buf(pl.dcat1);
  // d y3: the pooled gradient of each image, over its pixels
  const long long HW = (long long)Hp * Wp;
  const long long row = tr::head_save_floats(64, m, kN1, kN2);
  HIPCHK(tr::launch_bcast_rows(c.buf(pl.save) + tr::head_save_dgap(64, m, kN1, kN2), row, 64, B, HW, 1.f / (float)HW,
                               a0, 64, c.s));
  // up3
  TRY(layer_bwd(c, L[19], a0, 64, b0, 64));
  TRY(layer_bwd(c, L[18], b0, 64, dcat3, 128));
  HIPCHK(tr::launch_upsample2x_bwd(dcat3 + 64, 128, a1, 64, 64, B, Hp / 2, Wp / 2, c.s));
  // up2
  TRY(layer_bwd(c, L[17], a1, 64, b1, 64));
  TRY(layer_bwd(c, L[16], b1, 64, dcat2, 256));
  HIPCHK(tr::launch_upsample2x_bwd(dcat2 + 128, 256, a2, 128, 128, B, Hp / 4, Wp / 4, c.s));
  // up1
  TRY(layer_bwd(c, L[15], a2, 128, b2, 128));
  TRY(layer_bwd(c, L[14], b2, 128, dcat1, 512));
  HIPCHK(tr::launch_upsample2x_bwd(dcat1 + 256, 512, a3, 256, 256, B, Hp / 8, Wp / 8, c.s));
  // down3
  TRY(layer_bwd(c, L[13], a3, 256, b3, 256));
  TRY(layer_bwd(c, L[12], b3, 256, a3, 256));
  // the skip's gradient (first half of the concat gradient) + the pool's routed gradient, in place
  HIPCHK(tr::launch_maxpool2_bwd(c.buf(pl.cat1), 512, a3, 256, dcat1, 512, dcat1, 512, 256, B, 1, Hp / 8, Wp / 8,
                                 c.s));
  // down2
  TRY(layer_bwd(c, L[11], dcat1, 512, a2, 256));
  TRY(layer_bwd(c, L[10], a2, 256, b2, 128));
  HIPCHK(tr::launch_maxpool2_bwd(c.buf(pl.cat2), 256, b2, 128, dcat2, 256, dcat2, 256, 128, B, 1, Hp / 4, Wp / 4,
                                 c.s));
  // down1
  TRY(layer_bwd(c, L[9], dcat2, 256, a1, 128));
  TRY(layer_bwd(c, L[8], a1, 128, b1, 64));
  HIPCHK(tr::launch_maxpool2_bwd(c.buf(pl.cat3), 128, b1, 64, dcat3, 128, dcat3, 128, 64, B, 1, Hp / 2, Wp / 2, c.s));
  // inc
  TRY(layer_bwd(c, L[7], dcat3, 128, a0, 64));
  TRY(layer_bwd(c, L[6], a0, 64, c.buf(pl.gmerged), m));
  // extractors (the images get no gradient)
  for (int e = 0; e < 3; ++e) {
    TRY(layer_bwd(c, L[2 * e + 1], c.buf(pl.gmerged) + e * d, m, c.buf(pl.ge1) + e * d, m));
    TRY(layer_bwd(c, L[2 * e], c.buf(pl.ge1) + e * d, m, nullptr, 0));
  }
  return KDLAE_OK;
}

int check_shape(int B, const TPlan& pl) {
  // the GEMMs' M / K (pixel counts) and the first convs' pixel index are int; every view is indexed in
  // 64 bits, but no view may pass 2^31 elements (the tiled GEMM's per-image offsets)
  if (pl.P[0] >= (1LL << 31) || pl.max_elems >= (1LL << 31))
    return fail(KDLAE_EINVAL_SHAPE, "batch too large for one ASDQE training step: B*H'*W'*128 must be < 2^31 (" +
                                        std::to_string(B) + " x " + std::to_string(pl.Hp) + " x " +
                                        std::to_string(pl.Wp) + "); split the micro-batch");
  return KDLAE_OK;
}

}  // namespace

extern "C" {

// asdqe_train_* report a null argument as KDLAE_ESTATE (kdlae_tt_*: KDLAE_EINVAL_CONFIG)
int asdqe_train_create(const asdqe_config* cfg, int device, asdqe_train_handle** out) {
  if (!cfg || !out) return fail(KDLAE_ESTATE, "null argument");
  *out = nullptr;
  if (cfg->in_channels < 1 || cfg->in_channels > 4)
    return fail(KDLAE_EINVAL_CONFIG, "in_channels must be 1..4 on the HIP path");
  if (cfg->dim < 16 || cfg->dim > 256 || cfg->dim % 16)
    return fail(KDLAE_EINVAL_CONFIG, "dim must be a multiple of 16 in 16..256 on the HIP path");
  auto* h = new asdqe_train_handle();
  h->cfg = *cfg;
  h->device = device;
  h->nstat = asdqe_keys(*cfg, false, h->lay);  // the BatchNorm buffers live in the statistics buffer
  *out = h;
  return KDLAE_OK;
}

int asdqe_train_destroy(asdqe_train_handle* h) { return train_destroy(h); }

int asdqe_train_num_params(const asdqe_train_handle* h) { return train_num_params(h, -1); }

int asdqe_train_param_info(const asdqe_train_handle* h, int i, const char** name, int64_t* numel, int64_t* offset) {
  return train_param_info(h, i, name, numel, offset);
}

int64_t asdqe_train_num_floats(const asdqe_train_handle* h) { return train_num_floats(h); }
int64_t asdqe_train_num_stat_floats(const asdqe_train_handle* h) { return h ? h->nstat : -1; }

int64_t asdqe_train_workspace_bytes(const asdqe_train_handle* h, int B, int H, int W) {
  if (!h) return -1;
  if (B <= 0 || H <= 0 || W <= 0) {
    fail(KDLAE_EINVAL_SHAPE, "B, H, W must be positive");
    return -1;
  }
  const TPlan pl = make_plan(h, B, H, W);
  if (check_shape(B, pl)) return -1;
  return (int64_t)pl.total;
}

int asdqe_train_forward(asdqe_train_handle* h, const float* theta, float* stats, const float* lq, const float* gt,
                        int B, int H, int W, const float* mask1, const float* mask2, float* score, void* workspace,
                        int64_t workspace_bytes, void* stream) {
  if (!h || !theta || !stats || !lq || !gt || !score || !workspace) return fail(KDLAE_ESTATE, "null argument");
  if (B <= 0 || H <= 0 || W <= 0) return fail(KDLAE_EINVAL_SHAPE, "B, H, W must be positive");
  Ctx c{{&h->lay, theta, nullptr, reinterpret_cast<char*>(workspace)}, h, make_plan(h, B, H, W), (hipStream_t)stream,
        B};
  TRY(check_shape(B, c.pl));
  if ((int64_t)c.pl.total > workspace_bytes) return fail(KDLAE_ESTATE, "training workspace too small");
  if (((uintptr_t)theta | (uintptr_t)stats | (uintptr_t)workspace) & 15)
    return fail(KDLAE_ESTATE, "theta, stats and the workspace must be 16-byte aligned");
  DeviceGuard dg(h->device);
  h->last.valid = false;
  h->has_m1 = mask1 != nullptr;
  h->has_m2 = mask2 != nullptr;
  if (mask1)
    HIPCHK(hipMemcpyAsync(c.buf(c.pl.m1), mask1, (size_t)B * kN1 * sizeof(float), hipMemcpyDeviceToDevice, c.s));
  if (mask2)
    HIPCHK(hipMemcpyAsync(c.buf(c.pl.m2), mask2, (size_t)B * kN2 * sizeof(float), hipMemcpyDeviceToDevice, c.s));
  TRY(net_fwd(c, lq, gt, H, W, stats, score));
  h->last.set(workspace, B, 1, H, W);
  return KDLAE_OK;
}

int asdqe_train_backward(asdqe_train_handle* h, const float* theta, const float* dscore, float* grad, int accumulate,
                         void* workspace, int64_t workspace_bytes, void* stream) {
  if (!h || !theta || !dscore || !grad || !workspace) return fail(KDLAE_ESTATE, "null argument");
  TRY(h->last.check(workspace, "asdqe_train_backward", "asdqe_train_forward"));
  Ctx c{{&h->lay, theta, nullptr, reinterpret_cast<char*>(workspace)}, h, make_plan(h, h->last.B, h->last.H, h->last.W),
        (hipStream_t)stream, h->last.B};
  if ((int64_t)c.pl.total > workspace_bytes) return fail(KDLAE_ESTATE, "training workspace too small");
  if (((uintptr_t)theta | (uintptr_t)grad) & 15) return fail(KDLAE_ESTATE, "theta and grad must be 16-byte aligned");
  DeviceGuard dg(h->device);
  c.gr = c.buf(c.pl.gtmp);
  // zero: the pad floats and the BatchNorm-fed conv biases, whose gradient is exactly zero
  HIPCHK(zero_fill(c.gr, (size_t)h->lay.total * sizeof(float), c.s));
  h->last.valid = false;  // a forward's activations serve one backward
  TRY(net_bwd(c, dscore));
  HIPCHK(tr::launch_grad_commit(c.gr, grad, h->lay.total, accumulate ? 1 : 0, c.s));
  return KDLAE_OK;
}

}  // extern "C"

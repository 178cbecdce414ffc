// Launch interface of the ASDQE training kernels (bn_train.hip): BatchNorm2d in training mode over
// NHWC fp32 views, the adjoint of the bilinear x2 upsample, and the train-mode regressor head
// (ASDQE/ASDQE_model.py:20-34, :53, :144-154; Train/ASDQE.py:95-122).
//
// Views: x[p * ld + c], C % 4 == 0, ld % 4 == 0, 16-byte aligned bases (float4 loads / stores); the in
// and out views of one launch have their own ld, so either may be a channel slice of a concat buffer.
// Element indices are 64-bit.  Every reduction is two-stage in a fixed order (no atomics): a run with
// the same shapes gives the same bits.
#pragma once
#include <hip/hip_runtime.h>

namespace kdlae {
namespace train {

constexpr int kBnMaxBlocks = 1024;  // stage-1 blocks of the BatchNorm reductions
// floats of the `part` scratch the two BatchNorm reductions need for C channels
inline long long bn_part_floats(int C) { return 2LL * kBnMaxBlocks * C; }

// Batch statistics over P pixels: mean[C], rstd[C] = 1 / sqrt(biased var + 1e-5).  Per-thread Welford
// updates, then (count, mean, M2) partials merged with Chan's update in a fixed order: lanes of a
// block, blocks of a 16th of the grid, the 16 segments.  Never sum(x^2) - sum(x)^2 / P.
// rm / rv (nullable): nn.BatchNorm2d's running update, rm = (1 - mom) rm + mom mean,
// rv = (1 - mom) rv + mom var P / (P - 1), done by the finalising kernel.
hipError_t launch_bn_stats(const float* x, int ldx, int C, long long P, float* mean, float* rstd, float* rm,
                           float* rv, float momentum, float* part, hipStream_t s);
// y = relu((z - mean) rstd gamma + beta)
hipError_t launch_bn_apply_relu(const float* z, int ldz, const float* mean, const float* rstd, const float* gamma,
                                const float* beta, int C, long long P, float* y, int ldy, hipStream_t s);
// dbeta[c] = sum_p dy [y > 0], dgamma[c] = sum_p dy [y > 0] xhat, xhat = (z - mean) rstd, from one pass
hipError_t launch_bn_bwd_reduce(const float* dy, int ldd, const float* y, int ldy, const float* z, int ldz,
                                const float* mean, const float* rstd, int C, long long P, float* dgamma,
                                float* dbeta, float* part, hipStream_t s);
// dz = gamma rstd (dy [y > 0] - dbeta / P - xhat dgamma / P); dz may alias dy
hipError_t launch_bn_bwd_dx(const float* dy, int ldd, const float* y, int ldy, const float* z, int ldz,
                            const float* mean, const float* rstd, const float* gamma, const float* dgamma,
                            const float* dbeta, int C, long long P, float* dz, int lddz, hipStream_t s);

// Adjoint of launch_upsample2x (bilinear x2, align_corners=True): din[N][h][w][C] = for every low-
// resolution pixel the weighted sum of the high-resolution gradients dout[N][2h][2w][C] that read it
// (a gather with the forward's weights).
hipError_t launch_upsample2x_bwd(const float* dout, int ldo, float* din, int ldi, int C, int N, int h, int w,
                                 hipStream_t s);

// lq, gt NCHW [B][ci][H][W] -> xin [B Hp Wp][12]: per extractor (lq, gt, lq - gt) 4 channels, the
// channels past ci and the pixels past H x W zero (pad_to_multiple); the first convs' dW operand
hipError_t launch_asdqe_pack_inputs(const float* lq, const float* gt, int ci, int B, int H, int W, int Hp, int Wp,
                                    float* xin, hipStream_t s);
// dst [Cout][ci][9] = src [Cout][4][9] channels < ci
hipError_t launch_narrow_w_copy(const float* src, float* dst, int Cout, int ci, hipStream_t s);
// out[p][c] = v[(p / HW) * ldv + c] * scale (the GAP's gradient: a per-image constant row)
hipError_t launch_bcast_rows(const float* v, long long ldv, int C, int B, long long HW, float scale, float* out,
                             int ldo, hipStream_t s);
// grad[i] = (accumulate ? grad[i] : 0) + g[i]
hipError_t launch_grad_commit(const float* g, float* grad, long long n, int accumulate, hipStream_t s);

// Train-mode regressor (ASDQE_model.py:144-154, outc folded after the pool as in the eval head):
//   g = mean(partial) [C]; f = Wo g + bo [M]; a1 = W1 f + b1; h1 = relu(a1) mask1; a2 = W2 h1 + b2;
//   h2 = relu(a2) mask2; score = tanh(w3 . h2 + b3).  masks [B][N1] / [B][N2] hold 0 or 1 / (1 - p);
//   null = identity.  save [B][kHeadSave...]: g, f, a1, a2 and the backward's da1, da2, da3, df, dgap.
struct HeadTrain {
  const float* partial; int slots, C; float inv_hw;
  const float* wo; const float* bo; int M;
  const float* w1; const float* b1; int N1;
  const float* w2; const float* b2; int N2;
  const float* w3; const float* b3;
  const float* mask1; const float* mask2;
  float* score; int B;
  float* save;  // [B][head_save_floats(C, M, N1, N2)]
};
inline long long head_save_floats(int C, int M, int N1, int N2) { return 2LL * (C + M + N1 + N2) + 4; }
hipError_t launch_head_train_fwd(const HeadTrain& p, hipStream_t s);
// dscore [B] -> per image da3, da2, da1, df, dgap (into save), then every head / outc gradient as a
// fixed-order sum over the images: gwo [M][C], gbo [M], gw1, gb1, gw2, gb2, gw3, gb3
struct HeadTrainGrads {
  float *wo, *bo, *w1, *b1, *w2, *b2, *w3, *b3;
};
hipError_t launch_head_train_bwd(const HeadTrain& p, const float* dscore, const HeadTrainGrads& g, hipStream_t s);
// offset (floats) of dgap [C] inside one image's save row
inline long long head_save_dgap(int C, int M, int N1, int N2) { return (long long)C + M + N1 + N2 + N1 + N2 + 4 + M; }

// loss[0] = mean((s - t)^2), loss[1] = mean |s - t|; ds = scale 2 (s - t) / n.  One block, fixed order.
hipError_t launch_mse(const float* s_, const float* t, int n, float scale, float* ds, float* loss, hipStream_t s);

}  // namespace train
}  // namespace kdlae

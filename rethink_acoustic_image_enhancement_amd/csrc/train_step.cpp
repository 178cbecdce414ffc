// The model-independent entries of a training step (C ABI kdlae_train_*, include/kdlae.h): the three
// losses with their gradients, grad-norm clip + AdamW, mixup and the EMA, each over flat device
// buffers.  All three trainers (train.py) call the optimizer here.
#include <hip/hip_runtime.h>

#include "../../include/kdlae.h"
#include "runtime.h"
#include "train_a.h"
#include "train_kernels.h"
#include "train_s.h"

using kdlae::fail;
namespace tr = kdlae::train;

extern "C" {

int64_t kdlae_train_l1sr_scratch_floats(void) { return 4 * 1024; }

int kdlae_train_l1sr(const float* pred_hq, const float* gt_hq, int64_t n_hq, const float* pred_sr, const float* gt_sr,
                     int64_t n_sr, float* dhq, float* dsr, float* loss, float* scratch, void* stream) {
  if (!pred_hq || !gt_hq || !loss || !scratch || n_hq <= 0) return fail(KDLAE_EINVAL_CONFIG, "null argument");
  if (pred_sr && (!gt_sr || n_sr <= 0)) return fail(KDLAE_EINVAL_CONFIG, "pred_sr without gt_sr / n_sr");
  hipStream_t s = (hipStream_t)stream;
  const int nb = 1024;
  float* p0 = scratch;
  float* p1 = scratch + 2 * nb;
  // L1LossSr (losses.py:159-170): 0.5 l1(hq) + 0.25 l1(sr) + 0.25 (shadow(hq) + shadow(sr))
  hipError_t e = tr::launch_l1sr(pred_hq, gt_hq, n_hq, 0.5f, dhq, p0, nb, s);
  if (e == hipSuccess && pred_sr) e = tr::launch_l1sr(pred_sr, gt_sr, n_sr, 0.25f, dsr, p1, nb, s);
  if (e == hipSuccess)
    e = tr::launch_l1sr_final(p0, nb, n_hq, 0.5f, 0.25f, pred_sr ? p1 : nullptr, pred_sr ? nb : 0, pred_sr ? n_sr : 1,
                              0.25f, 0.25f, loss, s);
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int64_t kdlae_train_l1frames_scratch_floats(void) { return tr::l1frames_scratch_floats(); }

int kdlae_train_l1frames(const float* pred, const float* target, int N, int frames, int64_t hw, float l1loss_weight,
                         float temporal_weight, float binary, int reduction, float* dpred, float* loss, float* scratch,
                         void* stream) {
  if (!pred || !target || !dpred || !loss || !scratch) return fail(KDLAE_ESTATE, "null argument");
  if (N <= 0 || frames <= 0 || hw <= 0) return fail(KDLAE_EINVAL_SHAPE, "empty loss input");
  if (reduction != 0 && reduction != 1)
    return fail(KDLAE_EINVAL_CONFIG, "reduction: 0 = 'mean', 1 = 'sum' ('max' / 'mix' are not implemented)");
  HIPCHK(tr::launch_l1frames(pred, target, N, frames, hw, l1loss_weight, temporal_weight, binary, reduction, dpred,
                             loss, scratch, (hipStream_t)stream));
  return KDLAE_OK;
}

int64_t kdlae_train_l1sonar_scratch_floats(void) { return tr::l1sonar_scratch_floats(); }

int kdlae_train_l1sonar(const float* pred, const float* target, int64_t n, float loss_weight, float binary,
                        int reduction, const float* weight, float* dpred, float* loss, float* scratch, void* stream) {
  if (!pred || !target || !loss || !scratch) return fail(KDLAE_EINVAL_CONFIG, "null argument");
  if (n <= 0) return fail(KDLAE_EINVAL_CONFIG, "empty loss input");
  if (reduction != 0 && reduction != 1)
    return fail(KDLAE_EINVAL_CONFIG, "reduction: 0 = 'mean', 1 = 'sum' ('none' is not implemented)");
  if (weight)
    return fail(KDLAE_EINVAL_CONFIG, "L1LossSonar element weights are not implemented (ImageCleanModel passes none)");
  HIPCHK(tr::launch_l1sonar(pred, target, n, loss_weight, binary, reduction, dpred, loss, scratch, (hipStream_t)stream));
  return KDLAE_OK;
}

int kdlae_train_mse(const float* score, const float* target, int n, float scale, float* dscore, float* loss,
                    void* stream) {
  if (!score || !target || !dscore || !loss) return fail(KDLAE_ESTATE, "null argument");
  if (n <= 0) return fail(KDLAE_EINVAL_SHAPE, "empty loss input");
  HIPCHK(tr::launch_mse(score, target, n, scale, dscore, loss, (hipStream_t)stream));
  return KDLAE_OK;
}

int64_t kdlae_train_adamw_scratch_floats(void) { return 2048 + 2; }

int kdlae_train_clip_adamw(float* theta, const float* grad, float* exp_avg, float* exp_avg_sq, int64_t n, float gscale,
                           float max_norm, float lr, float beta1, float beta2, float eps, float weight_decay, int step,
                           const int64_t* ranges, int nranges, float* scratch, void* stream) {
  if (!theta || !grad || !exp_avg || !exp_avg_sq || !scratch || n <= 0 || step < 1 || nranges < 0 ||
      (nranges > 0 && !ranges))
    return fail(KDLAE_EINVAL_CONFIG, "bad argument");
  for (int r = 0; r < nranges; ++r)
    if (ranges[2 * r] < 0 || ranges[2 * r] > ranges[2 * r + 1] || ranges[2 * r + 1] > n)
      return fail(KDLAE_EINVAL_CONFIG, "bad parameter range");
  hipStream_t s = (hipStream_t)stream;
  const int nb = 2048;
  float* state = scratch + nb;  // [0] = grad norm, [1] = applied grad scale
  // the norm covers every gradient (clip_grad_norm_ over net_g.parameters()); the update only the
  // parameters that received a gradient (torch.optim skips p.grad is None, e.g. output_param when
  // params != 'cat')
  hipError_t e = tr::launch_sumsq(grad, n, scratch, nb, s);
  if (e == hipSuccess) e = tr::launch_clip_coef(scratch, nb, gscale, max_norm, state, s);
  const int64_t whole[2] = {0, n};
  const int64_t* rg = nranges ? ranges : whole;
  for (int r = 0; r < (nranges ? nranges : 1) && e == hipSuccess; ++r) {
    const int64_t b = rg[2 * r], len = rg[2 * r + 1] - b;
    if (len > 0)
      e = tr::launch_adamw(theta + b, grad + b, exp_avg + b, exp_avg_sq + b, len, state, lr, beta1, beta2, eps,
                           weight_decay, step, s);
  }
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int kdlae_train_mixup(const float* in, float* out, int B, int64_t per_sample, const int* perm, float lam,
                      void* stream) {
  if (!in || !out || !perm || B <= 0 || per_sample <= 0 || in == out) return fail(KDLAE_EINVAL_CONFIG, "bad argument");
  hipError_t e = tr::launch_mixup(in, out, B, per_sample, perm, lam, (hipStream_t)stream);
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

int kdlae_train_ema(float* ema, const float* theta, int64_t n, float decay, void* stream) {
  if (!ema || !theta || n <= 0) return fail(KDLAE_EINVAL_CONFIG, "bad argument");
  hipError_t e = tr::launch_ema(ema, theta, n, decay, (hipStream_t)stream);
  if (e != hipSuccess) return fail(KDLAE_EHIP, hipGetErrorString(e));
  return KDLAE_OK;
}

}  // extern "C"

"""References, fp32 emulations, mutants, bounds and input builders for the kernels that end every
training step: ``kdlae_train_l1sr``, ``kdlae_train_l1frames``, ``kdlae_train_clip_adamw``,
``kdlae_train_mixup``, ``kdlae_train_ema`` and ``kdlae_train_mse``.  Needs no GPU; imported by
tests/test_step_kernel_refs.py (which proves the float64 models against torch, and on the fp32
emulations that the bounds below are met by the kernels' arithmetic and missed by every mutant) and by
tests/test_step_kernels_gpu.py (which holds the shipped kernels to the same bounds).

Three layers per entry:

* a float64 numpy model that states the operation in plain terms.  The contract is the C entry and
  its arguments are ``float``, so every hyper-parameter is rounded to fp32 first (``f32``), the 0.1 of
  L1LossSr's binarisation included (torch compares an fp32 tensor with the fp32 constant as well);
  everything after that is float64;
* ``emu_*``: a numpy float32 emulation in the kernel's own operation order (grid-stride chain per
  thread, xor-butterfly per wave, ((w0 + w1) + w2) + w3 per block, double final sum), standing in for
  the GPU where there is none.  It rounds after every operation; the GPU may contract a multiply-add
  into one rounding, which only removes roundings the bounds count;
* ``mutant=`` on the emulations: deliberately wrong variants a GPU test must be able to catch.

Bounds (u = 2^-24), all derived by counting roundings in the kernels' expressions, none measured:

loss, dense all-positive   (ceil(n / T) + 6 + 3 + 4) u: per-thread chain (d rounds once, then
                           ceil(n/T) - 1 adds), wave tree (6), four-wave add (3; l1frames' 8-level
                           LDS tree is below 6 + 3), then divide / weight / combine / cast (4); the
                           final sum over blocks is in double
norm, dense                (ceil(n / 524288) + 9) / 2 u + 3 u: product + chain, 6, 3, halved by the
                           square root; cast, gscale, one spare
applied scale              norm bound + 3 u (add 1e-6, divide, multiply); 0 where no clip applies
                           (coef = 1 exactly, gscale * 1 is exact)
AdamW                      see ``adamw_bounds``: the roundings are counted beside each constant
mixup 3 u, ema 3 u, mse    dscore 3 u, loss[0] (n + 2) u, loss[1] (n + 1) u
"""
import math

import numpy as np

U = 2.0 ** -24
F = np.float32
SENTINEL = 1e30


def f32(x):
    """A hyper-parameter as the C ABI receives it."""
    return float(np.float32(x))


THRESH = f32(0.1)          # l1sr_kernel's `> 0.1f`

# launch geometry, quoted from the sources; T = blocks * 256 elements per grid-stride trip
L1SR_BLOCKS = 1024         # kdlae_train_l1sr: `const int nb = 1024` (always all of them)
L1F_BLOCKS = 1024          # train_s.hip kLossBlocks (min with ceil(n / 256))
SUMSQ_BLOCKS = 2048        # kdlae_train_clip_adamw: `const int nb = 2048` (always all of them)
ADAMW_CAP = 16384          # launch_adamw / launch_ema: grid_for(n, 256, 16384)
MIXUP_CAP = 65536          # launch_mixup: grid_for(B * per, 256, 65536)
T_L1 = L1SR_BLOCKS * 256   # 262144, l1sr_kernel and l1frames_kernel
T_SUMSQ = SUMSQ_BLOCKS * 256   # 524288
T_ADAMW = ADAMW_CAP * 256      # 4194304, adamw_kernel and ema_kernel
T_MIXUP = MIXUP_CAP * 256      # 16777216

SMALL_SIZES = (1, 63, 64, 65, 255, 256, 257, 1000)


def three_trip(T):
    """A size whose grid-stride loop takes a second and a third trip with a ragged tail."""
    return 2 * T + 257


# ===================================================================== float64 models
def _d(x):
    return np.asarray(x, dtype=np.float64)


def l1sr_parts(pred, tgt):
    """(mean |p - t|, mean |[p > 0.1] - [t > 0.1]|, sign(p - t)) of one image pair."""
    p, t = _d(pred).ravel(), _d(tgt).ravel()
    d = p - t
    sb = np.abs((p > THRESH).astype(np.float64) - (t > THRESH))
    return np.abs(d).sum() / p.size, sb.sum() / p.size, np.sign(d)


def l1sr(pred_hq, gt_hq, pred_sr=None, gt_sr=None):
    """L1LossSr: 0.5 l1(hq) + 0.25 l1(sr) + 0.25 (shadow(hq) + shadow(sr)); the gradients are
    0.5 sign(d) / n_hq and 0.25 sign(d) / n_sr (the shadows carry none).  -> (loss, dhq, dsr)"""
    a, s, sg = l1sr_parts(pred_hq, gt_hq)
    loss, dhq, dsr = 0.5 * a + 0.25 * s, 0.5 / sg.size * sg, None
    if pred_sr is not None:
        a, s, sg = l1sr_parts(pred_sr, gt_sr)
        loss += 0.25 * a + 0.25 * s
        dsr = 0.25 / sg.size * sg
    return loss, dhq, dsr


def l1frames_parts(pred, tgt, binary):
    """The three sums of L1LossForVideoFrames over pred / tgt [N, frames, hw] and the two sign fields."""
    p, t = _d(pred), _d(tgt)
    b = f32(binary)
    d = p - t
    s1 = np.abs(d).sum()
    sb = np.abs((p > b).astype(np.float64) - (t > b)).sum()
    u = (p[:, 1:] - p[:, :-1]) - (t[:, 1:] - t[:, :-1])
    return s1, sb, np.abs(u).sum(), np.sign(d), np.sign(u)


def l1frames(pred, tgt, l1loss_weight, temporal_weight, binary, reduction):
    """w1 red(|p - t| + |bin p - bin t|) + wt red(|dp - dt|) over frame differences, red = mean (0) or
    sum (1); one frame: no temporal term.  -> (loss, dpred)"""
    w1, wt = f32(l1loss_weight), f32(temporal_weight)
    N, Fr, HW = pred.shape
    s1, sb, st, sd, su = l1frames_parts(pred, tgt, binary)
    inv1 = 1.0 if reduction else 1.0 / (N * Fr * HW)
    inv2 = (1.0 if reduction else 1.0 / (N * (Fr - 1) * HW)) if Fr > 1 else 0.0
    loss = w1 * (s1 + sb) * inv1 + wt * st * inv2
    g = w1 * inv1 * sd
    g[:, :-1] -= wt * inv2 * su        # d|u_f| / d p_f = -sign(u_f)
    g[:, 1:] += wt * inv2 * su         # d|u_f| / d p_{f+1} = +sign(u_f)
    return loss, g


def _range_mask(n, ranges):
    mask = np.zeros(n, dtype=bool)
    if not ranges:
        mask[:] = True
    for b, e in ranges or ():
        mask[b:e] = True
    return mask


def clip_adamw(theta, grad, m, v, gscale, max_norm, lr, beta1, beta2, eps, weight_decay, step, ranges=None):
    """clip_grad_norm_ + AdamW over flat buffers.  g = gscale grad; norm = |g| over all n; g' = g
    min(1, max_norm / (norm + 1e-6)) (max_norm <= 0: no clip); on the `ranges` (None: all n):
    theta *= 1 - lr wd; m += (1 - b1)(g' - m); v = b2 v + (1 - b2) g'^2;
    theta -= lr / (1 - b1^step) m / (sqrt(v) / sqrt(1 - b2^step) + eps).
    -> dict: norm, scale (the applied gradient scale), theta, m, v, and the update's parts."""
    gscale, max_norm, lr, b1, b2, eps, wd = map(f32, (gscale, max_norm, lr, beta1, beta2, eps, weight_decay))
    th, g, m0, v0 = _d(theta), _d(grad), _d(m), _d(v)
    norm = math.sqrt(float((g * g).sum())) * gscale
    coef = min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0
    scale = gscale * coef
    gp = g * scale
    m1 = m0 + (1 - b1) * (gp - m0)
    v1 = v0 * b2 + (1 - b2) * gp * gp
    k = lr / (1 - b1 ** step)
    denom = np.sqrt(v1) / math.sqrt(1 - b2 ** step) + eps
    upd = k * m1 / denom
    th1 = th * (1 - lr * wd) - upd
    mask = _range_mask(th.size, ranges)
    return dict(norm=norm, scale=scale, clipped=coef < 1.0, mask=mask, gp=gp, m_old=m0, upd=upd, k=k, denom=denom,
                theta=np.where(mask, th1, th), m=np.where(mask, m1, m0), v=np.where(mask, v1, v0))


def mixup(x, perm, lam):
    """out[b] = lam x[b] + (1 - lam) x[perm[b]], x [B, per_sample]."""
    lam, x = f32(lam), _d(x)
    return lam * x + (1 - lam) * x[np.asarray(perm)]


def ema(e, theta, decay):
    """ema = decay ema + (1 - decay) theta."""
    decay = f32(decay)
    return decay * _d(e) + (1 - decay) * _d(theta)


def mse(score, target, scale):
    """-> (dscore = scale 2 (s - t) / n, mean (s - t)^2, mean |s - t|)"""
    d = _d(score) - _d(target)
    return f32(scale) * 2 * d / d.size, (d * d).mean(), np.abs(d).mean()


# ===================================================================== bounds
def loss_dense_bound(n, T=T_L1):
    return (math.ceil(n / T) + 6 + 3 + 4) * U


def norm_dense_bound(n):
    return (math.ceil(n / T_SUMSQ) + 9) / 2 * U + 3 * U


def scale_bound(n, clipped):
    return norm_dense_bound(n) + 3 * U if clipped else 0.0


def adamw_bounds(ref, theta_old, eps_s, beta1, beta2):
    """Element-wise bounds (bm, bv, bth) on |m - m64|, |v - v64|, |theta - theta64| for the update
    `ref` = clip_adamw(...), counted from adamw_kernel's expression.  eps_s bounds the applied scale.

    m = m + (1 - b1)(g gs - m): g gs (1, and eps_s), the subtraction (1), the product (1), the add (1),
      and 1 - b1 itself (1) unless b1 >= 0.5, where the subtraction is exact (Sterbenz): 4 or 5.  The
      roundings are relative to the operands, not to the (possibly cancelled) result, hence the
      factor |m_old| + |g'|.
    v = v b2 + ((1 - b2) g') g': g' twice (2, and 2 eps_s), two products (2), the add (1); v b2 (1) sits
      on the other term; 1 - b2 is exact for b2 >= 0.5: 5.  Every term is positive, so relative to v.
    theta: p (1 - lr wd) rounds the factor (1) and the product (1), the final subtraction (1) rounds
      relative to |theta| + |update|: 3 u |theta|.  The issue counted 2; the subtraction's share
      is the third.  The update (lr / bc1) m / denom: bc1 rounded once from double (1), lr / bc1 (1),
      times m (1), divided (1), the subtraction's share (1), and denom = sqrt(v) / bc2s + eps: half of
      v's 5 u + 2 eps_s, sqrt (1), bc2s (1), the division (1), the add (1) = 6.5 u + eps_s:
      (12 u + eps_s) |update|.  The issue's 8 u + 2 eps_s folded m's error in as if it were
      relative to m; it is relative to |m_old| + |g'| (above), so it enters as bm lr / bc1 / denom.
    """
    assert f32(beta2) >= 0.5, "the count for v assumes 1 - beta2 is exact"
    gp, m_old = np.abs(ref["gp"]), np.abs(ref["m_old"])
    bm = ((4 if f32(beta1) >= 0.5 else 5) * U + eps_s) * (m_old + gp)
    bv = (5 * U + 2 * eps_s) * ref["v"]
    bth = 3 * U * np.abs(_d(theta_old)) + (12 * U + eps_s) * np.abs(ref["upd"]) + bm * ref["k"] / ref["denom"]
    return bm, bv, bth


def mixup_bound(x, perm, lam):
    lam, x = f32(lam), np.abs(_d(x))
    return 3 * U * (lam * x + (1 - lam) * x[np.asarray(perm)])


def ema_bound(e, theta):
    return 3 * U * (np.abs(_d(e)) + np.abs(_d(theta)))


# ===================================================================== fp32 emulations
def _thread_partials(vals, blocks):
    """What each of blocks * 256 threads holds after its grid-stride loop `a += vals[i]`."""
    T = blocks * 256
    trips = max(1, math.ceil(vals.size / T))
    pad = np.zeros(trips * T, dtype=F)
    pad[:vals.size] = vals
    acc = np.zeros(T, dtype=F)
    for r in range(trips):
        acc = acc + pad[r * T:(r + 1) * T]
    return acc.reshape(blocks, 256)


_LANE = np.arange(64)


def _block_sum_256(a):
    """train.hip block_sum_256: wave_sum's xor butterfly, then ((w0 + w1) + w2) + w3."""
    w = a.reshape(-1, 4, 64)
    for o in (32, 16, 8, 4, 2, 1):
        w = w + w[..., _LANE ^ o]
    s = w[..., 0]
    return ((s[:, 0] + s[:, 1]) + s[:, 2]) + s[:, 3]


def _lds_tree_256(a):
    """l1frames_kernel's shared-memory tree: red[t] += red[t + w], w = 128 .. 1."""
    a = a.copy()
    w = 128
    while w:
        a[:, :w] = a[:, :w] + a[:, w:2 * w]
        w >>= 1
    return a[:, 0]


def _serial_f32(part):
    a = F(0)
    for x in part:
        a = F(a + x)
    return a


def _drop(part, mutant):
    """mutant 'drop_block': the last block that saw data never reaches the final sum."""
    if mutant == "drop_block":
        part = part.copy()
        part[np.nonzero(part)[0][-1]] = 0
    return part


def _emu_l1sr_term(pred, tgt, w, mutant):
    p, t = np.asarray(pred, dtype=F).ravel(), np.asarray(tgt, dtype=F).ravel()
    d = p - t
    gt_ = np.greater_equal if mutant == "ge" else np.greater
    sb = np.abs(gt_(p, F(THRESH)).astype(F) - gt_(t, F(THRESH)).astype(F))
    c = F(w / p.size)
    pos = d >= 0 if mutant == "sign0" else d > 0
    grad = np.where(pos, c, np.where(d < 0, -c, F(0))).astype(F)
    pa = _drop(_block_sum_256(_thread_partials(np.abs(d), L1SR_BLOCKS)), mutant)
    ps = _block_sum_256(_thread_partials(sb, L1SR_BLOCKS))
    return pa, ps, grad, float(p.size)


def emu_l1sr(pred_hq, gt_hq, pred_sr=None, gt_sr=None, mutant=None, final_double=True):
    """l1sr_kernel + l1sr_final_kernel.  final_double=False: the fp32 serial final sum the kernel had.
    mutants: sign0 (sign(0) = +1), ge (threshold >=), drop_block."""
    tot = (lambda part: float(_d(part).sum())) if final_double else (lambda part: float(_serial_f32(part)))
    pa, ps, dhq, n0 = _emu_l1sr_term(pred_hq, gt_hq, 0.5, mutant)
    loss = F(F(0.5) * F(tot(pa) / n0) + F(F(0.25) * F(tot(ps) / n0)))
    dsr = None
    if pred_sr is not None:
        pa, ps, dsr, n1 = _emu_l1sr_term(pred_sr, gt_sr, 0.25, mutant)
        loss = F(loss + F(F(F(0.25) * F(tot(pa) / n1)) + F(F(0.25) * F(tot(ps) / n1))))
    return loss, dhq, dsr


def emu_l1frames(pred, tgt, l1loss_weight, temporal_weight, binary, reduction, mutant=None):
    """l1frames_kernel + l1frames_final_kernel.  mutants: sign0, ge, swap_t (the temporal term's two
    neighbour signs swapped), drop_block."""
    p, t = np.asarray(pred, dtype=F), np.asarray(tgt, dtype=F)
    N, Fr, HW = p.shape
    n = p.size
    w1, wt, b = f32(l1loss_weight), f32(temporal_weight), F(f32(binary))
    inv1 = 1.0 if reduction else 1.0 / n
    inv2 = (1.0 if reduction else 1.0 / (N * (Fr - 1) * HW)) if Fr > 1 else 0.0
    g1, gt = F(w1 * inv1), F(wt * inv2)
    d = p - t
    gt_ = np.greater_equal if mutant == "ge" else np.greater
    sb = np.abs(gt_(p, b).astype(F) - gt_(t, b).astype(F))
    sd = np.where(d >= 0, 1, -1) if mutant == "sign0" else np.sign(d)
    u = (p[:, 1:] - p[:, :-1]) - (t[:, 1:] - t[:, :-1])
    st = np.zeros_like(p)
    st[:, :-1] = np.abs(u)
    nxt, prv = np.zeros_like(p), np.zeros_like(p)
    nxt[:, :-1] = gt * np.sign(u).astype(F)      # pair (f, f + 1), seen from f
    prv[:, 1:] = gt * np.sign(u).astype(F)       # pair (f - 1, f), seen from f
    if mutant == "swap_t":
        nxt, prv = -nxt, -prv
    g = ((g1 * sd.astype(F)) - nxt) + prv
    blocks = min(L1F_BLOCKS, math.ceil(n / 256))
    parts = [_lds_tree_256(_thread_partials(x.ravel(), blocks)) for x in (np.abs(d), sb, st)]
    parts[0] = _drop(parts[0], mutant)
    a, bb, c = (float(_d(x).sum()) for x in parts)
    loss = F(w1 * ((a + bb) * inv1) + (wt * (c * inv2) if inv2 > 0 else 0.0))
    return loss, g.astype(F)


def bias_corrections(beta1, beta2, step, fp32_pow=False):
    """(bc1, bc2s) as launch_adamw forms them: in double, rounded once.  fp32_pow: the earlier
    1.f - powf(beta, step) route."""
    b1, b2 = F(beta1), F(beta2)
    if fp32_pow:
        return F(F(1) - np.power(b1, F(step))), np.sqrt(F(F(1) - np.power(b2, F(step))))
    return F(1.0 - float(b1) ** step), F(math.sqrt(1.0 - float(b2) ** step))


def emu_clip_adamw(theta, grad, m, v, gscale, max_norm, lr, beta1, beta2, eps, weight_decay, step, ranges=None,
                   mutant=None, fp32_pow=False):
    """sumsq_kernel + clip_coef_kernel + adamw_kernel per range.  -> dict norm, scale, theta, m, v.
    mutants: eps_in_sqrt, no_bc1, no_bc2, l2_wd, no_1e6, no_clamp, norm_ranges."""
    th, g, m0, v0 = (np.asarray(x, dtype=F) for x in (theta, grad, m, v))
    gscale, max_norm, lr, b1, b2, eps, wd = map(F, (gscale, max_norm, lr, beta1, beta2, eps, weight_decay))
    mask = _range_mask(th.size, ranges)
    gn = np.where(mask, g, F(0)) if mutant == "norm_ranges" else g
    part = _block_sum_256(_thread_partials(gn * gn, SUMSQ_BLOCKS))
    norm = F(F(math.sqrt(float(_d(part).sum()))) * gscale)
    coef = F(1)
    if max_norm > 0:
        coef = max_norm / (norm if mutant == "no_1e6" else F(norm + F(1e-6)))
        if mutant != "no_clamp":
            coef = min(F(1), coef)
    gs = F(gscale * coef)
    bc1, bc2s = bias_corrections(b1, b2, step, fp32_pow)
    if mutant == "no_bc1":
        bc1 = F(1)
    if mutant == "no_bc2":
        bc2s = F(1)
    gr = g * gs
    if mutant == "l2_wd":
        gr, pv = gr + wd * th, th
    else:
        pv = th * F(F(1) - F(lr * wd))
    mv = m0 + F(F(1) - b1) * (gr - m0)
    vv = v0 * b2 + (F(F(1) - b2) * gr) * gr
    if mutant == "eps_in_sqrt":
        denom = np.sqrt(vv / (bc2s * bc2s) + eps)
    else:
        denom = np.sqrt(vv) / bc2s + eps
    pv = pv - (F(lr / bc1) * mv) / denom
    return dict(norm=norm, scale=gs, theta=np.where(mask, pv, th).astype(F), m=np.where(mask, mv, m0).astype(F),
                v=np.where(mask, vv, v0).astype(F))


def emu_mixup(x, perm, lam, mutant=None):
    """mixup_kernel.  mutants: perm_first (perm[b] for the first operand too), swapped."""
    x, lam, perm = np.asarray(x, dtype=F), F(lam), np.asarray(perm)
    a, b = x, x[perm]
    if mutant == "perm_first":
        a = b
    if mutant == "swapped":
        a, b = b, a
    return lam * a + F(F(1) - lam) * b


def emu_ema(e, theta, decay, mutant=None):
    """ema_kernel.  mutant: swapped (the two weights exchanged)."""
    e, theta, decay = np.asarray(e, dtype=F), np.asarray(theta, dtype=F), F(decay)
    if mutant == "swapped":
        e, theta = theta, e
    return e * decay + theta * F(F(1) - decay)


def emu_mse(score, target, scale, mutant=None):
    """mse_kernel.  mutants: no2, no_scale.  -> (dscore, loss[0], loss[1])"""
    s, t = np.asarray(score, dtype=F), np.asarray(target, dtype=F)
    n = F(s.size)
    k = F(F(F(1) if mutant == "no_scale" else F(scale)) * F(1 if mutant == "no2" else 2)) / n
    d = s - t
    a, m = F(0), F(0)
    for x in d:
        a = F(float(x) * float(x) + float(a))   # fmaf: the product is exact in double
        m = F(m + abs(x))
    return (k * d).astype(F), F(a / n), F(m / n)


# ===================================================================== input builders
def rng(seed):
    return np.random.default_rng(seed)


def dyadic(shape, seed, bits=10):
    """fp32 values k 2^-bits in [0, 1): differences of such values are exact in fp32."""
    return (rng(seed).integers(0, 1 << bits, size=shape) * 2.0 ** -bits).astype(F)


def loss_generic(shape, seed, tie_block=True):
    """Gradient class: dyadic pred / target (every sign is unambiguous in fp32), the whole second
    256-element block with pred == target where there are at least three, ties scattered elsewhere."""
    p, t = dyadic(shape, seed), dyadic(shape, seed + 1)
    pf, tf = p.reshape(-1), t.reshape(-1)
    if tie_block and pf.size >= 768:
        pf[256:512] = tf[256:512]
    pf[::7] = tf[::7]
    return p, t


def loss_one_hot(shape, j, pv, tv, seed):
    """pred == target everywhere but flat element j, which holds pred pv / target tv (dyadic, so every
    partial sum is exact)."""
    t = dyadic(shape, seed)
    p = t.copy()
    p.reshape(-1)[j], t.reshape(-1)[j] = pv, tv
    return p, t


def one_hot_positions(n, T):
    return sorted({j for j in (0, 255, 256, T - 1, T, n - 1) if 0 <= j < n})


def loss_threshold(n, binary=THRESH):
    """(pred, target, count): elements at the threshold and at nextafter either way, on the pred side
    against a target of 0 (bin 0) and on the target side against a pred of 0.5 (bin 1); count is the
    number of differing binarisations under the kernel's strict `>`.  Two triples in three are on the
    pred side, so a `>=` moves the count (on one side it adds what it removes on the other)."""
    b = F(binary)
    tri = np.array([np.nextafter(b, F(0)), b, np.nextafter(b, F(1))], dtype=F)
    vals = tri[np.arange(n) % 3]
    pred_side = (np.arange(n) // 3) % 3 != 2
    p = np.where(pred_side, vals, F(0.5)).astype(F)
    t = np.where(pred_side, F(0), vals).astype(F)
    above = (np.arange(n) % 3) == 2
    count = int(np.sum(np.where(pred_side, above, ~above)))
    return p, t, count


def loss_dense(shape, seed):
    """|d| in [0.25, 1] on a 2^-16 grid: pred - target and the frame differences are exact in fp32,
    the sums are not, and nothing cancels."""
    r = rng(seed)
    t = (r.integers(0, 1 << 16, size=shape) * 2.0 ** -16).astype(F)
    d = (r.integers(1 << 14, (1 << 16) + 1, size=shape) * 2.0 ** -16).astype(F)
    return t + d, t


def spread(n, lo, hi, seed, signed=True):
    """fp32 magnitudes log-uniform over [lo, hi]."""
    r = rng(seed)
    x = np.exp(r.uniform(math.log(lo), math.log(hi), size=n))
    if signed:
        x *= r.choice([-1.0, 1.0], size=n)
    return x.astype(F)


ADAMW_CLASSES = ("clip", "tiny", "noclip", "twice", "off0", "off-1", "gscale")


def adamw_inputs(n, cls, seed=0):
    """theta spread over 1e-4 .. 1 (its own ulp does not hide the update), a gradient per class, and
    nonzero moments of the clipped gradient's size.  -> dict theta, grad, m, v, gscale, max_norm

    clip    norm >> max_norm = 0.01 (the KDLAET.yml setting)
    tiny    max_norm = 1e-5, norm ~ 2e-5: the +1e-6 is 5% of the coefficient, and the clipped
            gradients spread over 1e-9 .. 1e-6, around eps = 1e-8
    noclip  norm = max_norm / 2: coefficient 1, applied scale == gscale
    twice   norm ~ 2 max_norm
    off0 / off-1   max_norm 0 / -1: no clip
    gscale  gscale = 0.125 (an 8-rank all-reduce), clipped
    """
    theta = spread(n, 1e-4, 1.0, seed)
    g = spread(n, 1e-3, 1.0, seed + 1)
    gscale, max_norm = 1.0, 0.01
    unit = g.astype(np.float64) / math.sqrt(float((g.astype(np.float64) ** 2).sum()))
    if cls == "tiny":
        max_norm, g = 1e-5, (unit * 2e-5).astype(F)
    elif cls == "noclip":
        g = (unit * 0.005).astype(F)
    elif cls == "twice":
        g = (unit * 0.02).astype(F)
    elif cls == "off0":
        max_norm, g = 0.0, (unit * 0.02).astype(F)
    elif cls == "off-1":
        max_norm, g = -1.0, (unit * 0.02).astype(F)
    elif cls == "gscale":
        gscale = 0.125
    else:
        assert cls == "clip", cls
    gd = g.astype(np.float64)
    norm = math.sqrt(float((gd * gd).sum())) * gscale
    s = gscale * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)
    r = rng(seed + 2)
    m = (gd * s * r.uniform(-1.0, 1.0, size=n)).astype(F)
    v = ((gd * s) ** 2 * r.uniform(0.25, 2.0, size=n)).astype(F)
    return dict(theta=theta, grad=g, m=m, v=v, gscale=gscale, max_norm=max_norm)


def one_hot_grad(n, j, value=0.75):
    g = np.zeros(n, dtype=F)
    g[j] = value
    return g


HYPER = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.5e-4)
HYPER_T = dict(lr=1e-3, beta1=0.2, beta2=0.999, eps=1e-8, weight_decay=0.5e-4)   # KDLAET.yml's betas


def check_adamw(got, ref, theta_old, n, beta1, beta2):
    """Worst ratio to each bound of one update `got` (dict norm, scale, theta, m, v: emulation or GPU)
    against `ref` = clip_adamw(...).  -> dict name: ratio (<= 1 passes)."""
    eps_s = scale_bound(n, ref["clipped"])
    bm, bv, bth = adamw_bounds(ref, theta_old, eps_s, beta1, beta2)
    tiny = 1e-300
    out = dict(norm=abs(float(got["norm"]) - ref["norm"]) / (norm_dense_bound(n) * ref["norm"] + tiny),
               m=float(np.max(np.abs(_d(got["m"]) - ref["m"]) / (bm + tiny))),
               v=float(np.max(np.abs(_d(got["v"]) - ref["v"]) / (bv + tiny))),
               theta=float(np.max(np.abs(_d(got["theta"]) - ref["theta"]) / (bth + tiny))))
    es = abs(float(got["scale"]) - ref["scale"])
    out["scale"] = es / (eps_s * abs(ref["scale"])) if eps_s else (0.0 if es == 0 else math.inf)
    return out

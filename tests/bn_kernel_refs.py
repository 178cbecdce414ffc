"""References, fp32 emulations, mutants, bounds and inputs for the batch-statistics BatchNorm kernels of
csrc/bn_train.hip (bn_stats_part / bn_stats_final, bn_apply_relu, bn_bwd_reduce, bn_bwd_dx) and the
bilinear x2 pair (upsample2x_kernel in asdqe_kernels.hip, upsample2x_bwd_kernel in bn_train.hip):
``kdlae_debug_bn`` ops 0-5.  Needs no GPU and loads no library; imported by tests/test_bn_kernel_refs.py
(which proves the float64 models against torch and shows, on the fp32 emulations, that the bounds below
are met by the kernels' arithmetic and missed by every mutant) and by tests/test_bn_kernels_gpu.py (which
holds the shipped kernels to the same bounds on the same inputs).

Every op is compared alone: its operands (mean, rstd, y, dgamma, dbeta as well) are fp32 arrays built
here on the host, so the float64 model, the emulation and the GPU see the same bits.

Three layers per op, as in tests/step_kernel_refs.py:

* a float64 numpy model in the operation's plain terms;
* ``emu_*``: numpy float32 in the kernel's own operation order with the launch geometry (``red_geom``,
  ``ew_blocks``, the (lane, quad) thread layout, the stage-2 segments, ``part_reduce_kernel``'s order)
  re-derived in Python.  It rounds after every operation; the GPU may contract a multiply-add into one
  rounding, which only removes roundings the bounds count;
* ``mutant=``: deliberately wrong variants that a GPU test must be able to catch.

Bounds (u = 2^-24, the largest relative error of one fp32 rounding).  Each is counted from the kernel's
expression; the count stands in a comment beside the function.  None was measured.
"""
import math

import numpy as np

from rethink_acoustic_image_enhancement_amd.hashweights import hash_normal, hash_uniform

U = 2.0 ** -24
F = np.float32
SENTINEL = 1e30
KT = 256                 # threads per block, every kernel here
KU = 4                   # bn_train.hip kU: pixels per thread per step of the element-wise kernels
BN_MAX_BLOCKS = 1024     # train_a.h kBnMaxBlocks
EW_CAP = 4096            # ew_blocks' cap
BWD_CAP = 8192           # flat_blocks' cap (upsample2x_bwd)
FWD_CAP = 65536          # launch_upsample2x's cap
EPS = float(F(1e-5))     # kBnEps as the kernel holds it
MOMENTUM = 0.1           # asdqe_train.cpp kMomentum


def _d(x):
    return np.asarray(x, dtype=np.float64)


def f32(x):
    return float(F(x))


# ===================================================================== launch geometry (bn_train.hip)
def lanes_of(C):
    return KT // (C // 4)


def red_geom(C, P):
    """-> (nblk, per): stage-1 blocks and pixels per block of bn_stats_part / bn_bwd_reduce."""
    lanes = lanes_of(C)
    nb = max(1, min(BN_MAX_BLOCKS, (P + 16 * lanes - 1) // (16 * lanes)))
    per = (P + nb - 1) // nb
    return (P + per - 1) // per, per


def ew_blocks(C, P):
    lanes = lanes_of(C)
    return max(1, min(EW_CAP, (P + lanes * KU - 1) // (lanes * KU)))


def ew_cover(C, P):
    """How often bn_apply_relu / bn_bwd_dx's loops store each pixel: must be 1 everywhere."""
    lanes, nb = lanes_of(C), ew_blocks(C, P)
    step = nb * lanes
    cnt = np.zeros(P, dtype=np.int64)
    start = (np.arange(nb)[:, None] * lanes + np.arange(lanes)[None, :]).ravel()
    p = start[start < P]
    while p.size:
        for u in range(KU):
            q = p + u * step
            np.add.at(cnt, q[q < P], 1)
        p = p + step * KU
        p = p[p < P]
    return cnt


def run_len(C, P):
    """The longest run of pixels one thread of a stage-1 block walks."""
    _, per = red_geom(C, P)
    return -(-per // lanes_of(C))


def part_depth(nblk):
    """Adds on the longest path of part_reduce_kernel: a wave's four chains of ceil(nblk / 64) terms,
    (a0 + a1) + (a2 + a3), then the 16 waves in order."""
    return max(0, -(-nblk // 64) - 1) + 2 + 15


def stage2_depth(nblk):
    """Chan merges on the longest path of bn_stats_final: a segment's blocks, then 15 segments."""
    return max(0, -(-nblk // 16) - 1) + 15


# ===================================================================== float64 models
def bn_stats(x, rm=None, rv=None, momentum=MOMENTUM):
    """x [P][C] -> dict(mean, var (biased), rstd = 1 / sqrt(var + eps), rm, rv).  The running update is
    nn.BatchNorm2d's: new = (1 - momentum) old + momentum stat with the unbiased variance; a single pixel
    has none, and the kernel then takes the biased one (0)."""
    x = _d(x)
    P = x.shape[0]
    mean = x.mean(0)
    var = ((x - mean) ** 2).mean(0)
    out = dict(mean=mean, var=var, rstd=1.0 / np.sqrt(var + EPS))
    if rm is not None:
        m = f32(momentum)
        unb = var * P / (P - 1) if P > 1 else var
        out["rm"] = (1 - m) * _d(rm) + m * mean
        out["rv"] = (1 - m) * _d(rv) + m * unb
    return out


def bn_apply_relu(z, mean, rstd, gamma, beta):
    return np.maximum((_d(z) - _d(mean)) * (_d(rstd) * _d(gamma)) + _d(beta), 0.0)


def bn_bwd_terms(dy, y, z, mean, rstd):
    g = _d(dy) * (_d(y) > 0)
    return g, (_d(z) - _d(mean)) * _d(rstd)


def bn_bwd_reduce(dy, y, z, mean, rstd):
    """-> (dgamma, dbeta)"""
    g, xh = bn_bwd_terms(dy, y, z, mean, rstd)
    return (g * xh).sum(0), g.sum(0)


def bn_bwd_dx(dy, y, z, mean, rstd, gamma, dgamma, dbeta):
    g, xh = bn_bwd_terms(dy, y, z, mean, rstd)
    P = g.shape[0]
    return _d(gamma) * _d(rstd) * (g - _d(dbeta) / P - xh * _d(dgamma) / P)


def up_matrix(n):
    """U (2n x n) of the bilinear x2 upsample, align_corners=True: src = o (n - 1) / (2n - 1)."""
    Um = np.zeros((2 * n, n))
    for o in range(2 * n):
        src = o * (n - 1) / (2 * n - 1) if n > 1 else 0.0
        i0 = min(int(math.floor(src)), n - 1)
        l1 = src - i0
        Um[o, i0] += 1 - l1
        Um[o, min(i0 + 1, n - 1)] += l1
    return Um


def up_matrix_f32(n, mutant=None):
    """The same matrix with the weights the kernels form in fp32: r = fl(fl(n - 1) / fl(2n - 1)),
    s = fl(r o), i0 = trunc(s), l1 = s - i0 (exact), l0 = fl(1 - l1); held in float64."""
    Um = np.zeros((2 * n, n))
    r = F(n - 1) / F(2 * n - 1) if n > 0 else F(0)
    if mutant == "half_pixel":
        r = F(0.5)
    for o in range(2 * n):
        s = r * F(o)
        if mutant == "half_pixel":   # align_corners=False: src = (o + 0.5) / 2 - 0.5, clamped at 0
            s = max(F(0), (F(o) + F(0.5)) * F(0.5) - F(0.5))
        i0 = int(s)
        l1 = F(s - F(i0))
        l0 = F(F(1) - l1)
        if mutant == "swap":
            l0, l1 = l1, l0
        Um[o, i0] += float(l0)
        Um[o, min(i0 + 1, n - 1)] += float(l1)
    return Um


def up_fwd(x, Uy, Ux):
    """x [N][h][w][C] -> [N][2h][2w][C] = Uy x Ux^T per (image, channel)."""
    return np.einsum("ai,nijc,bj->nabc", Uy, _d(x), Ux, optimize=True)


def up_bwd(v, Uy, Ux):
    """v [N][2h][2w][C] -> [N][h][w][C]: the transpose."""
    return np.einsum("ai,nabc,bj->nijc", Uy, _d(v), Ux, optimize=True)


def last_overshoots(n):
    """True where fl(r (2n - 1)) > n - 1: the last output row then has i0 = n - 1 with l1 > 0, and only
    the clamp of its second neighbour keeps the read inside the image."""
    return n > 1 and float(F(n - 1) / F(2 * n - 1) * F(2 * n - 1)) > n - 1


# ===================================================================== bounds
def _nnz_depth(depth, terms):
    """An add with a zero operand is exact, so a fixed-order sum of k nonzero terms rounds at most
    min(depth, k - 1) times on any path."""
    k = (np.asarray(terms) != 0).sum(0)
    return np.minimum(depth, np.maximum(k - 1, 0))


def stats_bounds(x, C, P, rm=None, rv=None, momentum=MOMENTUM):
    """Absolute bounds for mean, rm, rv and the relative bound of (var + eps) = 1 / rstd^2.

    depth = r + (lanes - 1) + stage2: the thread's Welford run of r pixels, the lanes' Chan merges, the
    segment's blocks and the 15 segment merges (every step below counts one per level).
    mean  Welford step: d = v - mean (u |d|), 1 / n (u), d * (1 / n) (u), mean += (u |mean|): 3 u D / k +
          u M at step k with D = 2 max |x - mean| >= |d|, M = max |x| >= |mean|; an error made at step k
          is scaled by k / r afterwards, so the run costs u M (r + 1) / 2 + 3 u D.  A level of K Chan merges
          in order (the lanes, a segment's blocks, the 16 segments): d (u), fb = nb / n (u), d fb (u): 3 u D
          fb with fb <= 2 / (k + 1) at merge k (the parts' counts differ by at most a factor 2), ma += (u M),
          scaled by about k / K afterwards: u M (K + 2) / 2 + 6 u D (1/2 + ... + 1/K) per level; the levels
          add because each level averages the errors of the one below.
    var   M2 is a sum of nonnegative terms d (v - mean): d (u), v - mean (u), product (u), add (depth u):
          (depth + 3) u M2; a Chan merge adds d d (na fb): 4 u of a nonnegative term, inside depth + 6.  The
          running mean's own error e (|e| <= the mean bound's u M part per step) enters through the cross
          term 2 e sum |x - mean|: 4 u M madev per unit of P with madev = mean |x - mean|.  var = q / P: u.
          abs(var) <= u ((depth + 7) var + 4 M madev).
    rstd  var + eps (u), sqrt (u), 1 / . (u): compared as |1 / rstd^2 - (var + eps)| / (var + eps)
          <= var_abs / (var + eps) + 7 u (2 x 3 u of rstd's own roundings, 1 spare).
    rm    (1 - m) (u), (1 - m) rm (u), m mean (u), sum (u): u (2 |a| + |b| + |a + b|) + m mean_abs.
    rv    unb = q / (P - 1) (u): m (var_abs P / (P - 1) + u unb) on top of the same form."""
    x = _d(x)
    mean = x.mean(0)
    dev = np.abs(x - mean)
    var = (dev ** 2).mean(0)
    M, D, madev = np.abs(x).max(0), 2 * dev.max(0), dev.mean(0)
    nblk, _ = red_geom(C, P)
    r = run_len(C, P)
    levels = (lanes_of(C), -(-nblk // 16), 16)
    depth = r + lanes_of(C) - 1 + stage2_depth(nblk)
    m_cost = (r + 1) / 2 + sum((K + 2) / 2 for K in levels if K > 1)
    d_cost = 1 + 2 * sum(sum(1.0 / k for k in range(2, K + 1)) for K in levels)
    b = dict(mean=U * (M * m_cost + 3 * D * d_cost))
    var_abs = U * ((depth + 7) * var + 4 * M * madev)
    b["var_rel"] = var_abs / (var + EPS) + 7 * U
    if rm is not None:
        m = f32(momentum)
        a, bb = (1 - m) * _d(rm), m * mean
        b["rm"] = U * (2 * np.abs(a) + np.abs(bb) + np.abs(a + bb)) + m * b["mean"]
        unb = var * P / (P - 1) if P > 1 else var
        a, bb = (1 - m) * _d(rv), m * unb
        b["rv"] = U * (2 * np.abs(a) + np.abs(bb) + np.abs(a + bb)) + m * (var_abs * P / max(P - 1, 1) + U * unb)
    return b


def apply_bound(z, mean, rstd, gamma, beta):
    """y = relu((z - mu) a + b), a = fl(rstd gamma): z - mu (u), a (u), product (u) on t = (z - mu) rstd
    gamma, the add (u) on t + beta; max is exact.  u (3 |t| + |t + beta|), element by element."""
    t = (_d(z) - _d(mean)) * _d(rstd) * _d(gamma)
    return U * (3 * np.abs(t) + np.abs(t + _d(beta)))


def reduce_bounds(dy, y, z, mean, rstd, C, P):
    """-> (dgamma bound, dbeta bound) per channel.
    depth = (r - 1) + (lanes - 1) + part_depth(nblk) adds, cut to the channel's nonzero terms - 1.
    dbeta   terms g are exact (a select): depth u sum |g|.
    dgamma  term g xh, xh = fl(fl(z - mu) rs): 3 u on each: (depth + 3) u sum |g xh|."""
    g, xh = bn_bwd_terms(dy, y, z, mean, rstd)
    nblk, _ = red_geom(C, P)
    depth = run_len(C, P) - 1 + lanes_of(C) - 1 + part_depth(nblk)
    return (_nnz_depth(depth, g * xh) + 3) * U * np.abs(g * xh).sum(0), _nnz_depth(depth, g) * U * np.abs(g).sum(0)


def dx_bound(dy, y, z, mean, rstd, gamma, dgamma, dbeta):
    """dz = a (g - kb - xh kg): invP = fl(1 / P) (u), kb = fl(dbeta invP) (u): 2 u |kb|; kg alike, xh = fl(fl(z -
    mu) rs) (2 u), xh kg (u): 5 u |xh kg|; g - kb (u |g - kb|); - xh kg (u |s|); a = fl(gamma rs) (u), a s (u):
    3 u |s| in all.  |a| u (2 |kb| + 5 |xh kg| + |g - kb| + 3 |s|), element by element."""
    g, xh = bn_bwd_terms(dy, y, z, mean, rstd)
    P = g.shape[0]
    kb, t = _d(dbeta) / P, xh * _d(dgamma) / P
    s = g - kb - t
    return np.abs(_d(gamma) * _d(rstd)) * U * (2 * np.abs(kb) + 5 * np.abs(t) + np.abs(g - kb) + 3 * np.abs(s))


def up_weight_err(n):
    """|fp32 weight - exact weight| of one row: s = fl(fl((n - 1) / (2n - 1)) o) carries 2 u s <= 2 u (n - 1),
    which moves l1 by as much (also across an integer: the two rows of weights then differ by that in three
    entries); l0 = fl(1 - l1) adds u."""
    return U * (2 * max(n - 1, 0) + 1)


def up_support(Ua, Ub):
    return ((Ua != 0) | (Ub != 0)).astype(np.float64)


FWD_ROUNDINGS = 5    # ly (lx a + lx b) + ...: product, product, add, product, add per term
BWD_ROUNDINGS = 16   # wy = l0 + l1 (1), v wx (1), a row's chain of at most 6 nonzero columns (6), racc wy (1),
                     # the rows' chain (6), one spare: at most 6 x 6 terms since src moves >= 1/3 per output


def up_fwd_bounds(x, h, w):
    """-> (bound against the fp32-weight matrices, bound against the exact ones).  The second adds the weight
    error of each dimension over the entries either matrix uses."""
    ax = np.abs(_d(x))
    Uy, Ux, Vy, Vx = up_matrix(h), up_matrix(w), up_matrix_f32(h), up_matrix_f32(w)
    tight = FWD_ROUNDINGS * U * up_fwd(ax, np.abs(Vy), np.abs(Vx))
    Ey, Ex = up_weight_err(h) * up_support(Uy, Vy), up_weight_err(w) * up_support(Ux, Vx)
    wide = tight + up_fwd(ax, Ey, np.abs(Ux) + Ex) + up_fwd(ax, np.abs(Uy), Ex)
    return tight, wide


def up_bwd_bounds(v, h, w):
    av = np.abs(_d(v))
    Uy, Ux, Vy, Vx = up_matrix(h), up_matrix(w), up_matrix_f32(h), up_matrix_f32(w)
    tight = BWD_ROUNDINGS * U * up_bwd(av, np.abs(Vy), np.abs(Vx))
    Ey, Ex = up_weight_err(h) * up_support(Uy, Vy), up_weight_err(w) * up_support(Ux, Vx)
    wide = tight + up_bwd(av, Ey, np.abs(Ux) + Ex) + up_bwd(av, np.abs(Uy), Ex)
    return tight, wide


# ===================================================================== fp32 emulations
def _chan(na, ma, qa, nb, mb, qb):
    """bn_train.hip chan(): a <- a (+) b, element-wise over arrays; counts broadcast."""
    na, nb = np.broadcast_to(F(na), ma.shape).astype(F), np.broadcast_to(F(nb), ma.shape).astype(F)
    with np.errstate(divide="ignore", invalid="ignore"):
        n = (na + nb).astype(F)
        d = (mb - ma).astype(F)
        fb = (nb / n).astype(F)
        m2 = (ma + (d * fb).astype(F)).astype(F)
        q2 = (qa + (qb + ((d * d).astype(F) * (na * fb).astype(F)).astype(F)).astype(F)).astype(F)
    skip, take = nb == 0, (na == 0) & (nb != 0)
    return (np.where(skip, na, n).astype(F), np.where(skip, ma, np.where(take, mb, m2)).astype(F),
            np.where(skip, qa, np.where(take, qb, q2)).astype(F))


def _thread_index(C, P):
    """-> idx [nblk][lanes][r] pixel of (block, lane, step) and its validity mask."""
    lanes = lanes_of(C)
    nblk, per = red_geom(C, P)
    r = -(-per // lanes)
    b, l, k = np.arange(nblk)[:, None, None], np.arange(lanes)[None, :, None], np.arange(r)[None, None, :]
    idx = b * per + l + k * lanes
    ok = idx < np.minimum(P, (b + 1) * per)
    return np.where(ok, idx, 0), ok


def emu_stats(x, C, P, rm=None, rv=None, momentum=MOMENTUM, mutant=None):
    x = np.asarray(x, dtype=F)
    lanes = lanes_of(C)
    nblk, per = red_geom(C, P)
    idx, ok = _thread_index(C, P)
    shape = (nblk, lanes, C)
    mean, m2, n = np.zeros(shape, F), np.zeros(shape, F), np.zeros((nblk, lanes, 1), F)
    if mutant == "subtractive":
        s1 = np.zeros(C, F)
        s2 = np.zeros(C, F)
        for p in range(P):
            s1 = (s1 + x[p]).astype(F)
            s2 = (s2 + (x[p] * x[p]).astype(F)).astype(F)
        m = (s1 / F(P)).astype(F)
        q = ((s2 / F(P)).astype(F) - (m * m).astype(F)).astype(F) * F(P)
        return _stats_tail(m, np.maximum(q, 0).astype(F), P, rm, rv, momentum, mutant)
    for k in range(idx.shape[2]):
        v, o = x[idx[:, :, k]], ok[:, :, k, None]
        n1 = (n + F(1)).astype(F)
        d = (v - mean).astype(F)
        mn = (mean + (d * (F(1) / n1).astype(F)).astype(F)).astype(F)
        qn = (m2 + (d * (v - mn).astype(F)).astype(F)).astype(F)
        mean, m2, n = np.where(o, mn, mean), np.where(o, qn, m2), np.where(o, n1, n)
    nb_, mb_, qb_ = n[:, 0], mean[:, 0], m2[:, 0]
    top = lanes - 1 if mutant == "lane_dropped" else lanes
    for l in range(1, top):
        nb_, mb_, qb_ = _chan(nb_, mb_, qb_, n[:, l], mean[:, l], m2[:, l])
    if mutant == "idle_garbage":   # an idle thread's LDS slot (never written: here 1.0 / 1 pixel) merged in
        nb_, mb_, qb_ = _chan(nb_, mb_, qb_, F(1), np.ones_like(mb_), np.zeros_like(qb_))
    # stage 2
    cnt = np.minimum(P, (np.arange(nblk) + 1) * per) - np.arange(nblk) * per
    if mutant == "ragged_full":
        cnt = np.full(nblk, per)
    N, Mn, Q = np.zeros((16, C), F), np.zeros((16, C), F), np.zeros((16, C), F)
    for j in range(16):
        b0, b1 = nblk * j // 16, nblk * (j + 1) // 16
        if mutant == "segment_skipped" and b1 > b0 and b1 == nblk:
            b1 -= 1                    # ceil in place of floor in b0 of the last non-empty segment
        for b in range(b0, b1):
            N[j:j + 1], Mn[j:j + 1], Q[j:j + 1] = _chan(N[j:j + 1], Mn[j:j + 1], Q[j:j + 1], F(cnt[b]),
                                                        mb_[b:b + 1], qb_[b:b + 1])
    nn, m, q = N[0:1], Mn[0:1], Q[0:1]
    for k in range(1, 16):
        nn, m, q = _chan(nn, m, q, N[k:k + 1], Mn[k:k + 1], Q[k:k + 1])
    return _stats_tail(m[0], q[0], P, rm, rv, momentum, mutant)


def _stats_tail(m, q, P, rm, rv, momentum, mutant):
    var = (q / F(P)).astype(F)
    unb = (q / F(P - 1)).astype(F) if P > 1 else var
    eps = F(1e-5)
    if mutant == "eps_outside":
        rstd = (F(1) / (np.sqrt(var).astype(F) + eps).astype(F)).astype(F)
    else:
        rstd = (F(1) / np.sqrt(((unb if mutant == "unbiased_rstd" else var) + eps).astype(F)).astype(F)).astype(F)
    out = dict(mean=m.astype(F), rstd=rstd)
    if rm is not None:
        mo = F(momentum)
        keep, new = F(F(1) - mo), mo
        if mutant == "momentum_old":
            keep, new = new, keep
        stat = var if mutant == "biased_running" else unb
        out["rm"] = ((keep * np.asarray(rm, F)).astype(F) + (new * m).astype(F)).astype(F)
        out["rv"] = ((keep * np.asarray(rv, F)).astype(F) + (new * stat).astype(F)).astype(F)
    return out


def emu_apply_relu(z, mean, rstd, gamma, beta, C, P):
    z, mu = np.asarray(z, F), np.asarray(mean, F)
    a = (np.asarray(rstd, F) * np.asarray(gamma, F)).astype(F)
    y = np.maximum((((z - mu).astype(F) * a).astype(F) + np.asarray(beta, F)).astype(F), F(0))
    assert (ew_cover(C, P) == 1).all()
    return y


def _gate(dy, y, z, mutant):
    y, z = np.asarray(y, F), np.asarray(z, F)
    keep = y >= 0 if mutant == "gate_ge" else (z > 0 if mutant == "gate_z" else y > 0)
    return np.where(keep, np.asarray(dy, F), F(0)).astype(F)


def _part_reduce(part):
    """part_reduce_kernel over part [nblk][C]."""
    nblk, C = part.shape
    red = np.zeros((16, C), F)
    for wv in range(16):
        acc = [np.zeros(C, F) for _ in range(4)]
        b = wv
        while b + 48 < nblk:
            for i in range(4):
                acc[i] = (acc[i] + part[b + 16 * i]).astype(F)
            b += 64
        while b < nblk:
            acc[0] = (acc[0] + part[b]).astype(F)
            b += 16
        red[wv] = ((acc[0] + acc[1]).astype(F) + (acc[2] + acc[3]).astype(F)).astype(F)
    s = np.zeros(C, F)
    for k in range(16):
        s = (s + red[k]).astype(F)
    return s


def emu_bwd_reduce(dy, y, z, mean, rstd, C, P, mutant=None):
    lanes = lanes_of(C)
    nblk, _ = red_geom(C, P)
    idx, ok = _thread_index(C, P)
    g = _gate(dy, y, z, mutant)
    xh = ((np.asarray(z, F) - np.asarray(mean, F)).astype(F) * np.asarray(rstd, F)).astype(F)
    gx = (g * xh).astype(F)
    dg, db = np.zeros((nblk, lanes, C), F), np.zeros((nblk, lanes, C), F)
    for k in range(idx.shape[2]):
        o = ok[:, :, k, None]
        db = np.where(o, (db + g[idx[:, :, k]]).astype(F), db)
        dg = np.where(o, (dg + gx[idx[:, :, k]]).astype(F), dg)
    pg, pb = dg[:, 0], db[:, 0]
    top = lanes - 1 if mutant == "lane_dropped" else lanes
    for l in range(1, top):
        pg, pb = (pg + dg[:, l]).astype(F), (pb + db[:, l]).astype(F)
    if mutant == "idle_garbage":
        pg, pb = (pg + F(1)).astype(F), (pb + F(1)).astype(F)
    if mutant == "block_dropped":
        pg, pb = pg[:-1] if nblk > 1 else pg * 0, pb[:-1] if nblk > 1 else pb * 0
    return _part_reduce(pg), _part_reduce(pb)


def emu_bwd_dx(dy, y, z, mean, rstd, gamma, dgamma, dbeta, C, P, mutant=None):
    g = _gate(dy, y, z, mutant)
    mu, rs = np.asarray(mean, F), np.asarray(rstd, F)
    a = (np.asarray(gamma, F) * rs).astype(F)
    Pw = red_geom(C, P)[0] * red_geom(C, P)[1] if mutant == "wrong_P" else P
    invP = F(1) / F(Pw)
    kb, kg = (np.asarray(dbeta, F) * invP).astype(F), (np.asarray(dgamma, F) * invP).astype(F)
    xh = ((np.asarray(z, F) - mu).astype(F) * rs).astype(F)
    s = g
    if mutant != "no_dbeta":
        s = (s - kb).astype(F)
    if mutant != "no_dgamma":
        s = (s - (xh * kg).astype(F)).astype(F)
    assert (ew_cover(C, P) == 1).all()
    return ((rs if mutant == "no_gamma" else a) * s).astype(F)


def _emu_weights(n, o, mutant):
    """fp32 (i0, ip, l0, l1) of output index o (arrays) as both upsample kernels compute them."""
    r = F(n - 1) / F(2 * n - 1) if 2 * n > 1 else F(0)
    s = (r * o.astype(F)).astype(F)
    if mutant == "half_pixel":
        s = np.maximum(F(0), ((o.astype(F) + F(0.5)).astype(F) * F(0.5)).astype(F) - F(0.5)).astype(F)
    i0 = s.astype(np.int64)
    ip = np.where(i0 < n - 1, 1, 0)
    if mutant == "no_clamp":
        ip = np.ones_like(i0)
    l1 = (s - i0.astype(F)).astype(F)
    l0 = (F(1) - l1).astype(F)
    if mutant == "swap":
        l0, l1 = l1, l0
    return i0, ip, l0, l1


def emu_up_fwd(x, mutant=None, after=SENTINEL):
    """x [N][h][w][C] fp32 -> [N][2h][2w][C].  A read past the tensor (mutant no_clamp) sees `after`."""
    x = np.asarray(x, F)
    N, h, w, C = x.shape
    flat = np.concatenate([x.reshape(N * h * w, C), np.full((w + 2, C), after, F)])
    y0, yp, ly0, ly1 = _emu_weights(h, np.arange(2 * h), mutant)
    x0, xp, lx0, lx1 = _emu_weights(w, np.arange(2 * w), mutant)
    n = np.arange(N)[:, None, None]
    base = (n * h + y0[None, :, None]) * w + x0[None, None, :]
    a, b = flat[base], flat[base + xp[None, None, :]]
    d, e = flat[base + yp[None, :, None] * w], flat[base + yp[None, :, None] * w + xp[None, None, :]]
    lx0, lx1 = lx0[None, None, :, None], lx1[None, None, :, None]
    ly0, ly1 = ly0[None, :, None, None], ly1[None, :, None, None]
    with np.errstate(over="ignore", invalid="ignore"):
        top = ((lx0 * a).astype(F) + (lx1 * b).astype(F)).astype(F)
        bot = ((lx0 * d).astype(F) + (lx1 * e).astype(F)).astype(F)
        return ((ly0 * top).astype(F) + (ly1 * bot).astype(F)).astype(F)


def _emu_bwd_w(n, mutant, lo, hi):
    """wk [n][8]: weight of candidate o = 2 i - 3 + k for low index i; candidates outside [lo, hi) dropped."""
    i = np.arange(n)[:, None]
    o = 2 * i - 3 + np.arange(8)[None, :]
    ok = (o >= 0) & (o < 2 * n) & (np.arange(8)[None, :] >= lo) & (np.arange(8)[None, :] < hi)
    oc = np.clip(o, 0, 2 * n - 1)
    i0, ip, l0, l1 = _emu_weights(n, oc.ravel(), mutant)
    i0, ip, l0, l1 = (t.reshape(o.shape) for t in (i0, ip, l0, l1))
    wk = (np.where(i0 == i, l0, F(0)).astype(F) + np.where(i0 + ip == i, l1, F(0)).astype(F)).astype(F)
    return np.where(ok, wk, F(0)).astype(F), oc


def emu_up_bwd(v, mutant=None):
    """v [N][2h][2w][C] fp32 -> [N][h][w][C] in upsample2x_bwd_kernel's order."""
    v = np.asarray(v, F)
    N, H2, W2, C = v.shape
    h, w = H2 // 2, W2 // 2
    lo = {"window_1short_lo": 1, "window_short_lo": 3}.get(mutant, 0)
    hi = {"window_1short_hi": 7, "window_short_hi": 5}.get(mutant, 8)
    wy, oy = _emu_bwd_w(h, mutant, lo, hi)
    wx, ox = _emu_bwd_w(w, mutant, lo, hi)
    acc = np.zeros((N, h, w, C), F)
    for ky in range(8):
        racc = np.zeros((N, h, w, C), F)
        rows = v[:, oy[:, ky]]                      # [N][h][2w][C]
        for kx in range(8):
            t = (rows[:, :, ox[:, kx]] * wx[None, None, :, kx, None]).astype(F)
            racc = np.where(wx[None, None, :, kx, None] != 0, (racc + t).astype(F), racc)
        t = (racc * wy[None, :, ky, None, None]).astype(F)
        acc = np.where(wy[None, :, ky, None, None] != 0, (acc + t).astype(F), acc)
    return acc


# ===================================================================== cases and inputs
CHANNELS = (4, 12, 20, 48, 64, 128, 256, 516, 1024)


def pixel_counts(C):
    """One P per class for this C's lane count: 1, 2, lanes - 1, 16 lanes -/+ 1 (the last pixel that keeps
    one stage-1 block, the first that makes two), 2 <= nblk < 16 with a ragged last block, nblk >= 17 and no
    multiple of 16."""
    lanes = lanes_of(C)
    out = []
    for P in (1, 2, lanes - 1, 16 * lanes - 1, 16 * lanes + 1, 16 * lanes * 5 + 3, 16 * lanes * 19 + 5):
        if P >= 1 and P not in out:
            out.append(P)
    return out


CAP_CASE = (516, 16 * BN_MAX_BLOCKS + 16)   # lanes 1: past kBnMaxBlocks (per = 17, 965 blocks, the last of 12) and
                                            # past ew_blocks' 4096 blocks x 4 pixels


def bn_cases():
    """Every (C, P) the GPU test launches: each lanes class x each P class, and the cap case."""
    return [(C, P) for C in CHANNELS for P in pixel_counts(C)] + [CAP_CASE]


def case_class(C, P):
    nblk, per = red_geom(C, P)
    return dict(lanes=lanes_of(C), nblk=nblk, per=per, ragged=P % per != 0, ew=ew_blocks(C, P))


def _key(C, P, what):
    return f"bnk.{what}.{C}.{P}"


def bn_inputs(C, P, kind="plain"):
    """fp32 operands of ops 0-3 for one case.
    plain    z = 3 + 2 n + 1.5 p / P (a trend, so that stage-1 blocks differ in mean and a wrong block weight
             shows); channel 1 is constant (variance exactly 0); gamma = 1 + 0.3 u, beta = 0.3 u with beta[2] = 0;
             dy normal; y = the model's y in fp32 with exact zeros planted over positive values on every 3rd
             pixel of the channels c % 4 == 2 (+0.0) and c % 4 == 3 (-0.0), where dy is not 0.
    bigmean  z = 64 + 0.05 n: |mean| >> std."""
    n = hash_normal(_key(C, P, "z"), (P, C)).astype(np.float64)
    if kind == "bigmean":
        z = (64.0 + 0.05 * n).astype(F)
    else:
        z = (3.0 + 2.0 * n + 1.5 * np.arange(P)[:, None] / P).astype(F)
        z[:, 1] = F(0.75)
    dy = hash_normal(_key(C, P, "dy"), (P, C)).astype(F)
    dy[dy == 0] = F(0.5)
    gamma = (1.0 + 0.3 * hash_uniform(_key(C, P, "g"), C)).astype(F)
    beta = (0.3 * hash_uniform(_key(C, P, "b"), C)).astype(F)
    beta[2] = F(0)
    st = bn_stats(z)
    mean, rstd = st["mean"].astype(F), st["rstd"].astype(F)
    y = bn_apply_relu(z, mean, rstd, gamma, beta).astype(F)
    ties = np.zeros((P, C), bool)
    ties[::3, 2::4] = True
    ties[::3, 3::4] = True
    y[::3, 2::4] = F(0.0)
    y[::3, 3::4] = F(-0.0)
    dgamma, dbeta = bn_bwd_reduce(dy, y, z, mean, rstd)
    rm = (0.5 * hash_uniform(_key(C, P, "rm"), C)).astype(F)
    rv = (1.0 + 0.5 * np.abs(hash_uniform(_key(C, P, "rv"), C))).astype(F)
    return dict(z=z, dy=dy, gamma=gamma, beta=beta, mean=mean, rstd=rstd, y=y, ties=ties,
                dgamma=dgamma.astype(F), dbeta=dbeta.astype(F), rm=rm, rv=rv)


def onehot_targets(C, P):
    """Pixels a one-hot dy must visit: one in every lane (of block l % nblk, at step l % its run), one in every
    stage-1 block, the first and the last pixel."""
    lanes = lanes_of(C)
    nblk, per = red_geom(C, P)
    t = []
    for l in range(lanes):
        b = l % nblk
        p1 = min(P, (b + 1) * per)
        steps = max(1, -(-(p1 - b * per - l) // lanes))
        p = b * per + l + (l % steps) * lanes
        if p < p1:
            t.append(p)
    for b in range(nblk):
        t.append(min(P, (b + 1) * per) - 1)
    return t + [0, P - 1]


def onehot_rounds(C, P):
    """-> list of dy [P][C], each with one nonzero per channel; together they visit onehot_targets."""
    t = onehot_targets(C, P)
    rounds = []
    for i in range(0, len(t), C):
        dy = np.zeros((P, C), F)
        for c in range(C):
            dy[t[(i + c) % len(t)], c] = F(1.5 + 0.25 * (c % 5))
        rounds.append(dy)
    return rounds


ONEHOT_CASES = [(C, pixel_counts(C)[-1]) for C in CHANNELS] + [(64, 16 * 16 * 5 + 3), (12, 84)]

UP_SIZES = ((1, 1), (1, 5), (5, 1), (2, 2), (2, 7), (3, 5), (8, 8), (17, 33), (96, 130))


def up_cases():
    """(N, C, h, w): every size, N in {1, 3} and C in {4, 20, 64, 256} each met by several sizes."""
    ncs = ((1, 4), (3, 20), (1, 64), (3, 256), (3, 4), (1, 20), (3, 64), (1, 256), (1, 4))
    return [(N, C, h, w) for (h, w), (N, C) in zip(UP_SIZES, ncs)]


BWD_CAP_CASE = (1, 4, 1025, 2048)    # N h w C / 4 = 8192 x 256 + 2048 threads' worth: a second grid-stride trip
FWD_CAP_CASE = (1, 4, 2049, 2048)    # N 2h 2w C / 4 = 65536 x 256 + 8192


def up_inputs(N, C, h, w):
    x = hash_normal(f"bnk.upx.{N}.{C}.{h}.{w}", (N, h, w, C)).astype(F)
    v = hash_normal(f"bnk.upv.{N}.{C}.{h}.{w}", (N, 2 * h, 2 * w, C)).astype(F)
    return x, v


def up_onehot_positions(h, w):
    """Output pixels for a one-hot v: the four corners and, around the middle, every row / column parity."""
    H2, W2 = 2 * h, 2 * w
    pos = {(0, 0), (0, W2 - 1), (H2 - 1, 0), (H2 - 1, W2 - 1)}
    for dy in range(4):
        for dx in range(4):
            pos.add((min(H2 - 1, max(0, h - 2 + dy)), min(W2 - 1, max(0, w - 2 + dx))))
    return sorted(pos)


def ratio(err, bound):
    """max err / bound over the elements, 0 / 0 = 0 and x / 0 = inf."""
    err, bound = np.abs(_d(err)), np.broadcast_to(_d(bound), np.shape(err))
    with np.errstate(divide="ignore", invalid="ignore"):
        r = np.where(err == 0, 0.0, err / bound)
    return float(np.max(r)) if r.size else 0.0


def bn_ratios(t, C, P, got, momentum=MOMENTUM):
    """error / bound per quantity for the outputs `got` (a dict; absent keys are skipped) of ops 0-3 on
    the inputs t = bn_inputs(...)."""
    r = {}
    if "mean" in got:
        st = bn_stats(t["z"], t["rm"], t["rv"], momentum)
        b = stats_bounds(t["z"], C, P, t["rm"], t["rv"], momentum)
        r["mean"] = ratio(_d(got["mean"]) - st["mean"], b["mean"])
        ve = st["var"] + EPS
        r["rstd"] = ratio((1.0 / _d(got["rstd"]) ** 2 - ve) / ve, b["var_rel"])
        if "rm" in got:
            r["rm"] = ratio(_d(got["rm"]) - st["rm"], b["rm"])
            r["rv"] = ratio(_d(got["rv"]) - st["rv"], b["rv"])
    ops = (t["dy"], t["y"], t["z"], t["mean"], t["rstd"])
    if "y" in got:
        a = (t["z"], t["mean"], t["rstd"], t["gamma"], t["beta"])
        r["y"] = ratio(_d(got["y"]) - bn_apply_relu(*a), apply_bound(*a))
    if "dgamma" in got:
        dg, db = bn_bwd_reduce(*ops)
        bg, bb = reduce_bounds(*ops, C, P)
        r["dgamma"], r["dbeta"] = ratio(_d(got["dgamma"]) - dg, bg), ratio(_d(got["dbeta"]) - db, bb)
    if "dz" in got:
        a = ops + (t["gamma"], t["dgamma"], t["dbeta"])
        r["dz"] = ratio(_d(got["dz"]) - bn_bwd_dx(*a), dx_bound(*a))
    return r


def emu_all(t, C, P, momentum=MOMENTUM, mutant=None, only=None):
    """The emulations' outputs in bn_ratios' form; a mutant name goes to the ops that know it."""
    sm = mutant if mutant in STATS_MUTANTS else None
    rm_ = mutant if mutant in REDUCE_MUTANTS else None
    dm = mutant if mutant in DX_MUTANTS else None
    got = {}
    if only in (None, "stats"):
        got.update(emu_stats(t["z"], C, P, t["rm"], t["rv"], momentum, mutant=sm))
    if only in (None, "apply"):
        got["y"] = emu_apply_relu(t["z"], t["mean"], t["rstd"], t["gamma"], t["beta"], C, P)
    if only in (None, "reduce"):
        got["dgamma"], got["dbeta"] = emu_bwd_reduce(t["dy"], t["y"], t["z"], t["mean"], t["rstd"], C, P, mutant=rm_)
    if only in (None, "dx"):
        got["dz"] = emu_bwd_dx(t["dy"], t["y"], t["z"], t["mean"], t["rstd"], t["gamma"], t["dgamma"], t["dbeta"],
                               C, P, mutant=dm)
    return got


STATS_MUTANTS = ("biased_running", "unbiased_rstd", "eps_outside", "momentum_old", "ragged_full", "segment_skipped",
                 "lane_dropped", "idle_garbage", "subtractive")
REDUCE_MUTANTS = ("gate_ge", "gate_z", "lane_dropped", "idle_garbage", "block_dropped")
DX_MUTANTS = ("gate_ge", "gate_z", "no_dbeta", "no_dgamma", "no_gamma", "wrong_P")


def up_rows(n, f32_weights=False):
    """The matrix of up_matrix / up_matrix_f32 as its two entries per row: (i0, i1, l0, l1) arrays of 2n."""
    Um = up_matrix_f32(n) if f32_weights else up_matrix(n)
    i0 = np.array([int(np.nonzero(Um[o])[0][0]) for o in range(2 * n)])
    i1 = np.minimum(i0 + 1, n - 1)
    l0 = Um[np.arange(2 * n), i0]
    l1 = np.where(i1 > i0, Um[np.arange(2 * n), i1], 0.0)
    return i0, i1, l0, l1

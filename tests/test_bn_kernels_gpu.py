"""The batch-statistics BatchNorm kernels and the bilinear x2 pair, one launch each through kdlae_debug_bn
ops 0-5, against the float64 models and counted bounds of tests/bn_kernel_refs.py (proven, with their
mutants, by tests/test_bn_kernel_refs.py).

Grid: every C of {4, 12, 20, 48, 64, 128, 256, 516, 1024} (lanes 256, 85, 51, 21, 16, 8, 4, 1, 1) meets every
P class of its lane count (1, 2, lanes - 1, 16 lanes -/+ 1, 2 <= nblk < 16 with a ragged last block, nblk
>= 17 and no multiple of 16); one case (C 516, P 16400) is past both the kBnMaxBlocks cap of the reductions
and the 4096-block cap of the element-wise kernels.  Every op is launched alone on host-built operands (the
same bits the CPU emulation saw), so each quantity has its own bound; RATIO lines print error / bound.

Every view has its own pixel stride and sits in storage filled with 1e30 at a 16-byte aligned offset; pad
columns and surround are checked bit-unchanged, every call is made twice with equal bits.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import bn_kernel_refs as R
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd._lib import BnDesc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENT = R.SENTINEL
OFF, TAIL = 8, 12


def _call(op, **kw):
    d = BnDesc()
    d.op = op
    for k, v in kw.items():
        setattr(d, k, v)
    rc = _lib.lib().kdlae_debug_bn(ctypes.byref(d), None)
    torch.cuda.synchronize()
    return rc


def _bn(op, **kw):
    _lib.check(_call(op, **kw), f"kdlae_debug_bn op {op}")


class View:
    """[P][C] at pixel stride ld inside 1e30-filled storage, OFF floats in (16-byte aligned)."""

    def __init__(self, P, C, ld, vals=None, off=OFF, col=0, fill=SENT):
        self.P, self.C, self.ld, self.off, self.col = P, C, ld, off, col
        self.s = torch.full((off + P * ld + TAIL,), fill, device=DEV)
        self.inside = torch.zeros(self.s.numel(), dtype=torch.bool, device=DEV)
        self.inside[off:off + P * ld].view(P, ld)[:, col:col + C] = True
        if vals is not None:
            self.rows()[:] = torch.from_numpy(np.ascontiguousarray(vals, dtype=np.float32).reshape(P, C)).to(DEV)
        self.before = self.s.clone()

    @property
    def ptr(self):
        return self.s.data_ptr() + 4 * (self.off + self.col)

    def rows(self):
        return self.s[self.off:self.off + self.P * self.ld].view(self.P, self.ld)[:, self.col:self.col + self.C]

    def get(self):
        return self.rows().cpu().numpy()

    def outside_unchanged(self):
        o = ~self.inside
        return torch.equal(self.s[o].view(torch.int32), self.before[o].view(torch.int32))

    def unchanged(self):
        return torch.equal(self.s.view(torch.int32), self.before.view(torch.int32))


def _vec(vals=None, C=None):
    return View(1, C if vals is None else len(vals), (C if vals is None else len(vals)) + 4, vals)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@functools.lru_cache(maxsize=4)
def _inputs(C, P, kind="plain"):
    return R.bn_inputs(C, P, kind)


def _report(r, tag):
    for k, v in sorted(r.items()):
        print(f"RATIO {k} {v:.4f} ({tag})")
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f"{tag}: error / bound above 1: {bad}"


def _run_ops(C, P, t, stats_only=False):
    """Ops 0-3 on the inputs t; returns bn_ratios' `got` dict after the bit-level checks."""
    got = {}
    part = View(1, 2048 * C, 2048 * C)
    z = View(P, C, C + 4, t["z"])
    stats = []
    for mom, running in ((R.MOMENTUM, True), (R.MOMENTUM, True), (R.MOMENTUM, False), (0.3, True)):
        mean, rstd = _vec(C=C), _vec(C=C)
        rm, rv = _vec(t["rm"]), _vec(t["rv"])
        _bn(0, x=z.ptr, ldx=z.ld, C=C, P=P, mean=mean.ptr, rstd=rstd.ptr, running_mean=rm.ptr if running else None,
            running_var=rv.ptr if running else None, momentum=mom, part=part.ptr, part_floats=2048 * C)
        assert z.unchanged() and mean.outside_unchanged() and rstd.outside_unchanged() and part.outside_unchanged()
        assert rm.outside_unchanged() and rv.outside_unchanged()
        if not running:
            assert rm.unchanged() and rv.unchanged()
        stats.append(dict(mean=mean.get()[0], rstd=rstd.get()[0], rm=rm.get()[0], rv=rv.get()[0]))
    for k in ("mean", "rstd", "rm", "rv"):
        assert np.array_equal(_bits(stats[0][k]), _bits(stats[1][k])), f"bn_stats {k}: two calls differ"
    for s in stats[2:]:   # null running statistics and another momentum: the same mean / rstd bits
        assert np.array_equal(_bits(s["mean"]), _bits(stats[0]["mean"])) and np.array_equal(_bits(s["rstd"]), _bits(stats[0]["rstd"]))
    got.update(stats[0])
    r3 = R.bn_ratios(t, C, P, stats[3], 0.3)
    got["_mom03"] = {k: r3[k] for k in ("rm", "rv")}
    if "plain" in t.get("kind", "plain"):
        assert np.array_equal(_bits(stats[0]["mean"][1]), _bits(np.float32(0.75))), "constant channel: mean not exact"
    if P == 1:
        assert np.array_equal(_bits(stats[0]["mean"]), _bits(t["z"][0]))
    if stats_only:
        return got
    vm, vr, vg, vb = _vec(t["mean"]), _vec(t["rstd"]), _vec(t["gamma"]), _vec(t["beta"])
    ys = []
    for _ in range(2):
        y = View(P, C, C + 8)
        _bn(1, x=z.ptr, ldx=z.ld, mean=vm.ptr, rstd=vr.ptr, gamma=vg.ptr, beta=vb.ptr, C=C, P=P, out=y.ptr, ldo=y.ld)
        assert y.outside_unchanged() and z.unchanged()
        ys.append(y.get())
    assert np.array_equal(_bits(ys[0]), _bits(ys[1])), "bn_apply_relu: two calls differ"
    got["y"] = ys[0]
    yv, dy = View(P, C, C + 8, t["y"]), View(P, C, C + 12, t["dy"])
    sums = []
    for _ in range(2):
        dg, db = _vec(C=C), _vec(C=C)
        _bn(2, dy=dy.ptr, ldd=dy.ld, y=yv.ptr, ldy=yv.ld, x=z.ptr, ldx=z.ld, mean=vm.ptr, rstd=vr.ptr, C=C, P=P,
            dgamma=dg.ptr, dbeta=db.ptr, part=part.ptr, part_floats=2048 * C)
        assert dg.outside_unchanged() and db.outside_unchanged() and part.outside_unchanged()
        assert dy.unchanged() and yv.unchanged()
        sums.append((dg.get()[0], db.get()[0]))
    assert all(np.array_equal(_bits(a), _bits(b)) for a, b in zip(*sums)), "bn_bwd_reduce: two calls differ"
    got["dgamma"], got["dbeta"] = sums[0]
    vdg, vdb = _vec(t["dgamma"]), _vec(t["dbeta"])
    common = dict(y=yv.ptr, ldy=yv.ld, x=z.ptr, ldx=z.ld, mean=vm.ptr, rstd=vr.ptr, gamma=vg.ptr, dgamma=vdg.ptr,
                  dbeta=vdb.ptr, C=C, P=P)
    dzs = []
    for inplace in (False, False, True, True):
        if inplace:   # as layer_bwd calls it: dz == dy, same stride
            o = View(P, C, dy.ld, t["dy"])
            _bn(3, dy=o.ptr, ldd=o.ld, out=o.ptr, ldo=o.ld, **common)
        else:
            o = View(P, C, C + 16)
            _bn(3, dy=dy.ptr, ldd=dy.ld, out=o.ptr, ldo=o.ld, **common)
            assert dy.unchanged()
        assert o.outside_unchanged() and yv.unchanged() and z.unchanged()
        dzs.append(o.get())
    for k in range(1, 4):
        assert np.array_equal(_bits(dzs[0]), _bits(dzs[k])), "bn_bwd_dx: in place / out of place / twice differ"
    got["dz"] = dzs[0]
    return got


@pytest.mark.parametrize("C,P", R.bn_cases(), ids=lambda v: str(v))
def test_bn_ops(C, P):
    """Ops 0-3 at one (C, P) of the grid (or the cap case): plain inputs with a trend over the pixels, a
    constant channel (variance exactly 0, mean exact), planted y == +0.0 / -0.0 where dy != 0; running
    statistics from nonzero values at momentum 0.1 and 0.3 and with null pointers; bn_bwd_dx in place."""
    t = _inputs(C, P)
    got = _run_ops(C, P, t)
    m03 = got.pop("_mom03")
    r = R.bn_ratios(t, C, P, got)
    r.update({k + "_mom0.3": v for k, v in m03.items()})
    # the planted ties: where y is +0.0 or -0.0 the incoming gradient takes no part (dy there is not 0)
    ties = t["ties"]
    no_g = R.bn_bwd_dx(np.zeros_like(t["dy"]), t["y"], t["z"], t["mean"], t["rstd"], t["gamma"], t["dgamma"], t["dbeta"])
    bound = R.dx_bound(t["dy"], t["y"], t["z"], t["mean"], t["rstd"], t["gamma"], t["dgamma"], t["dbeta"])
    assert (np.abs(got["dz"][ties] - no_g[ties]) <= bound[ties]).all() and (t["dy"][ties] != 0).all()
    _report(r, f"C{C} P{P}")


@pytest.mark.parametrize("C,P", [(64, 4097), (12, 1000)])
def test_bn_stats_large_mean(C, P):
    """z = 64 + 0.05 n: the subtractive E[x^2] - E[x]^2 form misses rstd's bound by 3e4 here."""
    t = dict(_inputs(C, P, "bigmean"), kind="bigmean")
    got = _run_ops(C, P, t)
    got.pop("_mom03")
    _report(R.bn_ratios(t, C, P, got), f"bigmean C{C} P{P}")


@pytest.mark.parametrize("C,P", R.ONEHOT_CASES, ids=lambda v: str(v))
def test_bn_bwd_reduce_onehot(C, P):
    """One nonzero of dy per channel, moved over every lane, every stage-1 block, the first and the last
    pixel: dbeta is that value bit for bit, dgamma within 3 u |g xhat|."""
    t = _inputs(C, P)
    part = View(1, 2048 * C, 2048 * C)
    z, yv = View(P, C, C + 4, t["z"]), View(P, C, C + 8, np.ones((P, C), np.float32))
    vm, vr = _vec(t["mean"]), _vec(t["rstd"])
    worst = 0.0
    ones = np.ones((P, C), np.float32)
    for dyh in R.onehot_rounds(C, P):
        dy = View(P, C, C + 12, dyh)
        dg, db = _vec(C=C), _vec(C=C)
        _bn(2, dy=dy.ptr, ldd=dy.ld, y=yv.ptr, ldy=yv.ld, x=z.ptr, ldx=z.ld, mean=vm.ptr, rstd=vr.ptr, C=C, P=P,
            dgamma=dg.ptr, dbeta=db.ptr, part=part.ptr, part_floats=2048 * C)
        assert np.array_equal(_bits(db.get()[0]), _bits(dyh.sum(0))), "one-hot dbeta is not the planted value"
        rg, _ = R.bn_bwd_reduce(dyh, ones, t["z"], t["mean"], t["rstd"])
        bg, _ = R.reduce_bounds(dyh, ones, t["z"], t["mean"], t["rstd"], C, P)
        worst = max(worst, R.ratio(dg.get()[0] - rg, bg))
    _report({"onehot_dgamma": worst}, f"C{C} P{P}")


def test_bn_argument_checks():
    """Refused before any launch: the outputs keep their 1e30.  Ops 0-4 are refused by the launchers' own
    precondition check (KDLAE_EHIP, "invalid argument"), a short part by the entry (KDLAE_EINVAL_CONFIG), op 5 by
    the entry (KDLAE_EINVAL_SHAPE)."""
    C, P = 8, 5
    z, out, part = View(P, 12, 12), View(P, 12, 12), View(1, 2048 * 12, 2048 * 12)
    vecs = [_vec(C=12) for _ in range(8)]
    mean, rstd, rm, rv, gam, bet, dg, db = (v.ptr for v in vecs)
    ok0 = dict(x=z.ptr, ldx=12, C=C, P=P, mean=mean, rstd=rstd, running_mean=rm, running_var=rv, momentum=0.1,
               part=part.ptr, part_floats=2048 * C)
    ok1 = dict(x=z.ptr, ldx=12, mean=mean, rstd=rstd, gamma=gam, beta=bet, C=C, P=P, out=out.ptr, ldo=12)
    ok2 = dict(dy=z.ptr, ldd=12, y=z.ptr, ldy=12, x=z.ptr, ldx=12, mean=mean, rstd=rstd, C=C, P=P, dgamma=dg, dbeta=db,
               part=part.ptr, part_floats=2048 * C)
    ok3 = dict(dy=z.ptr, ldd=12, y=z.ptr, ldy=12, x=z.ptr, ldx=12, mean=mean, rstd=rstd, gamma=gam, dgamma=dg, dbeta=db,
               C=C, P=P, out=out.ptr, ldo=12)
    bad = [dict(C=6), dict(C=0), dict(C=1028, ldx=1028), dict(P=0), dict(ldx=4), dict(ldx=10), dict(x=None)]
    for op, ok in ((0, ok0), (1, ok1), (2, ok2), (3, ok3)):
        for b in bad:
            kw = {**ok, **b}
            if "part_floats" in kw:
                kw["part_floats"] = 2048 * 1028
            assert _call(op, **kw) == 3 and "invalid argument" in _lib.last_error(), (op, b)
    assert _call(0, **{**ok0, "part_floats": 2048 * C - 1}) == 2 and _call(2, **{**ok2, "part_floats": 2048 * C - 1}) == 2
    assert _call(0, **{**ok0, "part": None}) == 2
    assert _call(0, **{**ok0, "running_var": None}) == 3
    assert _call(0, **{**ok0, "mean": None}) == 3 and _call(1, **{**ok1, "gamma": None}) == 3
    assert _call(1, **{**ok1, "ldo": 10}) == 3 and _call(1, **{**ok1, "out": out.ptr + 4}) == 3
    assert _call(2, **{**ok2, "dbeta": None}) == 3 and _call(3, **{**ok3, "dgamma": None}) == 3
    up = dict(x=z.ptr, ldx=12, out=out.ptr, ldo=12, C=C, N=1, h=1, w=1)
    for op in (4, 5):
        rc = 3 if op == 4 else 1
        for b in (dict(C=6), dict(C=0), dict(ldx=10), dict(ldo=10), dict(ldx=4), dict(x=z.ptr + 4), dict(out=out.ptr + 8),
                  dict(x=None), dict(out=None), dict(N=0), dict(h=0), dict(w=0)):
            assert _call(op, **{**up, **b}) == rc, (op, b)
    assert "16-byte" in _lib.last_error() or "upsample" in _lib.last_error()
    assert _call(5, **{**up, "C": 2, "ldx": 4, "ldo": 4}) == 1
    for v in [z, out, part] + vecs:
        assert v.unchanged()


# ------------------------------------------------------------------ bilinear x2 pair
def _up_launch(N, C, h, w, x, v):
    """Forward into the second half of a [.][2C] concat buffer, from storage with +inf behind the input (a
    read past the last row would show); backward out of the second half of a [.][2C] gradient buffer."""
    xin = View(N * h * w, C, C, x)
    xin.s[xin.off + xin.P * xin.ld:] = float("inf")
    xin.before = xin.s.clone()
    outs = []
    for _ in range(2):
        cat = View(N * 4 * h * w, C, 2 * C, col=C)
        _bn(5, x=xin.ptr, ldx=C, out=cat.ptr, ldo=2 * C, C=C, N=N, h=h, w=w)
        assert cat.outside_unchanged() and xin.unchanged(), "upsample2x wrote outside its concat half"
        outs.append(cat.get().reshape(N, 2 * h, 2 * w, C))
    assert np.array_equal(_bits(outs[0]), _bits(outs[1]))
    backs = []
    if v is not None:
        dcat = View(N * 4 * h * w, C, 2 * C, v, col=C)
        for _ in range(2):
            din = View(N * h * w, C, C + 4)
            _bn(4, x=dcat.ptr, ldx=2 * C, out=din.ptr, ldo=din.ld, C=C, N=N, h=h, w=w)
            assert din.outside_unchanged() and dcat.unchanged()
            backs.append(din.get().reshape(N, h, w, C))
        assert np.array_equal(_bits(backs[0]), _bits(backs[1]))
    return outs[0], backs[0] if backs else None


@pytest.mark.parametrize("N,C,h,w", R.up_cases(), ids=lambda v: str(v))
def test_upsample_pair(N, C, h, w):
    """Element-wise: forward against Uy x Ux^T, backward against the transpose, both with the exact float64
    weights (bound grows with u max(h, w)) and with the kernels' fp32 weights (a few u sum |w x|); then one-hot
    gradients at the corners and at every row / column parity around the middle."""
    x, v = R.up_inputs(N, C, h, w)
    up, back = _up_launch(N, C, h, w, x, v)
    Uy, Ux, Vy, Vx = R.up_matrix(h), R.up_matrix(w), R.up_matrix_f32(h), R.up_matrix_f32(w)
    ft, fw = R.up_fwd_bounds(x, h, w)
    bt, bw = R.up_bwd_bounds(v, h, w)
    r = dict(up_fp32w=R.ratio(up - R.up_fwd(x, Vy, Vx), ft), up_exact=R.ratio(up - R.up_fwd(x, Uy, Ux), fw),
             upbwd_fp32w=R.ratio(back - R.up_bwd(v, Vy, Vx), bt), upbwd_exact=R.ratio(back - R.up_bwd(v, Uy, Ux), bw))
    assert np.isfinite(up).all()
    worst = 0.0
    for oy, ox in R.up_onehot_positions(h, w):
        hot = np.zeros((N, 2 * h, 2 * w, C), np.float32)
        hot[N - 1, oy, ox] = 1.0 + 0.125 * (np.arange(C) % 7)
        dcat = View(N * 4 * h * w, C, 2 * C, hot, col=C)
        din = View(N * h * w, C, C + 4)
        _bn(4, x=dcat.ptr, ldx=2 * C, out=din.ptr, ldo=din.ld, C=C, N=N, h=h, w=w)
        g = din.get().reshape(N, h, w, C)
        ref = R.up_bwd(hot, Vy, Vx)
        assert not g[ref == 0].any(), f"one-hot at ({oy}, {ox}): gradient where no weight is"
        worst = max(worst, R.ratio(g - ref, 3 * R.U * np.abs(ref)))   # l0 + l1, v wx, racc wy: three roundings
    r["upbwd_onehot"] = worst
    _report(r, f"N{N} C{C} {h}x{w}")


def _pattern(n):
    i = torch.arange(n, device=DEV, dtype=torch.float64)
    return (((i * 0.6180339887498949) % 1.0) * 2 - 1).float()


def _rows_dev(n, f32w):
    return tuple(torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in R.up_rows(n, f32w))


def test_upsample_fwd_past_the_grid_cap():
    """65536 x 256 + 8192 threads' worth of output: the grid-stride loop's second trip.  The float64 reference
    is separable (two entries per row and column) and runs on the device."""
    N, C, h, w = R.FWD_CAP_CASE
    x = _pattern(N * h * w * C)
    out = torch.full((N * 4 * h * w * C + 8,), SENT, device=DEV)
    _bn(5, x=x.data_ptr(), ldx=C, out=out.data_ptr(), ldo=C, C=C, N=N, h=h, w=w)
    assert bool((out[-8:] == SENT).all())
    got = out[:-8].view(2 * h, 2 * w, C).double()
    X = x.view(h, w, C).double()
    r = {}
    for name, f32w in (("fp32w", True), ("exact", False)):
        y0, y1, ly0, ly1 = _rows_dev(h, f32w)
        x0, x1, lx0, lx1 = _rows_dev(w, f32w)

        def blend(T):
            cols = T[:, x0] * lx0[None, :, None] + T[:, x1] * lx1[None, :, None]
            return cols[y0] * ly0[:, None, None] + cols[y1] * ly1[:, None, None]

        bound = R.FWD_ROUNDINGS * R.U * blend(X.abs())
        if not f32w:   # two weights per dimension each off by at most up_weight_err
            bound = bound + 2 * (R.up_weight_err(h) + R.up_weight_err(w)) * float(X.abs().max())
        r["upcap_" + name] = float(((got - blend(X)).abs() / bound).max())
        del bound
    _report(r, f"fwd cap {h}x{w}")


def test_upsample_bwd_past_the_grid_cap():
    """8192 x 256 + 2048 threads' worth of low-resolution pixels."""
    N, C, h, w = R.BWD_CAP_CASE
    v = _pattern(N * 4 * h * w * C)
    out = torch.full((N * h * w * C + 8,), SENT, device=DEV)
    _bn(4, x=v.data_ptr(), ldx=C, out=out.data_ptr(), ldo=C, C=C, N=N, h=h, w=w)
    assert bool((out[-8:] == SENT).all())
    got = out[:-8].view(h, w, C).double()
    V = v.view(2 * h, 2 * w, C).double()
    y0, y1, ly0, ly1 = _rows_dev(h, True)
    x0, x1, lx0, lx1 = _rows_dev(w, True)

    def gather_t(T):
        rows = torch.zeros(h, 2 * w, C, dtype=torch.float64, device=DEV)
        rows.index_add_(0, y0, T * ly0[:, None, None])
        rows.index_add_(0, y1, T * ly1[:, None, None])
        o = torch.zeros(h, w, C, dtype=torch.float64, device=DEV)
        o.index_add_(1, x0, rows * lx0[None, :, None])
        o.index_add_(1, x1, rows * lx1[None, :, None])
        return o

    bound = R.BWD_ROUNDINGS * R.U * gather_t(V.abs())
    _report({"upbwdcap_fp32w": float(((got - gather_t(V)).abs() / bound).max())}, f"bwd cap {h}x{w}")

"""The kernels that end every training step, each entry called alone through the C ABI and held to the
float64 models and derived bounds of tests/step_kernel_refs.py (proven there, on fp32 emulations,
to be met by the kernels' arithmetic and missed by every listed mutant; tests/test_step_kernel_refs.py):

    kdlae_train_l1sr        l1sr_kernel, l1sr_final_kernel                  train.hip
    kdlae_train_clip_adamw  sumsq_kernel, clip_coef_kernel, adamw_kernel    train.hip
    kdlae_train_mixup / _ema  mixup_kernel, ema_kernel                      train.hip
    kdlae_train_l1frames    l1frames_kernel, l1frames_final_kernel          train_s.hip
    kdlae_train_mse         mse_kernel                                      bn_train.hip

Conventions of every case (``every_offset``): all buffers start 0..3 floats into larger storage that is
pre-filled with 1e30, everything outside an output's range must still hold 1e30 after the call, the
call runs twice per offset and all eight results must have equal bits (none of these kernels uses
atomics, and none may depend on alignment).

Sizes: 1, 63, 64, 65, 255, 256, 257, 1000, and per kernel 2 T + 257 with T = blocks * 256 at the
launch's own block cap (step_kernel_refs.py quotes the caps), so that the grid-stride loop takes a
second and a third, ragged trip.

The worst ratio to each bound is printed when the module finishes (run with ``-s``).
"""
import ctypes

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from tests import step_kernel_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
U = R.U
BIG = R.SENTINEL
PAD = 8
MARGINS = {}


def _note(name, ratio):
    MARGINS[name] = max(MARGINS.get(name, 0.0), float(ratio))
    return ratio


def teardown_module(module):
    for k in sorted(MARGINS):
        print(f"[GPU / bound] {k}: {MARGINS[k]:.3f}")


class Buf:
    """n floats (or int32) `off` elements into 1e30-filled storage."""

    def __init__(self, n, off, init=None):
        self.n, self.off = n, off
        self.store = torch.full((off + n + PAD,), BIG, device=DEV)
        if init is not None:
            self.view().copy_(torch.from_numpy(np.ascontiguousarray(init, dtype=np.float32).reshape(-1)))

    def view(self):
        return self.store[self.off:self.off + self.n]

    @property
    def ptr(self):
        return ctypes.c_void_p(self.store.data_ptr() + 4 * self.off)

    def intact(self):
        return bool(torch.all(self.store[:self.off] == BIG)) and bool(torch.all(self.store[self.off + self.n:] == BIG))

    def untouched(self):
        return bool(torch.all(self.store == BIG))


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _scratch(n):
    return Buf(int(n), 0)


def every_offset(fn):
    """fn(off) -> tuple of device tensors.  Twice at each offset 0..3, equal bits throughout; returns
    the first result as numpy arrays."""
    first = None
    for off in range(4):
        for _ in range(2):
            got = fn(off)
            torch.cuda.synchronize()
            if first is None:
                first = got
            else:
                for a, b in zip(first, got):
                    assert torch.equal(a, b), f"bits differ at offset {off}"
    return tuple(x.cpu().numpy() for x in first)


# ===================================================================== kdlae_train_l1sr
def run_l1sr(p, t, q=None, s=None, grads=True):
    L = _lib.lib()

    def fn(off):
        bp, bt = Buf(p.size, off, p), Buf(t.size, off, t)
        bq = bs = None
        if q is not None:
            bq, bs = Buf(q.size, off, q), Buf(s.size, off, s)
        dhq = Buf(p.size, off) if grads else None
        dsr = Buf(q.size, off) if grads and q is not None else None
        loss, scr = Buf(1, off), _scratch(L.kdlae_train_l1sr_scratch_floats())
        rc = L.kdlae_train_l1sr(bp.ptr, bt.ptr, p.size, bq.ptr if bq else None, bs.ptr if bs else None,
                                q.size if q is not None else 0, dhq.ptr if dhq else None, dsr.ptr if dsr else None,
                                loss.ptr, scr.ptr, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        outs = [loss] + [b for b in (dhq, dsr) if b is not None]
        assert all(b.intact() for b in outs), "wrote outside an output"
        return tuple(b.view().clone() for b in outs)

    r = every_offset(fn)
    return (r[0][0],) + tuple(r[1:])


L1_SIZES = R.SMALL_SIZES + (R.three_trip(R.T_L1),)     # T = 1024 blocks * 256 = 262144: 524545


def _sign_c(p, t, w):
    return (np.sign(p.astype(np.float64) - t) * np.float32(w / p.size)).astype(np.float32).ravel()


def _rel(got, ref):
    err = abs(float(got) - ref)
    return err / abs(ref) if err else 0.0


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1sr_gradient_is_sign_times_c(n):
    """Every element equals sign(d) float32(w / n) exactly, 0.0 where pred == target (a whole block of
    them at n >= 768); the loss of this generic input within the dense bound."""
    p, t = R.loss_generic((n,), n)
    q, s = R.loss_generic((n + 3,), n + 7)
    loss, dhq, dsr = run_l1sr(p, t, q, s)
    assert np.array_equal(dhq, _sign_c(p, t, 0.5)) and np.array_equal(dsr, _sign_c(q, s, 0.25))
    assert _note("l1sr generic loss", _rel(loss, R.l1sr(p, t, q, s)[0]) / R.loss_dense_bound(n + 3)) <= 1


@pytest.mark.parametrize("n", (257, R.three_trip(R.T_L1)))
def test_l1sr_loss_only_call(n):
    """dhq / dsr NULL: the loss alone, the same bits as with gradients; and no sr term."""
    p, t = R.loss_dense((n,), n)
    q, s = R.loss_dense((n + 5,), n + 1)
    assert run_l1sr(p, t, q, s, grads=False)[0] == run_l1sr(p, t, q, s)[0]
    loss, dhq = run_l1sr(p, t)
    assert _note("l1sr dense loss", _rel(loss, R.l1sr(p, t)[0]) / R.loss_dense_bound(n)) <= 1
    assert np.array_equal(dhq, _sign_c(p, t, 0.5))


@pytest.mark.parametrize("pv,tv", [(0.875, 0.125), (0.125, 0.0625)], ids=["l1", "shadow"])
def test_l1sr_one_hot_loss(pv, tv):
    """All tied but element j: the loss within 2u of float64, so no thread, block or tail element
    is dropped or counted twice.  0.875 / 0.125: the L1 term alone; 0.125 / 0.0625: the shadow too."""
    n = R.three_trip(R.T_L1)
    for j in R.one_hot_positions(n, R.T_L1):
        p, t = R.loss_one_hot((n,), j, pv, tv, 3)
        loss, dhq = run_l1sr(p, t)
        assert _note("l1sr one-hot loss / 2u", _rel(loss, R.l1sr(p, t)[0]) / (2 * U)) <= 1, j
        assert np.count_nonzero(dhq) == 1 and dhq[j] == np.float32(0.5 / n)


@pytest.mark.parametrize("n", (6, 257, 1000))
def test_l1sr_threshold(n):
    """Elements at float32(0.1) and one ulp either side, pred side and target side: the shadow part
    is count * 0.25 / n within 2u (the L1 part has its dense bound)."""
    p, t, count = R.loss_threshold(n)
    a, s, _ = R.l1sr_parts(p, t)
    assert s * n == count
    tol = 2 * U * 0.25 * s + R.loss_dense_bound(n) * 0.5 * a
    loss = run_l1sr(p, t)[0]
    assert _note("l1sr threshold loss", abs(float(loss) - R.l1sr(p, t)[0]) / tol) <= 1


@pytest.mark.parametrize("n", L1_SIZES)
def test_l1sr_dense_loss(n):
    """|d| in [0.25, 1], nothing cancels: (ceil(n / T) + 6 + 3 + 4) u with the double final sum."""
    p, t = R.loss_dense((n,), n)
    q, s = R.loss_dense((n + 5,), n + 1)
    loss = run_l1sr(p, t, q, s)[0]
    assert _note("l1sr dense loss", _rel(loss, R.l1sr(p, t, q, s)[0]) / R.loss_dense_bound(n + 5)) <= 1


# ===================================================================== kdlae_train_l1frames
def run_l1frames(p, t, w1, wt, binary, red):
    L = _lib.lib()
    N, Fr, HW = p.shape

    def fn(off):
        bp, bt, dp = Buf(p.size, off, p), Buf(t.size, off, t), Buf(p.size, off)
        loss, scr = Buf(1, off), _scratch(L.kdlae_train_l1frames_scratch_floats())
        rc = L.kdlae_train_l1frames(bp.ptr, bt.ptr, N, Fr, HW, w1, wt, binary, red, dp.ptr, loss.ptr, scr.ptr, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert dp.intact() and loss.intact(), "wrote outside an output"
        return loss.view().clone(), dp.view().clone()

    loss, g = every_offset(fn)
    return loss[0], g.reshape(p.shape)


# n = 1, 63, 64, 65, 255, 256, 257, 1000 and 524547 >= 2 T + 257 (T = kLossBlocks * 256 = 262144), 1..5 frames
L1F_SHAPES = [(1, 1, 1), (1, 3, 21), (1, 1, 64), (1, 5, 13), (3, 1, 85), (1, 2, 128), (1, 1, 257), (2, 4, 125),
              (1, 3, 174849)]


def _grad_tol(shape, red):
    n, n2 = shape[0] * shape[1] * shape[2], shape[0] * (shape[1] - 1) * shape[2]
    return 2 * U * (R.f32(0.9) * (1 if red else 1 / n) + 2 * R.f32(0.1) * (1 if red or not n2 else 1 / n2))


@pytest.mark.parametrize("shape", L1F_SHAPES, ids=str)
@pytest.mark.parametrize("red", [0, 1], ids=["mean", "sum"])
def test_l1frames_gradient_and_loss(shape, red):
    """The three-term gradient within 2u (|g1| + 2 |gt|) of float64; the generic loss within the dense
    bound (every sum is of non-negative terms; the dyadic inputs make every difference exact)."""
    p, t = R.loss_generic(shape, shape[2] + red)
    loss64, g64 = R.l1frames(p, t, 0.9, 0.1, 0.1, red)
    loss, g = run_l1frames(p, t, 0.9, 0.1, 0.1, red)
    assert _note("l1frames gradient", np.abs(g - g64).max() / _grad_tol(shape, red)) <= 1
    assert _note("l1frames generic loss", _rel(loss, loss64) / R.loss_dense_bound(p.size)) <= 1


def test_l1frames_ties():
    """pred == target on whole blocks in every frame: exactly 0.0 there.  pred = target + c(pixel),
    constant over frames: no temporal gradient, every element exactly float32(w1 / n)."""
    p, t = R.loss_generic((2, 3, 300), 4)
    p[:, :, :256] = t[:, :, :256]
    _, g = run_l1frames(p, t, 0.9, 0.1, 0.1, 0)
    assert np.all(g[:, :, :256] == 0.0) and np.count_nonzero(g[:, :, 256:]) > 200
    t = R.dyadic((2, 3, 300), 9)
    p = t + (R.dyadic((2, 1, 300), 10) + np.float32(2.0 ** -10))
    loss, g = run_l1frames(p, t, 0.9, 0.1, 0.1, 0)
    assert np.all(g == np.float32(R.f32(0.9) / p.size))
    assert _rel(loss, R.l1frames(p, t, 0.9, 0.1, 0.1, 0)[0]) <= R.loss_dense_bound(p.size)


@pytest.mark.parametrize("pv,tv", [(0.875, 0.125), (0.125, 0.0625)], ids=["l1", "binary"])
@pytest.mark.parametrize("red", [0, 1], ids=["mean", "sum"])
def test_l1frames_one_hot_loss(pv, tv, red):
    """One differing pixel in one frame feeds the L1, the binary (second pair) and the temporal term
    (both neighbouring pairs) at once; all partial sums are exact, the loss is within 2u."""
    shape = (1, 3, 174849)
    n = 3 * 174849
    for j in R.one_hot_positions(n, R.T_L1):
        p, t = R.loss_one_hot(shape, j, pv, tv, 5)
        loss64, g64 = R.l1frames(p, t, 0.9, 0.1, 0.1, red)
        loss, g = run_l1frames(p, t, 0.9, 0.1, 0.1, red)
        assert _note("l1frames one-hot loss / 2u", _rel(loss, loss64) / (2 * U)) <= 1, j
        assert np.abs(g - g64).max() <= _grad_tol(shape, red)


@pytest.mark.parametrize("binary", [0.1, 0.3])
def test_l1frames_threshold(binary):
    p, t, count = R.loss_threshold(2 * 3 * 50, R.f32(binary))
    p, t = p.reshape(2, 3, 50), t.reshape(2, 3, 50)
    sb = R.l1frames_parts(p, t, binary)[1]
    assert sb == count
    ref = R.l1frames(p, t, 0.9, 0.1, binary, 0)[0]
    part = R.f32(0.9) * sb / p.size
    tol = 2 * U * part + R.loss_dense_bound(p.size) * (ref - part)
    loss = run_l1frames(p, t, 0.9, 0.1, binary, 0)[0]
    assert _note("l1frames threshold loss", abs(float(loss) - ref) / tol) <= 1


@pytest.mark.parametrize("shape", L1F_SHAPES, ids=str)
@pytest.mark.parametrize("red", [0, 1], ids=["mean", "sum"])
def test_l1frames_dense_loss(shape, red):
    p, t = R.loss_dense(shape, shape[2])
    loss = run_l1frames(p, t, 0.9, 0.1, 0.1, red)[0]
    assert _note("l1frames dense loss", _rel(loss, R.l1frames(p, t, 0.9, 0.1, 0.1, red)[0]) / R.loss_dense_bound(p.size)) <= 1


# ===================================================================== kdlae_train_clip_adamw
def run_adamw(theta, grad, m, v, gscale, max_norm, step, hyper, ranges=None):
    """-> dict norm, scale, theta, m, v as the kernel left them"""
    L = _lib.lib()
    n = theta.size
    nr = len(ranges) if ranges else 0
    rg = (ctypes.c_int64 * (2 * nr))(*[x for r in ranges for x in r]) if nr else None

    def fn(off):
        bt, bg, bm, bv = (Buf(n, off, x) for x in (theta, grad, m, v))
        scr = Buf(int(L.kdlae_train_adamw_scratch_floats()), off)
        rc = L.kdlae_train_clip_adamw(bt.ptr, bg.ptr, bm.ptr, bv.ptr, n, gscale, max_norm, hyper["lr"], hyper["beta1"],
                                      hyper["beta2"], hyper["eps"], hyper["weight_decay"], step, rg, nr, scr.ptr,
                                      _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert all(b.intact() for b in (bt, bm, bv, scr)), "wrote outside a buffer"
        return scr.view()[2048:2050].clone(), bt.view().clone(), bm.view().clone(), bv.view().clone()

    st, th, mm, vv = every_offset(fn)
    return dict(norm=st[0], scale=st[1], theta=th, m=mm, v=vv)


def _three_steps(x, hyper, step0, ranges=None, steps=3):
    """Consecutive updates from the class's nonzero moments; the kernel is fed its own state, the
    model the same fp32 state, so each step is judged on its own roundings."""
    n = x["theta"].size
    th, m, v = x["theta"], x["m"], x["v"]
    for i in range(steps):
        g = x["grad"] if i == 0 else (x["grad"] * np.float32(1 - 0.25 * i)).astype(np.float32)[::-1].copy()
        ref = R.clip_adamw(th, g, m, v, x["gscale"], x["max_norm"], step=step0 + i, ranges=ranges, **hyper)
        got = run_adamw(th, g, m, v, x["gscale"], x["max_norm"], step0 + i, hyper, ranges)
        for k, r in R.check_adamw(got, ref, th, n, hyper["beta1"], hyper["beta2"]).items():
            assert _note(f"adamw {k}", r) <= 1, (k, r, step0 + i)
        if not ref["clipped"]:
            assert got["scale"] == np.float32(x["gscale"])      # bit for bit
        outside = ~ref["mask"]
        for k, old in (("theta", th), ("m", m), ("v", v)):
            assert np.array_equal(got[k][outside], old[outside]), f"{k} outside the ranges changed"
        th, m, v = got["theta"], got["m"], got["v"]


@pytest.mark.parametrize("cls", R.ADAMW_CLASSES)
@pytest.mark.parametrize("hyper", [R.HYPER, R.HYPER_T], ids=["b0.9", "b0.2"])
@pytest.mark.parametrize("step0", [1, 2, 1000, 300000])
def test_adamw_state_over_three_steps(cls, hyper, step0):
    """norm, applied scale, m, v and theta of three consecutive steps, every clip branch (see
    step_kernel_refs.adamw_inputs), from step 1, 2 (where 1 - beta2^step cancels), 1000 and 300000."""
    _three_steps(R.adamw_inputs(1000, cls, 1000), hyper, step0)


# adamw_kernel: T = 16384 blocks * 256 = 4194304 -> 8388865; sumsq_kernel: T = 524288 -> 1048833
@pytest.mark.parametrize("n", R.SMALL_SIZES[:-1] + (R.three_trip(R.T_SUMSQ), R.three_trip(R.T_ADAMW)))
def test_adamw_sizes(n):
    _three_steps(R.adamw_inputs(n, "clip", n), R.HYPER_T, 2, steps=3 if n < 4096 else 1)


def test_adamw_norm_one_hot_and_dense():
    n = R.three_trip(R.T_SUMSQ)
    z = np.zeros(n, dtype=np.float32)
    for j in R.one_hot_positions(n, R.T_SUMSQ):
        got = run_adamw(z, R.one_hot_grad(n, j), z, z, 0.125, 0.01, 1, R.HYPER)
        assert _note("adamw one-hot norm / 2u", _rel(got["norm"], 0.75 * 0.125) / (2 * U)) <= 1, j
    g = R.spread(n, 0.25, 1.0, 1, signed=False)
    ref = R.clip_adamw(z, g, z, z, 1.0, 0.01, step=1, **R.HYPER)
    got = run_adamw(z, g, z, z, 1.0, 0.01, 1, R.HYPER)
    assert _note("adamw norm", _rel(got["norm"], ref["norm"]) / R.norm_dense_bound(n)) <= 1
    assert _note("adamw scale", _rel(got["scale"], ref["scale"]) / R.scale_bound(n, True)) <= 1


@pytest.mark.parametrize("n", (257, 1000))
def test_adamw_zero_gradient(n):
    """norm 0, applied scale == gscale, m / v / the Adam term stay 0, theta moves by the decay alone."""
    x = R.adamw_inputs(n, "clip")
    z = np.zeros(n, dtype=np.float32)
    got = run_adamw(x["theta"], z, z, z, 0.125, 0.01, 1, R.HYPER)
    assert got["norm"] == 0 and got["scale"] == np.float32(0.125)
    assert not got["m"].any() and not got["v"].any()
    ref = R.clip_adamw(x["theta"], z, z, z, 0.125, 0.01, step=1, **R.HYPER)
    assert np.all(np.abs(got["theta"] - ref["theta"]) <= 2 * U * np.abs(x["theta"]))


RANGES3 = [(3, 130), (131, 131), (257, 999)]      # an empty one, unaligned begins


@pytest.mark.parametrize("ranges", [None, RANGES3, [(517, 518)]], ids=["all", "three", "one-element"])
def test_adamw_ranges(ranges):
    """Outside the ranges theta, m and v keep their bits (and the 1e30 around them); the norm still
    covers all n (the gradient is nonzero everywhere; the model's norm is over all of it)."""
    _three_steps(R.adamw_inputs(1000, "clip", 2), R.HYPER, 1, ranges=ranges)


# ===================================================================== mixup, EMA, MSE
def run_mixup(x, perm, lam):
    L = _lib.lib()
    B, per = x.shape
    pd = torch.tensor(perm, dtype=torch.int32, device=DEV)

    def fn(off):
        bi, bo = Buf(x.size, off, x), Buf(x.size, off)
        rc = L.kdlae_train_mixup(bi.ptr, bo.ptr, B, per, ctypes.c_void_p(pd.data_ptr()), lam, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert bo.intact(), "wrote outside the output"
        return (bo.view().clone(),)

    return every_offset(fn)[0].reshape(x.shape)


PERMS = {"identity": [0, 1, 2, 3, 4], "reversal": [4, 3, 2, 1, 0], "fixed points": [0, 3, 2, 4, 1]}


@pytest.mark.parametrize("per", [1, 3, 1000])
@pytest.mark.parametrize("lam", [0.0, 1.0, 0.5, 0.3])
def test_mixup(per, lam):
    x = R.spread(5 * per, 1e-3, 1.0, per).reshape(5, per)
    for name, perm in PERMS.items():
        err = np.abs(run_mixup(x, perm, lam) - R.mixup(x, perm, lam))
        assert _note("mixup", np.max(err / (R.mixup_bound(x, perm, lam) + 1e-300))) <= 1, name
    one = x[:1]
    assert np.all(np.abs(run_mixup(one, [0], lam) - R.mixup(one, [0], lam)) <= R.mixup_bound(one, [0], lam))


def test_mixup_second_trip():
    """mixup_kernel: T = 65536 blocks * 256 = 16777216; B * per = T + 259 = 5 * 3355495."""
    B, per = 5, (R.T_MIXUP + 259) // 5
    assert B * per == R.T_MIXUP + 259
    x = R.spread(B * per, 1e-3, 1.0, 7).reshape(B, per)
    perm = PERMS["fixed points"]
    err = np.abs(run_mixup(x, perm, 0.3) - R.mixup(x, perm, 0.3))
    assert _note("mixup", np.max(err / R.mixup_bound(x, perm, 0.3))) <= 1


def run_ema(e, theta, decay):
    L = _lib.lib()

    def fn(off):
        be, bt = Buf(e.size, off, e), Buf(e.size, off, theta)
        rc = L.kdlae_train_ema(be.ptr, bt.ptr, e.size, decay, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert be.intact(), "wrote outside the buffer"
        return (be.view().clone(),)

    return every_offset(fn)[0]


# ema_kernel: T = 16384 blocks * 256 = 4194304 -> 8388865
@pytest.mark.parametrize("n", R.SMALL_SIZES + (R.three_trip(R.T_ADAMW),))
def test_ema(n):
    e, th = R.spread(n, 1e-4, 1.0, n), R.spread(n, 1e-4, 1.0, n + 1)
    for decay in (0.999, 0.9, 0.0, 1.0) if n < 4096 else (0.999,):
        err = np.abs(run_ema(e, th, decay) - R.ema(e, th, decay))
        assert _note("ema", np.max(err / R.ema_bound(e, th))) <= 1, decay
        assert np.all(np.abs(run_ema(e, e, decay) - e) <= np.spacing(np.abs(e))), "ema == theta moved"


@pytest.mark.parametrize("n", [1, 63, 64, 65, 200])
@pytest.mark.parametrize("scale", [1.0, 1 / 32])
def test_mse(n, scale):
    L = _lib.lib()
    s, t = R.spread(n, 0.05, 1.0, n), R.spread(n, 0.05, 1.0, n + 1)

    def fn(off):
        bs, bt, ds, loss = Buf(n, off, s), Buf(n, off, t), Buf(n, off), Buf(2, off)
        rc = L.kdlae_train_mse(bs.ptr, bt.ptr, n, scale, ds.ptr, loss.ptr, _stream())
        assert rc == 0, _lib.last_error()
        torch.cuda.synchronize()
        assert ds.intact() and loss.intact(), "wrote outside an output"
        return ds.view().clone(), loss.view().clone()

    ds, loss = every_offset(fn)
    ds64, l0, l1 = R.mse(s, t, scale)
    assert _note("mse dscore", np.max(np.abs(ds - ds64) / (3 * U * np.abs(ds64) + 1e-300))) <= 1
    assert _note("mse loss[0]", _rel(loss[0], l0) / ((n + 2) * U)) <= 1
    assert _note("mse loss[1]", _rel(loss[1], l1) / ((n + 1) * U)) <= 1


# ===================================================================== argument checks (no launch)
def _refused(call, outs, poison="ema"):
    """`call()` must return an error code, set kdlae_last_error anew and leave every output at 1e30."""
    L = _lib.lib()
    if poison == "ema":
        assert L.kdlae_train_ema(None, None, 0, 0.5, None) != 0
    else:
        assert L.kdlae_train_l1frames(None, None, 0, 0, 0, 0.5, 0.5, 0.1, 0, None, None, None, None) != 0
    before = _lib.last_error()
    assert before
    rc = call()
    torch.cuda.synchronize()
    assert rc != 0, "accepted"
    assert _lib.last_error() and _lib.last_error() != before, "kdlae_last_error not set"
    assert all(b.untouched() for b in outs), "an output was written"


def test_l1sr_argument_checks():
    L = _lib.lib()
    a, b, d, e, loss = (Buf(64, 0) for _ in range(5))
    scr = _scratch(L.kdlae_train_l1sr_scratch_floats())
    outs, s, N = (d, e, loss, scr), _stream(), None
    for args in [(a.ptr, b.ptr, 0, N, N, 0), (a.ptr, b.ptr, -1, N, N, 0), (N, b.ptr, 64, N, N, 0),
                 (a.ptr, N, 64, N, N, 0),
                 (a.ptr, b.ptr, 64, a.ptr, N, 64),        # pred_sr without gt_sr
                 (a.ptr, b.ptr, 64, a.ptr, b.ptr, 0),     # pred_sr with n_sr <= 0
                 (a.ptr, b.ptr, 64, a.ptr, b.ptr, -5)]:
        _refused(lambda: L.kdlae_train_l1sr(*args, d.ptr, e.ptr, loss.ptr, scr.ptr, s), outs)
    _refused(lambda: L.kdlae_train_l1sr(a.ptr, b.ptr, 64, N, N, 0, d.ptr, e.ptr, N, scr.ptr, s), outs)
    _refused(lambda: L.kdlae_train_l1sr(a.ptr, b.ptr, 64, N, N, 0, d.ptr, e.ptr, loss.ptr, N, s), outs)


def test_clip_adamw_argument_checks():
    L = _lib.lib()
    th, g, m, v = (Buf(64, 0) for _ in range(4))
    scr = _scratch(L.kdlae_train_adamw_scratch_floats())
    outs, s = (th, m, v, scr), _stream()
    h = (1.0, 0.01, 1e-3, 0.9, 0.999, 1e-8, 0.0)

    def call(ptrs=(th.ptr, g.ptr, m.ptr, v.ptr), n=64, step=1, ranges=None, nranges=0, scratch=scr.ptr):
        rg = (ctypes.c_int64 * len(ranges))(*ranges) if ranges else None
        return lambda: L.kdlae_train_clip_adamw(*ptrs, n, *h, step, rg, nranges, scratch, s)

    cases = [call(n=0), call(n=-3), call(step=0), call(step=-1), call(nranges=-1), call(nranges=1),
             call(ranges=[5, 4], nranges=1), call(ranges=[0, 65], nranges=1), call(ranges=[-1, 4], nranges=1),
             call(ranges=[0, 8, 60, 70], nranges=2), call(scratch=None)]
    for i in range(4):
        ptrs = [th.ptr, g.ptr, m.ptr, v.ptr]
        ptrs[i] = None
        cases.append(call(ptrs=tuple(ptrs)))
    for c in cases:
        _refused(c, outs, poison="l1frames")


def test_mixup_ema_l1frames_mse_argument_checks():
    L = _lib.lib()
    a, b, loss = Buf(64, 0), Buf(64, 0), Buf(2, 0)
    perm = torch.zeros(4, dtype=torch.int32, device=DEV)
    pp, s, N = ctypes.c_void_p(perm.data_ptr()), _stream(), None
    for args in [(a.ptr, a.ptr, 4, 16, pp), (N, b.ptr, 4, 16, pp), (a.ptr, N, 4, 16, pp), (a.ptr, b.ptr, 4, 16, N),
                 (a.ptr, b.ptr, 0, 16, pp), (a.ptr, b.ptr, 4, 0, pp)]:
        _refused(lambda: L.kdlae_train_mixup(*args, 0.3, s), (a, b), poison="l1frames")
    for args in [(N, b.ptr, 64), (a.ptr, N, 64), (a.ptr, b.ptr, 0), (a.ptr, b.ptr, -1)]:
        _refused(lambda: L.kdlae_train_ema(*args, 0.9, s), (a, b), poison="l1frames")
    scr = _scratch(L.kdlae_train_l1frames_scratch_floats())
    d = Buf(64, 0)
    outs = (d, loss, scr)
    for args in [(a.ptr, b.ptr, 1, 4, 16, 2, d.ptr, loss.ptr, scr.ptr),      # reduction 2
                 (a.ptr, b.ptr, 1, 4, 16, -1, d.ptr, loss.ptr, scr.ptr),
                 (a.ptr, b.ptr, 0, 4, 16, 0, d.ptr, loss.ptr, scr.ptr), (a.ptr, b.ptr, 1, 0, 16, 0, d.ptr, loss.ptr, scr.ptr),
                 (a.ptr, b.ptr, 1, 4, 0, 0, d.ptr, loss.ptr, scr.ptr), (N, b.ptr, 1, 4, 16, 0, d.ptr, loss.ptr, scr.ptr),
                 (a.ptr, N, 1, 4, 16, 0, d.ptr, loss.ptr, scr.ptr), (a.ptr, b.ptr, 1, 4, 16, 0, N, loss.ptr, scr.ptr),
                 (a.ptr, b.ptr, 1, 4, 16, 0, d.ptr, N, scr.ptr), (a.ptr, b.ptr, 1, 4, 16, 0, d.ptr, loss.ptr, N)]:
        _refused(lambda: L.kdlae_train_l1frames(*args[:5], 0.9, 0.1, 0.1, *args[5:], s), outs, poison="ema")
    for args in [(a.ptr, b.ptr, 0, d.ptr, loss.ptr), (a.ptr, b.ptr, -2, d.ptr, loss.ptr), (N, b.ptr, 64, d.ptr, loss.ptr),
                 (a.ptr, N, 64, d.ptr, loss.ptr), (a.ptr, b.ptr, 64, N, loss.ptr), (a.ptr, b.ptr, 64, d.ptr, N)]:
        _refused(lambda: L.kdlae_train_mse(*args[:3], 1.0, *args[3:], s), (d, loss), poison="ema")

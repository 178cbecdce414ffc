"""The dx-only kernel variants of fine-tuning (frozen depthwise-conv and LayerNorm weights) against their full
parents on identical operands, through kdlae_debug_train ops 16-19:

    16 dwgate_bwd_dx   vs op 4      17 dwgate_bwd_rc_dx vs op 5      18 dw_bwd_dx vs op 6
    19 ln_bwd_dx       vs kdlae_debug_ln dir 1 (both routes)

The variants drop the weight-gradient accumulators, the LDS reduction and the partial stores and must not change
one bit of the input gradient: every comparison here is bit equality.  Every output is a view inside 1e30-filled
storage that must stay bit-unchanged outside the view."""
import ctypes

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd._lib import TrainDesc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BIG = 1e30
GUARD = 64
EINVAL_SHAPE = 1
c_int, c_int64, c_void_p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
LN_BWD_ROWS = 32   # KDLAE_LN_BWD_ROWS (kdlae_train.cpp): pixels per block of the engine's LayerNorm backward


class LnDesc(ctypes.Structure):
    """kdlae_debug_ln_desc (include/kdlae.h)."""
    _fields_ = [("dir", c_int), ("x", c_void_p), ("ldx", c_int), ("w", c_void_p), ("b", c_void_p),
                ("C", c_int), ("P", c_int64), ("biasfree", c_int), ("y", c_void_p), ("ldy", c_int),
                ("stats", c_void_p), ("dy", c_void_p), ("ldd", c_int), ("R", c_void_p), ("ldr", c_int),
                ("dx", c_void_p), ("lddx", c_int), ("part", c_void_p), ("nblk", c_int), ("route", c_int)]


def _rand(*shape, seed=0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).float()


def _view_in(x, ld):
    """[pixels, C] -> device [pixels][ld] with NaN in the row pad"""
    buf = torch.full((x.shape[0], ld), float("nan"))
    buf[:, :x.shape[1]] = x
    return buf.to(DEV)


class Out:
    """A [pixels][ld] output view of `C` used columns inside 1e30-filled storage with a guard on both sides."""

    def __init__(self, pixels, C, ld):
        self.store = torch.full((GUARD + pixels * ld + GUARD,), BIG, device=DEV)
        self.pixels, self.C, self.ld = pixels, C, ld
        self.ptr = self.store.data_ptr() + 4 * GUARD

    def take(self):
        """the view's bits; everything outside it must still hold 1e30"""
        body = self.store[GUARD:GUARD + self.pixels * self.ld].view(self.pixels, self.ld)
        fill = torch.tensor(BIG, device=DEV).view(torch.int32)
        assert bool((self.store[:GUARD].view(torch.int32) == fill).all()), "wrote before the view"
        assert bool((self.store[-GUARD:].view(torch.int32) == fill).all()), "wrote past the view"
        assert bool((body[:, self.C:].contiguous().view(torch.int32) == fill).all()), "wrote into the row pad"
        return body[:, :self.C].contiguous().view(torch.int32).clone()


def _train(op, ins, out, w, bias, part, C, Bn, H, W, **kw):
    d = TrainDesc()
    d.op = op
    for i, (t, ld) in enumerate(ins):
        d.inp[i], d.ldi[i] = (t.data_ptr() if t is not None else None), ld
    d.out[0], d.ldo[0] = out.ptr if out is not None else None, out.ld if out is not None else 0
    d.w = w.data_ptr() if w is not None else None
    d.bias = bias.data_ptr() if bias is not None else None
    d.part, d.part_floats = (part.data_ptr(), part.numel()) if part is not None else (None, 0)
    d.C, d.Bn, d.H, d.W = C, Bn, H, W
    for k, v in kw.items():
        setattr(d, k, v)
    rc = _lib.lib().kdlae_debug_train(ctypes.byref(d), None)
    torch.cuda.synchronize()
    return rc


# hid / C: 5 and 127 (odd halves, no float4 alignment), 48; H x W: ragged against the 16-column and 16 / 8 / 4-row
# blocks, and exact
DW_CASES = [(C, H, W) for C in (5, 127, 48) for H, W in ((5, 7), (17, 33), (16, 16))]


@pytest.mark.parametrize("C,H,W", DW_CASES, ids=[f"C{c}-{h}x{w}" for c, h, w in DW_CASES])
def test_depthwise_dx_only_variants_equal_their_parents(C, H, W):
    Bn = 2
    px = Bn * H * W
    pad = 0 if C % 4 == 0 else 3
    blocks = _lib.lib().kdlae_debug_train_blocks(0, Bn, H, W, 0)
    assert blocks > 0
    seed = 1000 * C + 10 * H + W
    dg = _view_in(_rand(px, C, seed=seed), C + pad)
    yd = _view_in(_rand(px, 2 * C, seed=seed + 1), 2 * C + pad)
    y = _view_in(_rand(px, 2 * C, seed=seed + 2), 2 * C + pad)
    w2 = _rand(2 * C, 9, seed=seed + 3).to(DEV)
    b2 = _rand(2 * C, seed=seed + 4).to(DEV)
    part2 = torch.empty(blocks * 10 * 2 * C, device=DEV)
    ld_o = 2 * C + (0 if C % 4 == 0 else 2)

    def pair(op_full, op_dx, ins, Cdesc, Cout, w, bias, part, ins_dx=None):
        full, dx = Out(px, Cout, Cout + (ld_o - 2 * C)), Out(px, Cout, Cout + (ld_o - 2 * C))
        assert _train(op_full, ins, full, w, bias, part, Cdesc, Bn, H, W) == 0, _lib.last_error()
        assert _train(op_dx, ins_dx or ins, dx, w, bias, None, Cdesc, Bn, H, W) == 0, _lib.last_error()   # part = NULL
        a, b = full.take(), dx.take()
        assert bool(torch.isfinite(a.view(torch.float32)).all())
        assert torch.equal(a, b), f"op {op_dx} differs from op {op_full} in {int((a != b).sum())} floats"
        return b

    pair(4, 16, [(dg, C + pad), (yd, 2 * C + pad), (y, 2 * C + pad)], C, 2 * C, w2, None, part2)
    pair(5, 17, [(dg, C + pad), (y, 2 * C + pad)], C, 2 * C, w2, b2, part2)
    # op 18 never reads in1: an all-NaN layer input, then a null one, give the parent's finite bits
    dyd = _view_in(_rand(px, C, seed=seed + 5), C + pad)
    xin = _view_in(_rand(px, C, seed=seed + 6), C + pad)
    w1 = _rand(C, 9, seed=seed + 7).to(DEV)
    part1 = torch.empty(blocks * 10 * C, device=DEV)
    nan_in = torch.full_like(xin, float("nan"))
    got = pair(6, 18, [(dyd, C + pad), (xin, C + pad)], C, C, w1, None, part1, ins_dx=[(dyd, C + pad), (nan_in, C + pad)])
    null_in = Out(px, C, C + (ld_o - 2 * C))
    assert _train(18, [(dyd, C + pad), (None, 0)], null_in, w1, None, None, C, Bn, H, W) == 0, _lib.last_error()
    assert torch.equal(null_in.take(), got)


def test_depthwise_dx_only_ops_refuse_bad_geometry():
    C, Bn, H, W = 5, 1, 5, 7
    px = Bn * H * W
    dg, y = _view_in(_rand(px, C), C), _view_in(_rand(px, 2 * C), 2 * C)
    w2, w1 = _rand(2 * C, 9).to(DEV), _rand(C, 9).to(DEV)
    for op, ins, Cout, w in ((16, [(dg, C), (y, 2 * C), (y, 2 * C)], 2 * C, w2), (17, [(dg, C), (y, 2 * C)], 2 * C, w2),
                             (18, [(dg, C), (None, 0)], C, w1)):
        out = Out(px, Cout, Cout)
        assert _train(op, ins, out, w, None, None, C, Bn, H, W) == 0, _lib.last_error()
        short = [(ins[0][0], C - 1)] + ins[1:]
        assert _train(op, short, out, w, None, None, C, Bn, H, W) == EINVAL_SHAPE          # ld < width
        narrow = Out(px, Cout, Cout)
        narrow.ld = Cout - 1
        assert _train(op, ins, narrow, w, None, None, C, Bn, H, W) == EINVAL_SHAPE
        assert _train(op, [(None, C)] + ins[1:], out, w, None, None, C, Bn, H, W) != 0     # null dy
        assert _train(op, ins, None, w, None, None, C, Bn, H, W) != 0
        assert _train(op, ins, out, None, None, None, C, Bn, H, W) != 0                    # null w
        assert _train(op, ins, out, w, None, None, C, 0, H, W) == EINVAL_SHAPE
    torch.cuda.synchronize()


def _ln_full(dy, x, w, stats, R, C, P, bf, route, nblk, ld):
    out = Out(P, C, ld)
    part = torch.empty(nblk * (C if bf else 2 * C), device=DEV)
    d = LnDesc()
    d.dir, d.x, d.ldx, d.w, d.C, d.P, d.biasfree = 1, x.data_ptr(), ld, w.data_ptr(), C, P, bf
    d.stats, d.dy, d.ldd = stats.data_ptr(), dy.data_ptr(), ld
    d.R, d.ldr = (R.data_ptr(), ld) if R is not None else (None, 0)
    d.dx, d.lddx, d.part, d.nblk, d.route = out.ptr, ld, part.data_ptr(), nblk, route
    _lib.check(_lib.lib().kdlae_debug_ln(ctypes.byref(d), None), "kdlae_debug_ln")
    torch.cuda.synchronize()
    return out.take()


# C: 5 / 127 (the generic kernel on both routes, 1 and 2 values per lane), 48 / 96 / 192 / 384 (the four lane-group
# shapes on route 0, 1 / 2 / 4 / 8 values per lane on route 1)
@pytest.mark.parametrize("biasfree", (1, 0), ids=("biasfree", "withbias"))
@pytest.mark.parametrize("C", (5, 48, 96, 127, 192, 384))
def test_layernorm_dx_only_equals_the_full_backward(C, biasfree):
    ld = C if C % 4 == 0 else C + 3
    w = _rand(C, seed=C).to(DEV)
    for P in (1, 31, 33, 4 * LN_BWD_ROWS + 1):
        nblk = max(1, P // LN_BWD_ROWS)
        xc = _rand(P, C, seed=C + P)
        mu = xc.mean(1)
        rstd = 1.0 / torch.sqrt(xc.var(1, unbiased=False) + 1e-5)
        stats = torch.stack([mu, rstd], 1).contiguous().to(DEV)
        x, dy, R = _view_in(xc, ld), _view_in(_rand(P, C, seed=C + P + 1), ld), _view_in(_rand(P, C, seed=C + P + 2), ld)
        for route in (0, 1):
            for res in (None, R):
                want = _ln_full(dy, x, w, stats, res, C, P, biasfree, route, nblk, ld)
                out = Out(P, C, ld)
                rc = _train(19, [(dy, ld), (x, ld), (stats, 2), (res, ld if res is not None else 0)], out, w, None, None,
                            C, 0, 0, 0, P=P, nblk=nblk, flag=biasfree | (route << 1))
                assert rc == 0, _lib.last_error()
                got = out.take()
                assert bool(torch.isfinite(got.view(torch.float32)).all())
                assert torch.equal(got, want), (P, route, res is not None, int((got != want).sum()))


def test_layernorm_dx_only_op_refuses_bad_geometry():
    C, P = 48, 33
    x, dy = _view_in(_rand(P, C), C), _view_in(_rand(P, C, seed=1), C)
    w, stats = _rand(C).to(DEV), torch.ones(P, 2, device=DEV)
    out = Out(P, C, C)
    ok = [(dy, C), (x, C), (stats, 2), (None, 0)]
    assert _train(19, ok, out, w, None, None, C, 0, 0, 0, P=P, nblk=1, flag=1) == 0, _lib.last_error()
    assert _train(19, [(dy, C - 1)] + ok[1:], out, w, None, None, C, 0, 0, 0, P=P, nblk=1, flag=1) == EINVAL_SHAPE
    assert _train(19, [(None, C)] + ok[1:], out, w, None, None, C, 0, 0, 0, P=P, nblk=1, flag=1) != 0
    assert _train(19, ok, out, None, None, None, C, 0, 0, 0, P=P, nblk=1, flag=1) != 0
    assert _train(19, ok, None, w, None, None, C, 0, 0, 0, P=P, nblk=1, flag=1) != 0
    assert _train(19, ok, out, w, None, None, 513, 0, 0, 0, P=P, nblk=1, flag=1) == EINVAL_SHAPE
    assert _train(19, ok, out, w, None, None, C, 0, 0, 0, P=0, nblk=1, flag=1) == EINVAL_SHAPE
    torch.cuda.synchronize()

"""Kernels that only whole-model tests reached, one launch each against the float64 references of
tests/narrow_kernel_refs.py (proven, with their mutants, by tests/test_narrow_kernel_refs.py):

* the 2-D narrow-input 3x3 conv, conv_small_in_kernel<1, NTO> (kdlae_debug_small_in): Cin 1..4, Cout 16 /
  48 / 96 / 144 (one live tile of an NTO = 2 kernel; a second 128-channel pass with a 16-channel rest),
  dilation 1 / 2, NCHW input and an NHWC channel slice of a wider buffer, 126 pixels (a partial last
  64-pixel chunk), a 2 x 3 image, ASDQE's (lq - gt) form with a 5 x 7 valid extent on an 8 x 8 grid, the
  transposed (wt) mode of the image heads' training dX, and one image pair of 2.2 M pixels that reaches
  the grid-stride loop past the launcher's 8192-block cap;
* the ASDQE train-mode regressor head, forward and backward (kdlae_debug_head_train);
* bit for bit: asdqe_pack_inputs, narrow_w_copy, bcast_rows, grad_commit (kdlae_debug_bn ops 6-9),
  KDLAE-S pack_conv and relu (kdlae_debug_train_s ops 6-7).

Conventions of tests/test_infer_kernels_gpu.py: Bn >= 2 different images, seeded uniform data with weights
scaled by 1 / sqrt(K), output views wider than their used columns, pre-filled with 7.0 and checked
untouched, tolerance 1e-5 (max|ref| + 1) sqrt(K) / 4.
"""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import infer_kernel_refs as IR
import narrow_kernel_refs as R
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd._lib import BnDesc, HeadTrainDesc, SmallInDesc, TrainSDesc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAD = 7.0


def _launch(fn, desc_cls, **kw):
    d = desc_cls()
    for k, v in kw.items():
        if isinstance(v, (list, tuple)):
            for i, x in enumerate(v):
                getattr(d, k)[i] = x
        else:
            setattr(d, k, v)
    _lib.check(getattr(_lib.lib(), fn)(ctypes.byref(d), None), fn)
    torch.cuda.synchronize()


def _dev(t):
    return None if t is None else t.to(DEV).contiguous()


def _ptr(t, offset=0):
    return None if t is None else t.data_ptr() + 4 * offset


def _close(got, ref, K, what):
    err = (got.double() - ref).abs().max().item()
    tol = R.tol(ref, K)
    print(f"RATIO {what.split()[0]} {err / tol:.4f} ({what})")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= tol, f"{what} max |err| {err:.3e} > {tol:.3e}"


# ------------------------------------------------------------------ narrow-input 3x3 conv, 2-D
def _small_in_launch(c, x, sub, w, bias):
    """x, sub [Bn][Cin][h][w] on the device (h x w: what the kernel may read) -> out rows [Bn H W][Cout + 4]."""
    Bn, Cin, h, wd = x.shape
    Cout, H, W = c["Cout"], c["H"], c["W"]
    keep = [x, sub]
    if c["layout"] == "nchw":
        strides = dict(sb=Cin * h * wd, sc=h * wd, sy=wd, sx=1)
        inp, insub = _ptr(x), _ptr(sub)
    else:  # channels c0 .. c0 + Cin of a wider NHWC buffer that holds other data around them
        c0, ld = 2, Cin + 5

        def slice_of(t, seed):
            buf = R.rand(Bn, h, wd, ld, seed=seed).to(DEV)
            buf[..., c0:c0 + Cin] = t.permute(0, 2, 3, 1)
            keep.append(buf)
            return _ptr(buf, c0)

        strides = dict(sb=h * wd * ld, sc=1, sy=wd * ld, sx=ld)
        inp, insub = slice_of(x, 91), None if sub is None else slice_of(sub, 92)
    ldo = Cout + 4
    out = torch.full((Bn * H * W, ldo), PAD, device=DEV)
    _launch("kdlae_debug_small_in", SmallInDesc, inp=inp, in_sub=insub, st=0, **strides, Cin=Cin, Cout=Cout,
            dil=c["dil"], kt=1, F=1, w=_ptr(w), bias=_ptr(bias), out=_ptr(out), ldo=ldo, Bn=Bn, H=H, W=W,
            vh=c["vh"], vw=c["vw"], relu=c["relu"], wt=Cout if c["wt"] else 0)
    del keep
    return out


@pytest.mark.parametrize("c", R.small_in_cases(), ids=R.small_in_id)
def test_small_in_2d(c):
    x, sub, w, bias = R.small_in_inputs(c)
    ref = R.small_in_2d(x, sub, w, bias, c["dil"], c["vh"], c["vw"], c["relu"], c["Cout"] if c["wt"] else 0)
    vh, vw = c["vh"] or c["H"], c["vw"] or c["W"]
    # the kernel is handed the valid extent only, as ASDQE hands it the unpadded image
    cut = lambda t: None if t is None else _dev(t[:, :, :vh, :vw])
    out = _small_in_launch(c, cut(x), cut(sub), _dev(w), _dev(bias))
    _close(out[:, :c["Cout"]].cpu(), R.nhwc_rows(ref), 9 * c["Cin"], f"small_in {R.small_in_id(c)}")
    assert bool((out[:, c["Cout"]:] == PAD).all()), "wrote past its Cout columns"


def test_small_in_2d_grid_stride():
    """2 x 1100 x 1001 pixels: more 64-pixel chunks than 4 waves of 8192 blocks take in one step, so the
    chunk loop runs a second time for some waves and the last chunk is partial.  Reference: torch's own
    float64 conv on the device.  The one large case of this file (about a second of kernels and copies)."""
    c = dict(Cin=1, Cout=16, dil=1, layout="nchw", bias=1, relu=0, Bn=2, H=1100, W=1001, sub=0, vh=0, vw=0, wt=0)
    assert c["Bn"] * c["H"] * c["W"] > 8192 * 256 and (c["Bn"] * c["H"] * c["W"]) % 64
    x, _, w, bias = (_dev(t) for t in R.small_in_inputs(c))
    out = _small_in_launch(c, x, None, w, bias)
    ref = F.conv2d(x.double(), w.double(), bias.double(), padding=1)
    _close(out[:, :16], R.nhwc_rows(ref), 9, "small_in grid-stride 2x1100x1001")
    assert bool((out[:, 16:] == PAD).all())


# ------------------------------------------------------------------ train-mode regressor head
@pytest.mark.parametrize("case", R.head_cases(), ids=lambda c: "-".join(map(str, c)))
def test_head_train(case):
    C, M, N1, N2, slots, masks = case
    B = R.HEAD_B
    t = R.head_inputs(*case)
    ref = R.head_train(inv_hw=R.HEAD_INV_HW, **t)
    d = {k: _dev(v) for k, v in t.items()}
    row = 2 * (C + M + N1 + N2) + 4
    save = torch.full((B * row + 8,), PAD, device=DEV)
    score = torch.full((B + 4,), PAD, device=DEV)
    shapes = dict(gwo=(M, C), gbo=(M,), gw1=(N1, M), gb1=(N1,), gw2=(N2, N1), gb2=(N2,), gw3=(N2,), gb3=(1,))
    # each gradient in its own buffer with 4 floats of padding after it
    grads = {k: torch.full((math.prod(s) + 4,), PAD, device=DEV) for k, s in shapes.items()}
    common = dict(partial=_ptr(d["partial"]), slots=slots, C=C, inv_hw=R.HEAD_INV_HW, M=M, N1=N1, N2=N2, B=B,
                  save=_ptr(save), save_floats=B * row, score=_ptr(score),
                  **{k: _ptr(d[k]) for k in ("wo", "bo", "w1", "b1", "w2", "b2", "w3", "b3", "mask1", "mask2")})
    _launch("kdlae_debug_head_train", HeadTrainDesc, dir=0, **common)
    what = "-".join(map(str, case))
    _close(score[:B].cpu(), ref["score"], R.head_K("score", C, M, N1, N2), f"head_score {what}")
    assert bool((score[B:] == PAD).all()) and bool((save[B * row:] == PAD).all())
    _launch("kdlae_debug_head_train", HeadTrainDesc, dir=1, dscore=_ptr(d["dscore"]), **common,
            **{k: _ptr(v) for k, v in grads.items()})
    off = C + 2 * (M + N1 + N2) + 4  # head_save_dgap
    dgap = save[:B * row].view(B, row)[:, off:off + C].cpu()
    _close(dgap, ref["dgap"], R.head_K("dgap", C, M, N1, N2), f"head_dgap {what}")
    got = {}
    for k, s in shapes.items():
        n = grads[k].numel() - 4
        got[k] = grads[k][:n].view(s).cpu()
        _close(got[k], ref[k].view(s), R.head_K(k, C, M, N1, N2), f"head_{k} {what}")
        assert bool((grads[k][n:] == PAD).all()), f"{k}: wrote past its end"
    assert bool((save[B * row:] == PAD).all())
    # the units whose pre-activation is exactly 0 (zero weights and bias): no gradient at all
    assert got["gw1"][3].abs().max() == 0 and got["gb1"][3] == 0
    assert got["gw2"][N2 - 1].abs().max() == 0 and got["gb2"][N2 - 1] == 0
    # the image whose dscore is 0 contributes nothing to dgap
    assert dgap[1].abs().max() == 0


# ------------------------------------------------------------------ exact kernels
def _bn(op, **kw):
    _launch("kdlae_debug_bn", BnDesc, op=op, **kw)


@pytest.mark.parametrize("ci", [1, 2, 3, 4])
def test_asdqe_pack_inputs(ci):
    B, H, W, Hp, Wp = 2, 5, 7, 8, 8
    lq, gt = R.rand(B, ci, H, W, seed=ci), R.rand(B, ci, H, W, seed=ci + 10)
    xin = torch.full((B * Hp * Wp * 12 + 4,), PAD, device=DEV)
    a, b = _dev(lq), _dev(gt)
    _bn(6, x=_ptr(a), y=_ptr(b), out=_ptr(xin), C=ci, N=B, h=H, w=W, Hp=Hp, Wp=Wp)
    got = xin[:-4].view(B, Hp, Wp, 12).cpu()
    assert torch.equal(got, R.asdqe_pack_inputs(lq, gt, Hp, Wp))
    assert torch.equal(got[:, :H, :W, 8:8 + ci], (lq - gt).permute(0, 2, 3, 1))
    assert got.view(B, Hp, Wp, 3, 4)[..., ci:].abs().max() == 0 if ci < 4 else True
    assert got[:, H:].abs().max() == 0 and got[:, :, W:].abs().max() == 0
    assert bool((xin[-4:] == PAD).all())


@pytest.mark.parametrize("Cout", [16, 96])
@pytest.mark.parametrize("ci", [1, 2, 3])
def test_narrow_w_copy(ci, Cout):
    src = R.rand(Cout, 4, 9, seed=ci + Cout)
    dst = torch.full((Cout * ci * 9 + 4,), PAD, device=DEV)
    s = _dev(src)
    _bn(7, x=_ptr(s), out=_ptr(dst), C=ci, N=Cout)
    assert torch.equal(dst[:-4].view(Cout, ci, 9).cpu(), R.narrow_w_copy(src, ci))
    assert bool((dst[-4:] == PAD).all())


@pytest.mark.parametrize("C", [4, 64])
def test_bcast_rows(C):
    B, HW, ldv, ldo = 2, 35, C + 8, C + 4
    v = R.rand(B, ldv, seed=C)
    out = torch.full((B * HW, ldo), PAD, device=DEV)
    vd = _dev(v)
    _bn(8, x=_ptr(vd), ldx=ldv, C=C, N=B, P=HW, scale=1 / 35, out=_ptr(out), ldo=ldo)
    assert torch.equal(out[:, :C].view(B, HW, C).cpu(), R.bcast_rows(v[:, :C], HW, 1 / 35))
    assert bool((out[:, C:] == PAD).all())


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("n", [4, 1028])
def test_grad_commit(n, accumulate):
    g, grad0 = R.rand(n, seed=n), R.rand(n, seed=n + 1)
    if not accumulate:
        grad0 = torch.full((n,), float("nan"))
    grad = torch.full((n + 4,), PAD, device=DEV)
    grad[:n] = grad0.to(DEV)
    gd = _dev(g)
    _bn(9, x=_ptr(gd), out=_ptr(grad), P=n, accumulate=accumulate)
    got = grad[:n].cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got, R.grad_commit(g, grad0, accumulate))
    assert bool((grad[n:] == PAD).all())


@pytest.mark.parametrize("dx", [0, 1])
@pytest.mark.parametrize("cout,cin", [(16, 16), (32, 16), (16, 48), (20, 8)])
def test_pack_conv(cout, cin, dx):
    w = R.rand(cout, cin, 27, seed=cout + cin + dx)
    nout, nin, in_pad, ntiles, kgroups = R.pack_conv_geometry(cout, cin, dx)
    n = ntiles * kgroups * 256
    out = torch.full((n + 4,), PAD, device=DEV)
    wd = _dev(w)
    _launch("kdlae_debug_train_s", TrainSDesc, op=6, inp=[_ptr(wd)], out=_ptr(out), C=cin, O=cout, dir=dx)
    Wm = R.unpack_fragments(out[:n].cpu(), ntiles, kgroups)
    assert torch.equal(Wm, R.pack_conv(w, dx))
    assert torch.equal(out[:n].cpu(), IR.pack_fragments(R.pack_conv(w, dx), ntiles, kgroups))
    v = Wm.view(16 * ntiles, 27, in_pad)
    if 16 * ntiles > nout:
        assert v[nout:].abs().max() == 0
    if in_pad > nin:
        assert v[:, :, nin:].abs().max() == 0
    assert bool((out[n:] == PAD).all())


def test_relu():
    B, Fr, H, W, C, ld = 2, 2, 3, 5, 6, 9
    y = R.rand(B * Fr * H * W, ld, seed=5)
    y[0, 0], y[1, 1], y[2, 2] = -0.0, 0.0, -1e-30
    y[:, C:] = -PAD  # the columns past C are negative and must stay so
    buf = _dev(y)
    _launch("kdlae_debug_train_s", TrainSDesc, op=7, out=_ptr(buf), ldo=ld, C=C, B=B, F=Fr, H=H, W=W)
    got = buf.cpu()
    assert not torch.isnan(got).any()
    assert torch.equal(got[:, :C], R.relu(y[:, :C])) and (got[:, :C] >= 0).all()
    assert bool((got[:, C:] == -PAD).all())

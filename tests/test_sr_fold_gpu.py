"""The sr head's folded conv (csrc/sr_fold.hip: cen and upen.body.0 composed into one 5x5 conv with 9
border-class weight sets, PixelShuffle store) against a float64 evaluation of the unfolded chain.

Every case runs the sr head alone (KDLAE_teacher.forward_sr) on the same hq twice: the default path and
KDLAE_DEBUG=no_sr_fold, which keeps the cen + upen launches of the parent commit.  Reference: conv -> conv ->
pixel_shuffle written here from torch.nn.functional in float64, then the enhance stage and outputen through
the float64 CPU oracle.  The folded path rounds the composed weights once more and sums its 75 products in
another order, so it may not be bit-equal to the parent path; it must sit at the same fp32-rounding level:
    max-abs error  <= 2   x the parent path's,   mean-abs error <= 1.5 x the parent path's.
Shapes: 8 x 8 (every pixel group holds both border columns, every row class in one block), 16 x 24 (a
half-filled pixel group, two row tiles), 40 x 16 (five row tiles, three of them without a border row).

Measured on MI355X (max-abs / mean-abs of sr against the float64 reference, folded | parent):
    8x8   nobias  2.93e-7 / 2.68e-8 | 2.45e-7 / 4.28e-8      8x8   bias  1.96e-7 / 3.00e-8 | 2.39e-7 / 4.51e-8
    16x24 nobias  3.13e-7 / 3.11e-8 | 3.26e-7 / 4.77e-8      16x24 bias  2.97e-7 / 3.44e-8 | 3.54e-7 / 5.04e-8
    40x16 nobias  3.36e-7 / 3.11e-8 | 3.36e-7 / 4.76e-8      40x16 bias  3.26e-7 / 3.41e-8 | 3.17e-7 / 5.10e-8
    16x24 bias, one channel  3.54e-7 / 3.75e-8 | 4.27e-7 / 5.91e-8
    8x8 ring nobias  1.39e-7 / 1.57e-8 | 2.37e-7 / 2.17e-8   8x8 ring bias  1.78e-7 / 1.97e-8 | 1.71e-7 / 2.80e-8
    8x8 ones bias    2.42e-7 / 4.89e-8 | 4.18e-7 / 8.00e-8
(worst ratios: max 1.20, mean 0.73; the folded path's mean is the lower one in every case)
"""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.kdlae_oracle import conv as o_conv, stage as o_stage
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from test_sr_fold_algebra import compose

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
B = 2
SHAPES = [(8, 8), (16, 24), (40, 16)]
DIM = 48

_models = {}


def _model(bias, oc, fold):
    """One small teacher per (bias, out_channels, path); the debug flag is read when its handle is built."""
    key = (bias, oc, fold)
    if key not in _models:
        m = KDLAE_teacher(inp_channels=oc, out_channels=oc, dim=DIM, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1,
                          bias=bias, LayerNorm_type="BiasFree", static="train", params="cat")
        load_hash_weights(m)
        m = m.to(DEV).eval()
        old = os.environ.get("KDLAE_DEBUG")
        try:
            if fold:
                os.environ.pop("KDLAE_DEBUG", None)
            else:
                os.environ["KDLAE_DEBUG"] = "no_sr_fold"
            m.engine(DEV)
        finally:
            if old is None:
                os.environ.pop("KDLAE_DEBUG", None)
            else:
                os.environ["KDLAE_DEBUG"] = old
        _models[key] = m
    return _models[key]


def _reference(m, hq):
    """float64: conv -> conv -> pixel_shuffle spelled out, then enhance and outputen through the oracle."""
    sd = {k: v.detach().double().cpu() for k, v in m.state_dict().items()}
    x = hq.double().cpu()
    s = F.conv2d(x, sd["cen.weight"], sd.get("cen.bias"), padding=1)
    s = F.pixel_shuffle(F.conv2d(s, sd["upen.body.0.weight"], None, padding=1), 2)
    s = o_stage(s, sd, "enhance", 1, 1, "BiasFree")
    return o_conv(s, sd, "outputen", padding=1)


def _errors(bias, oc, hq):
    """(max-abs, mean-abs) of sr against the float64 reference: folded path, parent path."""
    out = []
    ref = _reference(_model(bias, oc, True), hq)
    for fold in (True, False):
        with torch.no_grad():
            sr = _model(bias, oc, fold).forward_sr(hq.to(DEV))
        torch.cuda.synchronize()
        e = (sr.double().cpu() - ref).abs()
        assert torch.isfinite(sr).all()
        out.append((float(e.max()), float(e.mean())))
    return out


def _check(tag, bias, oc, hq):
    (nmax, nmean), (omax, omean) = _errors(bias, oc, hq)
    print(f"SRFOLD {tag} bias={bias} oc={oc}: folded {nmax:.3e} / {nmean:.3e} | parent {omax:.3e} / {omean:.3e}")
    assert nmax <= 2.0 * omax and nmean <= 1.5 * omean, (nmax, omax, nmean, omean)


def _hq(name, oc, H, W):
    return torch.from_numpy(hash_images(name, (B, oc, H, W))) * 2 - 1


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("shape", SHAPES, ids=[f"{h}x{w}" for h, w in SHAPES])
def test_folded_sr_at_parent_accuracy(shape, bias):
    _check(f"{shape[0]}x{shape[1]}", bias, 3, _hq("srfold", 3, *shape))


def test_one_channel():
    _check("16x24", True, 1, _hq("srfold1", 1, 16, 24))


def test_border_ring_input():
    """hq non-zero only in the outermost ring: every contribution passes through a border class."""
    hq = _hq("srfold_ring", 3, 8, 8)
    hq[:, :, 1:-1, 1:-1] = 0
    _check("8x8 ring", False, 3, hq)
    _check("8x8 ring", True, 3, hq)


def test_constant_image_with_bias():
    """hq = 1 with biases: on the border the composed bias differs per class by whole taps."""
    _check("8x8 ones", True, 3, torch.ones(B, 3, 8, 8))


def _record(eng):
    L = _lib.lib()
    n = L.kdlae_t_debug_sr_fold(eng.handle, None, 0, None)
    assert n > 0, _lib.last_error()
    buf = torch.empty(n, device=DEV)
    assert L.kdlae_t_debug_sr_fold(eng.handle, ctypes.c_void_p(buf.data_ptr()), n, None) == n
    torch.cuda.synchronize()
    return buf


@pytest.mark.parametrize("bias", [False, True], ids=["nobias", "bias"])
def test_pack_paths_give_the_same_record(bias):
    """kdlae_t_pack_device and set_param + kdlae_t_commit_params leave bit-equal folded records, and the
    record holds the float64 composition rounded to fp32 in the layout pack_fold_kernel documents."""
    m = _model(bias, 3, True)
    eng = m.engine(DEV)
    L = _lib.lib()
    stream = torch.cuda.current_stream(DEV).cuda_stream
    eng.sync_params(m, stream)
    dev_rec = _record(eng).clone()
    # overwrite the arena from other values, so a commit that skipped the fold could not pass on stale ones
    eng.pack_flat(torch.full((eng.numel,), 0.25, device=DEV), stream)
    assert not torch.equal(_record(eng), dev_rec)
    for name, t in m.state_dict().items():
        host = t.detach().cpu().contiguous()
        _lib.check(L.kdlae_t_set_param(eng.handle, name.encode(), ctypes.c_void_p(host.data_ptr()), host.numel()), name)
    _lib.check(L.kdlae_t_commit_params(eng.handle, None), "commit")
    assert torch.equal(_record(eng), dev_rec)
    # decode: [class][tile t][k-step s][lane]; row li of tile t = output 16 t + 4 (li & 3) + (li >> 2),
    # slot k = 4 s + (lane >> 4) = 25 c + 5 a + b, then the bias slot
    sd = m.state_dict()
    Wc, bc = compose(sd["upen.body.0.weight"].double().cpu().numpy(), sd["cen.weight"].double().cpu().numpy(),
                     sd["cen.bias"].double().cpu().numpy() if bias else None)
    nt, ks = 4 * DIM // 16, (25 * 3 + 4) // 4
    rec = dev_rec.cpu().numpy().reshape(9, nt, ks, 4, 16)             # [cls][t][s][lq][li]
    li = np.arange(16)
    n_of = 16 * np.arange(nt)[:, None] + 4 * (li & 3)[None, :] + (li >> 2)[None, :]   # [t][li]
    got = np.zeros((9, 16 * nt, 4 * ks))
    got[:, n_of] = rec.transpose(0, 1, 4, 2, 3).reshape(9, nt, 16, 4 * ks)
    want = np.concatenate([Wc.reshape(9, 16 * nt, 75), bc[:, :, None], np.zeros((9, 16 * nt, 4 * ks - 76))], axis=2)
    assert np.array_equal(got[:, :, 76:], want[:, :, 76:])
    ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
    assert (np.abs(got - want) <= ulp).all()

"""The PSNR kernel (csrc/metrics.hip) against the numpy oracle (tests/metrics_oracle.py) on the smallest
shapes where it can go wrong, and the Python surface of rethink_acoustic_image_enhancement_amd.metrics.

Bar: sse within 1e-9 relative of the oracle's, max exact.  Each term (float -> double, subtract, square)
is computed in fp64 on both sides; only the order of the fp64 additions differs, which is bounded by
n * 2^-53 relative (n <= 46080 here: 5e-12), orders below the 1e-9 this project uses for its fp64 restatements.
"""
import ctypes
import math

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, metrics
from tests import metrics_oracle as mo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _pair(shape, seed, noise=0.05):
    rng = np.random.RandomState(seed)
    a = rng.rand(*shape).astype(np.float32)
    b = (a + noise * rng.randn(*shape)).astype(np.float32)
    return a, b


def _check(a, b, valid_hw=None, crop_border=0, use_image=False):
    """Kernel reductions and psnr_batch for a [B,C,Hs,Ws] pair against the oracle, image by image."""
    red, n = metrics.psnr_reduce(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), valid_hw, crop_border,
                                 use_image)
    ps = metrics.psnr_batch(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), valid_hw, crop_border, use_image)
    red, ps = red.cpu().numpy(), ps.cpu().numpy()
    for i in range(a.shape[0]):
        sse, mx, n_ref = mo.reduce(a[i], b[i], valid_hw, crop_border, use_image)
        print(f"image {i}: sse {red[i, 0]!r} vs {sse!r}, max {red[i, 1]!r} vs {mx!r}")
        assert n == n_ref
        assert abs(red[i, 0] - sse) <= 1e-9 * abs(sse)
        assert red[i, 1] == mx
        want = mo.psnr_windowed(a[i], b[i], valid_hw, crop_border, use_image)
        assert metrics.finish_psnr(red[i, 0], red[i, 1], n) == pytest.approx(want, rel=1e-9)
        assert ps[i] == pytest.approx(want, rel=1e-9)
    return red


def test_window_1x1_inside_8x8():
    a, b = _pair((1, 1, 8, 8), 1)
    _check(a, b, (1, 1))


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("use_image", [False, True])
def test_unaligned_window_7x13_inside_8x16(C, use_image):
    a, b = _pair((3, C, 8, 16), 2 + C)
    red = _check(a, b, (7, 13), 0, use_image)
    assert len({float(v) for v in red[:, 0]}) == 3   # per-image separation: three different sums


def test_misaligned_operands_take_the_element_path():
    """pred and gt at different offsets within 16 bytes: no common float4 grid."""
    a, b = _pair((2, 3, 8, 16), 9)
    buf = torch.zeros(a.size + 4, device=DEV)
    for shift in (1, 2, 3):
        pa = buf[shift:shift + a.size].view(a.shape)
        pa.copy_(torch.from_numpy(a))
        assert pa.data_ptr() % 16 == 4 * shift and pa.is_contiguous()
        red, n = metrics.psnr_reduce(pa, torch.from_numpy(b).to(DEV), (7, 13))
        for i in range(2):
            sse, mx, _ = mo.reduce(a[i], b[i], (7, 13))
            assert abs(float(red[i, 0]) - sse) <= 1e-9 * sse and float(red[i, 1]) == mx


def test_padded_output_against_unpadded_target():
    """pred stored 8x16 (a padded output), gt stored 7x13 (its target): the window is read in place from both."""
    a, b = _pair((3, 3, 8, 16), 11)
    g = np.ascontiguousarray(b[:, :, :7, :13])
    for use_image in (False, True):
        red, n = metrics.psnr_reduce(torch.from_numpy(a).to(DEV), torch.from_numpy(g).to(DEV), (7, 13), 1, use_image)
        for i in range(3):
            sse, mx, n_ref = mo.reduce(a[i], b[i], (7, 13), 1, use_image)
            assert n == n_ref and abs(float(red[i, 0]) - sse) <= 1e-9 * sse and float(red[i, 1]) == mx
    with pytest.raises(ValueError):
        metrics.psnr_batch(torch.from_numpy(a).to(DEV), torch.from_numpy(g).to(DEV))


def test_crop_border_4_on_40x56():
    a, b = _pair((2, 3, 40, 56), 5)
    _check(a, b, None, 4)
    _check(a, b, (40, 56), 4, True)


def test_crop_border_too_large_is_an_error_not_a_launch():
    a = torch.rand(1, 1, 8, 8, device=DEV)
    L = _lib.lib()
    out = torch.full((1, 2), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(L.kdlae_metric_scratch_bytes()), dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    rc = L.kdlae_metric_psnr(vp(a), vp(a), 1, 1, 8, 8, 8, 8, 8, 8, 4, 0, vp(out), vp(scratch), None)
    assert rc == 1 and "crop_border" in _lib.last_error()          # KDLAE_EINVAL_SHAPE
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[-7.0, -7.0]]                      # nothing ran
    assert L.kdlae_metric_psnr(vp(a), vp(a), 1, 1, 8, 8, 8, 8, 9, 8, 0, 0, vp(out), vp(scratch), None) == 1
    assert L.kdlae_metric_psnr(vp(a), vp(a), 1, 1, 8, 8, 8, 8, 8, 8, 0, 2, vp(out), vp(scratch), None) == 2
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.psnr_batch(a, a, crop_border=4)


def test_multi_block_fixed_order():
    """[3,3,96,160]: 288 window rows per image = 36 blocks each, so the second stage adds real partials."""
    a, b = _pair((3, 3, 96, 160), 6)
    r1 = _check(a, b)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    r2 = metrics.psnr_reduce(ta, tb)[0].cpu().numpy()
    assert r1.tobytes() == r2.tobytes()
    p1, p2 = metrics.psnr_batch(ta, tb), metrics.psnr_batch(ta, tb)
    assert torch.equal(p1, p2)
    _check(a, b, (93, 157), 1, True)


def test_mode1_rounding_ties_and_out_of_range():
    t, u, _, _ = mo.cases()["ties_u8"]
    x = np.float32(255.0) * np.clip(t, 0, 1)
    assert np.count_nonzero(x - np.floor(x) == 0.5) >= 100   # the input really holds half-way cases
    assert t.min() < 0 and t.max() > 1
    red = _check(t[None], u[None], None, 0, True)
    assert red[0, 1] == 255.0


def test_equal_operands_give_inf():
    a, _ = _pair((2, 3, 8, 16), 7)
    ta = torch.from_numpy(a).to(DEV)
    ps = metrics.psnr_batch(ta, ta.clone(), (7, 13))
    assert ps.cpu().tolist() == [float("inf")] * 2
    assert metrics.calculate_psnr(ta[0], ta[0].clone(), 0) == float("inf")


def test_max_value_switch_at_one():
    c = mo.cases()
    a1, b, _, _ = c["max_one"]
    a2, _, _, _ = c["max_above_one"]
    assert a1.max() == 1.0 and a2.max() == np.nextafter(np.float32(1.0), np.float32(2.0))
    p1 = metrics.calculate_psnr(torch.from_numpy(a1).to(DEV), torch.from_numpy(b).to(DEV), 0)
    p2 = metrics.calculate_psnr(torch.from_numpy(a2).to(DEV), torch.from_numpy(b).to(DEV), 0)
    assert p1 == pytest.approx(mo.psnr(a1, b), rel=1e-9) and p2 == pytest.approx(mo.psnr(a2, b), rel=1e-9)
    assert p2 - p1 == pytest.approx(20 * math.log10(255.0), abs=1e-6)   # 48.13 dB


@pytest.mark.parametrize("name", sorted(k for k, v in mo.cases().items() if not v[3]))
def test_calculate_psnr_drop_in(name):
    """Called the reference's way (image_restoration_model.py:333-336) on [1,C,H,W] and [C,H,W]."""
    a, b, cb, _ = mo.cases()[name]
    want = mo.psnr(a, b, cb)
    ta, tb = torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV)
    for x, y in ((ta, tb), (ta[None], tb[None])):
        got = metrics.calculate_psnr(x, y, crop_border=cb, test_y_channel=False)
        assert isinstance(got, float)
        assert got == want or abs(got - want) <= 1e-9 * abs(want)
    with pytest.raises(NotImplementedError):
        metrics.calculate_psnr(ta, tb, cb, test_y_channel=True)


def test_psnr_batch_returns_a_device_tensor():
    a, b = _pair((4, 3, 8, 16), 8)
    ps = metrics.psnr_batch(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), valid_hw=(7, 13))
    assert ps.is_cuda and ps.dtype == torch.float64 and tuple(ps.shape) == (4,)

"""The SSIM kernels (csrc/ssim.hip) against the float64 numpy oracle (tests/ssim_oracle.py) on the smallest
shapes where they can go wrong, the Python surface of rethink_acoustic_image_enhancement_amd.metrics, and
``validate(metrics=("psnr", "ssim"))`` of the two KDLAE trainers.

Bar: 1e-9 absolute on the per-image SSIM (and on each of the kernel's two sums divided by the entry count),
the maximum and the count exact.  Taps, moments, map and sums are fp64 on both sides; the worst map error is
the cancellation in sigma + C2, at most 22 * 2^-53 * L^2 / C2 = 3e-12 relative, and 1e-9 leaves more than 100 x
for the order of the additions.  Identical operands must give exactly 1.0."""
import ctypes
import functools
import json
import os

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, metrics
from tests import ssim_oracle as so

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-9
CASES = so.cases()
PAIRS = sorted((name, v) for name, c in CASES.items() for v in c[4])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


@functools.lru_cache(maxsize=None)
def _want(name, variant):
    a, b, cb, use_image, _ = CASES[name]
    return so.reduce(a, b, None, cb, use_image, variant), so.ssim(a, b, None, cb, use_image, variant)


def _check_row(row, val, name, variant, what):
    (s1, s255, mx, n), want = _want(name, variant)
    print(f"{name} {variant} {what}: kernel {row!r} ssim {val!r}; oracle {(s1, s255, mx, n)!r} ssim {want!r}")
    assert row[3] == n and row[2] == mx
    assert abs(row[0] / n - s1 / n) <= TOL and abs(row[1] / n - s255 / n) <= TOL
    assert abs(val - want) <= TOL
    if name.startswith("equal"):
        assert val == 1.0


@pytest.mark.parametrize("name,variant", PAIRS)
def test_kernel_matches_oracle_and_repeats_bit_for_bit(name, variant):
    a, b, cb, use_image, _ = CASES[name]
    ta, tb = _dev(a[None]), _dev(b[None])
    r1 = metrics.ssim_reduce(ta, tb, None, cb, use_image, variant)
    r2 = metrics.ssim_reduce(ta, tb, None, cb, use_image, variant)
    v = metrics.ssim_batch(ta, tb, None, cb, use_image, variant)
    assert v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (1,)
    assert r1.cpu().numpy().tobytes() == r2.cpu().numpy().tobytes()
    _check_row(r1[0].tolist(), float(v[0]), name, variant, "plain")


@pytest.mark.parametrize("name,variant", PAIRS)
def test_window_inside_larger_storage_is_clamped_to_the_window(name, variant):
    """The case sits top-left in larger pred and gt storage (of different sizes) whose remainder holds 1e30:
    a replicate clamp to storage instead of to the window, or any read past it, gives a wrong number."""
    a, b, cb, use_image, _ = CASES[name]
    C, h, w = a.shape
    pa = np.full((1, C, h + 3, w + 5), 1e30, dtype=np.float32)
    pb = np.full((1, C, h + 1, w + 2), 1e30, dtype=np.float32)
    pa[0, :, :h, :w], pb[0, :, :h, :w] = a, b
    r = metrics.ssim_reduce(_dev(pa), _dev(pb), (h, w), cb, use_image, variant)
    v = metrics.ssim_batch(_dev(pa), _dev(pb), (h, w), cb, use_image, variant)
    _check_row(r[0].tolist(), float(v[0]), name, variant, "embedded")


@pytest.mark.parametrize("name,variant", PAIRS)
def test_operand_alignment_does_not_matter(name, variant):
    """pred and gt at every offset within 16 bytes (relative to each other too): same bits as aligned."""
    a, b, cb, use_image, _ = CASES[name]
    base = metrics.ssim_reduce(_dev(a[None]), _dev(b[None]), None, cb, use_image, variant).cpu().numpy().tobytes()
    bufa, bufb = torch.zeros(a.size + 4, device=DEV), torch.zeros(a.size + 4, device=DEV)
    for sa, sb in ((1, 0), (2, 3), (3, 3), (0, 2)):
        ta, tb = bufa[sa:sa + a.size].view((1,) + a.shape), bufb[sb:sb + a.size].view((1,) + a.shape)
        ta.copy_(_dev(a[None]))
        tb.copy_(_dev(b[None]))
        assert ta.data_ptr() % 16 == 4 * sa and tb.data_ptr() % 16 == 4 * sb and ta.is_contiguous()
        r = metrics.ssim_reduce(ta, tb, None, cb, use_image, variant)
        assert r.cpu().numpy().tobytes() == base
    _check_row(np.frombuffer(base, dtype=np.float64).tolist(), float(metrics.ssim_batch(ta, tb, None, cb, use_image,
                                                                                          variant)[0]),
               name, variant, "misaligned")


@pytest.mark.parametrize("variant", ["basicsr", "valid"])
@pytest.mark.parametrize("use_image", [False, True])
def test_batch_of_three_distinct_images(variant, use_image):
    a, b = so.batch()
    r = metrics.ssim_reduce(_dev(a), _dev(b), (19, 27), 1, use_image, variant).cpu().numpy()
    v = metrics.ssim_batch(_dev(a), _dev(b), (19, 27), 1, use_image, variant).cpu().numpy()
    assert len({float(x) for x in v}) == 3
    for i in range(3):
        s1, s255, mx, n = so.reduce(a[i], b[i], (19, 27), 1, use_image, variant)
        want = so.ssim(a[i], b[i], (19, 27), 1, use_image, variant)
        print(f"image {i}: {r[i]!r} {v[i]!r} vs {(s1, s255, mx, n)!r} {want!r}")
        assert r[i, 3] == n and r[i, 2] == mx
        assert abs(r[i, 0] - s1) / n <= TOL and abs(r[i, 1] - s255) / n <= TOL and abs(v[i] - want) <= TOL


def _period4(shape, seed):
    rng = np.random.RandomState(seed)
    a = rng.rand(4, *shape).astype(np.float32)
    b = np.clip(a + 0.05 * rng.randn(4, *shape), 0, 1).astype(np.float32)
    return a, b


def test_blocks_that_walk_several_tiles():
    """B = 4096 images of 3 x 2 tiles: the scratch holds 16384 / 4096 = 4 partials per image, so blocks 0 and 1
    take two tiles each.  The batch repeats four distinct images."""
    a, b = _period4((1, 33, 17), 31)
    ta, tb = _dev(a).repeat(1024, 1, 1, 1), _dev(b).repeat(1024, 1, 1, 1)
    v = metrics.ssim_batch(ta, tb).cpu().numpy()
    want = np.array([so.ssim(a[i], b[i]) for i in range(4)])
    print(v[:4], want)
    assert np.array_equal(v, np.tile(v[:4], 1024))
    assert np.abs(v[:4] - want).max() <= TOL


def test_batch_larger_than_the_scratch_goes_out_in_two_launches():
    a, b = _period4((1, 3, 5), 32)
    n = 16384 + 4
    ta, tb = _dev(a).repeat(n // 4, 1, 1, 1), _dev(b).repeat(n // 4, 1, 1, 1)
    v = metrics.ssim_batch(ta, tb).cpu().numpy()
    want = np.array([so.ssim(a[i], b[i]) for i in range(4)])
    assert v.shape == (n,) and np.array_equal(v, np.tile(v[:4], n // 4))
    assert np.abs(v[:4] - want).max() <= TOL


def test_errors_are_found_before_anything_runs():
    a = torch.rand(1, 3, 16, 16, device=DEV)
    L = _lib.lib()
    out = torch.full((1, 4), -7.0, dtype=torch.float64, device=DEV)
    scratch = torch.empty(int(L.kdlae_metric_ssim_scratch_bytes()), dtype=torch.uint8, device=DEV)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    call = lambda C, h, cb, mode, var: L.kdlae_metric_ssim(vp(a), vp(a), 1, C, 16, 16, 16, 16, h, 16, cb, mode, var,  # noqa: E731
                                                            vp(out), vp(scratch), None)
    assert call(3, 16, 8, 0, 0) == 1 and "crop_border" in _lib.last_error()
    assert call(3, 17, 0, 0, 0) == 1 and call(3, 16, 3, 0, 1) == 1 and call(5, 16, 0, 0, 0) == 1
    assert call(3, 16, 0, 2, 0) == 2 and call(3, 16, 0, 0, 2) == 2
    torch.cuda.synchronize()
    assert out.cpu().tolist() == [[-7.0] * 4]
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.ssim_batch(a, a, crop_border=3, variant="valid")
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.ssim_batch(torch.rand(1, 5, 16, 16, device=DEV), torch.rand(1, 5, 16, 16, device=DEV))
    # the valid flavour has no channel mix and takes any channel count
    x, y = np.random.RandomState(3).rand(2, 5, 12, 14).astype(np.float32)
    got = float(metrics.ssim_batch(_dev(x[None]), _dev(y[None]), variant="valid")[0])
    assert abs(got - so.ssim(x, y, variant="valid")) <= TOL


@pytest.mark.parametrize("name", sorted(k for k, c in CASES.items() if not c[3]))
def test_drop_ins_return_python_floats(name):
    a, b, cb, _, variants = CASES[name]
    ta, tb = _dev(a), _dev(b)
    want = so.ssim(a, b, None, cb, False, "basicsr")
    for x, y in ((ta, tb), (ta[None], tb[None])):
        got = metrics.calculate_ssim(x, y, crop_border=cb, test_y_channel=False)
        assert isinstance(got, float) and abs(got - want) <= TOL
    with pytest.raises(NotImplementedError):
        metrics.calculate_ssim(ta, tb, cb, test_y_channel=True)
    with pytest.raises(NotImplementedError):
        metrics.calculate_psnr(ta, tb, cb, test_y_channel=True)
    with pytest.raises(ValueError):
        metrics.calculate_ssim(torch.stack([ta, ta]), torch.stack([tb, tb]), cb)
    if "valid" in variants:
        # Train/utils.py's function works on the 0..255 scale
        got = metrics.calculate_ssim_valid(ta * 255.0, tb * 255.0, border=cb)
        want = so.ssim((a * np.float32(255.0)).astype(np.float32), (b * np.float32(255.0)).astype(np.float32), None, cb,
                       False, "valid")
        assert isinstance(got, float) and abs(got - want) <= TOL


# ------------------------------------------------------------------ validate(metrics=...)
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher  # noqa: E402
from rethink_acoustic_image_enhancement_amd.train import KDLAESTrainer, KDLAETrainer  # noqa: E402
from tests.util import GOLDEN  # noqa: E402

H, W = 20, 28   # ragged: pads to 24 x 32


def _img(tag, shape):
    return torch.from_numpy(hash_images(tag, shape)).to(DEV)


def test_teacher_validate_reports_ssim_over_the_psnr_windows():
    m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
    load_hash_weights(m)
    tr = KDLAETrainer(m.to(DEV), lr=1e-3)
    items = []
    for i in range(2):
        lq = {"img": _img(f"ssim_t_img{i}", (1, 3, H, W)), "denoise_rate": _img(f"ssim_t_rate{i}", (1, 1, H, W))}
        gt = {"hq": _img(f"ssim_t_hq{i}", (1, 3, H, W)), "sr": _img(f"ssim_t_sr{i}", (1, 3, 2 * H, 2 * W))}
        items.append((lq, gt))
    for cb, use_image in ((0, False), (2, True)):
        want_hq, want_sr = [], []
        for lq, gt in items:
            tr.validate([(lq, gt)])
            assert tuple(tr.val_output["hq"].shape) == (1, 3, H, W)
            want_hq.append(so.ssim(tr.val_output["hq"][0].cpu().numpy(), gt["hq"][0].cpu().numpy(), None, cb, use_image))
            want_sr.append(so.ssim(tr.val_output["sr"][0].cpu().numpy(), gt["sr"][0].cpu().numpy(), None, cb, use_image))
        base = tr.validate(items, crop_border=cb, use_image=use_image)
        res = tr.validate(items, crop_border=cb, use_image=use_image, metrics=("psnr", "ssim"))
        print(res, np.mean(want_hq), np.mean(want_sr))
        assert set(base) == {"psnr_hq", "psnr_sr"}                       # the default is what it was
        assert set(res) == {"psnr_hq", "psnr_sr", "ssim_hq", "ssim_sr"} and all(isinstance(v, float) for v in res.values())
        assert res["psnr_hq"] == base["psnr_hq"] and res["psnr_sr"] == base["psnr_sr"]
        assert abs(res["ssim_hq"] - np.mean(want_hq)) <= TOL and abs(res["ssim_sr"] - np.mean(want_sr)) <= TOL
    assert set(tr.validate(items, metrics=("ssim",))) == {"ssim_hq", "ssim_sr"}
    with pytest.raises(ValueError, match="unknown metric"):
        tr.validate(items, metrics=("psnr", "niqe"))


def test_student_validate_reports_ssim():
    d = np.load(os.path.join(GOLDEN, "train_s_1frame.npz"), allow_pickle=False)
    m = KDLAE_student(**json.loads(bytes(d["cfg"]).decode()))
    load_hash_weights(m)
    tr = KDLAESTrainer(m.to(DEV).train(), lr=1e-3)
    items = [(_img(f"ssim_s_x{i}", (2, 1, 12, 20)), _img(f"ssim_s_t{i}", (2, 1, 12, 20))) for i in range(2)]
    want = []
    for lq, gt in items:
        tr.validate([(lq, gt)])
        want += [so.ssim(tr.val_output[b].cpu().numpy(), gt[b].cpu().numpy()) for b in range(2)]
    base = tr.validate(items)
    res = tr.validate(items, metrics=("psnr", "ssim"))
    print(res, np.mean(want))
    assert set(base) == {"psnr"} and set(res) == {"psnr", "ssim"} and res["psnr"] == base["psnr"]
    assert abs(res["ssim"] - np.mean(want)) <= TOL
    assert tr.model.training
    with pytest.raises(ValueError, match="unknown metric"):
        tr.validate(items, metrics="fid")

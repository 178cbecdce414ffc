"""The NIQE kernels (csrc/niqe.hip) against the numpy oracle's float64 mode (tests/niqe_oracle.py), the Python
surface of rethink_acoustic_image_enhancement_amd.metrics, and ``validate(niqe=True)`` of the two KDLAE trainers.

Bars:
* both MSCN fields: bit for bit (the oracle walks the 49 taps in the kernel's order, fp64 multiply and add);
* the counts n_neg / n_pos: exact;
* each fp64 sum: 1e-11 of the sum of the magnitudes of its terms (all terms are >= 0, so of the sum itself): at
  most 9216 additions of 2^-53 each are 1.0e-12, and the bar is ten times that;
* the score: the tolerance recorded in tests/golden/niqe.json, 8 x the worst score change when the oracle's
  moments move by 1e-11 relative (tests/test_niqe.py re-measures it and checks that no argmin of the inputs is
  within reach of such a move).
Each case runs alone, inside larger storage filled with 1e30, at the four float offsets within 16 bytes, and
twice for equal bits."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, metrics
from tests import niqe_oracle as no

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SUM_TOL = 1e-11
SCORE_TOL = float(json.load(open(os.path.join(no.GOLDEN, "niqe.json")))["perturbation"]["gpu_score_tolerance"])
P = no.params()
CASES = no.cases()


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).to(DEV)


def _check(mom, f1, f2, want, what):
    """One image's kernel results against the oracle's (score, features, fields, margin, moments)."""
    s, _, (g1, g2), _, (m1, m2) = want
    assert f1.dtype == np.float32 and f1.shape == g1.shape and f2.shape == g2.shape
    for f, g, tag in ((f1, g1, "scale 1"), (f2, g2, "scale 2")):
        diff = int((f.view(np.uint32) != np.ascontiguousarray(g).view(np.uint32)).sum())
        print(f"{what} {tag}: {diff} of {f.size} field entries differ")
        assert diff == 0
    for scale, got, ref in ((1, mom[0], m1), (2, mom[1], m2)):
        assert got.shape == ref.shape
        assert np.array_equal(got[..., :2], ref[..., :2])
        err = np.abs(got[..., 2:] - ref[..., 2:])
        print(f"{what} scale {scale}: worst sum error {np.max(err / np.maximum(ref[..., 2:], 1e-300)):.3e} relative")
        assert (err <= SUM_TOL * ref[..., 2:]).all()
    got_s = metrics.finish_niqe(mom, P)
    print(f"{what}: score {got_s!r} oracle {s!r} (tol {SCORE_TOL:.3e})")
    assert abs(got_s - s) <= SCORE_TOL


def _run(t, valid_hw, cb, use_image):
    mom, f1, f2 = metrics.niqe_reduce(t, valid_hw, cb, use_image, P, fields=True)
    assert mom.is_cuda and mom.dtype == torch.float64
    return mom.cpu().numpy(), f1.cpu().numpy(), f2.cpu().numpy()


@pytest.mark.parametrize("name", sorted(CASES))
def test_kernel_matches_oracle_alone_embedded_and_at_every_offset(name):
    x, cb, use_image = CASES[name]
    want = no.reference(name)
    C, h, w = x.shape
    mom, f1, f2 = _run(_dev(x[None]), None, cb, use_image)
    assert mom.shape == (1, 2, (h - 2 * cb) // 96 * ((w - 2 * cb) // 96), 5, 5)
    _check(mom[0], f1[0], f2[0], want, f"{name} plain")
    again = _run(_dev(x[None]), None, cb, use_image)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((mom, f1, f2), again))
    # top-left in larger storage whose remainder holds 1e30: a clamp to storage, or any read past the window,
    # gives a wrong number
    big = np.full((1, C, h + 3, w + 5), 1e30, dtype=np.float32)
    big[0, :, :h, :w] = x
    emb = _run(_dev(big), (h, w), cb, use_image)
    assert all(a.tobytes() == b.tobytes() for a, b in zip((mom, f1, f2), emb))
    buf = torch.zeros(x.size + 4, device=DEV)
    for off in (1, 2, 3):
        t = buf[off:off + x.size].view((1,) + x.shape)
        t.copy_(_dev(x[None]))
        assert t.data_ptr() % 16 == 4 * off and t.is_contiguous()
        assert all(a.tobytes() == b.tobytes() for a, b in zip((mom, f1, f2), _run(t, None, cb, use_image)))
    if name.startswith("sonar"):
        assert (mom[0, :, 0, :, :2] == 0).all()   # the block of zeros: nothing on either side in any map
    got = float(metrics.niqe_batch(_dev(x[None]), None, cb, use_image, params=P)[0])
    assert abs(got - want[0]) <= SCORE_TOL


def test_batch_of_three_distinct_images():
    x = no.batch()
    mom, f1, f2 = _run(_dev(x), None, 0, False)
    v = metrics.niqe_batch(_dev(x), None, 0, False, params=P)
    assert not v.is_cuda and v.dtype == torch.float64 and tuple(v.shape) == (3,) and len({float(s) for s in v}) == 3
    for i in range(3):
        s, feat, (g1, g2), margin = no.niqe(x[i], 0, False, P, detail=True)
        _check(mom[i], f1[i], f2[i], (s, feat, (g1, g2), margin, (no.moments(g1, 1), no.moments(g2, 2))), f"image {i}")
        assert abs(float(v[i]) - s) <= SCORE_TOL


def test_drop_in_returns_python_floats():
    for name in ("noise_c1_192x96", "noise_c3_192x96", "sonar_c1_200x300_cb4"):
        x, cb, use_image = CASES[name]
        assert not use_image
        for t in (_dev(x), _dev(x[None])):
            got = metrics.calculate_niqe(t, cb, params=P)
            assert isinstance(got, float) and abs(got - no.reference(name)[0]) <= SCORE_TOL
    t = _dev(CASES["noise_c1_192x96"][0])
    with pytest.raises(NotImplementedError, match="gray"):
        metrics.calculate_niqe(t, 0, convert_to="gray", params=P)
    with pytest.raises(ValueError):
        metrics.calculate_niqe(torch.stack([t, t]), 0, params=P)
    with pytest.raises(FileNotFoundError):
        metrics.calculate_niqe(t, 0, params=os.path.join(no.GOLDEN, "no_such_params.npz"))
    # a single complete block: no covariance, nan (the reference raises from pinv)
    assert np.isnan(metrics.calculate_niqe(t[:, :96], 0, params=P))


def test_errors_are_found_before_anything_runs():
    a = torch.rand(1, 3, 200, 300, device=DEV)
    L = _lib.lib()
    out = torch.full((1, 2, 6, 5, 5), -7.0, dtype=torch.float64, device=DEV)
    nbytes = int(L.kdlae_metric_niqe_scratch_bytes(1, 200, 300))
    scratch = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    win = np.ascontiguousarray(P["gaussian_window"], dtype=np.float64)
    vp = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731

    def call(C=3, h=200, cb=0, mode=0, convert=0, nb=nbytes, o=out):
        return L.kdlae_metric_niqe(vp(a), 1, C, 200, 300, h, 300, cb, mode, convert,
                                   win.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), vp(o) if o is not None else None,
                                   None, None, vp(scratch), nb, None)
    assert call(C=2) == 1 and call(cb=100) == 1 and "crop_border" in _lib.last_error()
    assert call(cb=53) == 1 and call(h=95) == 1 and call(h=201) == 1 and call(nb=nbytes // 2) == 1
    assert call(mode=2) == 2 and call(convert=1) == 2 and call(o=None) == 2
    torch.cuda.synchronize()
    assert (out.cpu() == -7.0).all()
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.niqe_batch(torch.rand(1, 2, 96, 96, device=DEV), params=P)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.niqe_batch(torch.rand(1, 1, 96, 95, device=DEV), params=P)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        metrics.niqe_batch(a, crop_border=53, params=P)


# ------------------------------------------------------------------ validate(niqe=True)
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights  # noqa: E402
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher  # noqa: E402
from rethink_acoustic_image_enhancement_amd.train import KDLAESTrainer, KDLAETrainer  # noqa: E402
from tests.util import GOLDEN  # noqa: E402

H, W = 100, 196   # ragged: pads to 104 x 200; with crop_border 2 NIQE sees 96 x 192 (hq) and 192 x 384 (sr)


def _same(got, want):
    return (np.isnan(got) and np.isnan(want)) or abs(got - want) <= SCORE_TOL


def _img(tag, shape):
    return torch.from_numpy(hash_images(tag, shape)).to(DEV)


def test_teacher_validate_reports_niqe_and_leaves_the_other_metrics_alone():
    m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
    load_hash_weights(m)
    tr = KDLAETrainer(m.to(DEV), lr=1e-3)
    lq = {"img": _img("niqe_t_img", (1, 3, H, W)), "denoise_rate": _img("niqe_t_rate", (1, 1, H, W))}
    gt = {"hq": _img("niqe_t_hq", (1, 3, H, W)), "sr": _img("niqe_t_sr", (1, 3, 2 * H, 2 * W))}
    items = [(lq, gt)]
    base = tr.validate(items, crop_border=2, metrics=("psnr", "ssim"))
    res = tr.validate(items, crop_border=2, metrics=("psnr", "ssim"), niqe=True, niqe_params=P)
    assert set(res) == set(base) | {"niqe_hq", "niqe_sr"} and all(isinstance(v, float) for v in res.values())
    assert all(res[k] == base[k] for k in base)
    want_hq = no.niqe(tr.val_output["hq"][0].cpu().numpy(), 2, True, P)
    want_sr = no.niqe(tr.val_output["sr"][0].cpu().numpy(), 2, True, P)
    print(res, want_hq, want_sr)
    assert _same(res["niqe_hq"], want_hq) and _same(res["niqe_sr"], want_sr)
    assert set(tr.validate(items)) == {"psnr_hq", "psnr_sr"}                 # the default is what it was
    with pytest.raises(ValueError, match="unknown metric"):
        tr.validate(items, metrics=("psnr", "niqe"))
    with pytest.raises(FileNotFoundError):
        tr.validate(items, niqe=True, niqe_params=os.path.join(GOLDEN, "no_such_params.npz"))


def test_student_validate_reports_niqe():
    d = np.load(os.path.join(GOLDEN, "train_s_1frame.npz"), allow_pickle=False)
    m = KDLAE_student(**json.loads(bytes(d["cfg"]).decode()))
    load_hash_weights(m)
    tr = KDLAESTrainer(m.to(DEV).train(), lr=1e-3)
    items = [(_img(f"niqe_s_x{i}", (2, 1, 100, 196)), _img(f"niqe_s_t{i}", (2, 1, 100, 196))) for i in range(2)]
    want = []
    for lq, gt in items:
        tr.validate([(lq, gt)])
        want += [no.niqe(tr.val_output[b].cpu().numpy(), 0, True, P) for b in range(2)]
    base = tr.validate(items, metrics=("psnr", "ssim"))
    res = tr.validate(items, metrics=("psnr", "ssim"), niqe=True, niqe_params=P)
    print(res, np.mean(want))
    assert set(base) == {"psnr", "ssim"} and set(res) == {"psnr", "ssim", "niqe"}
    assert res["psnr"] == base["psnr"] and res["ssim"] == base["ssim"]
    assert _same(res["niqe"], np.mean(want))
    assert tr.model.training

"""Dataset sample transforms on the GPU (csrc/data.hip through dataset.py) against the numpy oracle
(tests/dataset_oracle.py) and the goldens recorded from the reference: bit for bit everywhere except the Philox
normals, which are held to the float64 Box-Muller model within the bound of profiles/dataset_probe.json."""
import ctypes
import itertools
import json
import os
import random

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, augment, dataset
from tests import dataset_oracle as do

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "dataset_sample.json")))
GOLD = np.load(os.path.join(HERE, "golden", "dataset_sample.npz"))
DEV = "cuda:0"
FILL = np.float32(1e30)


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def dev_src(a, layout):
    """u8 sources stay HWC-interleaved, fp32 ones go CHW-planar (the two layouts the strides must serve)."""
    if layout == "u8":
        return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return torch.from_numpy(np.ascontiguousarray(do.to_float(a).transpose(2, 0, 1))).to(DEV)


def slot(shape, offset):
    """A dst of ``shape`` at float offset ``offset`` inside 1e30-filled storage; (storage, view)."""
    n = int(np.prod(shape))
    store = torch.full((n + 8,), float(FILL), dtype=torch.float32, device=DEV)
    return store, store[offset:offset + n].view(*shape)


def check_slot(store, offset, want):
    got = store.cpu().numpy()
    n = want.size
    assert np.all(got[:offset] == FILL) and np.all(got[offset + n:] == FILL), "written outside the slot"
    assert same(got[offset:offset + n].reshape(want.shape), want)


def geometry_cases():
    """(source size, C, layout, item kwargs): every code, pad mode, pad length, deficit parity and canvas edge."""
    out = []
    k = 0
    for (H, W) in ((5, 7), (8, 8), (13, 6)):
        for C, layout in itertools.product((1, 3), ("u8", "f32")):
            for mode in ("none", "reflect101", "symmetric"):
                pads = (0,) if mode == "none" else (0, 1, min(H, W) - 1)
                for pad in pads:
                    if mode != "none" and pad == 0 and C == 3:
                        continue
                    Hc, Wc = H + (k % 3), W + ((k + 1) % 4)       # odd and even centre-pad deficits, and none
                    Hp, Wp = Hc + pad, Wc + (pad if k % 2 else 0)
                    if mode == "none":
                        Hp, Wp = Hc, Wc
                    h, w = min(4, Hp), min(5, Wp)
                    # windows touching each canvas edge in turn, and the whole canvas
                    win = ((0, 0, h, w), (Hp - h, Wp - w, h, w), (0, Wp - w, h, w), (Hp - h, 0, h, w), (0, 0, Hp, Wp))[k % 5]
                    out.append(((H, W), C, layout, dict(canvas=(Hc, Wc), padded=(Hp, Wp), pad_mode=mode, window=win,
                                                        code=k % 8, bgr2rgb=bool(k % 2) and C == 3)))
                    k += 1
    # every code on a non-square window of a u8 and an fp32 source, both channel orders
    for code, layout in itertools.product(range(8), ("u8", "f32")):
        out.append(((5, 7), 3, layout, dict(padded=(7, 9), pad_mode="symmetric", window=(1, 2, 5, 6), code=code,
                                            bgr2rgb=code % 2 == 0)))
    return out


def item_of(src, dst, kw, **extra):
    return dict(src=src, dst=dst, canvas=kw.get("canvas", None) or tuple(src.shape[:2] if src.dtype == torch.uint8
                                                                        else src.shape[1:]),
                padded=kw.get("padded") or kw.get("canvas") or tuple(src.shape[:2] if src.dtype == torch.uint8 else src.shape[1:]),
                pad_mode=kw.get("pad_mode", "none"), window=kw.get("window"), dihedral=kw.get("code", 0),
                bgr2rgb=kw.get("bgr2rgb", False), **extra)


def clean(d):
    return {k: v for k, v in d.items() if v is not None}


def test_geometry_bit_for_bit_one_item_per_launch():
    for n, ((H, W), C, layout, kw) in enumerate(geometry_cases()):
        a = do.hash_u8(f"geo/{n}", (H, W, C))
        want = do.sample(a, **kw)
        src = dev_src(a, layout)
        off = n % 4
        for _ in range(2):      # twice for equal bits
            store, dst = slot(want.shape, off)
            dataset.sample_transform([clean(item_of(src, dst, kw))])
            check_slot(store, off, want)


def test_geometry_seven_item_table_and_sr_at_twice_the_draw():
    cases = geometry_cases()[3::9][:5]
    items, checks = [], []
    for n, ((H, W), C, layout, kw) in enumerate(cases):
        a = do.hash_u8(f"table/{n}", (H, W, C))
        want = do.sample(a, **kw)
        store, dst = slot(want.shape, n % 4)
        items.append(clean(item_of(dev_src(a, layout), dst, kw)))
        checks.append((store, n % 4, want))
    # gt and sr of one draw: the same window at x2 on a source of twice the size, one dihedral code
    gt, sr = do.hash_u8("table/gt", (9, 7, 3)), do.hash_u8("table/sr", (18, 14, 3))
    for a, s in ((gt, 1), (sr, 2)):
        kw = dict(padded=(10 * s, 8 * s), pad_mode="reflect101", window=(2 * s, 1 * s, 6 * s, 5 * s), code=5, bgr2rgb=True)
        want = do.sample(a, **kw)
        store, dst = slot(want.shape, s)
        items.append(clean(item_of(dev_src(a, "u8"), dst, kw)))
        checks.append((store, s, want))
    assert len(items) == 7
    dataset.sample_transform(items)
    for store, off, want in checks:
        check_slot(store, off, want)


def test_u8_to_f32_is_a_true_division():
    v = np.arange(256, dtype=np.uint8).reshape(16, 16)
    dst = torch.empty((1, 16, 16), device=DEV)
    dataset.sample_transform([dict(src=torch.from_numpy(v).to(DEV), dst=dst)])
    assert same(dst.cpu().numpy()[0], v.astype(np.float32) / np.float32(255))


def test_normalisation_in_sample_and_channel_order():
    a = do.hash_u8("norm", (6, 5, 3))
    mean, std = [0.4, 0.5, 0.6], [0.2, 0.25, 0.3]
    want = do.sample(a, bgr2rgb=True, code=6, mean=mean, std=std)
    dst = torch.empty(want.shape, device=DEV)
    dataset.sample_transform([dict(src=torch.from_numpy(a).to(DEV), dst=dst, bgr2rgb=True, dihedral=6,
                                   mean=torch.tensor(mean, device=DEV), std=torch.tensor(std, device=DEV))])
    assert same(dst.cpu().numpy(), want)


def test_host_noise_route_against_oracle_and_reference():
    img = do.hash_u8("step/hwc", (13, 6, 3))
    for name, loc, scale, div, draw in (("add_random_noise", 0.3, 0.7, 1.0, "std"), ("add_gaussian_noise", 0.0, None, 255.0, "randn")):
        np.random.seed(META["steps"][name]["np_seed"])
        if draw == "randn":
            scale = np.random.uniform(1, 30)
            z = np.random.randn(13, 6, 3)
        else:
            z = np.random.standard_normal((13, 6, 3))
        ref = GOLD[f"steps/{name}/out"]                     # HWC, no flip
        dst = torch.empty((3, 13, 6), device=DEV)
        dataset.sample_transform([dict(src=torch.from_numpy(img).to(DEV), dst=dst,
                                       noise=dict(loc=loc, scale=scale, div=div, z=torch.from_numpy(z).to(DEV)))])
        assert same(dst.cpu().numpy(), ref.transpose(2, 0, 1))
    assert GOLD["steps/add_random_noise/out"].min() == 0.0 and GOLD["steps/add_random_noise/out"].max() == 1.0
    # noise is indexed before the dihedral map and the channel reversal; a non-square window, fp32 source
    a = do.hash_u8("noise/pre", (7, 9, 3))
    z = np.random.RandomState(3).standard_normal((5, 6, 3)) * 3     # clips at both ends
    for code in range(8):
        kw = dict(window=(1, 2, 5, 6), code=code, bgr2rgb=True)
        want = do.sample(a, z=z, loc=0.1, scale=0.5, div=3.0, **kw)
        assert want.min() == 0.0 and want.max() == 1.0
        dst = torch.empty(want.shape, device=DEV)
        dataset.sample_transform([dict(src=dev_src(a, "f32"), dst=dst, window=kw["window"], dihedral=code, bgr2rgb=True,
                                       noise=dict(loc=0.1, scale=0.5, div=3.0, z=torch.from_numpy(z).to(DEV)))])
        assert same(dst.cpu().numpy(), want), code


def test_conditional_noise_at_the_threshold():
    n, thr = 7 * 9 * 3, 0.64                 # 0.64 * 189 = 120.96: c / n == 0.64 has no solution, the at-case is 120
    c_at = int(np.floor(thr * n))
    assert c_at / n <= thr < (c_at + 1) / n
    a = do.hash_u8("cond", (7, 9, 3))
    z = np.random.RandomState(5).standard_normal((7, 9, 3))
    noisy, plain = do.sample(a, z=z, loc=0.3, scale=0.7), do.sample(a)
    assert not same(noisy, plain)
    for c0, c1, want in ((c_at - 1, 0, plain), (c_at, 3, plain), (0, c_at, plain), (c_at + 1, 0, noisy), (2, c_at + 1, noisy)):
        counts = torch.tensor([c0, c1], dtype=torch.int32, device=DEV)
        dst = torch.empty(want.shape, device=DEV)
        dataset.sample_transform([dict(src=torch.from_numpy(a).to(DEV), dst=dst,
                                       noise=dict(loc=0.3, scale=0.7, z=torch.from_numpy(z).to(DEV), counts=counts,
                                                  thr=thr, n=n))])
        assert same(dst.cpu().numpy(), want), (c0, c1)


def philox_bound():
    """8 x the largest |z_gpu - z_model| measured over one 64 x 64 x 3 draw on the MI355X
    (profiles/dataset_probe.json, tools/dataset_probe.py), capped at 1e-5 on z."""
    with open(os.path.join(os.path.dirname(HERE), "profiles", "dataset_probe.json")) as f:
        measured = float(json.loads(f.readline())["philox_normal"]["max_abs_z_err"])
    return min(8.0 * measured, 1e-5)


def philox_draw(h, w, C, seed, call, loc, scale, x, extra_items=0):
    """[h, w, C] of clip(x + loc + scale * z) with Philox normals over a constant fp32 source (item 0 of a table)."""
    return do.gpu_philox_draw(h, w, C, seed, call, loc, scale, x, extra_items)


def test_philox_noise_against_the_float64_model():
    bound = philox_bound()
    h, w, C, seed, call = 64, 64, 3, 0x123456789ABCDEF, 5
    zm = do.philox_normal(h, w, C, seed, call)
    zg = do.gpu_philox_z(h, w, C, seed, call)           # the kernel's fp32 z, recovered exactly
    err = np.abs(zg.astype(np.float64) - zm).max()
    print(f"philox: max |z_gpu - z_model| = {err:.3e} (bound {bound:.3e})")
    assert np.abs(zg).max() < 5.78 and err <= bound
    # the mask of clipped positions, except where the model's pre-clip value lies within the bound of 0 or 1
    # (the bound on z times the scale, plus half an ulp of the fp32 result)
    out2 = philox_draw(h, w, C, seed, call, 0.3, 0.7, 0.25)
    pre = 0.25 + (0.3 + 0.7 * zm)
    tol = 0.7 * bound + 2.0 ** -25
    sure = (np.abs(pre) > tol) & (np.abs(pre - 1) > tol)
    assert np.array_equal((out2 == 0)[sure], (pre <= 0)[sure]) and np.array_equal((out2 == 1)[sure], (pre >= 1)[sure])
    assert (out2 == 0).any() and (out2 == 1).any() and sure.mean() > 0.99
    inner = (pre > 0) & (pre < 1) & sure
    assert np.abs(out2.astype(np.float64) - pre)[inner].max() <= tol
    # equal bits twice, and across two grid sizes (48 blocks alone; 32 per item, grid-striding, in a 64-item table)
    assert same(out2, philox_draw(h, w, C, seed, call, 0.3, 0.7, 0.25))
    assert same(out2, philox_draw(h, w, C, seed, call, 0.3, 0.7, 0.25, extra_items=63))
    assert not same(out2, philox_draw(h, w, C, seed, call + 1, 0.3, 0.7, 0.25))


def test_count():
    B, n = 3, 256 * 5 + 37                    # more than one block and a last partial one
    rs = np.random.RandomState(0)
    x = rs.rand(B, n).astype(np.float32) * 0.9 + 0.05
    plant = [(0, 0), (n, 0), (17, 300)]
    for b, (c0, c1) in enumerate(plant):
        idx = rs.permutation(n)
        x[b, idx[:c0]] = 0.0
        x[b, idx[c0:c0 + c1]] = 1.0
    x[2, np.flatnonzero(x[2] == 0)[:5]] = -0.0          # -0.0 counts as zero
    x[0, -1] = 1.0                                       # the last element of a partial block
    counts = torch.full((B, 2), 0x7FFF1234, dtype=torch.int32, device=DEV)   # garbage on entry
    out = dataset.count_zeros_ones(torch.from_numpy(x).to(DEV), out=counts)
    want = [[int(np.sum(x[b] == 0)), int(np.sum(x[b] == 1))] for b in range(B)]
    assert out.cpu().tolist() == want == [[0, 1], [n, 0], [17, 300]]
    assert dataset.count_zeros_ones(torch.from_numpy(x).to(DEV).view(B, 1, n)).cpu().tolist() == want


def test_finish():
    C, H, W = 3, 5, 7
    n = C * H * W
    x = np.full((4, C, H, W), 0.5, np.float32)
    x[:, 0, 0, :3] = [1.0 / 255.0, 1.0, 0.0]
    x = x.astype(np.float32)
    x[:, 0, 0, 0] = np.float32(1) / np.float32(255)
    c_at = int(np.floor(0.10 * n))                       # 10: 10 / 105 < 0.1 < 11 / 105
    counts = torch.tensor([[c_at, 0], [c_at + 1, 0], [0, c_at + 1], [0, c_at]], dtype=torch.int32, device=DEV)
    t = torch.from_numpy(x).to(DEV)
    assert dataset.finish(t, counts, 0.10) is t
    got = t.cpu().numpy()
    assert same(got[0], x[0]) and same(got[3], x[3])
    for b in (1, 2):
        assert got[b, 0, 0, 2] == np.float32(1e-14) and got[b, 0, 0, 2].tobytes() == np.float32(1e-14).tobytes()
        keep = np.ones((C, H, W), bool)
        keep[0, 0, 2] = False
        assert same(got[b][keep], x[b][keep])            # 1 / 255, 1.0 and 0.5 bit-identical
    # normalisation bits, with and without the nudge; mean alone and std alone
    mean, std = np.array([0.4, 0.5, 0.6], np.float32), np.array([0.2, 0.25, 0.3], np.float32)
    y = do.to_float(do.hash_u8("finish", (4, C, H, W), 0.2))
    cnt = dataset.count_zeros_ones(torch.from_numpy(y).to(DEV))
    for m, s in ((mean, std), (mean, None), (None, std)):
        t = torch.from_numpy(y).to(DEV)
        dataset.finish(t, cnt, 0.10, 1e-14, None if m is None else torch.from_numpy(m).to(DEV),
                       None if s is None else torch.from_numpy(s).to(DEV))
        want = np.stack([do.finish(y[b], 0.10, 1e-14, m, s) for b in range(4)])
        assert same(t.cpu().numpy(), want)
    assert any(do.condition(*do.counts(y[b]), n, 0.10) for b in range(4))


def test_train_inputs_reproduces_the_reference():
    for name, (prob, py_seed, np_seed, frames) in do.train_cases().items():
        random.seed(py_seed)
        np.random.seed(np_seed)
        out = augment.train_inputs(torch.from_numpy(frames).to(DEV), prob, rng="numpy")
        assert same(out.cpu().numpy(), GOLD[f"train/{name}"]), name
        assert do.state_digest() == META["train"][name]["state"], name
    x = torch.from_numpy(do.train_cases()["train_f3_8x8_p0.3"][3]).to(DEV)
    random.seed(1)
    a = augment.train_inputs(x, 0.3, seed=3, call=9)
    random.seed(1)
    assert torch.equal(a, augment.train_inputs(x, 0.3, seed=3, call=9))
    with pytest.raises(ValueError, match="odd"):
        augment.train_inputs(x[:, :2].contiguous(), 0.3)


def test_teacher_batch_end_to_end():
    py_seed, np_seed, g, samples = do.teacher_batch()
    t = dataset.TeacherSampleTransform(g, rng="numpy")
    random.seed(py_seed)
    np.random.seed(np_seed)
    lq, gt = t(*[[torch.from_numpy(s[k].copy()).to(DEV) for s in samples] for k in range(3)], [s[3] for s in samples])
    assert do.state_digest() == META["teacher"]["state"]
    for tag, got in (("img", lq["img"]), ("denoise_rate", lq["denoise_rate"]), ("hq", gt["hq"]), ("sr", gt["sr"])):
        assert same(got.cpu().numpy(), np.stack([GOLD[f"teacher/{b}/{tag}"] for b in range(len(samples))])), tag
    # mean / std: img through finish, hq and sr in the sample launch
    mean, std = [0.4, 0.5, 0.6], [0.2, 0.25, 0.3]
    t = dataset.TeacherSampleTransform(g, mean=mean, std=std, rng="numpy")
    random.seed(py_seed)
    np.random.seed(np_seed)
    lq, gt = t(*[[torch.from_numpy(s[k].copy()).to(DEV) for s in samples] for k in range(3)], [s[3] for s in samples])
    random.seed(py_seed)
    np.random.seed(np_seed)
    for b, s in enumerate(samples):
        img, _, hq, sr, _ = do.teacher_sample(*s, g, mean=mean, std=std)
        assert same(lq["img"][b].cpu().numpy(), img) and same(gt["hq"][b].cpu().numpy(), hq)
        assert same(gt["sr"][b].cpu().numpy(), sr)
    # the Philox route: same geometry, noise only where the host route has it, reproducible
    outs = []
    for _ in range(2):
        t = dataset.TeacherSampleTransform(g, rng="philox", seed=11)
        random.seed(py_seed)
        np.random.seed(np_seed)
        outs.append(t(*[[torch.from_numpy(s[k].copy()).to(DEV) for s in samples] for k in range(3)], [s[3] for s in samples]))
    assert torch.equal(outs[0][0]["img"], outs[1][0]["img"])
    assert same(outs[0][1]["hq"].cpu().numpy(), np.stack([GOLD[f"teacher/{b}/hq"] for b in range(2)]))


def test_student_batch_end_to_end():
    py_seed, np_seed, g, prob, bursts = do.student_batch()

    def run(rng, seed=0):
        t = dataset.StudentSampleTransform(g, prob, rng=rng, seed=seed)
        random.seed(py_seed)
        np.random.seed(np_seed)
        return t([[torch.from_numpy(f.copy()).to(DEV) for f in b[0]] for b in bursts],
                 [[torch.from_numpy(f.copy()).to(DEV) for f in b[1]] for b in bursts]), t
    (lq, gt), t = run("numpy")
    assert do.state_digest() == META["student"]["state"]
    assert t.last_draw == [(d["top"], d["left"], d["mode"]) for d in META["student"]["draws"]]
    for b in range(len(bursts)):
        assert same(lq[b].cpu().numpy(), GOLD[f"student/{b}/lq"]), b
        assert same(gt[b].cpu().numpy(), GOLD[f"student/{b}/gt"]), b
    (lq_p, gt_p), _ = run("philox", 7)
    (lq_q, _), _ = run("philox", 7)
    assert torch.equal(lq_p, lq_q) and torch.equal(gt_p, gt)       # same geometry; reproducible
    assert not torch.equal(lq_p[1], lq[1])                         # sample 1 is noisy: other normals


def test_every_argument_check_returns_before_a_launch():
    L = _lib.lib()
    P = 0x10000

    def rc(**kw):
        it = _lib.DataItem(src=P, dst=P + (1 << 20), sy=7, sx=1, sc=0, src_u8=1, Hs=5, Ws=7, C=1, Hc=5, Wc=7, Hp=5, Wp=7,
                           top=0, left=0, h=5, w=7, div=1.0)
        for k, v in kw.items():
            setattr(it, k, v)
        return L.kdlae_data_sample(ctypes.byref(it), ctypes.c_void_p(P + (2 << 20)), 1, 0, 0, None)
    for kw, code in ((dict(src=None), 2), (dict(dst=None), 2), (dict(dst=P + (1 << 20) + 2), 2), (dict(src_u8=0, src=P + 1), 2),
                     (dict(Hs=0), 1), (dict(h=0), 1), (dict(sy=-1), 1), (dict(Hc=4), 1), (dict(Wp=6), 1), (dict(Hp=6), 1),
                     (dict(pad_mode=3), 2), (dict(pad_mode=1, Hp=4), 1), (dict(top=1), 1), (dict(left=-1), 1), (dict(w=8), 1),
                     (dict(dihedral=8), 2), (dict(noise=3), 2), (dict(noise=1), 2), (dict(noise=2, div=0.0), 2),
                     (dict(counts=P, count_n=0), 1), (dict(dst=P + 32), 2), (dict(src=P + (1 << 20) + 64), 2)):
        assert rc(**kw) == code, kw
    assert "overlaps" in _lib.last_error()
    it = _lib.DataItem()
    assert L.kdlae_data_sample(None, ctypes.c_void_p(P), 1, 0, 0, None) == 2
    assert L.kdlae_data_sample(ctypes.byref(it), None, 1, 0, 0, None) == 2
    assert L.kdlae_data_sample(ctypes.byref(it), ctypes.c_void_p(P), 0, 0, 0, None) == 2
    assert L.kdlae_data_count(None, 1, 4, ctypes.c_void_p(P), None) == 2 and L.kdlae_data_count(ctypes.c_void_p(P), 0, 4, ctypes.c_void_p(P), None) == 1
    assert L.kdlae_data_count(ctypes.c_void_p(P), 1, 1 << 31, ctypes.c_void_p(P), None) == 1
    assert L.kdlae_data_finish(None, 1, 1, 4, ctypes.c_void_p(P), 0.1, 0.0, None, None, None) == 2
    assert L.kdlae_data_finish(ctypes.c_void_p(P), 1, 0, 4, ctypes.c_void_p(P), 0.1, 0.0, None, None, None) == 1
    # the Python wrapper's own checks
    u8 = torch.zeros((5, 7, 3), dtype=torch.uint8, device=DEV)
    ok = torch.empty((3, 5, 7), device=DEV)
    for bad in (dict(src=u8, dst=torch.empty((3, 7, 5), device=DEV)), dict(src=u8, dst=ok, dihedral=4),
                dict(src=u8, dst=ok.double()), dict(src=u8.int(), dst=ok), dict(src=u8, dst=ok, noise=dict(scale=1.0, z=ok)),
                dict(src=u8, dst=ok, mean=torch.zeros(2, device=DEV)), dict(src=u8, dst=ok.cpu()),
                dict(src=u8, dst=ok, noise=dict(scale=1.0, counts=torch.zeros(2, device=DEV), thr=0.5, n=3))):
        with pytest.raises(RuntimeError):
            dataset.sample_transform([bad])
    for bad in (dict(src=u8, dst=ok, pad_mode="wrap"), dict(src=u8, dst=ok, dihedral=9), dict(src=u8, dst=ok, layout="nhwc")):
        with pytest.raises(ValueError):
            dataset.sample_transform([bad])
    with pytest.raises(RuntimeError, match="leaves"):
        dataset.sample_transform([dict(src=u8, dst=torch.empty((3, 6, 7), device=DEV), window=(0, 0, 6, 7))])
    f = torch.zeros((3, 5, 7), device=DEV)
    with pytest.raises(RuntimeError, match="overlaps"):
        dataset.sample_transform([dict(src=f, dst=f)])

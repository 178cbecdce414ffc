"""Dataset sample transforms, CPU side: the numpy oracle against the goldens recorded from the reference
(tests/golden/make_golden_dataset.py), the host draw order of both transforms against the recorded generator
states, the dihedral lowering table, and the argument checks that need no GPU."""
import itertools
import json
import os
import random

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import augment, dataset
from tests import dataset_oracle as do

HERE = os.path.dirname(os.path.abspath(__file__))
META = json.load(open(os.path.join(HERE, "golden", "dataset_sample.json")))
GOLD = np.load(os.path.join(HERE, "golden", "dataset_sample.npz"))


def same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


IMG = do.to_float(do.hash_u8("step/hwc", (13, 6, 3)))
GREY = do.to_float(do.hash_u8("step/grey", (5, 7)))
SR = do.to_float(do.hash_u8("step/sr", (26, 12, 3)))


def test_oracle_steps_equal_goldens():
    for mode in range(8):
        code = dataset.dihedral_code(*dataset.lower_data_augmentation(mode))
        assert same(GOLD[f"steps/data_augmentation/{mode}"], do.dihedral(IMG, code)), mode
    assert same(GOLD["steps/random_augmentation/0"],
                do.data_augmentation_model(IMG, META["steps"]["random_augmentation"]["flag"]))
    for (H, W) in ((8, 8), (11, 9)):   # even and odd deficits
        assert same(GOLD[f"steps/pad_image/{H}x{W}"], do.centre_pad(GREY, H, W))
    for g in (6, 8, 14):
        assert same(GOLD[f"steps/padding/{g}"], do.edge_pad(IMG, max(13, g), max(6, g), "symmetric"))
    assert same(GOLD["steps/multi_scale_padding/gt"], do.edge_pad(IMG, 13, 8, "reflect101"))
    assert same(GOLD["steps/multi_scale_padding/sr"], do.edge_pad(SR, 26, 16, "reflect101"))
    m = META["steps"]["paired_random_crop"]
    gt2 = do.to_float(do.hash_u8("step/gt2", (26, 12, 3)))
    assert same(GOLD["steps/paired_random_crop/lq"], IMG[m["top"]:m["top"] + 5, m["left"]:m["left"] + 5])
    assert same(GOLD["steps/paired_random_crop/gt"], gt2[2 * m["top"]:2 * m["top"] + 10, 2 * m["left"]:2 * m["left"] + 10])
    m = META["steps"]["multi_scale_crop"]
    assert m["top"] >= 1 and m["left"] >= 1     # the teacher's offsets start at 1
    big, big_sr = do.to_float(do.hash_u8("step/big", (12, 14, 3))), do.to_float(do.hash_u8("step/big_sr", (24, 28, 3)))
    assert same(GOLD["steps/multi_scale_crop/gt"], big[m["top"]:m["top"] + 8, m["left"]:m["left"] + 8])
    assert same(GOLD["steps/multi_scale_crop/sr"], big_sr[2 * m["top"]:2 * m["top"] + 16, 2 * m["left"]:2 * m["left"] + 16])
    np.random.seed(META["steps"]["add_random_noise"]["np_seed"])
    out = do.add_noise(IMG, np.random.standard_normal(IMG.shape), 0.3, 0.7)
    assert same(GOLD["steps/add_random_noise/out"], out) and out.min() == 0.0 and out.max() == 1.0   # clips at both ends
    np.random.seed(META["steps"]["add_gaussian_noise"]["np_seed"])
    sigma = np.random.uniform(1, 30)
    assert repr(float(sigma)) == META["steps"]["add_gaussian_noise"]["sigma"]
    assert same(GOLD["steps/add_gaussian_noise/out"], do.add_noise(IMG, np.random.randn(*IMG.shape), 0.0, sigma, 255.0))
    for name, zf in (("below", 0.05), ("above", 0.2)):
        x = do.to_float(do.hash_u8("step/nudge/" + name, (9, 8, 3), zf))
        got = do.finish(x.transpose(2, 0, 1), 0.10).transpose(1, 2, 0)
        assert same(GOLD[f"steps/nudge/{name}"], got)
        assert (name == "above") == bool((got != x).any())
    x = GOLD["steps/nudge/above"]
    assert x.min() == np.float32(1e-14) and same(x[x > 1e-3], do.to_float(do.hash_u8("step/nudge/above", (9, 8, 3), 0.2))[x > 1e-3])


def test_sync_augment_goldens_and_lowering():
    combos = set()
    for seed, m in META["steps"]["sync_augment"].items():
        combos.add((m["hflip"], m["vflip"], m["rot"]))
        code = dataset.dihedral_code(*dataset.lower_sync_augment(m["hflip"], m["vflip"], m["rot"]))
        assert same(GOLD[f"steps/sync_augment/{seed}"], do.dihedral(IMG, code)), m
    assert len(combos) == 16


def test_lowering_table():
    """Every word of both vocabularies lowers to the triple whose index map equals numpy's own."""
    for mode in range(8):
        want = do.code_of(lambda a: do.data_augmentation_model(a, mode))
        assert dataset.dihedral_code(*dataset.lower_data_augmentation(mode)) == want, mode
    assert sorted(dataset.dihedral_code(*dataset.lower_data_augmentation(m)) for m in range(8)) == list(range(8))
    codes = []
    for hf, vf, rot in itertools.product((False, True), (False, True), (None, 90, 180, 270)):
        want = do.code_of(lambda a: do.sync_augment_model(a, hf, vf, rot))
        got = dataset.dihedral_code(*dataset.lower_sync_augment(hf, vf, rot))
        assert got == want, (hf, vf, rot)
        codes.append(got)
    assert len(codes) == 16 and sorted(set(codes)) == list(range(8))       # exactly the 8 group elements
    assert all(codes.count(c) == 2 for c in range(8))
    with pytest.raises(ValueError):
        dataset.lower_data_augmentation(8)
    with pytest.raises(ValueError):
        dataset.lower_sync_augment(True, False, 45)
    with pytest.raises(ValueError):
        dataset.lower_ops(["rot45"])


def test_oracle_train_phase_equals_goldens():
    for name, (prob, py_seed, np_seed, frames) in do.train_cases().items():
        random.seed(py_seed)
        np.random.seed(np_seed)
        out = np.stack([do.train_phase(frames[b], prob)[0] for b in range(frames.shape[0])])
        assert same(GOLD[f"train/{name}"], out), name
        assert do.state_digest() == META["train"][name]["state"], name
    assert {r["interpolate"] for m in META["train"].values() for r in m["rows"]} == {True, False}


def test_oracle_whole_samples_equal_goldens():
    py_seed, np_seed, g, samples = do.teacher_batch()
    random.seed(py_seed)
    np.random.seed(np_seed)
    for b, (lq, gt, sr, rate) in enumerate(samples):
        out = do.teacher_sample(lq, gt, sr, rate, g)
        for tag, o in zip(("img", "denoise_rate", "hq", "sr"), out):
            assert same(GOLD[f"teacher/{b}/{tag}"], o), (b, tag)
    assert do.state_digest() == META["teacher"]["state"]
    py_seed, np_seed, g, prob, bursts = do.student_batch()
    random.seed(py_seed)
    np.random.seed(np_seed)
    for b, (lqf, gtf) in enumerate(bursts):
        lq, gt, _ = do.student_sample(lqf, gtf, g, prob)
        assert same(GOLD[f"student/{b}/lq"], lq) and same(GOLD[f"student/{b}/gt"], gt), b
    assert do.state_digest() == META["student"]["state"]


def test_philox_normal_model():
    z = do.philox_normal(16, 16, 3, 7, 3)
    assert z.dtype == np.float64 and np.abs(z).max() < 5.77 and abs(z.mean()) < 0.15 and abs(z.std() - 1) < 0.1
    assert not np.array_equal(z, do.philox_normal(16, 16, 3, 7, 4)) and np.array_equal(z, do.philox_normal(16, 16, 3, 7, 3))
    # an odd element count: the last block is half used
    assert np.array_equal(do.philox_normal(1, 3, 1, 7, 3).ravel()[:2], do.philox_normal(1, 2, 1, 7, 3).ravel())


# ------------------------------------------------------------------ host draw order of the transforms (no GPU: the
# launches are replaced, the draws are the transforms' own)
@pytest.fixture
def no_launch(monkeypatch):
    monkeypatch.setattr(dataset, "_dev", lambda t, what: t)
    monkeypatch.setattr(dataset, "sample_transform", lambda items, seed=0, call=0: None)
    monkeypatch.setattr(dataset, "finish", lambda x, *a, **k: x)

    def frames_by_item(frames, item_probs, interpolate, rng, seed, call, value, per_item):
        if rng == "numpy":
            for b in range(frames.shape[0]):
                for p in item_probs[b]:
                    if p >= 0:
                        augment._numpy_keep(1, frames.shape[2], frames.shape[3], p)
        return frames
    monkeypatch.setattr(augment, "_frames_by_item", frames_by_item)
    return monkeypatch


@pytest.mark.parametrize("rng", ["numpy", "philox"])
def test_teacher_draw_order(no_launch, rng):
    no_launch.setattr(dataset, "count_zeros_ones", lambda x: torch.zeros((x.shape[0], 2), dtype=torch.int32))
    py_seed, np_seed, g, samples = do.teacher_batch()
    t = dataset.TeacherSampleTransform(g, rng=rng)
    random.seed(py_seed)
    np.random.seed(np_seed)
    lq, gt = t(*[[torch.from_numpy(s[k].copy()) for s in samples] for k in range(3)], [s[3] for s in samples])
    for d, m in zip(t.last_draw, META["teacher"]["draws"]):
        assert d[:2] == (m["top"], m["left"]) and d[3:] == (m["hflip"], m["vflip"], m["rot"])
        assert (None if d[2] is None else repr(float(d[2]))) == m["sigma"]
    if rng == "numpy":
        assert do.state_digest() == META["teacher"]["state"]
    else:   # no normals are drawn on the host: `random` ends where the reference ends, numpy.random earlier
        want = random.getstate()
        random.seed(py_seed)
        np.random.seed(np_seed)
        for s in samples:
            do.teacher_sample(*s, g)
        assert random.getstate() == want
    assert same(lq["denoise_rate"].numpy(), np.stack([GOLD[f"teacher/{b}/denoise_rate"] for b in range(2)]))
    assert set(lq) == {"img", "denoise_rate"} and set(gt) == {"hq", "sr"} and gt["sr"].shape == (2, 3, 2 * g, 2 * g)


def test_student_draw_order(no_launch):
    py_seed, np_seed, g, prob, bursts = do.student_batch()
    F = len(bursts[0][0])
    noise = iter(d["noise"] for d in META["student"]["draws"])
    no_launch.setattr(dataset, "count_zeros_ones",
                      lambda x: torch.tensor([[F * g * g if next(noise) else 0, 0]], dtype=torch.int32))
    t = dataset.StudentSampleTransform(g, prob, rng="numpy")
    random.seed(py_seed)
    np.random.seed(np_seed)
    t([[torch.from_numpy(f.copy()) for f in b[0]] for b in bursts], [[torch.from_numpy(f.copy()) for f in b[1]] for b in bursts])
    assert do.state_digest() == META["student"]["state"]
    assert t.last_draw == [(d["top"], d["left"], d["mode"]) for d in META["student"]["draws"]]
    # the Philox route makes the same `random` draws in the same order and none from numpy.random
    want = random.getstate()
    np_state = np.random.get_state()[1].copy()
    t = dataset.StudentSampleTransform(g, prob, rng="philox")
    no_launch.setattr(dataset, "count_zeros_ones", lambda x: torch.zeros((x.shape[0], 2), dtype=torch.int32))
    random.seed(py_seed)
    t([[torch.from_numpy(f.copy()) for f in b[0]] for b in bursts], [[torch.from_numpy(f.copy()) for f in b[1]] for b in bursts])
    assert random.getstate() == want and np.array_equal(np.random.get_state()[1], np_state)
    assert t.last_draw == [(d["top"], d["left"], d["mode"]) for d in META["student"]["draws"]]


# ------------------------------------------------------------------ argument checks that need no GPU
def test_cpu_tensors_and_arguments_are_refused_before_any_draw():
    random.seed(1)
    np.random.seed(1)
    digest = do.state_digest()
    u8, f = torch.zeros((12, 12, 3), dtype=torch.uint8), torch.zeros((2, 3, 4, 4))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dataset.sample_transform([dict(src=u8, dst=torch.zeros(3, 12, 12))])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dataset.count_zeros_ones(f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dataset.finish(f, torch.zeros((2, 2), dtype=torch.int32), 0.1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dataset.TeacherSampleTransform(8)([u8], [u8], [torch.zeros((24, 24, 3), dtype=torch.uint8)], [None])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        dataset.StudentSampleTransform(8, 0.1)([[u8[:, :, 0]]], [[u8[:, :, 0]]])
    with pytest.raises(RuntimeError, match="ROCm tensors only"):
        augment.train_inputs(torch.zeros(1, 3, 4, 4), 0.1)
    with pytest.raises(ValueError):
        dataset.sample_transform([])
    with pytest.raises(ValueError, match="rng"):
        dataset.TeacherSampleTransform(8, rng="torch")
    with pytest.raises(ValueError, match="rng"):
        dataset.StudentSampleTransform(8, 0.1, rng="torch")
    with pytest.raises(ValueError, match="mean"):
        dataset.TeacherSampleTransform(8, mean=[0.5])
    with pytest.raises(ValueError, match="gt_size"):
        dataset.TeacherSampleTransform(0)
    with pytest.raises(ValueError, match="one length"):
        dataset.TeacherSampleTransform(8)([u8], [u8, u8], [u8], [None])
    with pytest.raises(ValueError, match="odd number"):
        dataset.StudentSampleTransform(8, 0.1)([[u8[:, :, 0]] * 2], [[u8[:, :, 0]] * 2])
    assert do.state_digest() == digest


def test_teacher_refuses_what_randint_refuses(no_launch):
    random.seed(1)
    state = random.getstate()
    small = torch.zeros((9, 12, 3), dtype=torch.uint8)     # 9 - 1 - 8 < 1
    with pytest.raises(ValueError, match="randint"):
        dataset.TeacherSampleTransform(8)([small], [small], [torch.zeros((18, 24, 3), dtype=torch.uint8)], [None])
    ok = torch.zeros((12, 12, 3), dtype=torch.uint8)
    with pytest.raises(ValueError, match="sr"):
        dataset.TeacherSampleTransform(8)([ok], [ok], [ok], [None])
    assert random.getstate() == state

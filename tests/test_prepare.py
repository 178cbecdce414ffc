"""Progressive-learning batch preparation on the CPU side: the numpy oracle (tests/prepare_oracle.py) against what
the reference's own statements produced (tests/golden/prepare_train.npz / .json, written by
tests/golden/make_golden_prepare.py), the stage rule on the released schedules, Philox4x32-10 known answers, the
mask's value rules, and every argument check of ``kdlae_train_prepare`` / ``kdlae_train_mask_frames`` through the
C ABI.  No call here touches the GPU.  All comparisons of tensors are bit for bit."""
import ctypes
import json
import os
import random

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, augment
from tests import prepare_oracle as po

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
META = json.load(open(os.path.join(GOLDEN, "prepare_train.json")))
ARRAYS = np.load(os.path.join(GOLDEN, "prepare_train.npz"))
P_CASES = po.progressive_cases()
F_CASES = po.frame_cases()

# datasets.train of Train/Denoising/Options/paper202508/KDLAET.yml and KDLAES.yml (the second `probs` key of
# KDLAES.yml is the one a yaml loader keeps)
T_YML = dict(iters=[3000, 2000, 1600, 1200, 1200, 800], gt_sizes=[32, 64, 96, 128, 128, 128],
             mini_batch_sizes=[6, 6, 2, 1, 1, 1], probs=[0.2, 0.1, 0.05, 0.03, 0.02, 0.02], prob=0, gt_size=128,
             batch_size=6)
S_YML = dict(iters=[30000, 20000, 16000, 12000, 12000, 10000], gt_sizes=[128, 160, 192, 256, 320, 384],
             mini_batch_sizes=[128, 128, 64, 32, 32, 32], probs=[0.1, 0.2, 0.22, 0.25, 0.27, 0.25], prob=0,
             gt_size=384, batch_size=4)


def bits(a):
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32
    return a.view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def golden_out(kind, name, tag, like):
    if isinstance(like, dict):
        return {k: ARRAYS[f"{kind}/{name}/{tag}/{k}"] for k in like}
    return ARRAYS[f"{kind}/{name}/{tag}"]


def test_golden_file_covers_the_cases():
    assert set(META["progressive"]) == set(P_CASES) and set(META["frames"]) == set(F_CASES)
    for key in ("progressive", "interpolation", "test1", "input_mask"):
        assert key in META["source"]


@pytest.mark.parametrize("name", sorted(P_CASES))
def test_oracle_equals_reference_progressive_block(name):
    cfg, it, py_seed, np_seed, lq, gt = P_CASES[name]
    m = META["progressive"][name]
    assert (m["cfg"], m["current_iter"], m["py_seed"], m["np_seed"]) == (cfg, it, py_seed, np_seed)
    lq_before = {k: v.copy() for k, v in lq.items()} if isinstance(lq, dict) else lq.copy()
    random.seed(py_seed)
    np.random.seed(np_seed)
    o_lq, o_gt, (j, indices, x0, y0, mp) = po.progressive(cfg, it, lq, gt)
    d = m["draws"]
    assert (j, indices, x0, y0, repr(float(mp))) == (d["stage"], d["indices"], d["x0"], d["y0"], d["mask_prob"])
    for got, want in ((o_lq, golden_out("progressive", name, "out_lq", o_lq)),
                      (o_gt, golden_out("progressive", name, "out_gt", o_gt))):
        for k in (got if isinstance(got, dict) else [None]):
            assert same(got[k], want[k]) if k else same(got, want), (name, k)
    # the oracle leaves its inputs alone
    for k in (lq if isinstance(lq, dict) else [None]):
        assert same(lq[k], lq_before[k]) if k else same(lq, lq_before)


@pytest.mark.parametrize("name", sorted(F_CASES))
def test_oracle_equals_reference_frame_rule(name):
    phase, prob, py_seed, np_seed, frames = F_CASES[name]
    m = META["frames"][name]
    assert (m["phase"], m["prob"], m["py_seed"], m["np_seed"]) == (phase, prob, py_seed, np_seed)
    keep, want = ARRAYS[f"frames/{name}/keep"], ARRAYS[f"frames/{name}/out"]
    probs = [[float(p) for p in row] for row in m["probs"]]
    # the recorded keep masks are what the seeded numpy stream gives, drawn per (item, frame)
    np.random.seed(np_seed)
    redrawn = np.stack([np.stack([po.numpy_keep(1, *frames.shape[2:], p)[0] for p in row]) for row in probs])
    assert np.array_equal(redrawn, keep)
    if phase == "test1":
        random.seed(py_seed)
        assert probs == [[prob + 0.6 if random.random() < 0.2 else prob for _ in row] for row in probs]
    else:
        assert probs == [[prob + 0.5 if f % 2 else prob for f in range(len(row))] for row in probs]
    got = np.stack([po.mask_frames(frames[b:b + 1], [min(p, 1.0) for p in probs[b]], phase == "interpolation",
                                   keep[b:b + 1])[0] for b in range(frames.shape[0])])
    assert same(got, want)


@pytest.mark.parametrize("yml", [T_YML, S_YML], ids=["KDLAET", "KDLAES"])
def test_stage_table_of_the_released_schedules(yml):
    sch = augment.ProgressiveSchedule(yml["iters"], yml["gt_sizes"], yml["mini_batch_sizes"], yml["probs"],
                                      yml["gt_size"], yml["batch_size"], prob=yml["prob"])
    n, total = len(yml["iters"]), 0
    rows = []
    for j, it in enumerate(yml["iters"]):
        total += it
        rows += [(total, j), (total + 1, min(j + 1, n - 1))]
    rows += [(1, 0), (total + 10 ** 6, n - 1)]
    for it, j in rows:
        want = (j, yml["gt_sizes"][j], yml["mini_batch_sizes"][j], yml["probs"][j] - yml["prob"])
        assert sch.stage(it) == want, it
        assert po.stage(yml["iters"], yml["gt_sizes"], yml["mini_batch_sizes"], yml["probs"], yml["prob"], it) == want
    # every stage of both released schedules masks: prob is 0 and every entry of probs is positive
    assert all(sch.stage(it)[3] > 0 for it, _ in rows)


def test_schedule_rejects_unequal_lists_and_reports_no_mask_at_or_below_prob():
    with pytest.raises(ValueError):
        augment.ProgressiveSchedule([1, 2], [8], [1, 1], [0.1, 0.1], 8, 1)
    with pytest.raises(ValueError):
        augment.ProgressiveSchedule([], [], [], [], 8, 1)
    sch = augment.ProgressiveSchedule([1, 1], [8, 8], [1, 1], [0.3, 0.2], 8, 1, prob=0.3)
    assert sch.stage(1)[3] == 0.0 and sch.stage(2)[3] == 0.0
    with pytest.raises(ValueError):
        augment.ProgressiveBatcher(sch, rng="torch")


PHILOX_KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.mark.parametrize("ctr,key,want", PHILOX_KAT)
def test_philox_known_answers(ctr, key, want):
    got = po.philox4x32_10(np.array(ctr, np.uint32), key)
    assert tuple(int(v) for v in got) == want
    # the element layout: block q = e // 4 with counter (q lo, q hi, call lo, call hi), word e % 4
    q = ctr[0] | ctr[1] << 32
    if q < 2 ** 40:
        call, seed = ctr[2] | ctr[3] << 32, key[0] | key[1] << 32
        words = po.philox_words(4 * q + 4, seed, call)
        assert tuple(int(v) for v in words[4 * q:]) == want


def test_philox_keep_rule_is_fp32():
    words = po.philox_words(64, 5, 9)
    u = (words >> 8).astype(np.float64) / 2 ** 24
    assert np.array_equal(po.philox_keep((64,), 0.3, 5, 9), (u.astype(np.float32) >= np.float32(0.3)).astype(np.uint8))
    assert u.max() < 1.0 and po.philox_keep((64,), 1.0, 5, 9).sum() == 0       # u < 1 always: p = 1 masks all


def test_kept_pixels_are_bit_identical_and_masked_ones_are_minus_value():
    src = po.hash_images("prepare/value_rule", (2, 3, 6, 8))
    src[0, 0, 0, :4] = [0.0, -0.0, 1.0, 1e-30]
    keep = po.philox_keep((2, 3, 6, 8), 0.4, 1, 2)
    out = po.prepare(src, None, 0, 0, 6, 8, prob=0.4, keep=keep)
    k = keep.astype(bool)
    assert 0 < k.sum() < k.size
    assert np.array_equal(bits(out)[k], bits(src)[k])
    assert np.all(bits(out)[~k] == np.float32(-0.1).view(np.uint32))
    assert np.float32(-0.1) == -np.float32(0.1) and not np.any(out[~k] == 0)


def test_prob_above_one_masks_everything():
    src = po.hash_images("prepare/above_one", (1, 2, 4, 4))
    for p in (1.0, 1.7):
        for keep in (None, np.ones((1, 2, 4, 4), np.uint8)):
            assert np.all(po.prepare(src, None, 0, 0, 4, 4, prob=p, keep=keep) == np.float32(-0.1))
        assert np.all(po.mask_frames(src, [p, p]) == np.float32(-0.1))
    assert augment.choice_threshold(1.7) == 1.0 == po.choice_threshold(1.7)
    np.random.seed(3)
    assert po.numpy_keep(2, 4, 4, 1.5).sum() == 0
    # and the reference agrees: the recorded case with probs[j] = 1.5
    assert np.all(ARRAYS["progressive/dict_prob_above_one/out_lq/img"] == np.float32(-0.1))


def test_interpolation_quirk_frame_1_sees_masked_frame_0_and_raw_frame_2():
    src = po.hash_images("prepare/quirk", (1, 3, 2, 4))
    keep = np.ones((1, 3, 2, 4), np.uint8)
    keep[0, 0, 0, :2] = 0            # frame 0 loses two pixels
    keep[0, 2] = 0                   # frame 2 loses everything, after frame 1 has read it raw
    out = po.mask_frames(src, [0.5, 0.5, 0.5], True, keep)
    m0 = np.where(keep[0, 0] != 0, src[0, 0], np.float32(-0.1))
    want1 = (m0 + src[0, 2]).astype(np.float32) * np.float32(0.5)
    assert same(out[0, 1], want1) and same(out[0, 0], m0)
    assert np.all(out[0, 2] == np.float32(-0.1))
    raw1 = (src[0, 0] + src[0, 2]) * np.float32(0.5)
    assert not np.array_equal(out[0, 1, 0, :2], raw1[0, :2]) and same(out[0, 1, 1], raw1[1])
    # without interpolation frame 1 is just masked
    assert same(po.mask_frames(src, [0.5, 0.5, 0.5], False, keep)[0, 1], src[0, 1])


def test_cpu_tensors_fail_loudly():
    sch = augment.ProgressiveSchedule([4], [8], [2], [0.2], 8, 2)
    b = augment.ProgressiveBatcher(sch)
    random.seed(5)
    state = random.getstate()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b(1, torch.zeros(2, 3, 8, 8), torch.zeros(2, 3, 8, 8))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        b(1, {"img": torch.zeros(2, 3, 8, 8)}, {"hq": torch.zeros(2, 3, 8, 8), "sr": torch.zeros(2, 3, 16, 16)})
    assert random.getstate() == state        # refused before any draw
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment.mask_frames(torch.zeros(1, 3, 4, 4), [0.1, 0.6, 0.1], True)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        augment.interpolation_inputs(torch.zeros(1, 3, 4, 4), 0.1)


# ------------------------------------------------------------------ argument checks through the C ABI
P = 0x1000  # a non-null, 16-byte aligned "device pointer"; never dereferenced: every call below fails before a launch


def _prep(segs, nseg=None, index=None, B=2):
    L = _lib.lib()
    arr = (_lib.PrepSeg * max(len(segs), 1))(*segs)
    rc = L.kdlae_train_prepare(arr, len(segs) if nseg is None else nseg, index, B,
                               0.1, 0, 0, None)
    return rc, _lib.last_error()


def _seg(**kw):
    d = dict(src=P, dst=P + 0x10000, B_src=2, C=3, Hs=12, Ws=12, h=8, w=8, y0=2, x0=3, prob=0.0, keep=None)
    d.update(kw)
    return _lib.PrepSeg(**d)


def test_prepare_refuses_bad_arguments_before_any_launch():
    L = _lib.lib()
    rc = L.kdlae_train_prepare(None, 1, None, 2, 0.1, 0, 0, None)
    assert rc == 2 and _lib.last_error()
    for nseg in (0, 5, -1):
        rc, err = _prep([_seg()] * 5, nseg=nseg)
        assert rc == 2 and "nseg" in err
    for B in (0, -3):
        rc, err = _prep([_seg()], B=B)
        assert rc == 1 and err
    for kw in (dict(src=None), dict(dst=None), dict(dst=P)):
        rc, err = _prep([_seg(**kw)])
        assert rc == 2 and err, kw
    # a window that leaves its source, on each side; non-positive extents
    for kw in (dict(y0=5), dict(x0=5), dict(y0=-1), dict(x0=-1), dict(h=13, y0=0), dict(w=13, x0=0),
               dict(y0=2 ** 31 - 1), dict(h=0), dict(w=0), dict(C=0), dict(B_src=0), dict(Hs=0), dict(Ws=-2)):
        rc, err = _prep([_seg(**kw)])
        assert rc == 1 and err, kw
    # the check covers every segment, not only the first
    rc, err = _prep([_seg(), _seg(), _seg(x0=5)])
    assert rc == 1 and "segment 2" in err
    # a null index needs B == B_src; with an index B is free
    rc, err = _prep([_seg(B_src=3)], B=2)
    assert rc == 1 and "index" in err


def _frames(src=P, dst=P + 0x10000, B=1, F=3, H=4, W=4, probs=(0.1, 0.6, 0.1), interpolate=1):
    L = _lib.lib()
    cp = (ctypes.c_float * len(probs))(*probs) if probs is not None else None
    rc = L.kdlae_train_mask_frames(src, dst, B, F, H, W, cp, interpolate, 0.1, None, 0, 0, None)
    return rc, _lib.last_error()


def test_mask_frames_refuses_bad_arguments_before_any_launch():
    for kw in (dict(src=None), dict(dst=None), dict(probs=None), dict(dst=P)):
        rc, err = _frames(**kw)
        assert rc == 2 and err, kw
    for kw in (dict(B=0), dict(F=0), dict(H=0), dict(W=-1)):
        rc, err = _frames(**kw)
        assert rc == 1 and err, kw
    rc, err = _frames(F=4, probs=(0.1,) * 4)                       # even F with interpolation
    assert rc == 1 and "odd" in err
    rc, err = _frames(F=17, probs=(0.1,) * 17, interpolate=0)       # F > 16
    assert rc == 1 and "16" in err
    rc, err = _frames(F=17, probs=(0.1,) * 17, interpolate=1)
    assert rc == 1 and err

"""Clip inference (kdlae_clip_plan, kdlae_clip_gather, kdlae_clip_blend, kdlae_clip_blend_u8): what holds without
a GPU.  The header declares and the library exports the entries, the plan equals a brute-force count, every
argument error is returned before a launch (the pointers here are never dereferenced), the named windows are the
tile windows on one axis, and the CPU model the GPU tests compare against (tests/clip_model.py) equals the host loop
it stands for and tells every mutant of the rule apart on the GPU tests' own inputs."""
import ctypes
import math
import os
import re

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, clips, pipeline
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student
from tests import clip_model as cm
from tests.util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kdlae_clip_plan", "kdlae_clip_gather", "kdlae_clip_blend", "kdlae_clip_blend_u8")
P = ctypes.c_void_p(FAKE)
SHAPE, CONFIG = 1, 2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    for name in ("ClipPlan", "clip_plan", "clip_gather", "clip_blend", "clip_blend_u8", "clip_window"):
        assert callable(getattr(clips, name))
    assert callable(KDLAE_student.forward_clip) and callable(pipeline.enhance_clip_u8)


# ------------------------------------------------------------------ the plan
def _plan(T, frames, overlap):
    out = [ctypes.c_int(-7) for _ in range(3)]
    rc = _lib.lib().kdlae_clip_plan(T, frames, overlap, *[ctypes.byref(v) for v in out])
    return rc, [v.value for v in out]


@pytest.mark.parametrize("frames", [1, 2, 3, 5, 7, 8])
def test_plan_equals_a_brute_force_cover(frames):
    for T in range(1, 41):
        for overlap in cm.overlaps(T, frames):
            rc, (f, n, stride) = _plan(T, frames, overlap)
            assert rc == 0, (T, frames, overlap, _lib.last_error())
            m_f, ss = cm.starts(T, frames, overlap)
            assert (f, n, stride) == (m_f, len(ss), m_f - overlap) == (min(frames, T), len(ss), f - overlap)
            assert n == math.ceil((T - f) / stride) + 1
            p = clips.clip_plan(T, frames, overlap)
            got = p.starts(T)
            assert tuple(p) == (f, n, stride) and got == ss, (T, frames, overlap)
            assert all(a < b for a, b in zip(got, got[1:])), "starts ascend"
            assert got[0] == 0 and got[-1] + f == T, "the last window ends at T"
            cover = np.zeros(T, np.int64)
            for s in got:
                assert 0 <= s and s + f <= T
                cover[s:s + f] += 1
            assert cover.min() >= 1, "every frame is covered"
            assert np.array_equal(cover, cm.cover_count(T, frames, overlap))


def test_plan_of_the_documented_sizes():
    assert tuple(clips.clip_plan(64)) == (7, 13, 5)          # 0, 5, ..., 55, then 57
    assert clips.clip_plan(64).starts(64) == list(range(0, 57, 5)) + [57]
    assert tuple(clips.clip_plan(7)) == (7, 1, 5) and tuple(clips.clip_plan(5, 7, 2)) == (5, 1, 3)
    assert tuple(clips.clip_plan(8, 3, 0)) == (3, 3, 3) and clips.clip_plan(8, 3, 0).starts(8) == [0, 3, 5]


BAD_PLANS = [(dict(T=0), CONFIG), (dict(T=-3), CONFIG), (dict(frames=0), CONFIG), (dict(frames=-7), CONFIG),
             (dict(overlap=-1), SHAPE), (dict(overlap=3), SHAPE), (dict(overlap=4), SHAPE),
             (dict(T=2, overlap=2), SHAPE), (dict(T=1, overlap=1), SHAPE), (dict(frames=50, overlap=8), SHAPE)]


def test_plan_argument_checks():
    ok = dict(T=8, frames=3, overlap=1)
    assert _plan(**ok)[0] == 0
    for kw, code in BAD_PLANS:
        rc, out = _plan(**{**ok, **kw})
        assert rc == code and "kdlae_clip_plan" in _lib.last_error(), kw
        assert out == [-7] * 3   # nothing is written on a refusal
        with pytest.raises(RuntimeError, match="EINVAL"):
            clips.clip_plan(**{**ok, **kw})
    L = _lib.lib()
    v = [ctypes.c_int() for _ in range(3)]
    for k in range(3):
        args = [ctypes.byref(x) for x in v]
        args[k] = None
        assert L.kdlae_clip_plan(8, 3, 1, *args) == CONFIG and "null" in _lib.last_error()


# ------------------------------------------------------------------ every refusal, without a launch
def _gather(src=P, B=2, T=8, H=5, W=7, frames=3, overlap=1, first=0, count=1, dst=P):
    return _lib.lib().kdlae_clip_gather(src, B, T, H, W, frames, overlap, first, count, dst, None)


def _blend(windows=P, B=2, T=8, H=5, W=7, frames=3, overlap=1, wt=None, dst=P):
    return _lib.lib().kdlae_clip_blend(windows, B, T, H, W, frames, overlap, wt, dst, None)


def _blend_u8(windows=P, B=2, T=8, H=5, W=7, h=5, w=7, frames=3, overlap=1, wt=None, dst=P):
    return _lib.lib().kdlae_clip_blend_u8(windows, B, T, H, W, h, w, frames, overlap, wt, dst, None)


SIZES = (dict(B=0), dict(B=-1), dict(H=0), dict(W=0), dict(H=-5), dict(W=-7))


def test_gather_argument_checks_need_no_launch():
    for kw in (dict(src=None), dict(dst=None)):
        assert _gather(**kw) == CONFIG and "null argument" in _lib.last_error(), kw
    for kw in SIZES + (dict(count=0), dict(count=-2), dict(first=-1)):
        assert _gather(**kw) == CONFIG and "kdlae_clip_gather" in _lib.last_error(), kw
    for kw, code in BAD_PLANS:
        assert _gather(**kw) == code and "kdlae_clip_gather" in _lib.last_error(), kw
    # T 8, frames 3, overlap 1: starts 0, 2, 4, 5; 4 windows per clip, 8 in all
    assert _plan(8, 3, 1) == (0, [3, 4, 2])
    for first, count in ((0, 9), (8, 1), (7, 2), (2**31 - 1, 2**31 - 1)):
        assert _gather(first=first, count=count) == CONFIG and "first + count" in _lib.last_error(), (first, count)


def test_blend_argument_checks_need_no_launch():
    for call in (_blend, _blend_u8):
        for kw in (dict(windows=None), dict(dst=None)):
            assert call(**kw) == CONFIG and "null argument" in _lib.last_error(), kw
        for kw in SIZES:
            assert call(**kw) == CONFIG and "kdlae_clip_blend" in _lib.last_error(), kw
        for kw, code in BAD_PLANS:
            assert call(**kw) == code and "kdlae_clip_blend" in _lib.last_error(), kw
    for kw in (dict(h=6), dict(w=8), dict(h=0), dict(w=0), dict(h=-1), dict(h=6, w=8)):
        assert _blend_u8(**kw) == CONFIG and "kdlae_clip_blend_u8" in _lib.last_error(), kw
    # an index range the kernels could not hold in an int
    assert _blend(B=2**30, T=8) == SHAPE and "2^31" in _lib.last_error()
    assert _blend(H=2**16, W=2**16) == SHAPE and "2^31" in _lib.last_error()


def test_wrappers_and_modules_refuse_without_a_device():
    with pytest.raises(RuntimeError, match="cuda float32"):
        clips.clip_gather(torch.zeros(1, 8, 4, 4), 3, 1)
    with pytest.raises(RuntimeError, match="cuda float32"):
        clips.clip_blend(torch.zeros(4, 3, 4, 4), 1, 8, 3, 1)
    with pytest.raises(RuntimeError, match="cuda float32"):
        clips.clip_blend_u8(torch.zeros(4, 3, 4, 4), 1, 8, 4, 4, 3, 1)
    m = KDLAE_student(hidden_channels=[8, 16]).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_clip(torch.zeros(1, 9, 4, 4), frames=3, overlap=1)
    with pytest.raises(RuntimeError, match="cuda uint8"):
        pipeline.enhance_clip_u8(m, torch.zeros(1, 9, 40, 40, dtype=torch.uint8), frames=3, overlap=1)


# ------------------------------------------------------------------ the windows
def test_clip_window_is_the_tile_window_on_one_axis():
    assert clips.clip_window("uniform", 20, 7, 2, "cpu") is None and clips.clip_window(None, 20, 7, 2, "cpu") is None
    for T, frames in cm.GRID + [(64, 7)]:
        for overlap in cm.overlaps(T, frames):
            f, ss = cm.starts(T, frames, overlap)
            ramp = clips.clip_window("ramp", T, frames, overlap, "cpu").wt
            hann = clips.clip_window("hann", T, frames, overlap, "cpu").wt
            assert ramp.dtype == hann.dtype == torch.float32 and ramp.shape == hann.shape == (f,)
            assert np.array_equal(ramp.numpy(), cm.ramp_table(f, len(ss), overlap).astype(np.float32))
            # two float64 sines may differ in the last place, so their fp32 roundings by one fp32 place
            want = cm.hann_table(f).astype(np.float32)
            assert np.all(np.abs(hann.numpy() - want) <= np.spacing(want)) and bool((hann > 0).all())
    t = torch.tensor([0.5, 2.0, 1.0], dtype=torch.float64)
    got = clips.clip_window(t, 8, 3, 1, "cpu")
    assert got.wt.dtype == torch.float32 and torch.equal(got.wt, t.float())
    assert clips.clip_window(got, 8, 3, 1, "cpu") is got          # a checked table is taken as it is


def test_ramp_weights_of_two_regular_neighbours_sum_to_overlap_plus_one():
    for frames in (2, 3, 5, 7, 8):
        for overlap in range(1, frames // 2 + 1):
            T = 4 * frames
            wt = clips.clip_window("ramp", T, frames, overlap, "cpu").wt.numpy()
            stride = frames - overlap
            for j in range(overlap):   # frame stride + j of one window is frame j of the next
                assert wt[stride + j] + wt[j] == overlap + 1, (frames, overlap, j)
    # overlap 0: nothing to fade into, a table of ones
    assert np.array_equal(clips.clip_window("ramp", 21, 7, 0, "cpu").wt.numpy(), np.ones(7, np.float32))


def test_clip_window_argument_checks():
    for bad, text in (("triangle", "must be one of"), (3, "must be one of"), (torch.ones(3, dtype=torch.int32),
                      "floating-point"), (torch.ones(4), "window's length 3"), (torch.ones(1, 3), "window's length 3"),
                      (torch.tensor([1.0, 0.0, 1.0]), "greater than 0"), (torch.tensor([1.0, -1.0, 1.0]),
                      "greater than 0"), (torch.tensor([1.0, float("nan"), 1.0]), "finite"),
                      (torch.tensor([1.0, float("inf"), 1.0]), "finite"),
                      (torch.tensor([1.0, 1e-60, 1.0], dtype=torch.float64), "greater than 0"),
                      (clips.ClipWindow(torch.ones(4)), "length 3")):
        with pytest.raises(RuntimeError, match=text):
            clips.clip_window(bad, 8, 3, 1, "cpu")
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        clips.clip_window("ramp", 8, 3, 3, "cpu")


# ------------------------------------------------------------------ the CPU model itself
def _grid():
    for T, frames in cm.GRID:
        for overlap in cm.overlaps(T, frames):
            for H, W in cm.FRAME_SIZES:
                yield T, frames, overlap, H, W


def test_model_equals_the_host_loop_bit_for_bit():
    for T, frames, overlap, H, W in _grid():
        win = cm.case_windows(T, frames, overlap, H, W)
        want = cm.host_loop(torch.from_numpy(win), cm.B, T, frames, overlap).numpy()
        assert _same_bits(cm.blend(win, cm.B, T, frames, overlap), want), (T, frames, overlap, H, W)


def test_model_gather_then_blend_of_an_exactly_summable_clip():
    """Small integers sum and divide exactly: blending the windows of a clip gives the clip back."""
    x = torch.randint(-8, 9, (2, 13, 4, 6), generator=torch.Generator().manual_seed(3)).float()
    for frames, overlap in ((4, 0), (4, 1), (4, 3), (7, 2), (13, 5), (20, 12)):
        win = cm.gather(x, frames, overlap)
        assert win.shape[1] == min(frames, 13)
        assert torch.equal(torch.from_numpy(cm.blend(win.numpy(), 2, 13, frames, overlap)), x)
        assert torch.equal(torch.from_numpy(cm.blend(win.numpy(), 2, 13, frames, overlap,
                                                     cm.random_table(min(frames, 13)) * 0 + 2)), x)


def test_tables_of_ones_give_the_uniform_models_bits_but_for_a_lone_negative_zero():
    for T, frames, overlap, H, W in _grid():
        win = cm.case_windows(T, frames, overlap, H, W)
        f = min(frames, T)
        assert _same_bits(cm.blend(win, cm.B, T, frames, overlap, np.ones(f, np.float32)),
                          cm.blend(win, cm.B, T, frames, overlap)), (T, frames, overlap, H, W)
    win = cm.case_windows(8, 3, 1, 4, 6)
    win[0, 0, 0, 0] = -0.0   # frame 0 lies under window 0 alone
    uni = cm.blend(win, cm.B, 8, 3, 1)
    one = cm.blend(win, cm.B, 8, 3, 1, np.ones(3, np.float32))
    assert not np.signbit(uni[0, 0, 0, 0]) and np.signbit(one[0, 0, 0, 0])   # 0 + -0 = +0; the copy keeps -0
    uni[0, 0, 0, 0] = -0.0
    assert _same_bits(uni, one)


def test_a_one_window_plan_returns_the_window():
    for T, frames in ((7, 7), (5, 7), (1, 1), (1, 7)):
        for overlap in cm.overlaps(T, frames):
            f, ss = cm.starts(T, frames, overlap)
            assert ss == [0] and f == T
            win = cm.case_windows(T, frames, overlap, 5, 7)
            assert _same_bits(cm.blend(win, cm.B, T, frames, overlap), win)
            for wt in (cm.random_table(f), cm.hann_table(f).astype(np.float32)):
                assert _same_bits(cm.blend(win, cm.B, T, frames, overlap, wt), win)
            assert np.array_equal(cm.blend_u8(win, cm.B, T, 4, 5, frames, overlap), cm.to_u8(win, 4, 5))


def test_u8_rule_rounds_exact_halves_to_even():
    halves = cm.exact_halves()
    assert halves.size >= 17   # enough to fill the smallest frame of the kernel test past the seven other plants
    prod = halves * np.float32(255)
    assert np.array_equal(prod - np.floor(prod), np.full(halves.size, 0.5, np.float32))
    got = cm.to_u8(halves.reshape(1, -1), 1, halves.size)[0]
    assert np.all(got % 2 == 0) and np.all(np.abs(got.astype(np.float32) - prod) == 0.5)
    k = np.floor(prod).astype(np.int64)
    assert (k % 2 == 0).any() and (k % 2 == 1).any()   # both directions occur: down to an even k, up to k + 1
    edge = np.array([[-3.0, -0.0, 0.0, 1.0, 7.5, 0.999, 0.001, 0.5]], np.float32)
    assert cm.to_u8(edge, 1, 8).tolist() == [[0, 0, 0, 255, 255, 255, 0, 128]]


# ------------------------------------------------------------------ the mutants, on the GPU tests' inputs
def _differs(mutant, form):
    """Whether `mutant` changes a bit of the compared output of `form` somewhere on the kernel tests' grid."""
    for T, frames, overlap, H, W in _grid():
        wt = cm.case_table(T, frames, overlap) if form == "weighted" else None
        if form == "u8":
            win = cm.case_windows_u8(T, frames, overlap, H, W)
            h, w = max(H - 1, 1), max(W - 2, 1)
            if not np.array_equal(cm.blend_u8(win, cm.B, T, h, w, frames, overlap),
                                  cm.blend_u8(win, cm.B, T, h, w, frames, overlap, mutant=mutant)):
                return True
            continue
        win = cm.case_windows(T, frames, overlap, H, W)
        good, bad = cm.blend(win, cm.B, T, frames, overlap, wt), cm.blend(win, cm.B, T, frames, overlap, wt, mutant)
        if not np.array_equal(_bits(good), _bits(bad)):   # on the bits: a NaN differs from a number
            return True
    return False


@pytest.mark.parametrize("mutant,form", [("descending", "uniform"), ("descending", "weighted"),
                                         ("stride_count", "uniform"), ("stride_count", "weighted"),
                                         ("last_start", "uniform"), ("last_start", "weighted"),
                                         ("fma", "weighted"), ("round_first", "u8"), ("stride_count", "u8"),
                                         ("last_start", "u8")])
def test_every_mutant_changes_a_compared_bit(mutant, form):
    assert mutant in cm.MUTANTS and _differs(mutant, form)


def test_mutants_leave_a_plan_they_do_not_touch_alone():
    """T == frames has one window: no order, no clamped start, no second term."""
    win = cm.case_windows(7, 7, 2, 4, 6)
    for mutant in ("descending", "stride_count", "last_start"):
        assert _same_bits(cm.blend(win, cm.B, 7, 7, 2, mutant=mutant), win)

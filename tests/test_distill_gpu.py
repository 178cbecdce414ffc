"""Distillation labels on the GPU: kdlae_distill_expand_u8 / kdlae_distill_expand_f32 / kdlae_distill_collapse against
the numpy model (tests/distill_model.py), then ``teacher_labels`` / ``teacher_labels_u8`` / ``DistillTrainer`` against
the per-frame host loop they replace (``distill_model.host_labels``: the project's own ``enhance_u8`` and the gray
rule in integer torch ops).

The kernels move, convert and quantise by stated rules and the forward is deterministic, so every comparison here is
bit for bit or byte for byte: no tolerance anywhere in this file."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, distill
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher, Restormer
from rethink_acoustic_image_enhancement_amd.pipeline import distill_clip_u8
from rethink_acoustic_image_enhancement_amd.train import DistillTrainer, KDLAESTrainer
from tests import distill_model as dm

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30      # the fill of fp32 storage that must stay untouched
POISON = 0xA5   # the same for u8 storage
G = 64          # guard elements either side of a buffer under test


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    return np.array_equal(a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else np.array_equal(a, b)


class _Buf:
    """A contiguous tensor of ``shape`` that starts ``off`` elements past a 16-byte boundary, inside poisoned storage
    with guards either side; ``init``: the contents (default: poison everywhere)."""

    def __init__(self, shape, dtype, off, init=None):
        self.n = int(np.prod(shape))
        self.fill = BIG if dtype == torch.float32 else POISON
        self.store = torch.full((G + off + self.n + G,), self.fill, dtype=dtype, device=DEV)
        assert self.store.data_ptr() % 16 == 0
        self.lo = G + off
        self.t = self.store[self.lo:self.lo + self.n].view(shape)
        assert self.t.data_ptr() % 16 == (off * self.t.element_size()) % 16
        if init is not None:
            self.t.copy_(torch.from_numpy(np.ascontiguousarray(init)))

    def snapshot(self):
        return self.store.clone()

    def check(self, want):
        """The buffer holds ``want`` bit for bit and the guards are whole."""
        got = self.store.cpu().numpy()
        assert _same_bits(got[self.lo:self.lo + self.n].reshape(want.shape), want)
        assert (got[:self.lo] == got.dtype.type(self.fill)).all() and (got[self.lo + self.n:] == got.dtype.type(self.fill)).all()


def _twice(call, *bufs):
    """Run ``call`` twice; the second run must leave every buffer's storage as the first did."""
    assert call() == 0, _lib.last_error()
    first = [b.snapshot() for b in bufs]
    assert call() == 0, _lib.last_error()
    for b, s in zip(bufs, first):
        assert torch.equal(b.store.view(torch.uint8), s.view(torch.uint8))


# (u8 source byte offset, img float offset, rate-map float offset): both fp32 buffers on 16 bytes is the 16-byte path
# (with the source on 4 bytes and w % 4 == 0 its bytes come as 32-bit words), anything else the 4-byte one
EXPAND_OFFSETS = [(0, 0, 0), (1, 0, 0), (1, 1, 0), (2, 0, 2), (3, 3, 3)]


# ------------------------------------------------------------------ 1. each entry against the model
@pytest.mark.parametrize("C", dm.CHANNELS)
@pytest.mark.parametrize("hw", dm.SIZES)
def test_expand_u8_equals_the_model(hw, C):
    L = _lib.lib()
    h, w = hw
    H, W = dm.padded_size(h, w, 8)
    for B, F in dm.STACKS:
        frames, rate = dm.case_frames_u8(B, F, h, w, C), dm.case_rate(B, F)
        d_rate = torch.from_numpy(rate).to(DEV)
        for src_off, img_off, map_off in EXPAND_OFFSETS:
            src = _Buf(frames.shape, torch.uint8, src_off, frames)
            for j0, n in dm.case_chunks(B, F):
                img, rmap = _Buf((n, 3, H, W), torch.float32, img_off), _Buf((n, 1, H, W), torch.float32, map_off)
                _twice(lambda: L.kdlae_distill_expand_u8(_c(src.t), B, F, h, w, C, 8, _c(d_rate), j0, n, _c(img.t),
                                                         _c(rmap.t), None), img, rmap)
                want_img, want_map = dm.expand_u8(frames, rate, j0, n)
                img.check(want_img)
                rmap.check(want_map)
            src.check(frames)
    # no rate, no map: a Restormer teacher's input
    img = _Buf((2, 3, H, W), torch.float32, 0)
    _twice(lambda: L.kdlae_distill_expand_u8(_c(src.t), B, F, h, w, C, 8, None, 1, 2, _c(img.t), None, None), img)
    img.check(dm.expand_u8(frames, None, 1, 2)[0])


@pytest.mark.parametrize("hw", dm.F32_SIZES)
def test_expand_f32_is_a_bit_copy(hw):
    L = _lib.lib()
    H, W = hw
    for B, F in dm.STACKS:
        frames, rate = dm.case_frames_f32(B, F, H, W), dm.case_rate(B, F)
        d_rate = torch.from_numpy(rate).to(DEV)
        for src_off, img_off, map_off in [(0, 0, 0), (1, 0, 0), (0, 1, 0), (2, 0, 2), (3, 3, 3)]:
            src = _Buf(frames.shape, torch.float32, src_off, frames)
            for j0, n in dm.case_chunks(B, F):
                img, rmap = _Buf((n, 3, H, W), torch.float32, img_off), _Buf((n, 1, H, W), torch.float32, map_off)
                _twice(lambda: L.kdlae_distill_expand_f32(_c(src.t), B, F, H, W, _c(d_rate), j0, n, _c(img.t),
                                                          _c(rmap.t), None), img, rmap)
                want_img, want_map = dm.expand_f32(frames, rate, j0, n)
                img.check(want_img)
                rmap.check(want_map)
    img = _Buf((1, 3, H, W), torch.float32, 0)
    _twice(lambda: L.kdlae_distill_expand_f32(_c(src.t), B, F, H, W, None, 1, 1, _c(img.t), None, None), img)
    img.check(dm.expand_f32(frames, None, 1, 1)[0])


# (hq float offset, dst element offset, u8 source byte offset)
COLLAPSE_OFFSETS = [(0, 0, 0), (0, 0, 1), (1, 0, 0), (0, 1, 2), (2, 2, 3), (3, 3, 0)]


@pytest.mark.parametrize("C", [0] + dm.CHANNELS)
@pytest.mark.parametrize("hw", dm.SIZES)
def test_collapse_equals_the_model(hw, C):
    """Both modes, both output types, with (C > 0) and without the mask; the items outside the chunk and the guards
    keep their fill."""
    L = _lib.lib()
    h, w = hw
    Hp, Wp = dm.padded_size(h, w, 8)
    for B, F in dm.STACKS:
        frames = dm.case_frames_u8(B, F, h, w, C) if C else None
        for hq_off, dst_off, src_off in COLLAPSE_OFFSETS:
            src = _Buf(frames.shape, torch.uint8, src_off, frames) if C else None
            for j0, n in dm.case_chunks(B, F):
                hq_np = dm.case_hq(n, Hp, Wp)
                hq = _Buf(hq_np.shape, torch.float32, hq_off, hq_np)
                for mode, dtype in ((dm.FILE, torch.float32), (dm.FILE, torch.uint8), (dm.MEAN, torch.float32)):
                    dst = _Buf((B, F, h, w), dtype, dst_off)
                    start = dst.t.cpu().numpy()
                    _twice(lambda: L.kdlae_distill_collapse(_c(hq.t), B, F, Hp, Wp, h, w, j0, n, distill.MODES[mode],
                                                            _c(src.t) if C else None, C, _c(dst.t),
                                                            int(dtype == torch.uint8), None), dst)
                    dst.check(dm.collapse(start, hq_np, j0, n, mode, frames))
                hq.check(hq_np)


def test_past_the_grid_cap():
    """More pixel groups than 4096 blocks of 256 threads take in one pass, on both paths of every kernel: 7 frames of
    390 x 402 (padded to 392 x 408) with single-element accesses, 7 frames of 776 x 792 with 16-byte ones."""
    L = _lib.lib()
    B, F = 1, 7
    for (h, w), off in (((390, 402), 1), ((776, 792), 0)):
        H, W = dm.padded_size(h, w, 8)
        assert B * F * h * (w // (1 if off else 4)) > 4096 * 256
        frames, rate = dm.case_frames_u8(B, F, h, w, 1), dm.case_rate(B, F)
        d_frames, d_rate = torch.from_numpy(frames).to(DEV), torch.from_numpy(rate).to(DEV)
        img, rmap = _Buf((B * F, 3, H, W), torch.float32, off), _Buf((B * F, 1, H, W), torch.float32, off)
        rc = L.kdlae_distill_expand_u8(_c(d_frames), B, F, h, w, 1, 8, _c(d_rate), 0, B * F, _c(img.t), _c(rmap.t), None)
        assert rc == 0, _lib.last_error()
        want_img, want_map = dm.expand_u8(frames, rate, 0, B * F)
        img.check(want_img)
        rmap.check(want_map)
        # the expanded frames as fp32 network inputs, then collapsed: a stand-in for the teacher's output
        x = _Buf((B, F, H, W), torch.float32, off, want_img[:, 0])
        img2 = _Buf((B * F, 3, H, W), torch.float32, off)
        rc = L.kdlae_distill_expand_f32(_c(x.t), B, F, H, W, None, 0, B * F, _c(img2.t), None, None)
        assert rc == 0, _lib.last_error()
        img2.check(want_img)
        hq_np = dm.case_hq(B * F, H, W)
        hq = _Buf(hq_np.shape, torch.float32, off, hq_np)
        for mode, dtype in ((dm.FILE, torch.float32), (dm.FILE, torch.uint8), (dm.MEAN, torch.float32)):
            dst = _Buf((B, F, h, w), dtype, off)
            rc = L.kdlae_distill_collapse(_c(hq.t), B, F, H, W, h, w, 0, B * F, distill.MODES[mode], _c(d_frames), 1,
                                          _c(dst.t), int(dtype == torch.uint8), None)
            assert rc == 0, _lib.last_error()
            dst.check(dm.collapse(dst.t.cpu().numpy(), hq_np, 0, B * F, mode, frames))


# ------------------------------------------------------------------ 2. teacher_labels against the host loop
T_CFG = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
LB, LF, LH, LW = 2, 5, 24, 40
TBS = [1, 4, 16]    # one frame a forward; a value that does not divide B F = 10; a value above it


@functools.lru_cache(maxsize=None)
def _teacher(kind="teacher"):
    m = (Restormer if kind == "restormer" else KDLAE_teacher)(**T_CFG)
    load_hash_weights(m)
    m.hip_graphs = False
    return m.to(DEV).eval()


@functools.lru_cache(maxsize=None)
def _clip(C=1):
    return torch.from_numpy(dm.case_frames_u8(LB, LF, LH, LW, C)).to(DEV)


def _rate(form):
    if form == "scalar":
        return 0.6
    if form == "per_sample":
        return torch.tensor([0.3, 0.8])
    return torch.from_numpy(dm.case_rate(LB, LF).reshape(LB, LF))


@functools.lru_cache(maxsize=None)
def _host(form, mode, u8_out=False, C=1, kind="teacher", tiled=False):
    """The host loop's labels, computed once per case and shared (never written to)."""
    kw = dict(tile=16, tile_overlap=4) if tiled else None
    rate = None if kind == "restormer" else _rate(form)
    return dm.host_labels(_teacher(kind), _clip(C), rate, mode, u8_out, kw)


def _eq(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and _same_bits(a.cpu().numpy(), b.cpu().numpy())


@pytest.mark.parametrize("mode", [dm.FILE, dm.MEAN])
@pytest.mark.parametrize("form", ["scalar", "per_item"])
def test_teacher_labels_equal_the_host_loop(form, mode):
    ref = _host(form, mode)
    assert ref.dtype == torch.float32 and tuple(ref.shape) == (LB, LF, LH, LW)
    for tb in TBS:
        got = distill.teacher_labels(_teacher(), _clip(), _rate(form), mode=mode, teacher_batch=tb)
        assert _eq(got, ref), tb
    if mode == dm.FILE:   # the quantised labels are not the unquantised ones
        assert not _eq(ref, _host(form, dm.MEAN))


def test_teacher_labels_u8_and_the_pipeline_wrapper():
    ref = _host("per_item", dm.FILE, True)
    assert ref.dtype == torch.uint8
    rate = _rate("per_item")
    for tb in TBS:
        assert _eq(distill.teacher_labels_u8(_teacher(), _clip(), rate, teacher_batch=tb), ref), tb
    assert _eq(distill_clip_u8(_teacher(), _clip(), rate, teacher_batch=4), ref)
    # the float labels are these bytes / 255; out= is written in place and returned
    out = torch.full((LB, LF, LH, LW), BIG, device=DEV)
    got = distill.teacher_labels(_teacher(), _clip(), rate, teacher_batch=4, out=out)
    assert got.data_ptr() == out.data_ptr()
    assert _same_bits(out.cpu().numpy(), ref.cpu().numpy().astype(np.float32) / np.float32(255))


def test_per_sample_rate_and_colour_frames():
    assert _eq(distill.teacher_labels(_teacher(), _clip(), _rate("per_sample"), teacher_batch=4),
               _host("per_sample", dm.FILE))
    for C in (3, 4):
        assert _eq(distill.teacher_labels_u8(_teacher(), _clip(C), 0.6, teacher_batch=4), _host("scalar", dm.FILE, True, C))


@pytest.mark.parametrize("mode", [dm.FILE, dm.MEAN])
def test_float_frames_equal_the_host_loop(mode):
    x = torch.from_numpy(hash_images("distill:f32", (LB, LF, LH, LW), -0.1, 1.1)).to(DEV)
    rate = _rate("per_item")
    ref = dm.host_labels(_teacher(), x, rate, mode)
    for tb in (4, 16):
        assert _eq(distill.teacher_labels(_teacher(), x, rate, mode=mode, teacher_batch=tb), ref), tb


def test_tiled_route_equals_the_loop_over_enhance_tiled_u8():
    ref = _host("scalar", dm.FILE, True, tiled=True)
    for tb in (1, 4):
        got = distill.teacher_labels_u8(_teacher(), _clip(), 0.6, teacher_batch=tb, tile=16, tile_overlap=4)
        assert _eq(got, ref), tb
    assert not _eq(ref, _host("scalar", dm.FILE, True))   # another function of the frame, as the docs say


def test_restormer_teacher():
    ref = _host("none", dm.FILE, True, kind="restormer")
    for tb in (4, 16):
        assert _eq(distill.teacher_labels_u8(_teacher("restormer"), _clip(), None, teacher_batch=tb), ref), tb
    ref = _host("none", dm.MEAN, kind="restormer")
    assert _eq(distill.teacher_labels(_teacher("restormer"), _clip(), None, mode=dm.MEAN, teacher_batch=4), ref)


def test_refusals_before_any_launch():
    t = _teacher()
    out = torch.full((LB, LF, LH, LW), BIG, device=DEV)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distill.teacher_labels(t, _clip().cpu(), 0.6, out=out)
    with pytest.raises(RuntimeError, match="expects cuda uint8"):
        distill.teacher_labels(t, _clip().to(torch.int32), 0.6, out=out)
    with pytest.raises(RuntimeError, match="uint8"):
        distill.teacher_labels_u8(t, _clip().to(torch.float32), 0.6)
    with pytest.raises(RuntimeError, match="denoise_rate"):
        distill.teacher_labels(t, _clip(), None, out=out)
    with pytest.raises(RuntimeError, match="out must be"):
        distill.teacher_labels(t, _clip(), 0.6, out=out[:, :, :, :-1])
    with pytest.raises(RuntimeError, match="teacher_batch"):
        distill.teacher_labels(t, _clip(), 0.6, teacher_batch=0, out=out)
    trainee = KDLAE_teacher(**T_CFG).to(DEV).train()
    with pytest.raises(RuntimeError, match="inference-only"):
        distill.teacher_labels(trainee, _clip(), 0.6, out=out)
    with pytest.raises(RuntimeError, match="eval mode"):
        DistillTrainer(KDLAE_student(hidden_channels=[16, 32, 64]).to(DEV), trainee, 0.6)
    assert bool((out == BIG).all())


# ------------------------------------------------------------------ 3. DistillTrainer against KDLAESTrainer
S_CFG = dict(hidden_channels=[16, 32, 64])
TB_, TF, TH, TW = 2, 7, 32, 32


def _student():
    m = KDLAE_student(**S_CFG)
    load_hash_weights(m)
    return m.to(DEV)


def _batch(i):
    return torch.from_numpy(hash_images(f"distill:lq{i}", (TB_, TF, TH, TW), 0.0, 1.0)).to(DEV)


@pytest.mark.parametrize("label_mode", [dm.MEAN, dm.FILE])
def test_distill_trainer_equals_the_trainer_on_host_labels(label_mode):
    teacher = _teacher()
    before = [p.detach().clone() for p in teacher.parameters()]
    rate = torch.from_numpy(dm.case_rate(TB_, TF).reshape(TB_, TF))
    kw = dict(lr=1e-3)
    dt = DistillTrainer(_student(), teacher, rate, label_mode=label_mode, teacher_batch=4, **kw)
    ref = KDLAESTrainer(_student(), **kw)
    assert _eq(dt.theta, ref.theta)
    ptr = None
    for i in range(2):
        lq = _batch(i)
        labels = dm.host_labels(teacher, lq, rate, label_mode)
        loss = dt.optimize_parameters(lq)
        loss_ref = ref.optimize_parameters(lq, labels)
        assert _eq(dt.labels, labels), i
        assert _eq(loss.reshape(1), loss_ref.reshape(1)), i
        for name in ("theta", "exp_avg", "exp_avg_sq"):
            assert _eq(getattr(dt, name), getattr(ref, name)), (i, name)
        assert ptr is None or dt.labels.data_ptr() == ptr   # the label buffer is kept across steps
        ptr = dt.labels.data_ptr()
    assert dt.step_count == 2 and not _eq(dt.theta, KDLAESTrainer(_student(), **kw).theta)
    for p, b in zip(teacher.parameters(), before):
        assert _eq(p.detach(), b)
    assert not teacher.training and "teacher" not in str(sorted(dt.training_state(0, 2)))


def test_distill_trainer_labels_come_from_clean():
    teacher = _teacher()
    dt = DistillTrainer(_student(), teacher, 0.6, teacher_batch=16, lr=1e-3)
    ref = KDLAESTrainer(_student(), lr=1e-3)
    clean = _batch(2)
    lq = clean.clone()
    lq[:, 2] = 0.0          # a masked frame, as augment.mask_frames leaves it
    lq[:, 5] = 0.0
    labels = dm.host_labels(teacher, clean, 0.6, dm.MEAN)
    loss = dt.optimize_parameters(lq, clean=clean)
    loss_ref = ref.optimize_parameters(lq, labels)
    assert _eq(dt.labels, labels) and not _eq(dt.labels, dm.host_labels(teacher, lq, 0.6, dm.MEAN))
    assert _eq(loss.reshape(1), loss_ref.reshape(1)) and _eq(dt.theta, ref.theta)

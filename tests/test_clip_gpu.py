"""Clip inference on the GPU: kdlae_clip_gather / kdlae_clip_blend / kdlae_clip_blend_u8 against slicing and the
CPU model (tests/clip_model.py), then KDLAE_student.forward_clip and pipeline.enhance_clip_u8 against the
per-window host loop they replace.

The kernels copy, multiply, add in a fixed order, divide and round, each operation on its own, and batch rows of
the student's forward are bit for bit independent of the batch size
(test_kdlae_s_gpu.test_batch_invariance_and_determinism), so every comparison here is on the bits: no tolerance
anywhere in this file."""
import functools

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, clips
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_clip_u8, frames_preprocess_u8, postprocess_u8
from tests import clip_model as cm
from tests.test_tile_gpu import BIG, DEV, G, OFFSETS, _c, _expect_store, _same_bits, _stored

pytestmark = pytest.mark.gpu
B = cm.B
GUARD = 0xAB   # the byte either side of a u8 destination under test


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


# ------------------------------------------------------------------ 1. kdlae_clip_gather against slicing
@pytest.mark.parametrize("hw", cm.FRAME_SIZES)
@pytest.mark.parametrize("T,frames", cm.GRID)
def test_gather_equals_slicing(T, frames, hw):
    L = _lib.lib()
    H, W = hw
    x = _t(hash_images(f"clip:g:{T}:{H}x{W}", (B, T, H, W)))
    for overlap in cm.overlaps(T, frames):
        want = cm.gather(x, frames, overlap)
        n, per = want.shape[0], want.shape[0] // B
        ranges = sorted({(0, n), (n // 2, 1), (per - 1, 2), (n - 1, 1)})   # all, one window, across two clips, last
        for so, do in OFFSETS:
            src_store, src = _stored(x, so)
            src0 = src_store.clone()
            for first, count in ranges:
                exp = _expect_store(want[first:first + count], do)
                got = []
                for _ in range(2):
                    dst_store = torch.full((exp.numel(),), BIG, device=DEV)
                    rc = L.kdlae_clip_gather(_c(src), B, T, H, W, frames, overlap, first, count,
                                             _c(dst_store[G + do:]), None)
                    assert rc == 0, _lib.last_error()
                    got.append(dst_store)
                assert _same_bits(got[0], got[1])
                assert _same_bits(got[0], exp), (overlap, so, do, first, count)
            assert _same_bits(src_store, src0)


def test_gather_wrapper():
    x = _t(hash_images("clip:gw", (2, 13, 4, 6))).to(DEV)
    want = cm.gather(x.cpu(), 4, 1)
    assert torch.equal(clips.clip_gather(x, 4, 1).cpu(), want)
    assert torch.equal(clips.clip_gather(x, 4, 1, first=3).cpu(), want[3:])
    out = torch.empty((3, 4, 4, 6), device=DEV)
    assert clips.clip_gather(x, 4, 1, 2, 3, out=out) is out and torch.equal(out.cpu(), want[2:5])
    with pytest.raises(RuntimeError, match="first \\+ count"):
        clips.clip_gather(x, 4, 1, first=want.shape[0], count=1)
    with pytest.raises(RuntimeError, match="out must be"):
        clips.clip_gather(x, 4, 1, 0, 3, out=torch.empty((3, 4, 4, 5), device=DEV))


# ------------------------------------------------------------------ 2. kdlae_clip_blend against the model
def _blend_abi(win_view, T, H, W, frames, overlap, wt, do):
    """Two calls into BIG-filled storage at destination offset `do` -> the storage (equal bits asserted)."""
    got = []
    for _ in range(2):
        dst_store = torch.full((G + do + B * T * H * W + G,), BIG, device=DEV)
        rc = _lib.lib().kdlae_clip_blend(_c(win_view), B, T, H, W, frames, overlap, _c(wt), _c(dst_store[G + do:]), None)
        assert rc == 0, _lib.last_error()
        got.append(dst_store)
    assert _same_bits(got[0], got[1])
    return got[0]


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hw", cm.FRAME_SIZES)
@pytest.mark.parametrize("T,frames", cm.GRID)
def test_blend_equals_the_model(T, frames, hw, weighted):
    H, W = hw
    for overlap in cm.overlaps(T, frames):
        win = cm.case_windows(T, frames, overlap, H, W)
        wt = cm.case_table(T, frames, overlap) if weighted else None
        want = _t(cm.blend(win, B, T, frames, overlap, wt))
        wt_store, wt_view = _stored(_t(wt), 1) if weighted else (None, None)   # the table needs no alignment
        for so, do in OFFSETS:
            w_store, w_view = _stored(_t(win), so)
            w0 = w_store.clone()
            got = _blend_abi(w_view, T, H, W, frames, overlap, wt_view, do)
            assert _same_bits(got, _expect_store(want, do)), (overlap, so, do)
            assert _same_bits(w_store, w0)
        if weighted:
            assert _same_bits(wt_store, _expect_store(_t(wt), 1))


@pytest.mark.parametrize("shape", [(17, 257, 257), (20, 512, 512)])
def test_blend_more_items_than_one_pass_of_the_grid(shape):
    """The launcher caps the grid at 4096 blocks of 256 threads and loops over the rest: more than 4096 * 256 items,
    of 1 float on the 4-byte path (257 x 257 frames) and of 4 floats on the 16-byte path (512 x 512 frames)."""
    T, H, W = shape
    assert T * H * W // (4 if H * W % 4 == 0 else 1) > 4096 * 256
    f, ss = cm.starts(T, 7, 2)
    win = (torch.rand((len(ss), f, H, W), generator=torch.Generator().manual_seed(T)) * 2 - 1)
    wt = cm.random_table(f, 5)
    dev = win.to(DEV)
    for table in (None, wt):
        want = _t(cm.blend(win.numpy(), 1, T, 7, 2, table)).to(DEV)
        got = clips.clip_blend(dev, 1, T, 7, 2, window=_t(table) if table is not None else "uniform")
        assert _same_bits(got, want)
        assert _same_bits(clips.clip_blend(dev, 1, T, 7, 2, window=_t(table) if table is not None else None), got)


def test_blend_wrapper_names_out_and_one_window():
    T, frames, overlap, H, W = 13, 4, 1, 4, 6
    win = cm.case_windows(T, frames, overlap, H, W)
    dev = _t(win).to(DEV)
    for name in ("ramp", "hann"):
        table = _table(name, T, frames, overlap)[1]
        want = _t(cm.blend(win, B, T, frames, overlap, table)).to(DEV)
        assert _same_bits(clips.clip_blend(dev, B, T, frames, overlap, window=name), want), name
    out = torch.empty((B, T, H, W), device=DEV)
    assert clips.clip_blend(dev, B, T, frames, overlap, out=out) is out
    assert _same_bits(out, _t(cm.blend(win, B, T, frames, overlap)).to(DEV))
    with pytest.raises(RuntimeError, match="expected windows"):
        clips.clip_blend(dev[1:], B, T, frames, overlap)
    with pytest.raises(RuntimeError, match="out must be"):
        clips.clip_blend(dev, B, T, frames, overlap, out=torch.empty((B, T, H, W + 1), device=DEV))
    # one window per clip: the window, under every table
    one = _t(cm.case_windows(5, 7, 2, 5, 7)).to(DEV)
    for window in ("uniform", "ramp", "hann", _t(cm.random_table(5))):
        assert _same_bits(clips.clip_blend(one, B, 5, 7, 2, window=window), one)


# ------------------------------------------------------------------ 3. kdlae_clip_blend_u8
def _crops(H, W):
    """(h, w): a crop on both axes (single-byte stores), none, and, where W allows, a crop that keeps w % 4 == 0."""
    return sorted({(H - 1, W - 2), (H, W)} | ({(H - 1, 4)} if W % 4 == 0 else set()))


@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("hw", cm.FRAME_SIZES)
@pytest.mark.parametrize("T,frames", cm.GRID)
def test_blend_u8_equals_postprocess_of_the_f32_blend(T, frames, hw, weighted):
    H, W = hw
    for overlap in cm.overlaps(T, frames):
        win = cm.case_windows_u8(T, frames, overlap, H, W)
        wt = cm.case_table(T, frames, overlap) if weighted else None
        dev, wt_dev = _t(win).to(DEV), (_t(wt).to(DEV) if weighted else None)
        f32 = clips.clip_blend(dev, B, T, frames, overlap, window=wt_dev)
        for h, w in _crops(H, W):
            want = postprocess_u8(f32, h, w, 1, None).permute(0, 3, 1, 2).contiguous()   # [B,h,w,T] -> [B,T,h,w]
            assert torch.equal(want.cpu(), _t(cm.blend_u8(win, B, T, h, w, frames, overlap, wt))), (overlap, h, w)
            n = want.numel()
            for do in range(4):
                got = []
                for _ in range(2):
                    store = torch.full((G + do + n + G,), GUARD, device=DEV, dtype=torch.uint8)
                    assert store.data_ptr() % 16 == 0
                    rc = _lib.lib().kdlae_clip_blend_u8(_c(dev), B, T, H, W, h, w, frames, overlap, _c(wt_dev),
                                                        _c(store[G + do:]), None)
                    assert rc == 0, _lib.last_error()
                    got.append(store)
                assert torch.equal(got[0], got[1])
                exp = torch.full_like(store, GUARD)
                exp[G + do:G + do + n] = want.view(-1)
                assert torch.equal(got[0], exp), (overlap, h, w, do)
        assert _same_bits(dev, _t(win).to(DEV))


def test_blend_u8_wrapper():
    T, frames, overlap, H, W = 8, 3, 1, 8, 8
    win = cm.case_windows_u8(T, frames, overlap, H, W)
    dev = _t(win).to(DEV)
    for window in ("uniform", "ramp", "hann"):
        want = postprocess_u8(clips.clip_blend(dev, B, T, frames, overlap, window=window), 7, 5, 1, None)
        got = clips.clip_blend_u8(dev, B, T, 7, 5, frames, overlap, window=window)
        assert got.dtype == torch.uint8 and got.shape == (B, T, 7, 5) and torch.equal(got, want.permute(0, 3, 1, 2))
    out = torch.empty((B, T, 8, 8), device=DEV, dtype=torch.uint8)
    assert clips.clip_blend_u8(dev, B, T, 8, 8, frames, overlap, out=out) is out
    assert torch.equal(out.cpu(), _t(cm.blend_u8(win, B, T, 8, 8, frames, overlap)))
    with pytest.raises(RuntimeError, match="h <= H"):
        clips.clip_blend_u8(dev, B, T, 9, 8, frames, overlap)
    with pytest.raises(RuntimeError, match="out must be"):
        clips.clip_blend_u8(dev, B, T, 8, 8, frames, overlap, out=torch.empty((B, T, 8, 8), device=DEV))


# ------------------------------------------------------------------ 4. KDLAE_student.forward_clip
MODELS = {"three": (dict(hidden_channels=[16, 32, 64]), (2, 9, 8, 8), 3, (0, 1, 2)),
          "two_residual": (dict(hidden_channels=[8, 16], residual=True), (1, 6, 4, 6), 4, (1, 3))}
WINDOWS = ("uniform", "ramp", "hann", "custom")


@functools.lru_cache(maxsize=None)
def _model(name):
    m = KDLAE_student(**MODELS[name][0])
    load_hash_weights(m)
    return m.to(DEV).eval()


def _window_outputs(m, x, frames, overlap):
    """What a user has without the feature: every window through forward alone, at batch 1 -> numpy
    [B n, f, H, W] in flat-index order."""
    f, ss = cm.starts(x.shape[1], frames, overlap)
    with torch.no_grad():
        return torch.cat([m(x[b:b + 1, s:s + f].contiguous()).cpu() for b in range(x.shape[0]) for s in ss]).numpy()


@functools.lru_cache(maxsize=None)
def _case(name, overlap):
    """(model, clip, per-window outputs), computed once and shared; nothing below writes to them."""
    m = _model(name)
    _, shape, frames, _ = MODELS[name]
    x = _t(hash_images(f"clip:m:{name}", shape)).to(DEV)
    return m, x, _window_outputs(m, x, frames, overlap)


def _table(window, T, frames, overlap):
    """-> (the value a caller passes as ``window``, the model's fp32 table or None)."""
    f, ss = cm.starts(T, frames, overlap)
    if window == "uniform":
        return "uniform", None
    if window == "custom":
        wt = cm.random_table(f, 7)
        return _t(wt), wt
    wt = cm.ramp_table(f, len(ss), overlap) if window == "ramp" else \
        clips.clip_window("hann", T, frames, overlap, "cpu").wt.numpy()
    return window, wt.astype(np.float32)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_forward_clip_equals_the_per_window_loop(name, window):
    _, shape, frames, ovs = MODELS[name]
    Bc, T = shape[:2]
    for overlap in ovs:
        m, x, outs = _case(name, overlap)
        arg, wt = _table(window, T, frames, overlap)
        if wt is None:   # the loop's own sum: E.add_, W.add_(1), E.div_(W)
            want = cm.host_loop(_t(outs), Bc, T, frames, overlap)
        else:
            want = _t(cm.blend(outs, Bc, T, frames, overlap, wt))
        n = outs.shape[0]
        for window_batch in (1, 3, n, n + 5):
            for _ in range(2):
                got = m.forward_clip(x, frames, overlap, window_batch, window=arg)
                assert got.shape == x.shape and _same_bits(got.cpu(), want), (overlap, window_batch)
    if window != "uniform":   # the window is read
        assert not torch.equal(m.forward_clip(x, frames, ovs[-1], 8).cpu(), want)


@pytest.mark.parametrize("name", sorted(MODELS))
def test_forward_clip_of_one_window_equals_forward(name):
    m = _model(name)
    Bc, _, H, W = MODELS[name][1]
    for T, frames, overlap in ((7, 7, 2), (5, 7, 2), (3, 3, 0), (2, 9, 1), (1, 7, 0)):
        x = _t(hash_images(f"clip:one:{name}:{T}", (Bc, T, H, W))).to(DEV)
        with torch.no_grad():
            ref = m(x)
        for window in ("uniform", "ramp", "hann", _t(cm.random_table(T, 3))):
            for window_batch in (1, 8):
                assert _same_bits(m.forward_clip(x, frames, overlap, window_batch, window), ref), (T, frames)


def test_forward_clip_defaults_and_train_mode():
    """frames 7, overlap 2, window_batch 8, uniform; no autograd graph in either mode, and the input is not written."""
    m = _model("three")
    x = _t(hash_images("clip:default", (1, 17, 8, 8))).to(DEV)
    x0 = x.clone()
    outs = _window_outputs(m, x, 7, 2)
    want = cm.host_loop(_t(outs), 1, 17, 7, 2)
    got = m.forward_clip(x)
    assert _same_bits(got.cpu(), want) and not got.requires_grad and got.grad_fn is None
    assert torch.equal(x, x0)
    assert _same_bits(m.forward_clip(x, window=None), got)


# ------------------------------------------------------------------ 5. pipeline.enhance_clip_u8
UH, UW = 20, 27   # reflect-padded to 32 x 32


@pytest.mark.parametrize("window", ["uniform", "ramp"])
@pytest.mark.parametrize("channels", [0, 3])
def test_enhance_clip_u8_equals_the_notebook_loop(channels, window):
    m = _model("three")
    Bc, T, frames, overlap = 2, 9, 3, 1
    shape = (Bc, T, UH, UW) + ((channels,) if channels else ())
    clip = torch.randint(0, 256, shape, dtype=torch.uint8, generator=torch.Generator().manual_seed(11)).to(DEV)
    clip[0, 0, :4, :4] = 0
    # the loop: preprocess, every window at batch 1, the host sum and divide, postprocess, permute
    x = frames_preprocess_u8(clip, 32)
    assert x.shape == (Bc, T, 32, 32)
    outs = _window_outputs(m, x, frames, overlap)
    arg, wt = _table(window, T, frames, overlap)
    blended = cm.host_loop(_t(outs), Bc, T, frames, overlap) if wt is None else \
        _t(cm.blend(outs, Bc, T, frames, overlap, wt))
    want = postprocess_u8(blended.to(DEV), UH, UW, 1, None).permute(0, 3, 1, 2)
    for window_batch in (8, 1, 5):
        got = enhance_clip_u8(m, clip, frames, overlap, window_batch, window=arg)
        assert got.dtype == torch.uint8 and got.shape == (Bc, T, UH, UW) and got.is_contiguous()
        assert torch.equal(got, want), window_batch
    assert torch.equal(got.cpu(), _t(cm.blend_u8(outs, Bc, T, UH, UW, frames, overlap, wt)))


def test_enhance_clip_u8_of_one_window_equals_enhance_frames_u8():
    from rethink_acoustic_image_enhancement_amd.pipeline import enhance_frames_u8
    m = _model("three")
    clip = torch.randint(0, 256, (2, 5, UH, UW), dtype=torch.uint8, generator=torch.Generator().manual_seed(12)).to(DEV)
    assert torch.equal(enhance_clip_u8(m, clip), enhance_frames_u8(m, clip).permute(0, 3, 1, 2))


# ------------------------------------------------------------------ 6. argument errors of the two Python entries
def test_forward_clip_argument_errors():
    m = _model("three")
    x = torch.zeros(1, 9, 8, 8, device=DEV)
    for call, text in ((lambda: m.forward_clip(x[0]), "expected x"),
                       (lambda: m.forward_clip(torch.zeros(1, 9, 8, 6, device=DEV)), "divisible by 4"),
                       (lambda: m.forward_clip(x.cpu()), "no CPU fallback"),
                       (lambda: m.forward_clip(x, window_batch=0), "window_batch"),
                       (lambda: m.forward_clip(x, frames=3, overlap=3), "EINVAL_SHAPE"),
                       (lambda: m.forward_clip(x, frames=3, overlap=-1), "EINVAL_SHAPE"),
                       (lambda: m.forward_clip(x, frames=0), "EINVAL_CONFIG"),
                       (lambda: m.forward_clip(x[:, :2], frames=7, overlap=2), "EINVAL_SHAPE"),
                       (lambda: m.forward_clip(x, window="triangle"), "must be one of"),
                       (lambda: m.forward_clip(x, window=torch.ones(6)), "window's length 7"),
                       (lambda: m.forward_clip(x, window=torch.zeros(7)), "greater than 0")):
        with pytest.raises(RuntimeError, match=text):
            call()


def test_enhance_clip_u8_argument_errors():
    m = _model("three")
    clip = torch.zeros(1, 9, UH, UW, dtype=torch.uint8, device=DEV)
    for call, text in ((lambda: enhance_clip_u8(m, clip[0]), "cuda uint8"),
                       (lambda: enhance_clip_u8(m, clip.float()), "cuda uint8"),
                       (lambda: enhance_clip_u8(m, clip.cpu()), "cuda uint8"),
                       (lambda: enhance_clip_u8(m, clip, window_batch=0), "window_batch"),
                       (lambda: enhance_clip_u8(m, clip, frames=3, overlap=3), "EINVAL_SHAPE"),
                       (lambda: enhance_clip_u8(m, clip, frames=-1), "EINVAL_CONFIG"),
                       (lambda: enhance_clip_u8(m, clip, window="box"), "must be one of"),
                       (lambda: enhance_clip_u8(m, clip, multiple=1), "divisible by 4"),
                       (lambda: enhance_clip_u8(m, clip[:, :, :, :, None].expand(-1, -1, -1, -1, 2)), "channels")):
        with pytest.raises(RuntimeError, match=text):
            call()

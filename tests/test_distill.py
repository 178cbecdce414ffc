"""Distillation labels without a GPU: the numpy model (tests/distill_model.py) proved against torch on the CPU, the
chunk schedule, the item order and the rate forms of ``distill.py``, every refusal of the three C entries through
ctypes (no card: the pointers are never dereferenced), and the model's mutants shown to differ on the inputs that
tests/test_distill_gpu.py gives the kernels.  Every comparison is bit for bit."""
import ctypes
import inspect

import numpy as np
import pytest
import torch
import torch.nn.functional as Fn

from rethink_acoustic_image_enhancement_amd import _lib, distill
from tests import distill_model as dm


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32) if a.dtype == np.float32 else a


def _same(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(_bits(a), _bits(b))


def _torch_gray(bgr):   # integer torch ops, [..., 3+] as B, G, R
    v = torch.from_numpy(np.ascontiguousarray(bgr)).to(torch.int64)
    return ((1868 * v[..., 0] + 9617 * v[..., 1] + 4899 * v[..., 2] + 8192) >> 14).to(torch.uint8)


# ------------------------------------------------------------------ 1. the model against torch
@pytest.mark.parametrize("C", dm.CHANNELS)
@pytest.mark.parametrize("hw", dm.SIZES)
def test_expand_u8_model_is_reflect_pad_of_the_replicated_frame(hw, C):
    h, w = hw
    B, F = 2, 3
    frames = dm.case_frames_u8(B, F, h, w, C)
    rate = dm.case_rate(B, F)
    H, W = dm.padded_size(h, w, 8)
    for j0, n in dm.case_chunks(B, F):
        img, rmap = dm.expand_u8(frames, rate, j0, n)
        assert img.shape == (n, 3, H, W) and img.dtype == np.float32 and rmap.shape == (n, 1, H, W)
        for q in range(n):
            b, f = divmod(j0 + q, F)
            y = torch.from_numpy(frames[b, f].copy()) if C == 1 else _torch_gray(frames[b, f])
            rep = y[:, :, None].expand(h, w, 3)                            # the frame a user hands to enhance_u8
            x = rep.permute(2, 0, 1).to(torch.float32) / 255.0             # preprocess_u8's rule on the CPU
            ref = Fn.pad(x[None], (0, W - w, 0, H - h), mode="reflect")[0] if (H, W) != (h, w) else x
            assert _same(img[q], ref.numpy()), (j0, q)
            assert _same(rmap[q], np.full((1, H, W), rate[j0 + q], np.float32))
    assert dm.expand_u8(frames, None, 0, 1)[1] is None


def test_expand_f32_model_is_a_bit_copy():
    B, F, H, W = 2, 3, 8, 16
    x = dm.case_frames_f32(B, F, H, W)
    rate = dm.case_rate(B, F)
    img, rmap = dm.expand_f32(x, rate, 1, 4)
    for q in range(4):
        for c in range(3):
            assert _same(img[q, c], x.reshape(B * F, H, W)[1 + q])
        assert _same(rmap[q], np.full((1, H, W), rate[1 + q], np.float32))


def test_quantiser_is_torch_clamp_and_round_with_ties_to_even():
    halves = dm.exact_halves()
    assert halves.size >= 32   # x 255 = k + 1/2 exactly: where rintf and torch.round must both go to the even byte
    x = np.concatenate([halves, dm.case_hq(2, 16, 16).reshape(-1)])
    ref = torch.round(torch.clamp(torch.from_numpy(x), 0.0, 1.0) * 255.0).to(torch.uint8).numpy()
    assert _same(dm.quantise(x), ref)
    k = np.round(halves.astype(np.float64) * 255 - 0.5).astype(np.int64)
    assert np.array_equal(dm.quantise(halves), (k + (k % 2)).astype(np.uint8))


@pytest.mark.parametrize("C", [0] + dm.CHANNELS)
@pytest.mark.parametrize("hw", dm.SIZES)
def test_collapse_model_against_torch(hw, C):
    """file: torch.clamp / torch.round per channel, the black mask postprocess_u8 applies when its lq is the
    replicated gray frame, the gray rule in integer torch ops, / 255.  mean: ((c0 + c1) + c2) / 3 in CPU fp32."""
    h, w = hw
    B, F = 1, 7
    Hp, Wp = dm.padded_size(h, w, 8)
    src = dm.case_frames_u8(B, F, h, w, C) if C else None
    for j0, n in dm.case_chunks(B, F):
        hq = dm.case_hq(n, Hp, Wp)
        t = torch.from_numpy(hq)[..., :h, :w]
        v = torch.round(torch.clamp(t, 0.0, 1.0) * 255.0).to(torch.uint8)            # [n, 3, h, w] as R, G, B
        if src is not None:
            items = src.reshape((B * F,) + src.shape[2:])[j0:j0 + n]
            y = torch.from_numpy(items.copy()) if C == 1 else _torch_gray(items)
            v = torch.where((y == 0)[:, None], torch.zeros_like(v), v)
        g = _torch_gray(v.permute(0, 2, 3, 1).numpy()[..., ::-1])                    # R, G, B -> B, G, R
        for dtype, ref in ((np.uint8, g.numpy()), (np.float32, (g.to(torch.float32) / 255.0).numpy())):
            dst = np.full((B, F, h, w), 0xA5 if dtype == np.uint8 else 1e30, dtype)
            out = dm.collapse(dst, hq, j0, n, dm.FILE, src)
            flat = out.reshape(B * F, h, w)
            assert _same(flat[j0:j0 + n], ref)
            assert _same(np.delete(flat, np.s_[j0:j0 + n], 0), np.delete(dst.reshape(B * F, h, w), np.s_[j0:j0 + n], 0))
        mean = ((t[:, 0] + t[:, 1]) + t[:, 2]) / 3.0
        out = dm.collapse(np.zeros((B, F, h, w), np.float32), hq, j0, n, dm.MEAN, src)
        assert _same(out.reshape(B * F, h, w)[j0:j0 + n], mean.numpy())


# ------------------------------------------------------------------ 2. schedule, item order, rate forms
@pytest.mark.parametrize("total,tb", [(10, 1), (10, 4), (10, 16), (10, 10), (7, 3), (1, 1)])
def test_chunk_schedule(total, tb):
    plan = distill.chunks(total, tb)
    assert plan == dm.chunks(total, tb)
    assert [j for j0, n in plan for j in range(j0, j0 + n)] == list(range(total))
    assert all(n == tb for _, n in plan[:-1]) and 1 <= plan[-1][1] <= tb
    with pytest.raises(RuntimeError):
        distill.chunks(total, 0)


def test_item_order_and_rate_forms():
    B, F = 2, 5
    per_item = np.arange(B * F, dtype=np.float32).reshape(B, F) / 16
    for form, want in ((0.4, np.full(B * F, 0.4, np.float32)),
                       (np.array([0.25, 0.75], np.float32), np.repeat(np.array([0.25, 0.75], np.float32), F)),
                       (per_item, per_item.reshape(-1))):
        got = distill.item_rates(torch.as_tensor(form), B, F, "cpu")
        assert got.dtype == torch.float32 and got.is_contiguous()
        assert _same(got.numpy(), want) and _same(dm.item_rates(form, B, F), want)
    for b in range(B):
        for f in range(F):
            assert distill.item_rates(per_item, B, F, "cpu")[b * F + f] == per_item[b, f]   # j = b F + f
    for bad in (np.zeros(3, np.float32), np.zeros((F, B), np.float32), np.zeros((B, F, 1), np.float32)):
        with pytest.raises(RuntimeError):
            distill.item_rates(bad, B, F, "cpu")


def test_public_signatures():
    sig = inspect.signature(distill.teacher_labels)
    assert list(sig.parameters) == ["teacher", "frames", "denoise_rate", "mode", "teacher_batch", "tile",
                                    "tile_overlap", "window", "out"]
    d = {k: v.default for k, v in sig.parameters.items()}
    assert (d["mode"], d["teacher_batch"], d["tile"], d["tile_overlap"], d["window"], d["out"]) == \
        ("file", 16, None, 32, "uniform", None)
    from rethink_acoustic_image_enhancement_amd import pipeline, train
    assert callable(pipeline.distill_clip_u8) and issubclass(train.DistillTrainer, train.KDLAESTrainer)
    sig = inspect.signature(train.DistillTrainer.__init__)
    assert list(sig.parameters)[:6] == ["self", "student", "teacher", "denoise_rate", "label_mode", "teacher_batch"]
    assert sig.parameters["label_mode"].default == "mean" and sig.parameters["teacher_batch"].default == 16


def test_python_refusals_come_before_any_launch():
    """A CPU tensor, a wrong dtype and a teacher in train mode: RuntimeError with no card in the machine."""
    from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
    t = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree").eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        distill.teacher_labels(t, torch.zeros((1, 2, 8, 8), dtype=torch.uint8), 0.5)
    with pytest.raises(RuntimeError, match="uint8"):
        distill.teacher_labels_u8(t, torch.zeros((1, 2, 8, 8)), 0.5)
    with pytest.raises(RuntimeError):
        distill.teacher_labels(t, torch.zeros((1, 2, 8, 8), dtype=torch.uint8), 0.5, mode="median")
    with pytest.raises(RuntimeError):
        distill.teacher_labels(object(), torch.zeros((1, 2, 8, 8), dtype=torch.uint8), 0.5)


# ------------------------------------------------------------------ 3. the C entries' refusals
P = 0x1000   # a non-null, 16-byte aligned "device pointer"
SHAPE, CONFIG = 1, 2


def _eu8(frames=P, B=2, F=3, h=9, w=13, C=1, mult=8, rate=P, j0=0, n=6, img=P, rmap=P):
    return _lib.lib().kdlae_distill_expand_u8(frames, B, F, h, w, C, mult, rate, j0, n, img, rmap, None)


def _ef32(frames=P, B=2, F=3, H=8, W=16, rate=P, j0=0, n=6, img=P, rmap=P):
    return _lib.lib().kdlae_distill_expand_f32(frames, B, F, H, W, rate, j0, n, img, rmap, None)


def _col(hq=P, B=2, F=3, Hp=16, Wp=16, h=9, w=13, j0=0, n=6, mode=0, src=P, C=1, dst=P, u8=0):
    return _lib.lib().kdlae_distill_collapse(hq, B, F, Hp, Wp, h, w, j0, n, mode, src, C, dst, u8, None)


def test_entries_refuse_bad_arguments_before_any_launch():
    for call in (_eu8, _ef32, _col):
        assert call(n=0) == CONFIG and call(n=-1) == CONFIG and call(j0=-1, n=1) == CONFIG
        assert call(j0=5, n=2) == CONFIG and "passes the last frame" in _lib.last_error()
        assert call(j0=6, n=1) == CONFIG and call(B=0) == CONFIG and call(F=0) == CONFIG
        assert call(B=65536, F=65536, n=1) == SHAPE                         # B F past 2^31 - 1
    # null required pointers; the rate pair comes together or not at all
    assert _eu8(frames=None) == CONFIG and _eu8(img=None) == CONFIG
    assert _eu8(rate=None) == CONFIG and _eu8(rmap=None) == CONFIG
    assert _ef32(frames=None) == CONFIG and _ef32(img=None) == CONFIG
    assert _ef32(rate=None) == CONFIG and _ef32(rmap=None) == CONFIG
    assert _col(hq=None) == CONFIG and _col(dst=None) == CONFIG
    # channels
    for C in (0, 2, 5, -1):
        assert _eu8(C=C) == CONFIG and _col(C=C) == CONFIG, C
    # a frame smaller than its reflect padding: 4 rows pad to 8, 3 columns pad to 8
    assert _eu8(h=4) == SHAPE and "reflect" in _lib.last_error() and _eu8(w=3) == SHAPE
    assert _eu8(h=0) == CONFIG and _eu8(mult=0) == CONFIG
    # fp32 frames are network inputs
    assert _ef32(H=12) == SHAPE and _ef32(W=20) == SHAPE and "multiples of 8" in _lib.last_error()
    assert _ef32(H=0) == CONFIG
    # mode
    assert _col(mode=1, u8=1) == CONFIG and "mean" in _lib.last_error()
    assert _col(mode=2) == CONFIG and _col(mode=-1) == CONFIG
    # the crop must fit
    assert _col(h=17) == SHAPE and _col(w=17) == SHAPE and _col(h=0) == CONFIG
    # element counts the kernels keep in 32 bits: the pixels of one frame
    assert _eu8(B=1, F=1, h=65536, w=65536, n=1) == SHAPE and "2^31" in _lib.last_error()
    assert _ef32(B=1, F=1, H=65536, W=65536, n=1) == SHAPE
    assert _col(B=1, F=1, Hp=65536, Wp=65536, h=8, w=8, n=1) == SHAPE
    assert _col(B=1, F=1, Hp=65536, Wp=65536, h=65536, w=65536, n=1) == SHAPE
    assert _eu8(B=1, F=1, h=2 ** 31 - 4, w=16, mult=8, n=1) == SHAPE      # the padded size itself
    # fp32 pointers off 4 bytes
    assert _eu8(img=P + 2) == SHAPE and _eu8(rmap=P + 1) == SHAPE and _ef32(frames=P + 2) == SHAPE
    assert _col(hq=P + 2) == SHAPE and _col(dst=P + 2) == SHAPE


# ------------------------------------------------------------------ 4. every mutant shows on the GPU test's inputs
def _expand_u8_cases(mutant=None):
    out = []
    for B, F in dm.STACKS:
        for h, w in dm.SIZES:
            for C in dm.CHANNELS:
                fr, rate = dm.case_frames_u8(B, F, h, w, C), dm.case_rate(B, F)
                for j0, n in dm.case_chunks(B, F):
                    out.extend(dm.expand_u8(fr, rate, j0, n, mutant=mutant))
    return out


def _expand_f32_cases(mutant=None):
    out = []
    for B, F in dm.STACKS:
        for H, W in dm.F32_SIZES:
            fr, rate = dm.case_frames_f32(B, F, H, W), dm.case_rate(B, F)
            for j0, n in dm.case_chunks(B, F):
                out.extend(dm.expand_f32(fr, rate, j0, n, mutant=mutant))
    return out


def _collapse_cases(mode, mutant=None):
    out = []
    for B, F in dm.STACKS:
        for h, w in dm.SIZES:
            Hp, Wp = dm.padded_size(h, w, 8)
            for C in [0] + dm.CHANNELS:
                src = dm.case_frames_u8(B, F, h, w, C) if C and mode == dm.FILE else None
                for j0, n in dm.case_chunks(B, F):
                    hq = dm.case_hq(n, Hp, Wp)
                    for dtype in (np.float32, np.uint8) if mode == dm.FILE else (np.float32,):
                        dst = np.full((B, F, h, w), 0xA5 if dtype == np.uint8 else 1e30, dtype)
                        out.append(dm.collapse(dst, hq, j0, n, mode, src, mutant))
    return out


def _differs(a, b):
    assert len(a) == len(b)
    return sum(not _same(x, y) for x, y in zip(a, b))


SHOWS_IN = {   # mutant -> the entries whose compared bits it must change
    "swap_rb": ("expand_u8", "file"), "no_round_bias": ("expand_u8", "file"), "gray_first": ("file",),
    "no_mask": ("file",), "mask_per_channel": ("file",), "sum_right": ("mean",), "mul_third": ("mean",),
    "edge_pad": ("expand_u8",), "ignore_j0": ("expand_u8", "expand_f32", "file", "mean"),
    "rate_item0": ("expand_u8", "expand_f32"), "crop_bottom_right": ("file", "mean"),
}
_CASES = {"expand_u8": _expand_u8_cases, "expand_f32": _expand_f32_cases,
          "file": lambda mutant=None: _collapse_cases(dm.FILE, mutant),
          "mean": lambda mutant=None: _collapse_cases(dm.MEAN, mutant)}


@pytest.fixture(scope="module")
def model_outputs():
    return {k: f() for k, f in _CASES.items()}


def test_every_mutant_is_listed():
    assert set(SHOWS_IN) == set(dm.MUTANTS)


@pytest.mark.parametrize("mutant", dm.MUTANTS)
def test_mutant_changes_a_compared_bit(mutant, model_outputs):
    for entry in SHOWS_IN[mutant]:
        assert _differs(model_outputs[entry], _CASES[entry](mutant)) > 0, (mutant, entry)


def test_inputs_hold_the_values_the_mutants_need():
    hq = dm.case_hq(2, 8, 8)
    first = hq[0, :, :8, :8].reshape(3, -1)
    assert (first == 0).any() and (first == 1).any() and np.signbit(first[first == 0]).any()
    assert ((first > 1) & (first < 1.001)).any() and ((first < 0) & (first > -1e-20)).any()
    q = dm.quantise(first).astype(np.int64)
    assert ((q[1] - q[0] == 1) & (q[2] == q[0])).any()                   # channels one byte apart
    assert np.isin(first, dm.exact_halves()).any()                        # x 255 = k + 1/2
    assert hq.min() < 0 and hq.max() > 1
    fr = dm.case_frames_u8(2, 3, 9, 13, 3)
    y = dm.gray_frames(fr)
    assert ((y == 0) & (fr.max(-1) > 0)).any() and ((y == 0) & (fr.max(-1) == 0)).any()
    assert ((y > 0) & (fr.min(-1) == 0)).any()                             # a black channel in a pixel that is not
    rate = dm.case_rate(2, 3)
    assert len(set(rate.tolist())) == rate.size

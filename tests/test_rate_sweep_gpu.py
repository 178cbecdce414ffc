"""Rate sweep on the GPU: KDLAE_teacher.forward_rates / forward_sr (kdlae_t_forward_rates, kdlae_t_forward_sr),
kdlae_rate_select and pipeline.enhance_rates_u8 / enhance_auto_u8.

Batch invariance is a bit-exact property of this library (test_kdlae_gpu.test_batch_invariance_and_determinism),
and the sweep only re-batches the forward's own launches behind a copy, so every sweep output is compared with
torch.equal: no tolerance anywhere in this file."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from rethink_acoustic_image_enhancement_amd.pipeline import (asdqe_scores, enhance_auto_u8, enhance_rates_u8,
                                                             enhance_u8, postprocess_u8, preprocess_u8, rate_select)
from tests.rate_select_model import MODES, select_cases, select_model

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30

KW = dict(dim=48, LayerNorm_type="BiasFree", num_blocks=[2, 1, 1, 1], num_refinement_blocks=1)
MODELS = {"biasfree": KW,
          "withbias": {**KW, "LayerNorm_type": "WithBias", "bias": True},
          "gray": {**KW, "inp_channels": 1, "out_channels": 1}}
H, W = 128, 96


@functools.lru_cache(maxsize=None)
def _model(name, **extra):
    m = KDLAE_teacher(**{**MODELS[name], **extra})
    load_hash_weights(m)
    m.hip_graphs = False   # the sweep is eager; compare with the eager forward
    return m.to(DEV).eval()


def _img(key, m, B, h=H, w=W):
    return torch.from_numpy(hash_images(key, (B, m._cfg["inp_channels"], h, w))).to(DEV)


def _forward(m, img, rate_map):
    with torch.no_grad():
        out = m({"img": img, "denoise_rate": rate_map})
    return out


def _sweep(m, img, rates, sr=True):
    with torch.no_grad():
        return m.forward_rates(img, rates, sr=sr)


def _as_maps(rates, B, h, w):
    """R scalars / [R,B] / maps -> [R,B,1,h,w] maps, the form forward takes."""
    rt = torch.as_tensor(rates, dtype=torch.float32).to(DEV)
    if rt.dim() == 1:
        rt = rt[:, None].expand(-1, B)
    if rt.dim() == 2:
        rt = rt[:, :, None, None, None].expand(-1, -1, 1, h, w)
    return rt.contiguous()


def _assert_sweep_equals_forwards(m, img, rates):
    B, _, h, w = img.shape
    maps = _as_maps(rates, B, h, w)
    out = _sweep(m, img, rates)
    again = _sweep(m, img, rates)
    assert torch.equal(out["hq"], again["hq"]) and torch.equal(out["sr"], again["sr"])
    oc = m._cfg["out_channels"]
    assert out["hq"].shape == (maps.shape[0], B, oc, h, w) and out["sr"].shape == (maps.shape[0], B, oc, 2 * h, 2 * w)
    for r in range(maps.shape[0]):
        ref = _forward(m, img, maps[r])
        assert torch.equal(out["hq"][r], ref["hq"]), f"hq of rate {r}"
        assert torch.equal(out["sr"][r], ref["sr"]), f"sr of rate {r}"
    return out


@pytest.mark.parametrize("kind", ["scalar", "per_image", "map"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_equals_single_forwards(name, kind):
    m = _model(name)
    B, R = 2, 3
    img = _img(f"rs:{name}", m, B)
    if kind == "scalar":
        rates = [0.15, 0.6, 0.9]
    elif kind == "per_image":
        rates = torch.tensor([[0.15, 0.3], [0.6, 0.7], [0.9, 0.05]])
    else:
        rates = torch.from_numpy(hash_images(f"rsm:{name}", (R, B, 1, H, W)))
    out = _assert_sweep_equals_forwards(m, img, rates)
    assert not torch.equal(out["hq"][0], out["hq"][1])   # the rates do reach the output


def test_one_rate_equals_forward_and_one_image_five_rates():
    m = _model("biasfree")
    _assert_sweep_equals_forwards(m, _img("rs:r1", m, 3), torch.tensor([0.4]))
    _assert_sweep_equals_forwards(m, _img("rs:b1", m, 1), np.linspace(0.0, 1.0, 5).tolist())


def test_without_sr_and_the_sr_head_alone():
    m = _model("withbias")
    img = _img("rs:nosr", m, 2)
    rates = [0.2, 0.8]
    full = _sweep(m, img, rates, sr=True)
    lean = _sweep(m, img, rates, sr=False)
    assert lean["sr"] is None and torch.equal(lean["hq"], full["hq"])
    maps = _as_maps(rates, 2, H, W)
    for r in range(2):
        ref = _forward(m, img, maps[r])
        with torch.no_grad():
            assert torch.equal(m.forward_sr(lean["hq"][r]), ref["sr"])
    # a model without the sr head sweeps hq alone
    m2 = _model("biasfree", static="no")
    out = _sweep(m2, img, rates, sr=False)
    assert out["sr"] is None and torch.equal(out["hq"][1], _forward(m2, img, maps[1])["hq"])


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def test_no_overrun_at_64_rates_and_short_workspace_refused():
    """24 x 16 (the smallest legal H, W with W != H), R = 64, B = 2 through the C ABI: hq, sr and the workspace
    are slices of one 1e30-filled allocation; the floats around them keep their bits."""
    m = _model("biasfree")
    L = _lib.lib()
    B, R, h, w, G = 2, 64, 24, 16, 4096
    img = _img("rs:over", m, B, h, w)
    rates = torch.linspace(0.0, 1.0, R * B, device=DEV).view(R, B).contiguous()
    eng = m.engine(torch.device(DEV))
    stream = torch.cuda.current_stream().cuda_stream
    eng.sync_params(m, stream)
    nbytes = L.kdlae_t_rates_workspace_bytes(eng.handle, B, R, h, w, 1)
    assert nbytes > 0 and nbytes % 256 == 0
    n_hq, n_sr, n_ws = R * B * 3 * h * w, R * B * 3 * 4 * h * w, nbytes // 4
    store = torch.full((G + n_hq + G + n_sr + G + n_ws + G,), BIG, device=DEV)
    o_hq, o_sr, o_ws = G, 2 * G + n_hq, 3 * G + n_hq + n_sr
    hq, sr, ws = store[o_hq:o_hq + n_hq], store[o_sr:o_sr + n_sr], store[o_ws:o_ws + n_ws]
    assert ws.data_ptr() % 256 == 0

    def call(ws_bytes):
        return L.kdlae_t_forward_rates(eng.handle, _c(img), _c(rates), 0, B, R, h, w, _c(hq), _c(sr), _c(ws), ws_bytes,
                                       ctypes.c_void_p(stream))
    assert call(nbytes - 1) == 6 and "workspace too small" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((store == BIG).all()), "a refused call launched something"
    assert call(nbytes) == 0, _lib.last_error()
    torch.cuda.synchronize()
    for lo, hi in ((0, o_hq), (o_hq + n_hq, o_sr), (o_sr + n_sr, o_ws), (o_ws + n_ws, store.numel())):
        assert bool((store[lo:hi] == BIG).all()), f"guard [{lo}, {hi}) was written"
    out = _sweep(m, img, rates)
    assert torch.equal(hq.view(R, B, 3, h, w), out["hq"]) and torch.equal(sr.view(R, B, 3, 2 * h, 2 * w), out["sr"])
    maps = _as_maps(rates, B, h, w)
    for r in (0, 37, 63):
        ref = _forward(m, img, maps[r])
        assert torch.equal(out["hq"][r], ref["hq"]) and torch.equal(out["sr"][r], ref["sr"])


def test_workspace_sizes():
    """Sized on a committed handle (the plan needs the packed blocks): one rate with the sr head needs at least
    the forward's workspace, more rates never need less, and dropping the sr head never needs more."""
    m = _model("biasfree")
    L = _lib.lib()
    eng = m.engine(torch.device(DEV))
    eng.sync_params(m, torch.cuda.current_stream().cuda_stream)
    for B, h, w in ((1, 24, 16), (2, 128, 96), (16, 512, 512)):
        base = L.kdlae_t_workspace_bytes(eng.handle, B, h, w)
        sizes = [L.kdlae_t_rates_workspace_bytes(eng.handle, B, R, h, w, 1) for R in (1, 2, 3, 8, 64)]
        lean = [L.kdlae_t_rates_workspace_bytes(eng.handle, B, R, h, w, 0) for R in (1, 2, 3, 8, 64)]
        assert base > 0 and sizes[0] >= base
        assert sizes == sorted(sizes) and lean == sorted(lean) and sizes[-1] > sizes[0]
        assert all(0 < a <= b for a, b in zip(lean, sizes))
        assert 0 < L.kdlae_t_sr_workspace_bytes(eng.handle, B, h, w) <= base


def test_refusals():
    m = _model("biasfree")
    img = _img("rs:ref", m, 1, 32, 32)
    L = _lib.lib()
    eng = m.engine(torch.device(DEV))
    eng.sync_params(m, torch.cuda.current_stream().cuda_stream)
    buf = torch.zeros(1 << 16, device=DEV)

    def c_abi(handle, R=2, h=32, w=32, sr=buf):
        return L.kdlae_t_forward_rates(handle, _c(img), _c(buf), 0, 1, R, h, w, _c(buf), _c(sr), _c(buf), 0, None)
    for R in (0, 65):
        assert c_abi(eng.handle, R=R) == 1 and "1 <= R <= 64" in _lib.last_error()
        with pytest.raises(RuntimeError, match="1..64 rates"):
            _sweep(m, img, [0.5] * R)
    assert c_abi(eng.handle, h=36) == 1 and "H % 8" in _lib.last_error()
    with pytest.raises(RuntimeError, match="divisible by 8"):
        _sweep(m, img[:, :, :28], [0.5])
    assert c_abi(eng.handle) == 6 and "workspace too small" in _lib.last_error()
    with pytest.raises(RuntimeError, match="rates must be"):
        _sweep(m, img, torch.zeros(2, 3))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        _sweep(m, img.cpu(), [0.5])
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            _sweep(m, img, [0.5])
        with pytest.raises(RuntimeError, match="eval"):
            m.forward_sr(img)
    finally:
        m.eval()
    plus = _model("biasfree", params="plus")
    e2 = plus.engine(torch.device(DEV))
    e2.sync_params(plus, torch.cuda.current_stream().cuda_stream)
    assert c_abi(e2.handle) == 2 and "params=='cat'" in _lib.last_error()
    with pytest.raises(RuntimeError, match="params='cat'"):
        _sweep(plus, img, [0.5])
    nosr = _model("biasfree", static="no")
    e3 = nosr.engine(torch.device(DEV))
    e3.sync_params(nosr, torch.cuda.current_stream().cuda_stream)
    assert c_abi(e3.handle) == 2 and "no sr head" in _lib.last_error()
    assert L.kdlae_t_forward_sr(e3.handle, _c(img), 1, 32, 32, _c(buf), _c(buf), 0, None) == 2
    with pytest.raises(RuntimeError, match="static='train'"):
        _sweep(nosr, img, [0.5], sr=True)
    with pytest.raises(RuntimeError, match="static='train'"):
        nosr.forward_sr(img)
    torch.cuda.synchronize()
    assert bool((buf == 0).all())   # nothing was launched on the refused calls' buffers


# (source offset, destination offset) in floats from a 16-byte boundary: equal offsets take the float4 body
# with a scalar head and tail, unequal ones the scalar copy
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (2, 0)]


@pytest.mark.parametrize("R,B", [(1, 1), (1, 5), (3, 1), (3, 5), (64, 1), (64, 5)])
def test_rate_select_equals_the_numpy_model(R, B):
    L = _lib.lib()
    G = 64
    rng = np.random.default_rng(R * 100 + B)
    for per_image in (1, 3, 4, 1021):
        n = R * B * per_image
        cand = rng.standard_normal(n).astype(np.float32)
        for so, do in OFFSETS:
            src = torch.full((G + so + n + G,), BIG, device=DEV)
            src[G + so:G + so + n] = torch.from_numpy(cand).to(DEV)
            src0 = src.clone()
            for name, scores, target in select_cases(R, B):
                sc, tg = torch.from_numpy(scores).to(DEV), torch.from_numpy(target).to(DEV)
                for mode in (0, 1, 2):
                    want = select_model(scores, mode, target)
                    res = []
                    for _ in range(2):
                        dst = torch.full((G + do + B * per_image + G,), BIG, device=DEV)
                        idx = torch.full((B + 2,), -7, device=DEV, dtype=torch.int32)
                        rc = L.kdlae_rate_select(_c(sc), R, B, mode, _c(tg), _c(src[G + so:]), per_image, _c(idx[1:]),
                                                 _c(dst[G + do:]), None)
                        assert rc == 0, _lib.last_error()
                        res.append((idx.cpu().numpy(), dst.cpu().numpy()))
                    (i0, d0), (i1, d1) = res
                    assert np.array_equal(i0, i1) and np.array_equal(d0.view(np.uint32), d1.view(np.uint32))
                    tag = (name, mode, per_image, so, do)
                    assert i0[0] == -7 and i0[-1] == -7 and np.array_equal(i0[1:-1], want), tag
                    exp = np.full(d0.shape, np.float32(BIG))
                    picked = cand.reshape(R, B, per_image)[want, np.arange(B)]
                    exp[G + do:G + do + B * per_image] = picked.reshape(-1)
                    assert np.array_equal(d0.view(np.uint32), exp.view(np.uint32)), tag
            assert torch.equal(src, src0)


def test_rate_select_wrapper():
    scores = torch.tensor([[0.1, 0.9], [0.5, 0.2], [0.5, float("nan")]], device=DEV)
    hq = torch.arange(3 * 2 * 4, device=DEV, dtype=torch.float32).view(3, 2, 2, 2)
    for select, target, want in (("closest", 0.45, [1, 1]), ("max", None, [1, 0]), ("min", None, [0, 1])):
        idx, out = rate_select(scores, hq, select, target)
        assert idx.tolist() == want and torch.equal(out, hq[want, [0, 1]])
    with pytest.raises(RuntimeError, match="needs a target"):
        rate_select(scores, hq, "closest")
    with pytest.raises(RuntimeError, match="select must be"):
        rate_select(scores, hq, "median")


def _u8(seed, B, h, w):
    rng = np.random.default_rng(seed)
    x = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    x[:, : h // 3, : w // 4] = 0   # an all-black region: masked in every candidate
    return torch.from_numpy(x).to(DEV)


@functools.lru_cache(maxsize=None)
def _scorer():
    s = DenoiseRatePredictor()
    load_hash_weights(s)
    return s.to(DEV).eval()


@pytest.mark.parametrize("select", ["closest", "max", "min"])
def test_enhance_auto_u8_end_to_end(select):
    """45 x 70 images: reflect-padded to 48 x 72 for the sweep and cropped back."""
    m, scorer = _model("biasfree"), _scorer()
    B, h, w = 2, 45, 70
    images = _u8(11, B, h, w)
    rates = [0.1, 0.5, 0.9]
    cands = enhance_rates_u8(m, images, rates)
    assert cands.shape == (3, B, h, w, 3) and cands.dtype == torch.uint8
    want_scores = np.stack([asdqe_scores(scorer, images, cands[r]) for r in range(3)])
    for r in (0, 2):
        assert torch.equal(cands[r], enhance_u8(m, images, rates[r])[0])
    target = float(np.float32(want_scores.mean())) if select == "closest" else None
    out = enhance_auto_u8(m, scorer, images, rates, target=target, select=select, want_sr=True)
    scores = out["scores"].cpu().numpy()
    assert scores.dtype == np.float32 and np.array_equal(scores.view(np.uint32), want_scores.view(np.uint32))
    tg = np.full(B, target, np.float32) if target is not None else None
    want_idx = select_model(scores, MODES[select], tg)
    assert out["index"].dtype == torch.int32 and np.array_equal(out["index"].cpu().numpy(), want_idx)
    assert out["rate"].cpu().tolist() == [np.float32(rates[i]) for i in want_idx]
    for b in range(B):
        assert torch.equal(out["hq"][b], cands[want_idx[b], b])
    # the sr head ran on the chosen float hq
    img, _ = preprocess_u8(images, None, 8, False)
    hq = _sweep(m, img, rates, sr=False)["hq"]
    chosen = hq[torch.from_numpy(want_idx).long().to(DEV), torch.arange(B, device=DEV)]
    with torch.no_grad():
        want_sr = postprocess_u8(m.forward_sr(chosen), h, w, 2, images)
    assert out["sr"].shape == (B, 2 * h, 2 * w, 3) and torch.equal(out["sr"], want_sr)
    lean = enhance_auto_u8(m, scorer, images, rates, target=target, select=select)
    assert lean["sr"] is None and torch.equal(lean["hq"], out["hq"]) and torch.equal(lean["index"], out["index"])

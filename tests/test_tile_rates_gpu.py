"""Tiled rate sweep on the GPU: kdlae_tile_blend_rates against kdlae_tile_blend and the CPU models
(tests/tile_model.py, tests/tile_rates_model.py), KDLAE_teacher.forward_rates_tiled against R calls of
forward_tiled, pipeline.enhance_rates_tiled_u8 / enhance_auto_tiled_u8 against enhance_tiled_u8.

The blend copies, adds in a fixed order and divides; the sweep only re-batches the forward's own launches, and
batch rows of the forward are bit for bit independent of the batch size
(test_kdlae_gpu.test_batch_invariance_and_determinism).  So every comparison here is on the bits: no tolerance
anywhere in this file."""
import ctypes
import functools
import gc

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, tiling
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher, Restormer
from rethink_acoustic_image_enhancement_amd.pipeline import (asdqe_scores, enhance_auto_tiled_u8,
                                                             enhance_rates_tiled_u8, enhance_tiled_u8)
from tests import tile_model as tm
from tests import tile_rates_model as trm
from tests.rate_select_model import MODES, select_model
from tests.test_rate_sweep_gpu import MODELS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
G = 64   # guard floats (256 bytes) either side of a buffer under test

SHAPES = [(40, 56), (16, 72), (24, 24)]
OVERLAPS = (0, 4, 5, 8)
# (staging offset, destination offset) in floats from a 16-byte boundary; (0, 0) with an aligned stride is the
# float4 path, everything else the scalar one
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (2, 0), (0, 3)]


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def _stored(values, off):
    """`values` (flat, on the device) inside BIG-filled storage at float offset `off` from a 16-byte boundary."""
    store = torch.full((G + off + values.numel() + G,), BIG, device=DEV)
    assert store.data_ptr() % 16 == 0
    store[G + off:G + off + values.numel()] = values
    return store


def _blend_rates_abi(view, R, B, C, H, W, tile, overlap, tile_batch, scale, do):
    """Two calls into BIG-filled storage at destination offset `do` -> the storage (equal bits asserted)."""
    n = R * B * C * scale * H * scale * W
    got = []
    for _ in range(2):
        dst = torch.full((G + do + n + G,), BIG, device=DEV)
        rc = _lib.lib().kdlae_tile_blend_rates(_c(view), R, B, C, H, W, tile, overlap, tile_batch, scale,
                                               _c(dst[G + do:]), None)
        assert rc == 0, _lib.last_error()
        got.append(dst)
    assert _same_bits(got[0], got[1])
    return got[0]


# ------------------------------------------------------------------ 1. the blend kernel alone
@pytest.mark.parametrize("tile", [16, 24])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_blend_rates_equals_blend_of_every_slice(C, hw, tile):
    B, (H, W) = 2, hw
    for R in (1, 3):
        for overlap in OVERLAPS:
            th, tw, ys, xs = tm.plan(H, W, tile, overlap)
            n = B * len(ys) * len(xs)
            for scale in (1, 2):
                x = torch.from_numpy(hash_images(f"tr:b:{R}:{C}:{H}x{W}:{tile}:{overlap}:{scale}",
                                                 (R, n, C, scale * th, scale * tw), -1.0, 1.0))
                want = torch.stack([tm.blend(x[r], B, H, W, tile, overlap, scale) for r in range(R)])
                x_dev = x.to(DEV)
                for r in range(R):   # the existing blend on the r-th slice, laid out [n][C][sth][stw]
                    assert _same_bits(tiling.tile_blend(x_dev[r], B, H, W, tile, overlap, scale), want[r].to(DEV))
                for tile_batch in (1, 5, n, n + 3):
                    staged = trm.to_staged(x, tile_batch).to(DEV)
                    for so, do in OFFSETS:
                        s_store = _stored(staged, so)
                        s0 = s_store.clone()
                        got = _blend_rates_abi(s_store[G + so:], R, B, C, H, W, tile, overlap, tile_batch, scale, do)
                        exp = torch.full((got.numel(),), BIG)
                        exp[G + do:G + do + want.numel()] = want.reshape(-1)
                        assert _same_bits(got, exp.to(DEV)), (R, overlap, scale, tile_batch, so, do)
                        assert _same_bits(s_store, s0)


@pytest.mark.parametrize("vec", [True, False])
def test_blend_rates_more_items_than_one_pass_of_the_grid(vec):
    """The launcher caps the grid at 4096 blocks of 256 threads and loops over the rest: more than 4096 * 256
    items (of 4 floats on the float4 path, of 1 float on the scalar path)."""
    gen = torch.Generator().manual_seed(7)
    if vec:
        R, B, C, H, W, tile, overlap = 3, 2, 3, 512, 512, 256, 64
    else:
        R, B, C, H, W, tile, overlap = 3, 2, 3, 256, 256, 128, 33
    assert R * B * C * H * W // (4 if vec else 1) > 4096 * 256
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    n = B * len(ys) * len(xs)
    x = torch.rand((R, n, C, th, tw), generator=gen) * 2 - 1
    want = torch.stack([tm.blend(x[r], B, H, W, tile, overlap) for r in range(R)]).to(DEV)
    staged = trm.to_staged(x, 5).to(DEV)
    got = tiling.tile_blend_rates(staged, R, B, H, W, tile, overlap, 5)
    assert got.shape == (R, B, C, H, W) and _same_bits(got, want)
    assert _same_bits(tiling.tile_blend_rates(staged, R, B, H, W, tile, overlap, 5), got)


def test_blend_rates_wrapper():
    R, B, C, H, W, tile, overlap, tb = 2, 2, 3, 40, 56, 16, 4, 7
    x = torch.from_numpy(hash_images("tr:w", (R, 30, C, 16, 16)))
    want = torch.stack([tm.blend(x[r], B, H, W, tile, overlap) for r in range(R)]).to(DEV)
    staged = trm.to_staged(x, tb).to(DEV)
    assert _same_bits(tiling.tile_blend_rates(staged, R, B, H, W, tile, overlap, tb), want)
    # any shape with the right number of elements; `out` is filled and returned
    out = torch.empty((R, B, C, H, W), device=DEV)
    assert tiling.tile_blend_rates(staged.view(R * 30, C, 16, 16), R, B, H, W, tile, overlap, tb, out=out) is out
    assert _same_bits(out, want)
    with pytest.raises(RuntimeError, match="floats per channel"):
        tiling.tile_blend_rates(staged[:-1], R, B, H, W, tile, overlap, tb)
    with pytest.raises(RuntimeError, match="out must be"):
        tiling.tile_blend_rates(staged, R, B, H, W, tile, overlap, tb, out=torch.empty((R, B, C, H, 48), device=DEV))
    for kw in (dict(scale=3), dict(tile_batch=0), dict(R=0), dict(R=65), dict(B=0)):
        with pytest.raises(RuntimeError, match="need 1 <= R <= 64, B >= 1, tile_batch >= 1 and a scale of 1 or 2"):
            tiling.tile_blend_rates(staged, **{**dict(R=R, B=B, H=H, W=W, tile=tile, tile_overlap=overlap,
                                                      tile_batch=tb), **kw})
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        tiling.tile_blend_rates(staged, R, B, H, W, 20, overlap, tb)


# ------------------------------------------------------------------ 2. the sweep equals R tiled forwards
IH, IW, TILE, OVERLAP, NR = 56, 80, 32, 8, 3


@functools.lru_cache(maxsize=None)
def _model(name, **extra):
    m = KDLAE_teacher(**{**MODELS[name], **extra})
    load_hash_weights(m)
    m.hip_graphs = False   # the sweep is eager; compare with the eager tiled forward
    return m.to(DEV).eval()


def _img(key, m, B, h=IH, w=IW):
    return torch.from_numpy(hash_images(key, (B, m._cfg["inp_channels"], h, w))).to(DEV)


def _rates(kind, B, h=IH, w=IW):
    if kind == "scalar":
        return [0.15, 0.6, 0.9]
    if kind == "per_image":   # a different rate for every image
        return torch.tensor([[0.15, 0.3], [0.6, 0.7], [0.9, 0.05]])[:, :B].contiguous()
    # per-pixel ramps that differ per image and per rate: a tile that took its rate from the wrong place, the
    # wrong image or the wrong rate would differ
    ramp = torch.linspace(0.05, 0.95, h * w, device=DEV).view(h, w)
    maps = [[(ramp if b % 2 == 0 else ramp.flip(-1)) * (1.0 - 0.3 * r) + 0.01 * b for b in range(B)]
            for r in range(NR)]
    return torch.stack([torch.stack(row) for row in maps])[:, :, None].contiguous()


def _as_maps(rates, B, h, w):
    """R scalars / [R,B] / maps -> [R,B,1,h,w] maps, the form forward_tiled takes."""
    rt = torch.as_tensor(rates, dtype=torch.float32).to(DEV)
    if rt.dim() == 1:
        rt = rt[:, None].expand(-1, B)
    if rt.dim() == 2:
        rt = rt[:, :, None, None, None].expand(-1, -1, 1, h, w)
    return rt.contiguous()


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(model, img, rates, [forward_tiled at rates[r]]), computed once and shared; nothing below writes to them."""
    m = _model(name)
    img, rates = _img(f"tr:m:{name}", m, 2), _rates(kind, 2)
    maps = _as_maps(rates, 2, IH, IW)
    refs = [m.forward_tiled({"img": img, "denoise_rate": maps[r]}, TILE, OVERLAP, 16) for r in range(NR)]
    return m, img, rates, refs


@pytest.mark.parametrize("kind", ["scalar", "per_image", "map"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_sweep_equals_tiled_forwards(name, kind):
    m, img, rates, refs = _case(name, kind)
    oc = m._cfg["out_channels"]
    assert tuple(tiling.tile_plan(IH, IW, TILE, OVERLAP)) == (32, 32, 2, 3, 24, 24)
    for tile_batch in (1, 5, 16):
        out = m.forward_rates_tiled(img, rates, sr=True, tile=TILE, tile_overlap=OVERLAP, tile_batch=tile_batch)
        assert out["hq"].shape == (NR, 2, oc, IH, IW) and out["sr"].shape == (NR, 2, oc, 2 * IH, 2 * IW)
        for r in range(NR):
            assert torch.equal(out["hq"][r], refs[r]["hq"]), f"hq of rate {r} at tile_batch {tile_batch}"
            assert torch.equal(out["sr"][r], refs[r]["sr"]), f"sr of rate {r} at tile_batch {tile_batch}"
    lean = m.forward_rates_tiled(img, rates, sr=False, tile=TILE, tile_overlap=OVERLAP, tile_batch=5)
    assert lean["sr"] is None and torch.equal(lean["hq"], out["hq"])
    assert not torch.equal(out["hq"][0], out["hq"][1])   # the rates do reach the output
    assert not torch.equal(out["hq"][0, 0], out["hq"][0, 1])


def test_one_tile_per_image_equals_forward_rates():
    m, img, _, _ = _case("withbias", "map")
    for kind in ("scalar", "per_image", "map"):
        rates = _rates(kind, 2)
        with torch.no_grad():
            ref = m.forward_rates(img, rates, sr=True)
        for tile, overlap, tile_batch in ((80, 8, 16), (512, 32, 1)):
            assert tiling.tile_plan(IH, IW, tile, overlap)[2:4] == (1, 1)
            out = m.forward_rates_tiled(img, rates, sr=True, tile=tile, tile_overlap=overlap, tile_batch=tile_batch)
            assert torch.equal(out["hq"], ref["hq"]) and torch.equal(out["sr"], ref["sr"])


def test_a_model_without_the_sr_head_sweeps_hq():
    m = _model("biasfree", static="no")
    img, rates = _img("tr:nosr", m, 2), _rates("per_image", 2)
    maps = _as_maps(rates, 2, IH, IW)
    out = m.forward_rates_tiled(img, rates, tile=TILE, tile_overlap=OVERLAP, tile_batch=5)
    assert out["sr"] is None
    for r in range(NR):
        ref = m.forward_tiled({"img": img, "denoise_rate": maps[r]}, TILE, OVERLAP, 16)
        assert torch.equal(out["hq"][r], ref["hq"])


# ------------------------------------------------------------------ 3. refusals
def test_forward_rates_tiled_refusals():
    m, img, rates, _ = _case("biasfree", "scalar")
    kw = dict(tile=TILE, tile_overlap=OVERLAP, tile_batch=16)
    plus, nosr = _model("biasfree", params="plus"), _model("biasfree", static="no")
    restormer = Restormer(**MODELS["biasfree"]).to(DEV).eval()
    u8 = torch.zeros((1, 45, 70, 3), dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.memory_allocated()
    with pytest.raises(RuntimeError, match="params='cat'"):
        plus.forward_rates_tiled(img, rates, **kw)
    with pytest.raises(RuntimeError, match="static='train'"):
        nosr.forward_rates_tiled(img, rates, sr=True, **kw)
    for R in (0, 65):
        with pytest.raises(RuntimeError, match="1..64 rates"):
            m.forward_rates_tiled(img, [0.5] * R, **kw)
    for tile, overlap in ((20, 4), (8, 0), (32, 32), (32, -1)):
        with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
            m.forward_rates_tiled(img, rates, tile=tile, tile_overlap=overlap)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        m.forward_rates_tiled(img[..., :44, :], rates, **kw)
    for tile_batch in (0, -3):
        with pytest.raises(RuntimeError, match="tile_batch"):
            m.forward_rates_tiled(img, rates, tile=TILE, tile_overlap=OVERLAP, tile_batch=tile_batch)
    with pytest.raises(RuntimeError, match="rates must be"):
        m.forward_rates_tiled(img, torch.zeros(2, 3), **kw)
    with pytest.raises(RuntimeError, match="rates must be"):
        m.forward_rates_tiled(img, torch.zeros(2, 2, 1, IH, IW - 8), **kw)
    with pytest.raises(RuntimeError, match="expected img"):
        m.forward_rates_tiled(img[:, :2], rates, **kw)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_rates_tiled(img.cpu(), rates, **kw)
    m.train()
    try:
        with pytest.raises(RuntimeError, match="eval"):
            m.forward_rates_tiled(img, rates, **kw)
    finally:
        m.eval()
    with pytest.raises(RuntimeError, match="no denoise_rate input"):
        restormer.forward_rates_tiled(img, rates, **kw)
    with pytest.raises(RuntimeError, match="params='cat'"):
        enhance_rates_tiled_u8(restormer, u8, [0.5], **kw)
    gc.collect()   # a raised exception's frames may still hold the refused call's small temporaries
    assert torch.cuda.memory_allocated() == before   # refused before the staging or an output is allocated


# ------------------------------------------------------------------ 4, 5. the u8 pipeline
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


UH, UW = 45, 70   # reflect-padded to 48 x 72: 2 x 3 tiles of 32 at overlap 8
U_RATES = torch.tensor([[0.1, 0.2], [0.5, 0.6], [0.9, 0.8]])


@functools.lru_cache(maxsize=None)
def _u8_case():
    """(model, images, candidates of the tiled sweep at tile_batch 16), computed once and shared."""
    m = _model("biasfree")
    images = _u8(31, 2, UH, UW)
    cands = enhance_rates_tiled_u8(m, images, U_RATES, tile=TILE, tile_overlap=OVERLAP, tile_batch=16)
    return m, images, cands


def test_enhance_rates_tiled_u8_equals_enhance_tiled_u8_per_rate():
    m, images, cands = _u8_case()
    assert tuple(tiling.tile_plan(48, 72, TILE, OVERLAP))[:4] == (32, 32, 2, 3)
    assert cands.shape == (3, 2, UH, UW, 3) and cands.dtype == torch.uint8
    for r in range(3):
        want = enhance_tiled_u8(m, images, U_RATES[r], tile=TILE, tile_overlap=OVERLAP, tile_batch=16)[0]
        assert torch.equal(cands[r], want), f"rate {r}"
    assert bool((cands[:, :, : UH // 3, : UW // 4] == 0).all()) and not torch.equal(cands[0], cands[2])
    # another chunking, and scalars shared by the batch
    again = enhance_rates_tiled_u8(m, images, U_RATES, tile=TILE, tile_overlap=OVERLAP, tile_batch=5)
    assert torch.equal(again, cands)
    shared = enhance_rates_tiled_u8(m, images, [0.1, 0.9], tile=TILE, tile_overlap=OVERLAP, tile_batch=4)
    for r, rate in enumerate((0.1, 0.9)):
        want = enhance_tiled_u8(m, images, rate, tile=TILE, tile_overlap=OVERLAP, tile_batch=16)[0]
        assert torch.equal(shared[r], want)


@pytest.mark.parametrize("select", ["closest", "max", "min"])
def test_enhance_auto_tiled_u8_end_to_end(select):
    m, images, cands = _u8_case()
    scorer = _scorer()
    B = 2
    want_scores = np.stack([asdqe_scores(scorer, images, cands[r]) for r in range(3)])
    target = float(np.float32(want_scores.mean())) if select == "closest" else None
    tile_batch = {"closest": 5, "max": 16, "min": 1}[select]
    out = enhance_auto_tiled_u8(m, scorer, images, U_RATES, target=target, select=select, want_sr=True, tile=TILE,
                                tile_overlap=OVERLAP, tile_batch=tile_batch)
    scores = out["scores"].cpu().numpy()
    assert scores.dtype == np.float32 and np.array_equal(scores.view(np.uint32), want_scores.view(np.uint32))
    tg = np.full(B, target, np.float32) if target is not None else None
    want_idx = select_model(scores, MODES[select], tg)
    assert out["index"].dtype == torch.int32 and np.array_equal(out["index"].cpu().numpy(), want_idx)
    chosen = U_RATES[torch.from_numpy(want_idx).long(), torch.arange(B)]
    assert torch.equal(out["rate"].cpu(), chosen)
    # what a user gets from the tiled call with the rates the sweep chose, image by image
    want_hq, want_sr = enhance_tiled_u8(m, images, chosen, tile=TILE, tile_overlap=OVERLAP, tile_batch=16)
    assert out["hq"].shape == (B, UH, UW, 3) and out["sr"].shape == (B, 2 * UH, 2 * UW, 3)
    assert torch.equal(out["hq"], want_hq) and torch.equal(out["sr"], want_sr)
    lean = enhance_auto_tiled_u8(m, scorer, images, U_RATES, target=target, select=select, tile=TILE,
                                 tile_overlap=OVERLAP, tile_batch=tile_batch)
    assert lean["sr"] is None and torch.equal(lean["hq"], out["hq"]) and torch.equal(lean["index"], out["index"])
    with pytest.raises(RuntimeError, match="select must be"):
        enhance_auto_tiled_u8(m, scorer, images, U_RATES, select="median")

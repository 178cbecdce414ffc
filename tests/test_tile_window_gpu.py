"""Weighted tile blend on the GPU: kdlae_tile_blend_w / kdlae_tile_blend_rates_w against the numpy model
(tests/tile_window_model.py), against the uniform kernel and against each other, then ``window=`` through
KDLAE_teacher.forward_tiled / forward_rates_tiled, Restormer.forward_tiled, the u8 pipeline and validate().

The kernels multiply, add in a fixed order and divide, each operation rounded on its own, and batch rows of the
forward are bit for bit independent of the batch size, so every comparison here is on the bits: no tolerance
anywhere in this file except the PSNR of validate(), a float64 sum taken in another order (the tolerance of
tests/test_tile_gpu.py's validate test)."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rethink_acoustic_image_enhancement_amd import _lib, tiling
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher, Restormer
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.pipeline import (enhance_auto_tiled_u8, enhance_rates_tiled_u8,
                                                             enhance_tiled_u8, postprocess_u8, preprocess_u8)
from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer
from tests import metrics_oracle as mo
from tests import tile_model as tm
from tests import tile_window_model as twm
from tests.test_rate_sweep_gpu import MODELS
from tests.test_tile_gpu import (BIG, DEV, G, IH, IW, OVERLAP, T_CFG, TILE, VH, VW, _c, _expect_store, _img, _model,
                                 _rate, _same_bits, _stored)
from tests.test_tile_rates_gpu import _scorer, _u8

pytestmark = pytest.mark.gpu

# (tiles, destination, wx) offsets in floats from a 16-byte boundary: all three at 0 with an aligned stride is the
# float4 path, anything else the scalar one (a wx off the boundary alone is enough)
OFFSETS = [(0, 0, 0), (0, 0, 1), (0, 0, 2), (1, 1, 0), (2, 2, 2), (3, 3, 3), (1, 3, 2), (2, 0, 0), (0, 3, 0)]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def _blend_w_abi(tiles_view, B, C, H, W, tile, overlap, scale, wy, wx_view, do):
    """Two calls into BIG-filled storage at destination offset `do` -> the storage (equal bits asserted)."""
    n = B * C * scale * H * scale * W
    got = []
    for _ in range(2):
        dst_store = torch.full((G + do + n + G,), BIG, device=DEV)
        rc = _lib.lib().kdlae_tile_blend_w(_c(tiles_view), B, C, H, W, tile, overlap, scale, _c(wy), _c(wx_view),
                                           _c(dst_store[G + do:]), None)
        assert rc == 0, _lib.last_error()
        got.append(dst_store)
    assert _same_bits(got[0], got[1])
    return got[0]


# ------------------------------------------------------------------ 1. kdlae_tile_blend_w against the model
@pytest.mark.parametrize("window", twm.KERNEL_WINDOWS)
@pytest.mark.parametrize("tile", twm.TILES)
@pytest.mark.parametrize("hw", twm.SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_blend_w_equals_the_model(C, hw, tile, window):
    B, (H, W) = 2, hw
    for overlap in twm.overlaps(tile):
        for scale in (1, 2):
            tiles = twm.case_tiles(C, H, W, tile, overlap, scale)
            wy, wx = twm.case_tables(window, H, W, tile, overlap, scale)
            want = _t(twm.blend(tiles, wy, wx, B, H, W, tile, overlap, scale))
            wy_dev = _t(wy).to(DEV)
            for so, do, wo in OFFSETS:
                t_store, t_view = _stored(_t(tiles), so)
                w_store, w_view = _stored(_t(wx), wo)
                t0, w0 = t_store.clone(), w_store.clone()
                got = _blend_w_abi(t_view, B, C, H, W, tile, overlap, scale, wy_dev, w_view, do)
                assert _same_bits(got, _expect_store(want, do)), (overlap, scale, so, do, wo)
                assert _same_bits(t_store, t0) and _same_bits(w_store, w0)


@pytest.mark.parametrize("vec", [True, False])
def test_blend_w_more_items_than_one_pass_of_the_grid(vec):
    """The launcher caps the grid at 4096 blocks of 256 threads and loops over the rest: more than 4096 * 256
    items (of 4 floats on the float4 path, of 1 float on the scalar path), sized as tests/test_tile_gpu.py does."""
    gen = torch.Generator().manual_seed(5)
    if vec:
        B, C, H, W, tile, overlap = 2, 3, 768, 1024, 512, 64
    else:
        B, C, H, W, tile, overlap = 2, 3, 384, 512, 256, 33
    assert B * C * H * W // (4 if vec else 1) > 4096 * 256
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    tiles = torch.rand((B * len(ys) * len(xs), C, th, tw), generator=gen) * 2 - 1
    wy, wx = twm.tables("random", H, W, tile, overlap, 1, seed=9)
    want = _t(twm.blend(tiles.numpy(), wy, wx, B, H, W, tile, overlap)).to(DEV)
    got = tiling.tile_blend(tiles.to(DEV), B, H, W, tile, overlap, window=(_t(wy), _t(wx)))
    assert _same_bits(got, want)
    assert _same_bits(tiling.tile_blend(tiles.to(DEV), B, H, W, tile, overlap, window=(_t(wy), _t(wx))), got)


@pytest.mark.parametrize("scale", [1, 2])
def test_blend_w_long_thin_image(scale):
    """8 x 20000, tile 16, overlap 4: one tile along y, 1667 along x, a row of 2 x 20000 floats at scale 2."""
    B, C, H, W, tile, overlap = 1, 1, 8, 20000, 16, 4
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    assert (th, tw, len(ys), len(xs)) == (8, 16, 1, 1667)
    tiles = hash_images(f"tilew:thin:{scale}", (1667, 1, scale * 8, scale * 16), -1.0, 1.0)
    for window in ("ramp", "hann"):
        wy, wx = twm.tables(window, H, W, tile, overlap, scale)
        want = _t(twm.blend(tiles, wy, wx, B, H, W, tile, overlap, scale)).to(DEV)
        got = tiling.tile_blend(_t(tiles).to(DEV), B, H, W, tile, overlap, scale, window=window)
        assert _same_bits(got, want), window


# ------------------------------------------------------------------ 2. the uniform kernel, and the copy rule
@pytest.mark.parametrize("hw", twm.SHAPES)
def test_tables_of_ones_give_the_bits_of_the_uniform_kernel(hw):
    B, C, (H, W) = 2, 3, hw
    for tile in twm.TILES:
        for overlap in twm.overlaps(tile):
            for scale in (1, 2):
                tiles = _t(twm.case_tiles(C, H, W, tile, overlap, scale)).to(DEV)
                th, tw, _, _ = tm.plan(H, W, tile, overlap)
                want = tiling.tile_blend(tiles, B, H, W, tile, overlap, scale)
                got = tiling.tile_blend(tiles, B, H, W, tile, overlap, scale, window=(torch.ones(th), torch.ones(tw)))
                assert _same_bits(got, want), (tile, overlap, scale)
    # "ramp" at overlap 0 and scale 1 is a table of ones
    tiles = _t(twm.case_tiles(C, H, W, 16, 0, 1)).to(DEV)
    assert _same_bits(tiling.tile_blend(tiles, B, H, W, 16, 0, window="ramp"), tiling.tile_blend(tiles, B, H, W, 16, 0))


@pytest.mark.parametrize("scale", [1, 2])
def test_one_tile_image_returns_its_tile_under_every_window(scale):
    B, C, H, W = 2, 3, 24, 40
    tiles = _t(hash_images(f"tilew:one:{scale}", (B, C, scale * H, scale * W), -1.0, 1.0)).to(DEV)
    pair = tuple(_t(a) for a in twm.random_pair(H, W, 4))
    for tile, overlap in ((40, 8), (64, 63), (512, 32)):
        assert tiling.tile_plan(H, W, tile, overlap)[:4] == (H, W, 1, 1)
        for window in ("ramp", "hann", pair):
            got = tiling.tile_blend(tiles, B, H, W, tile, overlap, scale, window=window)
            assert _same_bits(got, tiles), (tile, overlap, window if isinstance(window, str) else "pair")


# ------------------------------------------------------------------ 3. kdlae_tile_blend_rates_w
@pytest.mark.parametrize("window", twm.KERNEL_WINDOWS)
@pytest.mark.parametrize("hw,tile,overlap", [((40, 56), 16, 5), ((40, 56), 16, 8), ((16, 72), 24, 16),
                                             ((24, 24), 16, 4)])
def test_blend_rates_w_equals_blend_w_of_every_slice(hw, tile, overlap, window):
    R, B, C, (H, W) = 3, 2, 3, hw
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    n = B * len(ys) * len(xs)
    for scale in (1, 2):
        x = _t(hash_images(f"tilew:r:{H}x{W}:{tile}:{overlap}:{scale}", (R, n, C, scale * th, scale * tw), -1.0, 1.0))
        wy, wx = twm.case_tables(window, H, W, tile, overlap, scale)
        wy_dev = _t(wy).to(DEV)
        x_dev = x.to(DEV)
        want = torch.stack([_blend_w_abi(x_dev[r].contiguous(), B, C, H, W, tile, overlap, scale, wy_dev,
                                         _t(wx).to(DEV), 0)[G:-G] for r in range(R)])
        # ... which is the model's
        assert _same_bits(want[1], _t(twm.blend(x[1].numpy(), wy, wx, B, H, W, tile, overlap, scale)).to(DEV).view(-1))
        for tile_batch in (1, 4, n + 3):
            staged = twm.to_staged(x, tile_batch)
            for so, do, wo in ((0, 0, 0), (0, 0, 3), (1, 2, 0), (2, 0, 1)):
                s_store, s_view = _stored(staged, so)
                w_store, w_view = _stored(_t(wx), wo)
                s0 = s_store.clone()
                got = []
                for _ in range(2):
                    dst = torch.full((G + do + want.numel() + G,), BIG, device=DEV)
                    rc = _lib.lib().kdlae_tile_blend_rates_w(_c(s_view), R, B, C, H, W, tile, overlap, tile_batch,
                                                             scale, _c(wy_dev), _c(w_view), _c(dst[G + do:]), None)
                    assert rc == 0, _lib.last_error()
                    got.append(dst)
                assert _same_bits(got[0], got[1])
                assert _same_bits(got[0], _expect_store(want.cpu(), do)), (scale, tile_batch, so, do, wo)
                assert _same_bits(s_store, s0)
        # the wrapper, by name, for the named windows
        if window != "random":
            out = tiling.tile_blend_rates(twm.to_staged(x, 4).to(DEV), R, B, H, W, tile, overlap, 4, scale,
                                          window=window)
            assert out.shape == (R, B, C, scale * H, scale * W) and _same_bits(out.view(R, -1), want)


@pytest.mark.parametrize("vec", [True, False])
def test_blend_rates_w_more_items_than_one_pass_of_the_grid(vec):
    gen = torch.Generator().manual_seed(7)
    if vec:
        R, B, C, H, W, tile, overlap = 3, 2, 3, 512, 512, 256, 64
    else:
        R, B, C, H, W, tile, overlap = 3, 2, 3, 256, 256, 128, 33
    assert R * B * C * H * W // (4 if vec else 1) > 4096 * 256
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    n = B * len(ys) * len(xs)
    x = torch.rand((R, n, C, th, tw), generator=gen) * 2 - 1
    wy, wx = twm.tables("hann", H, W, tile, overlap)
    want = torch.stack([_t(twm.blend(x[r].numpy(), wy, wx, B, H, W, tile, overlap)) for r in range(R)]).to(DEV)
    got = tiling.tile_blend_rates(twm.to_staged(x, 5).to(DEV), R, B, H, W, tile, overlap, 5, window="hann")
    assert _same_bits(got, want)


# ------------------------------------------------------------------ 4. the seam, on the device
def _largest_step(img):
    return max(float((img[1:] - img[:-1]).abs().max()), float((img[:, 1:] - img[:, :-1]).abs().max()))


def test_the_ramp_lowers_the_seam_of_constant_tiles():
    """48 x 72, tile 32, overlap 8, a distinct constant per tile (tests/test_tile_window.py's 2-D seam case), and
    the 1-D case of the issue: 32 x 56 with tiles 0 and 1."""
    vals = torch.tensor([0.0, 1.0, 0.25, 0.75, 0.125, 0.5], device=DEV)
    tiles = vals.view(6, 1, 1, 1).expand(6, 1, 32, 32).contiguous()
    uni = tiling.tile_blend(tiles, 1, 48, 72, 32, 8)[0, 0]
    ramp = tiling.tile_blend(tiles, 1, 48, 72, 32, 8, window="ramp")[0, 0]
    print(f"2 x 3 plan: uniform {_largest_step(uni)!r}, ramp {_largest_step(ramp)!r}")
    assert _largest_step(ramp) < _largest_step(uni)
    two = vals[:2].view(2, 1, 1, 1).expand(2, 1, 32, 32).contiguous()
    uni = tiling.tile_blend(two, 1, 32, 56, 32, 8)[0, 0]
    ramp = tiling.tile_blend(two, 1, 32, 56, 32, 8, window="ramp")[0, 0]
    print(f"two tiles: uniform {_largest_step(uni)!r}, ramp {_largest_step(ramp)!r}")
    assert _largest_step(uni) == 0.5 and _largest_step(ramp) <= 1.0 / 9 + 2.0 ** -20


# ------------------------------------------------------------------ 5. the modules
PAIR = twm.random_pair(TILE, TILE, 7)
WINDOWS = ("ramp", "hann", "pair")


def _arg(window):
    """The value a caller passes as ``window``."""
    return (_t(PAIR[0]), _t(PAIR[1]).to(DEV)) if window == "pair" else window   # one table on each side


def _model_tables(window, scale, h=IH, w=IW, tile=TILE, overlap=OVERLAP):
    if window == "pair":
        return np.repeat(PAIR[0], scale), np.repeat(PAIR[1], scale)
    return twm.tables(window, h, w, tile, overlap, scale)


def _tile_outputs(m, img, rate, tile=TILE, overlap=OVERLAP):
    """What a user has without the feature: every tile through forward alone -> (hq tiles, sr tiles or None),
    numpy, in flat-index order."""
    B, _, h, w = img.shape
    th, tw, ys, xs = tm.plan(h, w, tile, overlap)
    hqs, srs = [], []
    with torch.no_grad():
        for b in range(B):
            for y in ys:
                for x in xs:
                    sl = (slice(b, b + 1), slice(None), slice(y, y + th), slice(x, x + tw))
                    if isinstance(m, Restormer):
                        o = {"hq": m(img[sl].contiguous()), "sr": None}
                    else:
                        o = m({"img": img[sl].contiguous(),
                               "denoise_rate": rate[sl].contiguous() if rate is not None else None})
                    hqs.append(o["hq"].cpu())
                    srs.append(o["sr"].cpu() if o["sr"] is not None else None)
    return torch.cat(hqs).numpy(), (torch.cat(srs).numpy() if srs[0] is not None else None)


def _route(hq_t, sr_t, B, window, h=IH, w=IW, tile=TILE, overlap=OVERLAP):
    """The per-tile outputs blended by the numpy model -> (hq, sr or None) as CPU tensors."""
    hq = _t(twm.blend(hq_t, *_model_tables(window, 1, h, w, tile, overlap), B, h, w, tile, overlap, 1))
    sr = _t(twm.blend(sr_t, *_model_tables(window, 2, h, w, tile, overlap), B, h, w, tile, overlap, 2)) \
        if sr_t is not None else None
    return hq, sr


@functools.lru_cache(maxsize=None)
def _case(name):
    """(model, img, rate, hq tiles, sr tiles), computed once and shared; nothing below writes to them."""
    m = _model(name)
    img, rate = _img(f"tilew:m:{name}", m, 2), _rate("ramp", 2)
    return (m, img, rate) + _tile_outputs(m, img, rate)


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("name", sorted(MODELS))
def test_forward_tiled_window_equals_the_per_tile_route(name, window):
    m, img, rate, hq_t, sr_t = _case(name)
    r_hq, r_sr = _route(hq_t, sr_t, 2, window)
    for tile_batch in (1, 3, 16):
        for _ in range(2):
            out = m.forward_tiled({"img": img, "denoise_rate": rate}, TILE, OVERLAP, tile_batch, window=_arg(window))
            assert torch.equal(out["hq"].cpu(), r_hq), f"hq at tile_batch {tile_batch}"
            assert torch.equal(out["sr"].cpu(), r_sr), f"sr at tile_batch {tile_batch}"
    uni = m.forward_tiled({"img": img, "denoise_rate": rate}, TILE, OVERLAP, 16)
    assert not torch.equal(uni["hq"].cpu(), r_hq) and not torch.equal(uni["sr"].cpu(), r_sr)   # the window is read


def test_uniform_given_explicitly_equals_the_default():
    m, img, rate, _, _ = _case("biasfree")
    inp = {"img": img, "denoise_rate": rate}
    a = m.forward_tiled(inp, TILE, OVERLAP, 3)
    for window in ("uniform", None):
        b = m.forward_tiled(inp, TILE, OVERLAP, 3, window=window)
        assert torch.equal(a["hq"], b["hq"]) and torch.equal(a["sr"], b["sr"])
    rates = [0.2, 0.7]
    a = m.forward_rates_tiled(img, rates, sr=True, tile=TILE, tile_overlap=OVERLAP, tile_batch=5)
    b = m.forward_rates_tiled(img, rates, sr=True, tile=TILE, tile_overlap=OVERLAP, tile_batch=5, window="uniform")
    assert torch.equal(a["hq"], b["hq"]) and torch.equal(a["sr"], b["sr"])
    with pytest.raises(RuntimeError, match="must be one of"):
        m.forward_tiled(inp, TILE, OVERLAP, 3, window="triangle")


def test_one_tile_per_image_equals_forward_under_every_window():
    m, img, rate, _, _ = _case("withbias")
    with torch.no_grad():
        ref = m({"img": img, "denoise_rate": rate})
    pair = tuple(_t(a) for a in twm.random_pair(IH, IW, 2))
    for window in ("ramp", "hann", pair):
        for tile, overlap in ((72, 8), (512, 32)):
            out = m.forward_tiled({"img": img, "denoise_rate": rate}, tile, overlap, 16, window=window)
            assert torch.equal(out["hq"], ref["hq"]) and torch.equal(out["sr"], ref["sr"])


@pytest.mark.parametrize("window", WINDOWS)
def test_restormer_forward_tiled_window(window):
    m = Restormer(**MODELS["biasfree"])
    load_hash_weights(m)
    m = m.to(DEV).eval()
    m.hip_graphs = False
    img = _t(hash_images("tilew:restormer", (2, 3, IH, IW))).to(DEV)
    hq_t, _ = _tile_outputs(m, img, None)
    want, _ = _route(hq_t, None, 2, window)
    for tile_batch in (1, 16):
        assert torch.equal(m.forward_tiled(img, TILE, OVERLAP, tile_batch, window=_arg(window)).cpu(), want)
    assert torch.equal(m.forward_tiled(img, TILE, OVERLAP, 16, window="uniform"),
                       m.forward_tiled(img, TILE, OVERLAP, 16))


@pytest.mark.parametrize("window", WINDOWS)
def test_forward_rates_tiled_window_equals_forward_tiled_window_per_rate(window):
    m, img, _, _, _ = _case("biasfree")
    rates = torch.tensor([[0.15, 0.3], [0.6, 0.7], [0.9, 0.05]])
    maps = rates.to(DEV)[:, :, None, None, None].expand(-1, -1, 1, IH, IW).contiguous()
    refs = [m.forward_tiled({"img": img, "denoise_rate": maps[r]}, TILE, OVERLAP, 16, window=_arg(window))
            for r in range(3)]
    for tile_batch in (1, 5, 16):
        out = m.forward_rates_tiled(img, rates, sr=True, tile=TILE, tile_overlap=OVERLAP, tile_batch=tile_batch,
                                    window=_arg(window))
        for r in range(3):
            assert torch.equal(out["hq"][r], refs[r]["hq"]), f"hq of rate {r} at tile_batch {tile_batch}"
            assert torch.equal(out["sr"][r], refs[r]["sr"]), f"sr of rate {r} at tile_batch {tile_batch}"
    assert not torch.equal(out["hq"][0], out["hq"][1])


# ------------------------------------------------------------------ 6. the u8 pipeline
UH, UW = 45, 70   # reflect-padded to 48 x 72: 2 x 3 tiles of 32 at overlap 8
U_RATES = torch.tensor([[0.1, 0.2], [0.5, 0.6], [0.9, 0.8]])


@pytest.mark.parametrize("window", WINDOWS)
def test_enhance_tiled_u8_window_equals_pre_and_post_around_the_route(window):
    m = _model("biasfree")
    images = _u8(21, 2, UH, UW)
    img, rmap = preprocess_u8(images, 0.6, 8, False)
    assert img.shape == (2, 3, IH, IW)
    r_hq, r_sr = _route(*_tile_outputs(m, img, rmap), 2, window)
    want_hq = postprocess_u8(r_hq.to(DEV), UH, UW, 1, images)
    want_sr = postprocess_u8(r_sr.to(DEV), UH, UW, 2, images)
    for tile_batch in (16, 4):
        hq, sr = enhance_tiled_u8(m, images, 0.6, tile=TILE, tile_overlap=OVERLAP, tile_batch=tile_batch,
                                  window=_arg(window))
        assert hq.dtype == torch.uint8 and torch.equal(hq, want_hq) and torch.equal(sr, want_sr)


@pytest.mark.parametrize("window", WINDOWS)
def test_enhance_rates_and_auto_tiled_u8_window(window):
    m, scorer = _model("biasfree"), _scorer()
    images = _u8(31, 2, UH, UW)
    kw = dict(tile=TILE, tile_overlap=OVERLAP, window=_arg(window))
    cands = enhance_rates_tiled_u8(m, images, U_RATES, tile_batch=5, **kw)
    assert cands.shape == (3, 2, UH, UW, 3) and cands.dtype == torch.uint8
    for r in range(3):   # pre- and post-processing around the tiled forward with the same window
        img, rmap = preprocess_u8(images, U_RATES[r], 8, False)
        pred = m.forward_tiled({"img": img, "denoise_rate": rmap}, TILE, OVERLAP, 16, window=_arg(window))
        assert torch.equal(cands[r], postprocess_u8(pred["hq"], UH, UW, 1, images)), f"rate {r}"
    assert not torch.equal(cands, enhance_rates_tiled_u8(m, images, U_RATES, tile=TILE, tile_overlap=OVERLAP))
    out = enhance_auto_tiled_u8(m, scorer, images, U_RATES, select="max", want_sr=True, tile_batch=4, **kw)
    chosen = U_RATES[out["index"].long().cpu(), torch.arange(2)]
    assert torch.equal(out["rate"].cpu(), chosen)
    img, rmap = preprocess_u8(images, chosen, 8, False)
    pred = m.forward_tiled({"img": img, "denoise_rate": rmap}, TILE, OVERLAP, 16, window=_arg(window))
    assert torch.equal(out["hq"], postprocess_u8(pred["hq"], UH, UW, 1, images))
    assert torch.equal(out["sr"], postprocess_u8(pred["sr"], UH, UW, 2, images))
    want_hq, want_sr = enhance_tiled_u8(m, images, chosen, tile_batch=16, **kw)
    assert torch.equal(out["hq"], want_hq) and torch.equal(out["sr"], want_sr)


# ------------------------------------------------------------------ 7. validate
def test_validate_tile_window_equals_the_route_and_the_default_keeps_its_value():
    m = KDLAE_teacher(**T_CFG)
    load_hash_weights(m)
    tr = KDLAETrainer(m.to(DEV), lr=1e-3, ema_decay=0.999)
    lq = {"img": _img("tilew:v:img", m, 2, 32, 32), "denoise_rate": torch.full((2, 1, 32, 32), 0.6, device=DEV)}
    gt = {"hq": _img("tilew:v:hq", m, 2, 32, 32), "sr": _img("tilew:v:sr", m, 2, 64, 64)}
    tr.optimize_parameters(lq, gt)
    items = []
    for i in range(2):
        lq = {"img": _img(f"tilew:v:vimg{i}", m, 1, VH, VW), "denoise_rate": _rate("ramp", 1, VH, VW)}
        gt = {"hq": _img(f"tilew:v:vhq{i}", m, 1, VH, VW), "sr": _img(f"tilew:v:vsr{i}", m, 1, 2 * VH, 2 * VW)}
        items.append((lq, gt))
    ref = KDLAE_teacher(**T_CFG)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in tr.ema_state_dict().items()})
    ref = ref.to(DEV).eval()
    ref.hip_graphs = False
    outs = []
    for lq, _ in items:
        img = F.pad(lq["img"], (0, IW - VW, 0, IH - VH), "reflect")
        rate = F.pad(lq["denoise_rate"], (0, IW - VW, 0, IH - VH), "reflect")
        hq, sr = _route(*_tile_outputs(ref, img, rate), 1, "ramp")
        outs.append((hq[..., :VH, :VW], sr[..., :2 * VH, :2 * VW]))
    kw = dict(tile=TILE, tile_overlap=OVERLAP, tile_batch=4)
    for (lq, gt), (r_hq, r_sr) in zip(items, outs):   # item by item: the outputs bit for bit
        tr.validate([(lq, gt)], tile_window="ramp", **kw)
        assert torch.equal(tr.val_output["hq"].cpu(), r_hq) and torch.equal(tr.val_output["sr"].cpu(), r_sr)
    res = tr.validate(items, tile_window="ramp", **kw)
    want_hq = np.mean([mo.psnr(o[0][0].numpy(), gt["hq"][0].cpu().numpy()) for (_, gt), o in zip(items, outs)])
    want_sr = np.mean([mo.psnr(o[1][0].numpy(), gt["sr"][0].cpu().numpy()) for (_, gt), o in zip(items, outs)])
    print(f"psnr_hq {res['psnr_hq']!r} vs {want_hq!r}; psnr_sr {res['psnr_sr']!r} vs {want_sr!r}")
    # fp64 sums in another order: n * 2^-53 << 1e-9
    assert abs(res["psnr_hq"] - want_hq) <= 1e-9 * abs(want_hq)
    assert abs(res["psnr_sr"] - want_sr) <= 1e-9 * abs(want_sr)
    # without tile_window: today's value, tiled and untiled
    plain = tr.validate(items, **kw)
    assert plain == tr.validate(items, tile_window="uniform", **kw) and plain != res
    assert tr.validate(items) == tr.validate(items, tile_window="ramp")   # not read without tile

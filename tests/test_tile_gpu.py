"""Tiled inference on the GPU: kdlae_tile_gather / kdlae_tile_blend against slicing and the CPU model
(tests/tile_model.py), KDLAE_teacher.forward_tiled, pipeline.enhance_tiled_u8 and KDLAETrainer.validate(tile=).

The kernels copy, add in a fixed order and divide, and batch rows of the forward are bit for bit independent of
the batch size (test_kdlae_gpu.test_batch_invariance_and_determinism), so every comparison here is on the bits:
no tolerance anywhere in this file except the PSNR of validate(), a float64 sum taken in another order."""
import ctypes
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from rethink_acoustic_image_enhancement_amd import _lib, tiling
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from rethink_acoustic_image_enhancement_amd.pipeline import enhance_tiled_u8, postprocess_u8, preprocess_u8
from rethink_acoustic_image_enhancement_amd.train import KDLAETrainer
from tests import metrics_oracle as mo
from tests import tile_model as tm
from tests.test_rate_sweep_gpu import MODELS

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BIG = 1e30
G = 64   # guard floats (256 bytes) either side of a buffer under test

SHAPES = [(40, 56), (16, 72), (24, 24)]
# (source offset, destination offset) in floats from a 16-byte boundary; (0, 0) with an aligned stride is the
# float4 path, everything else the scalar one
OFFSETS = [(0, 0), (1, 1), (2, 2), (3, 3), (1, 3), (2, 0), (0, 3)]


def _overlaps(tile):
    return sorted({0, 4, 5, 8, tile - 8})


def _c(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _stored(values, off):
    """`values` (CPU) inside BIG-filled device storage at float offset `off` from a 16-byte boundary ->
    (storage, view of the values)."""
    n = values.numel()
    store = torch.full((G + off + n + G,), BIG, device=DEV)
    assert store.data_ptr() % 16 == 0
    view = store[G + off:G + off + n]
    view.copy_(values.reshape(-1))
    return store, view


def _expect_store(values, off):
    exp = torch.full((G + off + values.numel() + G,), BIG)
    exp[G + off:G + off + values.numel()] = values.reshape(-1)
    return exp.to(DEV)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


# ------------------------------------------------------------------ tile_gather
@pytest.mark.parametrize("tile", [16, 24])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_gather_equals_slicing(C, hw, tile):
    L = _lib.lib()
    B, (H, W) = 2, hw
    img = torch.from_numpy(hash_images(f"tile:g:{C}:{H}x{W}", (B, C, H, W)))
    for overlap in _overlaps(tile):
        want = tm.gather(img, tile, overlap)
        n, per = want.shape[0], want.shape[0] // B
        ranges = sorted({(0, n), (n // 2, 1), (per - 1, 2), (n - 1, 1)})   # all, one tile, across two images, last
        for so, do in OFFSETS:
            src_store, src = _stored(img, so)
            src0 = src_store.clone()
            for first, count in ranges:
                exp = _expect_store(want[first:first + count], do)
                got = []
                for _ in range(2):
                    dst_store = torch.full((exp.numel(),), BIG, device=DEV)
                    rc = L.kdlae_tile_gather(_c(src), B, C, H, W, tile, overlap, first, count, _c(dst_store[G + do:]),
                                             None)
                    assert rc == 0, _lib.last_error()
                    got.append(dst_store)
                assert _same_bits(got[0], got[1])
                assert _same_bits(got[0], exp), (overlap, so, do, first, count)
            assert _same_bits(src_store, src0)


def test_gather_wrapper():
    img = torch.from_numpy(hash_images("tile:gw", (2, 3, 40, 56))).to(DEV)
    want = tm.gather(img.cpu(), 16, 5)
    assert torch.equal(tiling.tile_gather(img, 16, 5).cpu(), want)
    assert torch.equal(tiling.tile_gather(img, 16, 5, first=7).cpu(), want[7:])
    out = torch.empty((4, 3, 16, 16), device=DEV)
    assert tiling.tile_gather(img, 16, 5, 3, 4, out=out) is out and torch.equal(out.cpu(), want[3:7])
    with pytest.raises(RuntimeError, match="first \\+ count"):
        tiling.tile_gather(img, 16, 5, first=want.shape[0], count=1)
    with pytest.raises(RuntimeError, match="out must be"):
        tiling.tile_gather(img, 16, 5, 0, 4, out=torch.empty((4, 3, 16, 8), device=DEV))


# ------------------------------------------------------------------ tile_blend
def _tiles_for(key, B, C, H, W, tile, overlap, scale):
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    return torch.from_numpy(hash_images(key, (B * len(ys) * len(xs), C, scale * th, scale * tw), -1.0, 1.0))


def _blend_abi(tiles_view, B, C, H, W, tile, overlap, scale, do):
    """Two calls into BIG-filled storage at destination offset `do` -> the storage (equal bits asserted)."""
    n = B * C * scale * H * scale * W
    got = []
    for _ in range(2):
        dst_store = torch.full((G + do + n + G,), BIG, device=DEV)
        rc = _lib.lib().kdlae_tile_blend(_c(tiles_view), B, C, H, W, tile, overlap, scale, _c(dst_store[G + do:]), None)
        assert rc == 0, _lib.last_error()
        got.append(dst_store)
    assert _same_bits(got[0], got[1])
    return got[0]


@pytest.mark.parametrize("tile", [16, 24])
@pytest.mark.parametrize("hw", SHAPES)
@pytest.mark.parametrize("C", [1, 3])
def test_blend_equals_the_model(C, hw, tile):
    B, (H, W) = 2, hw
    for overlap in _overlaps(tile):
        for scale in (1, 2):
            tiles = _tiles_for(f"tile:b:{C}:{H}x{W}:{tile}:{overlap}:{scale}", B, C, H, W, tile, overlap, scale)
            want = tm.blend(tiles, B, H, W, tile, overlap, scale)
            for so, do in OFFSETS:
                t_store, t_view = _stored(tiles, so)
                t0 = t_store.clone()
                got = _blend_abi(t_view, B, C, H, W, tile, overlap, scale, do)
                assert _same_bits(got, _expect_store(want, do)), (overlap, scale, so, do)
                assert _same_bits(t_store, t0)


@pytest.mark.parametrize("scale", [1, 2])
@pytest.mark.parametrize("overlap", [8, 5])
def test_blend_visits_exactly_the_covering_tiles(overlap, scale):
    """A +inf in one position of one tile reaches exactly one output pixel: a loop that missed the tile would
    leave that pixel finite, a loop that visited a tile too many would spoil another pixel."""
    B, C, H, W, tile = 2, 3, 40, 56, 16
    th, tw, ys, xs = tm.plan(H, W, tile, overlap)
    tiles = _tiles_for(f"tile:inf:{overlap}:{scale}", B, C, H, W, tile, overlap, scale)
    # image 1, tile row 1, tile column 2, channel 1, a position inside the overlap with the neighbours before it
    i, j, c, y, x = 1, 2, 1, 1, 2
    k = (1 * len(ys) + i) * len(xs) + j
    tiles[k, c, y, x] = float("inf")
    Y, X = scale * ys[i] + y, scale * xs[j] + x
    assert tm.cover_count(H, W, tile, overlap)[Y // scale, X // scale] == 4
    want = tm.blend(tiles, B, H, W, tile, overlap, scale)
    assert int((~torch.isfinite(want)).sum()) == 1 and want[1, c, Y, X] == float("inf")
    for so, do in ((0, 0), (1, 2)):
        _, t_view = _stored(tiles, so)
        got = _blend_abi(t_view, B, C, H, W, tile, overlap, scale, do)
        assert _same_bits(got, _expect_store(want, do))
        out = got[G + do:G + do + want.numel()].view(want.shape)
        assert int((~torch.isfinite(out)).sum()) == 1 and float(out[1, c, Y, X]) == float("inf")


@pytest.mark.parametrize("scale", [1, 2])
def test_long_thin_image(scale):
    """8 x 20000, tile 16, overlap 0: 1250 tiles of 8 x 16 side by side, a row of 2 x 20000 floats at scale 2."""
    B, C, H, W, tile, overlap = 1, 1, 8, 20000, 16, 0
    img = torch.from_numpy(hash_images("tile:thin", (B, C, H, W)))
    want_t = tm.gather(img, tile, overlap)
    assert want_t.shape == (1250, 1, 8, 16)
    got_t = tiling.tile_gather(img.to(DEV), tile, overlap)
    assert _same_bits(got_t, want_t.to(DEV))
    tiles = _tiles_for(f"tile:thin:{scale}", B, C, H, W, tile, overlap, scale)
    want = tm.blend(tiles, B, H, W, tile, overlap, scale)
    got = tiling.tile_blend(tiles.to(DEV), B, H, W, tile, overlap, scale)
    assert _same_bits(got, want.to(DEV))
    # overlap 0 and a length that is a multiple of the tile: the blend puts the tiles side by side
    assert torch.equal(want[0, 0, :, :scale * 16], tiles[0, 0])


@pytest.mark.parametrize("vec", [True, False])
def test_more_items_than_one_pass_of_the_grid(vec):
    """The launchers cap the grid at 4096 blocks of 256 threads and loop over the rest: sizes past
    4096 * 256 items (of 4 floats on the float4 path, of 1 float on the scalar path) on both kernels."""
    gen = torch.Generator().manual_seed(5)
    if vec:
        B, C, H, W, tile, overlap = 2, 3, 768, 1024, 512, 64
    else:
        B, C, H, W, tile, overlap = 2, 3, 384, 512, 256, 33
    per_item = 4 if vec else 1
    img = torch.rand((B, C, H, W), generator=gen) * 2 - 1
    want_t = tm.gather(img, tile, overlap)
    assert want_t.numel() // per_item > 4096 * 256 and img.numel() // per_item > 4096 * 256
    got_t = tiling.tile_gather(img.to(DEV), tile, overlap)
    assert _same_bits(got_t, want_t.to(DEV))
    tiles = torch.rand(want_t.shape, generator=gen) * 2 - 1
    want = tm.blend(tiles, B, H, W, tile, overlap)
    got = tiling.tile_blend(tiles.to(DEV), B, H, W, tile, overlap)
    assert _same_bits(got, want.to(DEV))
    assert _same_bits(tiling.tile_blend(tiles.to(DEV), B, H, W, tile, overlap), got)


def test_blend_wrapper_refusals():
    tiles = torch.zeros((30, 3, 16, 16), device=DEV)
    assert tiling.tile_blend(tiles, 2, 40, 56, 16, 4).shape == (2, 3, 40, 56)
    with pytest.raises(RuntimeError, match="expected tiles"):
        tiling.tile_blend(tiles[:29], 2, 40, 56, 16, 4)
    with pytest.raises(RuntimeError, match="scale must be 1 or 2"):
        tiling.tile_blend(tiles, 2, 40, 56, 16, 4, scale=3)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        tiling.tile_blend(tiles, 2, 40, 56, 20, 4)


# ------------------------------------------------------------------ whole model
IH, IW, TILE, OVERLAP = 48, 72, 32, 8


@functools.lru_cache(maxsize=None)
def _model(name, **extra):
    m = KDLAE_teacher(**{**MODELS[name], **extra})
    load_hash_weights(m)
    m.hip_graphs = False
    return m.to(DEV).eval()


def _img(key, m, B, h=IH, w=IW):
    return torch.from_numpy(hash_images(key, (B, m._cfg["inp_channels"], h, w))).to(DEV)


def _rate(kind, B, h=IH, w=IW):
    if kind == "scalar":
        return torch.full((B, 1, h, w), 0.6, device=DEV)
    # a per-pixel ramp, different for every image: a tile that took its rate from the wrong place would differ
    ramp = torch.linspace(0.05, 0.95, h * w, device=DEV).view(1, 1, h, w)
    return torch.cat([ramp if b % 2 == 0 else ramp.flip(-1) * 0.5 for b in range(B)]).contiguous()


def _route(m, img, rate, tile=TILE, overlap=OVERLAP):
    """What a user writes without the feature: slice each tile, run forward on it alone, blend on the CPU."""
    B, _, h, w = img.shape
    th, tw, ys, xs = tm.plan(h, w, tile, overlap)
    hqs, srs = [], []
    with torch.no_grad():
        for b in range(B):
            for y in ys:
                for x in xs:
                    sl = (slice(b, b + 1), slice(None), slice(y, y + th), slice(x, x + tw))
                    o = m({"img": img[sl].contiguous(), "denoise_rate": rate[sl].contiguous() if rate is not None
                           else None})
                    hqs.append(o["hq"].cpu())
                    srs.append(o["sr"].cpu() if o["sr"] is not None else None)
    hq = tm.blend(torch.cat(hqs), B, h, w, tile, overlap, 1)
    sr = tm.blend(torch.cat(srs), B, h, w, tile, overlap, 2) if srs[0] is not None else None
    return hq, sr


@functools.lru_cache(maxsize=None)
def _case(name, kind):
    """(model, img, rate, route hq, route sr), computed once and shared; nothing below writes to them."""
    m = _model(name)
    img, rate = _img(f"tile:m:{name}", m, 2), _rate(kind, 2)
    return (m, img, rate) + _route(m, img, rate)


def _tiled(m, img, rate, tile_batch, tile=TILE, overlap=OVERLAP):
    out = m.forward_tiled({"img": img, "denoise_rate": rate}, tile, overlap, tile_batch)
    return out["hq"], out["sr"]


@pytest.mark.parametrize("kind", ["scalar", "ramp"])
@pytest.mark.parametrize("name", sorted(MODELS))
def test_forward_tiled_equals_the_per_tile_route(name, kind):
    m, img, rate, r_hq, r_sr = _case(name, kind)
    oc = m._cfg["out_channels"]
    assert tuple(tiling.tile_plan(IH, IW, TILE, OVERLAP)) == (32, 32, 2, 3, 24, 24)
    for tile_batch in (1, 3, 16):
        hq, sr = _tiled(m, img, rate, tile_batch)
        assert hq.shape == (2, oc, IH, IW) and sr.shape == (2, oc, 2 * IH, 2 * IW)
        assert torch.equal(hq.cpu(), r_hq), f"hq at tile_batch {tile_batch}"
        assert torch.equal(sr.cpu(), r_sr), f"sr at tile_batch {tile_batch}"
        hq2, sr2 = _tiled(m, img, rate, tile_batch)
        assert torch.equal(hq2, hq) and torch.equal(sr2, sr)
    if kind == "ramp":   # the rate does reach the tiles
        assert not torch.equal(r_hq, _case(name, "scalar")[3])


def test_forward_tiled_with_graph_replay_gives_the_same_bits():
    _, img, rate, r_hq, r_sr = _case("biasfree", "ramp")
    m = KDLAE_teacher(**MODELS["biasfree"])
    load_hash_weights(m)
    m = m.to(DEV).eval()
    assert m.hip_graphs
    # 12 tiles, 4 chunks of 3: the first chunk runs launch by launch, the second captures, the rest replay;
    # a second call replays every chunk
    for _ in range(2):
        hq, sr = _tiled(m, img, rate, 3)
        assert torch.equal(hq.cpu(), r_hq) and torch.equal(sr.cpu(), r_sr)
    assert len(m.__dict__.get("_graphs", {})) == 1
    # 5 + 5 + 2: the tail chunk is a second shape
    hq, sr = _tiled(m, img, rate, 5)
    assert torch.equal(hq.cpu(), r_hq) and torch.equal(sr.cpu(), r_sr)


def test_one_tile_per_image_equals_forward():
    m, img, rate, _, _ = _case("withbias", "ramp")
    with torch.no_grad():
        ref = m({"img": img, "denoise_rate": rate})
    for tile, overlap in ((72, 8), (512, 32), (80, 79)):
        assert tiling.tile_plan(IH, IW, tile, overlap)[2:4] == (1, 1)
        for tile_batch in (1, 16):
            hq, sr = _tiled(m, img, rate, tile_batch, tile, overlap)
            assert torch.equal(hq, ref["hq"]) and torch.equal(sr, ref["sr"])
    # one tile along y only: 48 < 64 clamps th, the x axis still tiles
    assert tuple(tiling.tile_plan(IH, IW, 64, 56)) == (48, 64, 1, 2, 48, 8)
    hq, sr = _tiled(m, img, rate, 16, 64, 56)
    r_hq, r_sr = _route(m, img, rate, 64, 56)
    assert torch.equal(hq.cpu(), r_hq) and torch.equal(sr.cpu(), r_sr)


def test_variants_without_the_rate_input_and_without_the_sr_head():
    plus = _model("biasfree", params="plus")
    img = _img("tile:plus", plus, 2)
    r_hq, r_sr = _route(plus, img, None)
    for rate in (None, _rate("ramp", 2), torch.zeros(1, device=DEV)):   # not read: any value, any shape
        hq, sr = _tiled(plus, img, rate, 3)
        assert torch.equal(hq.cpu(), r_hq) and torch.equal(sr.cpu(), r_sr)
    nosr = _model("biasfree", static="no")
    rate = _rate("ramp", 2)
    r_hq, r_sr = _route(nosr, img, rate)
    hq, sr = _tiled(nosr, img, rate, 16)
    assert sr is None and r_sr is None and torch.equal(hq.cpu(), r_hq)
    both = _model("biasfree", static="no", params="plus")
    hq, sr = _tiled(both, img, None, 5)
    assert sr is None and torch.equal(hq.cpu(), _route(both, img, None)[0])


def test_forward_tiled_refusals():
    m, img, rate, _, _ = _case("biasfree", "scalar")
    before = torch.cuda.memory_allocated()
    for tile, overlap in ((20, 4), (8, 0), (32, 32), (32, -1)):
        with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
            _tiled(m, img, rate, 16, tile, overlap)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        _tiled(m, img[..., :44, :], rate[..., :44, :], 16)
    with pytest.raises(RuntimeError, match="tile_batch"):
        _tiled(m, img, rate, 0)
    with pytest.raises(RuntimeError, match="denoise_rate must be"):
        _tiled(m, img, rate[:1], 16)
    with pytest.raises(RuntimeError, match="denoise_rate must be"):
        _tiled(m, img, None, 16)
    assert torch.cuda.memory_allocated() == before   # refused before the staging is allocated


def test_enhance_tiled_u8_equals_pre_and_post_around_the_route():
    """45 x 70 images: reflect-padded to 48 x 72, tiled, blended, cropped back."""
    m = _model("biasfree")
    B, h, w = 2, 45, 70
    rng = np.random.default_rng(21)
    x = rng.integers(0, 256, (B, h, w, 3), dtype=np.uint8)
    x[:, : h // 3, : w // 4] = 0   # an all-black region: masked in the output
    images = torch.from_numpy(x).to(DEV)
    img, rmap = preprocess_u8(images, 0.6, 8, False)
    assert img.shape == (B, 3, IH, IW)
    r_hq, r_sr = _route(m, img, rmap)
    want_hq = postprocess_u8(r_hq.to(DEV), h, w, 1, images)
    want_sr = postprocess_u8(r_sr.to(DEV), h, w, 2, images)
    for tile_batch in (16, 4):
        hq, sr = enhance_tiled_u8(m, images, 0.6, tile=TILE, tile_overlap=OVERLAP, tile_batch=tile_batch)
        assert hq.dtype == torch.uint8 and hq.shape == (B, h, w, 3) and sr.shape == (B, 2 * h, 2 * w, 3)
        assert torch.equal(hq, want_hq) and torch.equal(sr, want_sr)
    assert bool((hq[:, : h // 3, : w // 4] == 0).all())


# the smallest teacher the training and the inference engine both take (tests/test_validate_gpu.py)
T_CFG = dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, LayerNorm_type="BiasFree")
VH, VW = 45, 70   # pads to 48 x 72


def test_validate_tiled_equals_the_route_and_untiled_is_unchanged():
    m = KDLAE_teacher(**T_CFG)
    load_hash_weights(m)
    tr = KDLAETrainer(m.to(DEV), lr=1e-3, ema_decay=0.999)
    for i in range(2):
        lq = {"img": _img(f"tile:v:img{i}", m, 2, 32, 32), "denoise_rate": torch.full((2, 1, 32, 32), 0.6, device=DEV)}
        gt = {"hq": _img(f"tile:v:hq{i}", m, 2, 32, 32), "sr": _img(f"tile:v:sr{i}", m, 2, 64, 64)}
        tr.optimize_parameters(lq, gt)
    assert not torch.equal(tr.theta, tr.theta_ema)
    items = []
    for i in range(2):
        lq = {"img": _img(f"tile:v:vimg{i}", m, 1, VH, VW), "denoise_rate": _rate("ramp", 1, VH, VW)}
        gt = {"hq": _img(f"tile:v:vhq{i}", m, 1, VH, VW), "sr": _img(f"tile:v:vsr{i}", m, 1, 2 * VH, 2 * VW)}
        items.append((lq, gt))
    # a fresh module with the evaluated (EMA) weights is the reference for both paths
    ref = KDLAE_teacher(**T_CFG)
    ref.load_state_dict({k: v.detach().cpu().clone() for k, v in tr.ema_state_dict().items()})
    ref = ref.to(DEV).eval()
    ref.hip_graphs = False
    tiled, plain = [], []
    for lq, _ in items:
        img = F.pad(lq["img"], (0, IW - VW, 0, IH - VH), "reflect")
        rate = F.pad(lq["denoise_rate"], (0, IW - VW, 0, IH - VH), "reflect")
        hq, sr = _route(ref, img, rate)
        tiled.append((hq[..., :VH, :VW], sr[..., :2 * VH, :2 * VW]))
        with torch.no_grad():
            o = ref({"img": img, "denoise_rate": rate})
        plain.append((o["hq"][..., :VH, :VW].cpu(), o["sr"][..., :2 * VH, :2 * VW].cpu()))

    def psnrs(outs):
        return (np.mean([mo.psnr(o[0][0].numpy(), gt["hq"][0].cpu().numpy()) for (_, gt), o in zip(items, outs)]),
                np.mean([mo.psnr(o[1][0].numpy(), gt["sr"][0].cpu().numpy()) for (_, gt), o in zip(items, outs)]))

    for kw, outs in ((dict(tile=TILE, tile_overlap=OVERLAP, tile_batch=4), tiled), (dict(), plain)):
        for (lq, gt), (r_hq, r_sr) in zip(items, outs):   # item by item: the outputs bit for bit
            tr.validate([(lq, gt)], **kw)
            assert torch.equal(tr.val_output["hq"].cpu(), r_hq) and torch.equal(tr.val_output["sr"].cpu(), r_sr)
        res = tr.validate(items, **kw)
        want_hq, want_sr = psnrs(outs)
        print(f"{kw}: psnr_hq {res['psnr_hq']!r} vs {want_hq!r}; psnr_sr {res['psnr_sr']!r} vs {want_sr!r}")
        # fp64 sums in another order: n * 2^-53 << 1e-9
        assert abs(res["psnr_hq"] - want_hq) <= 1e-9 * abs(want_hq)
        assert abs(res["psnr_sr"] - want_sr) <= 1e-9 * abs(want_sr)
    assert not torch.equal(tiled[0][0], plain[0][0])   # tiling is a different function of the image

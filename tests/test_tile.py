"""Tiled inference (kdlae_tile_plan, kdlae_tile_gather, kdlae_tile_blend): what holds without a GPU.
The header declares and the library exports the entries, the plan equals the CPU model's ranges, every argument
error of the three entries is returned before a launch (the pointers here are never dereferenced), and the CPU
model the GPU tests compare against does what a hand count says."""
import ctypes
import itertools
import os
import re

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, tiling
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from tests import tile_model as tm
from tests.util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kdlae_tile_plan", "kdlae_tile_gather", "kdlae_tile_blend")
P = ctypes.c_void_p(FAKE)
SHAPE, CONFIG = 1, 2

LENGTHS = (16, 24, 40, 56, 72)
TILES = (16, 24, 32, 64)


def _overlaps(tile):
    return sorted({0, 1, 4, 5, 8, tile - 8, tile - 1})


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.kdlae_abi_version() == 1
    for name in ("tile_plan", "tile_gather", "tile_blend"):
        assert callable(getattr(tiling, name))
    assert callable(KDLAE_teacher.forward_tiled)


def _plan(H, W, tile, overlap):
    out = [ctypes.c_int(-7) for _ in range(6)]
    rc = _lib.lib().kdlae_tile_plan(H, W, tile, overlap, *[ctypes.byref(v) for v in out])
    return rc, [v.value for v in out]


@pytest.mark.parametrize("tile", TILES)
def test_plan_equals_the_models_ranges(tile):
    for H, W, overlap in itertools.product(LENGTHS, LENGTHS, _overlaps(tile)):
        rc, (th, tw, ni, nj, sy, sx) = _plan(H, W, tile, overlap)
        assert rc == 0, (H, W, tile, overlap, _lib.last_error())
        m_th, m_tw, ys, xs = tm.plan(H, W, tile, overlap)
        assert (th, tw, ni, nj) == (m_th, m_tw, len(ys), len(xs)), (H, W, tile, overlap)
        # start i is i * stride, the last one L - t
        assert [i * sy for i in range(ni - 1)] + [H - th] == ys, (H, tile, overlap)
        assert [j * sx for j in range(nj - 1)] + [W - tw] == xs, (W, tile, overlap)
        assert sy >= 1 and sx >= 1
        p = tiling.tile_plan(H, W, tile, overlap)
        assert tuple(p) == (th, tw, ni, nj, sy, sx) and p.starts(H, W) == (ys, xs)


def test_plan_of_the_documented_sizes():
    # a 512 x 8000 waterfall keeps 512-wide tiles: the clamp is per axis
    assert tuple(tiling.tile_plan(512, 8000, 512, 32)) == (512, 512, 1, 17, 512, 480)
    assert tuple(tiling.tile_plan(2048, 2048, 512, 32)) == (512, 512, 5, 5, 480, 480)
    assert tuple(tiling.tile_plan(1024, 4096, 512, 32)) == (512, 512, 3, 9, 480, 480)
    # tile >= image: one tile, whatever the overlap
    assert tuple(tiling.tile_plan(48, 72, 512, 500))[:4] == (48, 72, 1, 1)


BAD_PLANS = [dict(tile=20), dict(tile=36), dict(tile=8), dict(tile=0), dict(tile=-16), dict(overlap=-1),
             dict(overlap=16), dict(overlap=17), dict(tile=24, overlap=24), dict(H=20), dict(W=60), dict(H=12, W=12)]


def test_plan_argument_checks():
    ok = dict(H=40, W=56, tile=16, overlap=4)
    assert _plan(**ok)[0] == 0
    for kw in BAD_PLANS:
        a = {**ok, **kw}
        rc, out = _plan(**a)
        assert rc == SHAPE and "kdlae_tile_plan" in _lib.last_error(), kw
        assert out == [-7] * 6   # nothing is written on a refusal
        with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
            tiling.tile_plan(a["H"], a["W"], a["tile"], a["overlap"])
    for kw in (dict(H=0), dict(W=0), dict(H=-8), dict(W=-8)):
        assert _plan(**{**ok, **kw})[0] == CONFIG and "positive" in _lib.last_error(), kw
    # a null result pointer
    L = _lib.lib()
    v = [ctypes.c_int() for _ in range(6)]
    for k in range(6):
        args = [ctypes.byref(x) for x in v]
        args[k] = None
        assert L.kdlae_tile_plan(40, 56, 16, 4, *args) == CONFIG and "null" in _lib.last_error()


def _gather(src=P, B=2, C=3, H=40, W=56, tile=16, overlap=4, first=0, count=1, dst=P):
    return _lib.lib().kdlae_tile_gather(src, B, C, H, W, tile, overlap, first, count, dst, None)


def _blend(tiles=P, B=2, C=3, H=40, W=56, tile=16, overlap=4, scale=1, dst=P):
    return _lib.lib().kdlae_tile_blend(tiles, B, C, H, W, tile, overlap, scale, dst, None)


def test_gather_argument_checks_need_no_launch():
    for kw in (dict(src=None), dict(dst=None)):
        assert _gather(**kw) == CONFIG and "null argument" in _lib.last_error(), kw
    for kw in (dict(B=0), dict(C=0), dict(count=0), dict(B=-1), dict(C=-3), dict(count=-2), dict(first=-1),
               dict(H=0), dict(W=0), dict(H=-8)):
        assert _gather(**kw) == CONFIG, kw
    for kw in BAD_PLANS:
        assert _gather(**kw) == SHAPE and "kdlae_tile_gather" in _lib.last_error(), kw
    # 40 x 56, tile 16, overlap 4: 3 x 5 tiles per image, 30 in all
    rc, (_, _, ni, nj, _, _) = _plan(40, 56, 16, 4)
    assert (ni, nj) == (3, 5)
    for first, count in ((0, 31), (30, 1), (29, 2), (2**31 - 1, 2**31 - 1)):
        assert _gather(first=first, count=count) == CONFIG and "first + count" in _lib.last_error(), (first, count)


def test_blend_argument_checks_need_no_launch():
    for kw in (dict(tiles=None), dict(dst=None)):
        assert _blend(**kw) == CONFIG and "null argument" in _lib.last_error(), kw
    for kw in (dict(B=0), dict(C=0), dict(B=-1), dict(C=-3), dict(H=0), dict(W=0), dict(W=-8)):
        assert _blend(**kw) == CONFIG, kw
    for scale in (0, 3, -1, 4):
        assert _blend(scale=scale) == CONFIG and "scale must be 1 or 2" in _lib.last_error(), scale
    for kw in BAD_PLANS:
        assert _blend(**kw) == SHAPE and "kdlae_tile_blend" in _lib.last_error(), kw


def test_wrappers_and_module_refuse_without_a_device():
    with pytest.raises(RuntimeError, match="cuda float32"):
        tiling.tile_gather(torch.zeros(1, 3, 16, 16), 16, 0)
    with pytest.raises(RuntimeError, match="cuda float32"):
        tiling.tile_blend(torch.zeros(1, 3, 16, 16), 1, 16, 16, 16, 0)
    m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).eval()
    inp = {"img": torch.zeros(1, 3, 16, 24), "denoise_rate": torch.zeros(1, 1, 16, 24)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_tiled(inp, tile=16, tile_overlap=4)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_tiled(inp, tile=16, tile_overlap=4)


# ------------------------------------------------------------------ the CPU model itself
@pytest.mark.parametrize("scale", [1, 2])
def test_model_constant_image_blends_to_the_constant(scale):
    for H, W, tile, overlap in ((40, 56, 16, 5), (40, 56, 16, 8), (24, 72, 24, 16), (56, 40, 16, 12)):
        th, tw, ys, xs = tm.plan(H, W, tile, overlap)
        cover = torch.from_numpy(tm.cover_count(H, W, tile, overlap))
        cover = cover.repeat_interleave(scale, 0).repeat_interleave(scale, 1)
        assert int(cover.max()) >= 3
        # constants with a short significand: k x is exact for every cover k <= 16, and so is (k x) / k
        for value in (1.0, 0.5, -3.75, 2.0 ** -100, 1536.0):
            tiles = torch.full((2 * len(ys) * len(xs), 3, scale * th, scale * tw), value)
            out = tm.blend(tiles, 2, H, W, tile, overlap, scale)
            assert out.shape == (2, 3, scale * H, scale * W)
            assert torch.equal(out, torch.full_like(out, value)), (H, W, tile, overlap, value)
        # a full significand: x + x is exact, so covers of 1 and 2 return x itself; a longer sum rounds at every
        # step and its quotient may be a neighbour of x (k <= 16 roundings of 2^-24 relative each)
        for value in (0.1, -3.7, 1e-30):
            tiles = torch.full((2 * len(ys) * len(xs), 3, scale * th, scale * tw), value)
            out = tm.blend(tiles, 2, H, W, tile, overlap, scale)
            assert bool((out[:, :, cover <= 2] == np.float32(value)).all())
            assert torch.allclose(out, torch.full_like(out, value), rtol=17 * 2.0 ** -24, atol=0)


def test_model_one_tile_plan_is_the_identity():
    x = torch.randn(2, 3, 24, 40, generator=torch.Generator().manual_seed(1))
    for tile, overlap in ((40, 8), (64, 63), (512, 32)):
        t = tm.gather(x, tile, overlap)
        assert t.shape == (2, 3, 24, 40) and torch.equal(t, x)
        assert torch.equal(tm.blend(t, 2, 24, 40, tile, overlap), x)
    up = torch.randn(2, 3, 48, 80, generator=torch.Generator().manual_seed(2))
    assert torch.equal(tm.blend(up, 2, 24, 40, 64, 0, scale=2), up)


def test_model_gather_then_blend_of_an_exactly_summable_image():
    """Small integers sum and divide exactly: blending the tiles of an image gives the image back."""
    x = torch.randint(-8, 9, (2, 3, 40, 56), generator=torch.Generator().manual_seed(3)).float()
    for tile, overlap in ((16, 0), (16, 5), (16, 8), (24, 16), (16, 15)):
        assert torch.equal(tm.blend(tm.gather(x, tile, overlap), 2, 40, 56, tile, overlap), x), (tile, overlap)


def test_model_cover_count_matches_a_hand_count():
    """overlap = tile - 8 with tile 24 on 40 x 56: stride 8.  Starts along y: 0, 8, 16 (range(0, 16, 8) + [16]);
    along x: 0, 8, 16, 24, 32.  Row 0 lies in the first tile only, row 12 in tiles 0 and 1, row 20 in all three;
    column 0 in one tile, column 12 in two, column 28 in three (starts 8, 16, 24)."""
    assert tm.starts(40, 24, 16) == (24, [0, 8, 16]) and tm.starts(56, 24, 16) == (24, [0, 8, 16, 24, 32])
    n = tm.cover_count(40, 56, 24, 16)
    assert n[0, 0] == 1            # corner
    assert n[39, 55] == 1          # the opposite corner
    assert n[0, 28] == 3           # top edge
    assert n[12, 0] == 2           # left edge
    assert n[20, 28] == 9          # interior: 3 x 3
    assert n[12, 12] == 4
    assert n.min() == 1 and n.max() == 9
    # and the blend divides by exactly that count
    th, tw, ys, xs = tm.plan(40, 56, 24, 16)
    ones = torch.ones((len(ys) * len(xs), 1, th, tw))
    assert torch.equal(tm.blend(ones, 1, 40, 56, 24, 16), torch.ones(1, 1, 40, 56))

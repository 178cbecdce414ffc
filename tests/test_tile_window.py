"""Weighted tile blend (kdlae_tile_blend_w, kdlae_tile_blend_rates_w, tiling.tile_window): what holds without a GPU.
The numpy fp32 model the GPU tests compare against (tests/tile_window_model.py) is held against the float64
weighted mean, the named tables against their formulas, the seam a window is there to remove is measured on the
model, the model is tied to the uniform blend's model, every way of getting the rule wrong is shown to change a bit
on the GPU test's own inputs, and every argument error is returned before a launch (the pointers here are never
dereferenced)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, tiling
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher, Restormer
from tests import tile_model as tm
from tests import tile_window_model as twm
from tests.util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("kdlae_tile_blend_w", "kdlae_tile_blend_rates_w")
P = ctypes.c_void_p(FAKE)
SHAPE, CONFIG = 1, 2
U = 2.0 ** -24   # the unit roundoff of fp32


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _kernel_cases():
    """The (C, H, W, tile, overlap, scale) of tests/test_tile_window_gpu.py's model comparison, at C = 3."""
    for H, W in twm.SHAPES:
        for tile in twm.TILES:
            for overlap in twm.overlaps(tile):
                for scale in (1, 2):
                    yield 3, H, W, tile, overlap, scale


def test_header_declares_and_library_exports_the_entry_points():
    src = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    L = _lib.lib()
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name) and name in _lib.EXPORTS, name
    assert L.kdlae_abi_version() == 1   # symbols were only added
    assert callable(tiling.tile_window)


# ------------------------------------------------------------------ the model against the float64 mean
@pytest.mark.parametrize("window", twm.KERNEL_WINDOWS)
def test_fp32_model_against_the_float64_weighted_mean(window):
    """|model - exact| <= (2 cnt + 3) 2^-24 sum(w |o|) / sum(w) where cnt >= 2, equality where cnt == 1.

    Recount of the bound, u = 2^-24, to first order: every term of the numerator carries the rounding of w, the
    rounding of w o and up to cnt - 1 roundings of the adds into E (the first add, to 0, is exact): (cnt + 1) u on
    sum(w |o|).  Every term of the denominator carries the rounding of w and up to cnt - 1 adds into S: cnt u on
    sum(w), which moves the quotient by cnt u |sum(w o)| / sum(w) <= cnt u sum(w |o|) / sum(w).  The division
    adds u.  That is (2 cnt + 2) u; the bound's remaining u holds the second-order terms ((2 cnt + 2)^2 u^2 with
    cnt <= 9 is below 2^-15 u).  The values here are of order 1, nowhere near the subnormal range."""
    worst = 0.0
    for C, H, W, tile, overlap, scale in _kernel_cases():
        tiles = twm.case_tiles(C, H, W, tile, overlap, scale)
        wy, wx = twm.case_tables(window, H, W, tile, overlap, scale)
        got = twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale)
        exact, mean_abs, cnt = twm.blend_exact(tiles, wy, wx, 2, H, W, tile, overlap, scale)
        assert got.dtype == np.float32 and got.shape == exact.shape
        one = np.broadcast_to(cnt == 1, got.shape)
        th, tw, ys, xs = tm.plan(H, W, tile, overlap)
        k = 0
        for b in range(2):   # a pixel under one tile: the mean is the tile's value, and the model's is that, bit for bit
            for y in ys:
                for x in xs:
                    sl = (slice(scale * y, scale * (y + th)), slice(scale * x, scale * (x + tw)))
                    m = cnt[sl] == 1
                    assert np.array_equal(_bits(got[b][(slice(None),) + sl][:, m]), _bits(tiles[k][:, m]))
                    k += 1
        bound = (2 * cnt + 3) * U * mean_abs
        err = np.abs(got.astype(np.float64) - exact)
        many = ~one
        assert bool((err[many] <= bound[many]).all()), (window, H, W, tile, overlap, scale,
                                                        float((err[many] / bound[many]).max()))
        if many.any():
            worst = max(worst, float((err[many] / bound[many]).max()))
    print(f"{window}: largest error over its bound {worst:.3f}")
    assert worst > 0   # the comparison did see pixels under several tiles


# ------------------------------------------------------------------ the named tables
def _cpu_tables(window, H, W, tile, overlap, scale=1):
    t = tiling.tile_window(window, H, W, tile, overlap, scale, device="cpu")
    assert t[0].dtype == torch.float32 and t[1].dtype == torch.float32
    return t[0].numpy(), t[1].numpy()


def test_uniform_has_no_tables():
    assert tiling.tile_window("uniform", 40, 56, 16, 4) is None
    assert tiling.tile_window(None, 40, 56, 16, 4, 2) is None


def test_ramp_tables_are_exact_integers_and_neighbours_cross_fade():
    for H, W in twm.SHAPES + [(2048, 2048)]:
        for tile in twm.TILES + (512,):
            for overlap in twm.overlaps(tile) + [32]:
                if overlap >= tile:
                    continue
                th, tw, ys, xs = tm.plan(H, W, tile, overlap)
                for scale in (1, 2):
                    wy, wx = _cpu_tables("ramp", H, W, tile, overlap, scale)
                    for w, t, n in ((wy, th, len(ys)), (wx, tw, len(xs))):
                        assert w.shape == (scale * t,)                           # doubled length at scale 2
                        assert np.array_equal(w, np.rint(w)) and w.min() >= 1    # integers, exact in fp32
                        assert np.array_equal(w.astype(np.float64), twm.ramp_axis(t, n, overlap, scale))
                        if n == 1:
                            assert np.array_equal(w, np.ones(scale * t, np.float32))
                            continue
                        m = scale * max(overlap, 1)
                        assert w.max() == min(m, scale * t // 2) and np.array_equal(w, w[::-1])
                        if overlap >= 1 and 2 * overlap <= t:
                            # two regular neighbours (starts one stride apart) across their overlap: the left
                            # tile's last m weights plus the right tile's first m are m + 1, a linear cross-fade
                            assert np.array_equal(w[scale * t - m:] + w[:m], np.full(m, m + 1, np.float32))


def test_hann_tables_are_strictly_positive_and_follow_the_formula():
    for t in (16, 24, 48, 72, 512, 1024):
        for scale in (1, 2):
            wy, wx = _cpu_tables("hann", t, t, t, 8, scale)
            assert wy.shape == (scale * t,) and np.array_equal(wy, wx)
            assert wy.min() > 0 and wy.max() <= 1 and np.array_equal(wy, wy[::-1])
            assert np.array_equal(wy, twm.hann_axis(t, scale).astype(np.float32))   # float64, rounded once


def test_a_given_pair_is_checked_and_repeated():
    wy, wx = twm.random_pair(16, 16, 3)
    for scale in (1, 2):
        for conv in (torch.from_numpy, lambda a: torch.from_numpy(a).double()):
            got = tiling.tile_window((conv(wy), conv(wx)), 40, 56, 16, 4, scale, device="cpu")
            assert np.array_equal(got.wy.numpy(), np.repeat(wy, scale))
            assert np.array_equal(got.wx.numpy(), np.repeat(wx, scale))
    # built tables pass through as they are, and only for the plan and scale they were built for
    t2 = tiling.tile_window("ramp", 40, 56, 16, 4, 2, device="cpu")
    assert tiling.tile_window(t2, 40, 56, 16, 4, 2, device="cpu") is t2
    with pytest.raises(RuntimeError, match="tables of lengths"):
        tiling.tile_window(t2, 40, 56, 16, 4, 1, device="cpu")


def test_tile_window_refusals():
    ok = torch.ones(16)
    kw = dict(H=40, W=56, tile=16, tile_overlap=4, device="cpu")
    with pytest.raises(RuntimeError, match="must be one of"):
        tiling.tile_window("triangle", **kw)
    with pytest.raises(RuntimeError, match="must be one of"):
        tiling.tile_window((ok, ok, ok), **kw)
    with pytest.raises(RuntimeError, match="must be one of"):
        tiling.tile_window(3, **kw)
    for bad in (torch.ones(15), torch.ones(17), torch.ones(32), torch.ones(4, 4)):   # wrong lengths
        with pytest.raises(RuntimeError, match="tile's length 16"):
            tiling.tile_window((bad, ok), **kw)
        with pytest.raises(RuntimeError, match="tile's length 16"):
            tiling.tile_window((ok, bad), **kw)
    with pytest.raises(RuntimeError, match="tile's length 16"):   # scale 2 still takes tables of the tile's length
        tiling.tile_window((torch.ones(32), torch.ones(32)), scale=2, **kw)
    for value in (0.0, -1.0, float("nan"), float("inf"), 1e-60):   # 1e-60 is 0 in fp32
        bad = torch.ones(16, dtype=torch.float64)
        bad[5] = value
        with pytest.raises(RuntimeError, match="finite and greater than 0"):
            tiling.tile_window((bad, ok), **kw)
        with pytest.raises(RuntimeError, match="finite and greater than 0"):
            tiling.tile_window((ok, bad), **kw)
    for bad in (torch.ones(16, dtype=torch.int32), torch.ones(16, dtype=torch.bool), [1.0] * 16, np.ones(16)):
        with pytest.raises(RuntimeError, match="floating-point tensor"):
            tiling.tile_window((bad, ok), **kw)
    with pytest.raises(RuntimeError, match="scale must be 1 or 2"):
        tiling.tile_window("ramp", scale=3, **kw)
    with pytest.raises(RuntimeError, match="EINVAL_SHAPE"):
        tiling.tile_window("ramp", 40, 56, 20, 4, device="cpu")


# ------------------------------------------------------------------ the seam
def _largest_step(img):
    """Largest difference between horizontal or vertical neighbours of [H, W]."""
    return max(float(np.abs(np.diff(img, axis=0)).max(initial=0.0)), float(np.abs(np.diff(img, axis=1)).max(initial=0.0)))


def _constant_tiles(values, th, tw):
    return np.stack([np.full((1, th, tw), v, np.float32) for v in values])


def test_seam_of_two_constant_tiles():
    """L = 56, tile 32, overlap 8: starts 0 and 24, tiles 0 and 1.  The uniform blend steps by exactly 1/2 at
    either end of the band; the ramp climbs it in m + 1 steps of 1 / (m + 1)."""
    H, L, tile, m = 32, 56, 32, 8
    assert tm.plan(H, L, tile, m) == (32, 32, [0], [0, 24])
    tiles = _constant_tiles([0.0, 1.0], 32, 32)
    uni = tm.blend(torch.from_numpy(tiles), 1, H, L, tile, m).numpy()[0, 0]
    assert _largest_step(uni) == 0.5
    wy, wx = _cpu_tables("ramp", H, L, tile, m)
    ramp = twm.blend(tiles, wy, wx, 1, H, L, tile, m)[0, 0]
    step = _largest_step(ramp)
    print(f"largest neighbour difference: uniform {_largest_step(uni)!r}, ramp {step!r}")
    assert step <= 1.0 / (m + 1) + 2.0 ** -20
    assert step >= 1.0 / (m + 1) - 2.0 ** -20   # and it is that cross-fade, not something flatter by accident
    assert np.array_equal(ramp[:, :24], np.zeros((32, 24), np.float32))
    assert np.array_equal(ramp[:, 32:], np.ones((32, 24), np.float32))
    # the same along y
    tiles_t = _constant_tiles([0.0, 1.0], 32, 32)
    wy, wx = _cpu_tables("ramp", L, H, tile, m)
    ramp_t = twm.blend(tiles_t, wy, wx, 1, L, H, tile, m)[0, 0]
    assert np.array_equal(_bits(ramp_t), _bits(ramp.T))


SEAM_2D = dict(H=48, W=72, tile=32, overlap=8)
SEAM_VALUES = [0.0, 1.0, 0.25, 0.75, 0.125, 0.5]   # a distinct constant per tile of the 2 x 3 plan


def test_seam_of_a_two_by_three_plan():
    """48 x 72, tile 32, overlap 8: starts (0, 16) x (0, 24, 40), so the last row and the last column overlap their
    neighbours by 16, more than the overlap: the two ramps are joined by a band of equal weights."""
    H, W, tile, m = (SEAM_2D[k] for k in ("H", "W", "tile", "overlap"))
    assert tm.plan(H, W, tile, m) == (32, 32, [0, 16], [0, 24, 40])
    tiles = _constant_tiles(SEAM_VALUES, 32, 32)
    uni = tm.blend(torch.from_numpy(tiles), 1, H, W, tile, m).numpy()[0, 0]
    wy, wx = _cpu_tables("ramp", H, W, tile, m)
    ramp = twm.blend(tiles, wy, wx, 1, H, W, tile, m)[0, 0]
    print(f"largest neighbour difference: uniform {_largest_step(uni)!r}, ramp {_largest_step(ramp)!r}")
    assert _largest_step(ramp) < _largest_step(uni)


# ------------------------------------------------------------------ the link to the uniform blend's model
def test_ones_and_ramp_at_overlap_0_give_the_bits_of_the_uniform_model():
    for C, H, W, tile, overlap, scale in _kernel_cases():
        tiles = twm.case_tiles(C, H, W, tile, overlap, scale)
        want = tm.blend(torch.from_numpy(tiles), 2, H, W, tile, overlap, scale).numpy()
        wy, wx = twm.tables("ones", H, W, tile, overlap, scale)
        assert np.array_equal(_bits(twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale)), _bits(want))
        if overlap == 0 and scale == 1:   # m = 1: min(p + 1, t - p, 1) is 1 everywhere
            wy, wx = _cpu_tables("ramp", H, W, tile, 0)
            assert wy.max() == 1 and wx.max() == 1
            assert np.array_equal(_bits(twm.blend(tiles, wy, wx, 2, H, W, tile, 0)), _bits(want))


# ------------------------------------------------------------------ mutants of the model
def _differs_somewhere(mutant, windows=twm.KERNEL_WINDOWS, need=lambda H, W, tile, overlap: True):
    for C, H, W, tile, overlap, scale in _kernel_cases():
        if not need(H, W, tile, overlap):
            continue
        tiles = twm.case_tiles(C, H, W, tile, overlap, scale)
        for window in windows:
            wy, wx = twm.case_tables(window, H, W, tile, overlap, scale)
            a = twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale)
            b = twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale, mutant=mutant)
            if not np.array_equal(_bits(a), _bits(b)):
                return True
    return False


def _square(H, W, tile, overlap):
    th, tw, _, _ = tm.plan(H, W, tile, overlap)
    return th == tw


@pytest.mark.parametrize("mutant", twm.MUTANTS)
def test_a_mutant_of_the_model_changes_a_bit_on_the_kernel_tests_inputs(mutant):
    """fma in place of mul + add; S summed in reverse tile order; the copy rule dropped; wy and wx swapped (on the
    plans with square tiles); the table read at the image coordinate; the last tile's start taken as i * stride."""
    assert _differs_somewhere(mutant, need=_square if mutant == "swapped" else lambda *a: True)


def test_the_model_is_deterministic():
    C, H, W, tile, overlap, scale = 3, 40, 56, 16, 8, 2
    tiles = twm.case_tiles(C, H, W, tile, overlap, scale)
    wy, wx = twm.case_tables("random", H, W, tile, overlap, scale)
    a = twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale)
    assert np.array_equal(_bits(a), _bits(twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, scale)))


def test_scale_2_ramp_is_not_the_scale_1_ramp_repeated():
    """min(p + 1, 2 t - p, 2 m) climbs in steps of 1 over 2 m pixels; the repeated scale-1 table climbs in steps
    of 1 every two pixels and stops at m: another table, and another blend."""
    differs = False
    for C, H, W, tile, overlap, scale in _kernel_cases():
        if scale != 2:
            continue
        wy, wx = twm.case_tables("ramp", H, W, tile, overlap, 2)
        wy1, wx1 = twm.case_tables("ramp", H, W, tile, overlap, 1)
        ry, rx = np.repeat(wy1, 2), np.repeat(wx1, 2)
        if np.array_equal(wy, ry) and np.array_equal(wx, rx):
            continue   # one tile along both axes: all ones either way
        tiles = twm.case_tiles(C, H, W, tile, overlap, 2)
        a = twm.blend(tiles, wy, wx, 2, H, W, tile, overlap, 2)
        b = twm.blend(tiles, ry, rx, 2, H, W, tile, overlap, 2)
        differs = differs or not np.array_equal(_bits(a), _bits(b))
    assert differs


def test_rates_staging_is_the_rate_sweeps():
    x = torch.arange(2 * 7 * 3 * 4 * 4, dtype=torch.float32).view(2, 7, 3, 4, 4)
    for tb in (1, 3, 7, 9):
        assert torch.equal(twm.from_staged(twm.to_staged(x, tb), 2, 7, 3, 4, 4, tb), x)


# ------------------------------------------------------------------ argument checks without a launch
def _blend_w(tiles=P, B=2, C=3, H=40, W=56, tile=16, overlap=4, scale=1, wy=P, wx=P, dst=P):
    return _lib.lib().kdlae_tile_blend_w(tiles, B, C, H, W, tile, overlap, scale, wy, wx, dst, None)


def _rates_w(staged=P, R=3, B=2, C=3, H=40, W=56, tile=16, overlap=4, tile_batch=4, scale=1, wy=P, wx=P, dst=P):
    return _lib.lib().kdlae_tile_blend_rates_w(staged, R, B, C, H, W, tile, overlap, tile_batch, scale, wy, wx, dst,
                                               None)


BAD_PLANS = [dict(tile=20), dict(tile=8), dict(overlap=-1), dict(overlap=16), dict(H=20), dict(W=60)]


@pytest.mark.parametrize("entry,name", [(_blend_w, "kdlae_tile_blend_w"), (_rates_w, "kdlae_tile_blend_rates_w")])
def test_weighted_entries_check_their_arguments_before_any_launch(entry, name):
    for kw in (dict(wy=None), dict(wx=None), dict(wy=None, wx=None)):
        assert entry(**kw) == CONFIG and name + ": null window table" in _lib.last_error(), kw
    first = "tiles" if entry is _blend_w else "staged"
    for kw in ({first: None}, dict(dst=None)):
        assert entry(**kw) == CONFIG and name + ": null argument" in _lib.last_error(), kw
    for scale in (0, 3, -1, 4):
        assert entry(scale=scale) == CONFIG and name + ": scale must be 1 or 2" in _lib.last_error(), scale
    for kw in (dict(B=0), dict(C=0), dict(B=-1), dict(C=-3), dict(H=0), dict(W=-8)):
        assert entry(**kw) == CONFIG, kw
    for kw in BAD_PLANS:
        assert entry(**kw) == SHAPE and name + ":" in _lib.last_error(), kw


def test_weighted_rates_entry_checks_r_and_tile_batch():
    for R in (0, -1, 65, 1000):
        assert _rates_w(R=R) == CONFIG and "need 1 <= R <= 64" in _lib.last_error(), R
    for tb in (0, -4):
        assert _rates_w(tile_batch=tb) == CONFIG and "tile_batch" in _lib.last_error(), tb


def test_wrappers_and_modules_take_the_keyword_and_refuse_without_a_device():
    with pytest.raises(RuntimeError, match="cuda float32"):
        tiling.tile_blend(torch.zeros(1, 3, 16, 16), 1, 16, 16, 16, 0, window="ramp")
    with pytest.raises(RuntimeError, match="cuda float32"):
        tiling.tile_blend_rates(torch.zeros(3 * 16 * 16), 1, 1, 16, 16, 16, 0, window="hann")
    m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).eval()
    inp = {"img": torch.zeros(1, 3, 16, 24), "denoise_rate": torch.zeros(1, 1, 16, 24)}
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_tiled(inp, tile=16, tile_overlap=4, window="ramp")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_rates_tiled(inp["img"], [0.5], tile=16, tile_overlap=4, window="ramp")
    r = Restormer(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).eval()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        r.forward_tiled(inp["img"], tile=16, tile_overlap=4, window="hann")

"""Tiled rate sweep (kdlae_tile_blend_rates, tiling.tile_blend_rates, KDLAE_teacher.forward_rates_tiled,
pipeline.enhance_rates_tiled_u8 / enhance_auto_tiled_u8): what holds without a GPU.  The header declares and the
library exports the entry, the CPU model of the staging layout (tests/tile_rates_model.py) round-trips and agrees
with the offsets the header states, and every argument error of the entry is returned before a launch (the
pointers here are never dereferenced)."""
import ctypes
import os
import re

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib, pipeline, tiling
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher, Restormer
from tests import tile_rates_model as trm
from tests.test_tile import BAD_PLANS
from tests.util import FAKE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = ctypes.c_void_p(FAKE)
SHAPE, CONFIG = 1, 2
N = 12                               # tiles of the GPU tests' sweep case (2 images of 2 x 3 tiles)
TILE_BATCHES = (1, 4, 5, N, N + 3)   # one tile a chunk, a divisor of n, a non-divisor, n, more than n


def test_header_declares_and_library_exports_the_entry_point():
    src = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    L = _lib.lib()
    assert re.search(r"\bkdlae_tile_blend_rates\s*\(", src)
    assert hasattr(L, "kdlae_tile_blend_rates") and "kdlae_tile_blend_rates" in _lib.EXPORTS
    assert L.kdlae_abi_version() == 1
    assert callable(tiling.tile_blend_rates) and callable(KDLAE_teacher.forward_rates_tiled)
    assert callable(pipeline.enhance_rates_tiled_u8) and callable(pipeline.enhance_auto_tiled_u8)


@pytest.mark.parametrize("tile_batch", TILE_BATCHES)
def test_layout_model_round_trips_and_matches_the_stated_offsets(tile_batch):
    R, C, h, w = 3, 2, 4, 6
    T = C * h * w
    # every element names its own (r, tile, position): nothing can move unnoticed
    x = torch.arange(R * N * T, dtype=torch.float32).view(R, N, C, h, w)
    flat = trm.to_staged(x, tile_batch)
    assert flat.shape == (R * N * T,)
    assert torch.equal(trm.from_staged(flat, R, N, C, h, w, tile_batch), x)
    # chunks: count_k = min(tile_batch, n - k tile_batch), back to back, so chunk k starts where the chunks
    # before it end; that running sum is the header's k tile_batch R T
    ch = trm.chunks(N, tile_batch)
    assert [f for f, _ in ch] == list(range(0, N, tile_batch))
    assert all(c == min(tile_batch, N - k * tile_batch) for k, (_, c) in enumerate(ch))
    assert sum(c for _, c in ch) == N
    pos = 0
    for k, (first, count) in enumerate(ch):
        assert trm.chunk_offset(k, tile_batch, R, T) == pos == first * R * T
        for r in range(R):
            for q in range(count):
                off = trm.tile_offset(first + q, r, N, tile_batch, R, T)
                assert off == pos + (r * count + q) * T
                assert torch.equal(flat[off:off + T].view(C, h, w), x[r, first + q])
        pos += R * count * T
    assert pos == flat.numel()
    if tile_batch >= N:   # one chunk: the buffer is [R][n][C][h][w] itself
        assert torch.equal(flat, x.reshape(-1))
    if tile_batch == 1:   # one tile a chunk: [n][R][C][h][w]
        assert torch.equal(flat, x.transpose(0, 1).reshape(-1))


@pytest.mark.parametrize("tile_batch", TILE_BATCHES)
def test_staged_slots_match_the_layout_model(tile_batch):
    """tiling.staged_slots (the chosen rate's tiles, as enhance_auto_tiled_u8 selects them for the sr head)."""
    R, B, per = 3, 2, N // 2
    for index in ([0, 0], [2, 1], [1, 2]):
        slots = tiling.staged_slots(torch.tensor(index, dtype=torch.int32), per, R, tile_batch)
        assert slots.dtype == torch.int64
        want = [trm.tile_offset(t, index[t // per], N, tile_batch, R, 1) for t in range(B * per)]
        assert slots.tolist() == want


def _blend_rates(staged=P, R=3, B=2, C=3, H=40, W=56, tile=16, overlap=4, tile_batch=5, scale=1, dst=P):
    return _lib.lib().kdlae_tile_blend_rates(staged, R, B, C, H, W, tile, overlap, tile_batch, scale, dst, None)


def test_blend_rates_argument_checks_need_no_launch():
    for kw in (dict(staged=None), dict(dst=None)):
        assert _blend_rates(**kw) == CONFIG and "null argument" in _lib.last_error(), kw
    for R in (0, 65, -1, 1 << 20):
        assert _blend_rates(R=R) == CONFIG and "1 <= R <= 64" in _lib.last_error(), R
    for kw in (dict(B=0), dict(C=0), dict(tile_batch=0), dict(B=-1), dict(C=-3), dict(tile_batch=-16)):
        assert _blend_rates(**kw) == CONFIG and "tile_batch" in _lib.last_error(), kw
    for scale in (0, 3, -1, 4):
        assert _blend_rates(scale=scale) == CONFIG and "scale must be 1 or 2" in _lib.last_error(), scale
    # plan errors come through make_plan unchanged
    for kw in (dict(H=0), dict(W=0), dict(W=-8)):
        assert _blend_rates(**kw) == CONFIG and "positive" in _lib.last_error(), kw
    for kw in BAD_PLANS:
        assert _blend_rates(**kw) == SHAPE and "kdlae_tile_blend_rates" in _lib.last_error(), kw


def test_wrappers_and_modules_refuse_without_a_device():
    with pytest.raises(RuntimeError, match="cuda float32"):
        tiling.tile_blend_rates(torch.zeros(30 * 3 * 3 * 16 * 16), 3, 2, 40, 56, 16, 4, 5)
    m = KDLAE_teacher(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).eval()
    img = torch.zeros(1, 3, 16, 24)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m.forward_rates_tiled(img, [0.5], tile=16, tile_overlap=4)
    m.train()
    with pytest.raises(RuntimeError, match="eval"):
        m.forward_rates_tiled(img, [0.5], tile=16, tile_overlap=4)
    r = Restormer(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1).eval()
    with pytest.raises(RuntimeError, match="no denoise_rate input"):
        r.forward_rates_tiled(img, [0.5])

"""CPU model of the staging layout of a tiled rate sweep (include/kdlae.h, kdlae_tile_blend_rates).

``kdlae_t_forward_rates`` at batch ``count`` writes ``[R][count][C][h][w]``.  Run over ``n`` tiles ``tile_batch`` at
a time, chunk after chunk into one buffer, it leaves the chunks back to back: chunk ``k`` holds tiles
``k * tile_batch ... k * tile_batch + count_k - 1`` as ``[R][count_k][C][h][w]``.  The model below builds that buffer
by concatenating the chunks and never uses the closed-form offsets, which ``chunk_offset`` / ``tile_offset`` state
separately so that a test can hold one against the other."""
import torch


def chunks(n: int, tile_batch: int):
    """[(first tile, count)] of the sweep's chunks."""
    return [(first, min(tile_batch, n - first)) for first in range(0, n, tile_batch)]


def to_staged(x: torch.Tensor, tile_batch: int) -> torch.Tensor:
    """[R, n, C, h, w] -> the flat chunk-major buffer."""
    n = x.shape[1]
    return torch.cat([x[:, first:first + count].contiguous().reshape(-1) for first, count in chunks(n, tile_batch)])


def from_staged(flat: torch.Tensor, R: int, n: int, C: int, h: int, w: int, tile_batch: int) -> torch.Tensor:
    """The flat chunk-major buffer -> [R, n, C, h, w]."""
    assert flat.numel() == R * n * C * h * w, (flat.numel(), R, n, C, h, w)
    out, pos = torch.empty((R, n, C, h, w), dtype=flat.dtype), 0
    for first, count in chunks(n, tile_batch):
        size = R * count * C * h * w
        out[:, first:first + count] = flat[pos:pos + size].view(R, count, C, h, w)
        pos += size
    return out


def chunk_offset(k: int, tile_batch: int, R: int, T: int) -> int:
    """Float offset of chunk k; T = floats of one staged tile (C s^2 th tw)."""
    return k * tile_batch * R * T


def tile_offset(t: int, r: int, n: int, tile_batch: int, R: int, T: int) -> int:
    """Float offset of tile t (flat index) at rate r."""
    k = t // tile_batch
    count_k = min(tile_batch, n - k * tile_batch)
    return chunk_offset(k, tile_batch, R, T) + (r * count_k + (t - k * tile_batch)) * T

"""CPU model of tiled inference, written as the demo loop of upstream Restormer (``--tile`` / ``--tile_overlap``):
the start ranges, ``E`` and ``W`` accumulators, ``add_`` per tile in index order and a true fp32 division.  The
only departures are the ones the library documents: the tile is clamped per axis (``th = min(tile, H)``,
``tw = min(tile, W)``) and an axis the tile covers whole has the single start 0 whatever the overlap.

Tile ``(b, i, j)`` has flat index ``(b * ni + i) * nj + j``."""
import numpy as np
import torch


def starts(L: int, tile: int, overlap: int):
    """Tile starts along an axis of length L -> (t, list of starts)."""
    t = min(tile, L)
    if L == t:
        return t, [0]
    return t, list(range(0, L - t, t - overlap)) + [L - t]


def plan(H: int, W: int, tile: int, overlap: int):
    """(th, tw, ys, xs)"""
    th, ys = starts(H, tile, overlap)
    tw, xs = starts(W, tile, overlap)
    return th, tw, ys, xs


def gather(img: torch.Tensor, tile: int, overlap: int) -> torch.Tensor:
    """[B,C,H,W] -> every tile by slicing, [B*ni*nj, C, th, tw] in flat-index order."""
    B, C, H, W = img.shape
    th, tw, ys, xs = plan(H, W, tile, overlap)
    return torch.stack([img[b, :, y:y + th, x:x + tw] for b in range(B) for y in ys for x in xs])


def blend(tiles: torch.Tensor, B: int, H: int, W: int, tile: int, overlap: int, scale: int = 1) -> torch.Tensor:
    """tiles [B*ni*nj, C, scale*th, scale*tw] (CPU fp32) -> [B, C, scale*H, scale*W]: E.add_, W.add_, E.div_(W)."""
    th, tw, ys, xs = plan(H, W, tile, overlap)
    tiles = tiles.to(torch.float32)
    C = tiles.shape[1]
    assert tuple(tiles.shape) == (B * len(ys) * len(xs), C, scale * th, scale * tw), tuple(tiles.shape)
    E = torch.zeros((B, C, scale * H, scale * W), dtype=torch.float32)
    Wt = torch.zeros_like(E)
    k = 0
    for b in range(B):
        for y in ys:
            for x in xs:
                sl = (b, slice(None), slice(scale * y, scale * (y + th)), slice(scale * x, scale * (x + tw)))
                E[sl].add_(tiles[k])
                Wt[sl].add_(1)
                k += 1
    return E.div_(Wt)


def cover_count(H: int, W: int, tile: int, overlap: int) -> np.ndarray:
    """Number of tiles over each pixel, int [H, W]."""
    th, tw, ys, xs = plan(H, W, tile, overlap)
    n = np.zeros((H, W), np.int64)
    for y in ys:
        for x in xs:
            n[y:y + th, x:x + tw] += 1
    return n

"""The algebra of the sr head's fold (csrc/sr_fold.hip, csrc/pack.hip pack_fold_kernel), without a GPU.

cen (3x3, padding 1, bias) followed by upen.body.0 (3x3, padding 1, no bias) is one 5x5 conv with padding 2,
except on the one-pixel image border: upen zero-pads cen's OUTPUT, so an upen tap that lands outside the
image contributes nothing.  `compose` builds the 9 border-class weight sets and biases in float64 the way the
pack kernel does; applied as a per-class 5x5 conv they must reproduce the float64 two-conv chain.
tests/test_sr_fold_gpu.py imports `compose` and `apply_classes` as its statement of the record's contents."""
import numpy as np
import torch
import torch.nn.functional as F


def valid_taps(cls):
    """The upen taps of a row / column class that land inside the image: 0 first, 1 interior, 2 last."""
    return {0: (1, 2), 1: (0, 1, 2), 2: (0, 1)}[cls]


def compose(U, Cw, Cb=None):
    """U [O][M][3][3] (upen), Cw [M][C][3][3] (cen), Cb [M] or None, float64 ->
    W [9][O][C][5][5], bias [9][O]; class = 3 * row class + column class."""
    U, Cw = np.asarray(U, np.float64), np.asarray(Cw, np.float64)
    O, C = U.shape[0], Cw.shape[1]
    W = np.zeros((9, O, C, 5, 5))
    bias = np.zeros((9, O))
    for rc in range(3):
        for cc in range(3):
            k = 3 * rc + cc
            for dy in valid_taps(rc):
                for dx in valid_taps(cc):
                    # sum over m of U[o][m][dy][dx] * Cw[m][c][ey][ex] lands on tap (dy + ey, dx + ex)
                    W[k, :, :, dy:dy + 3, dx:dx + 3] += np.einsum("om,mcyx->ocyx", U[:, :, dy, dx], Cw)
                    if Cb is not None:
                        bias[k] += U[:, :, dy, dx] @ np.asarray(Cb, np.float64)
    return W, bias


def apply_classes(W, bias, x):
    """x [B][C][H][W] float64 -> [B][O][H][W]: every pixel's class set applied as a 5x5 conv, padding 2."""
    Wt, bt = torch.from_numpy(W), torch.from_numpy(bias)
    B, _, H, Wd = x.shape
    out = torch.empty(B, W.shape[1], H, Wd, dtype=torch.float64)
    rows = torch.ones(H, dtype=torch.long)
    rows[0], rows[-1] = 0, 2
    cols = torch.ones(Wd, dtype=torch.long)
    cols[0], cols[-1] = 0, 2
    cls = 3 * rows[:, None] + cols[None, :]
    for k in range(9):
        y = F.conv2d(x, Wt[k], bt[k], padding=2)
        m = (cls == k)[None, None]
        out = torch.where(m, y, out)
    return out


def chain(U, Cw, Cb, x):
    """The two convs as the model runs them, float64."""
    cb = None if Cb is None else torch.from_numpy(np.asarray(Cb, np.float64))
    return F.conv2d(F.conv2d(x, torch.from_numpy(np.asarray(Cw, np.float64)), cb, padding=1),
                    torch.from_numpy(np.asarray(U, np.float64)), None, padding=1)


def _case(seed, O, M, C, with_bias):
    g = np.random.default_rng(seed)
    U = g.standard_normal((O, M, 3, 3))
    Cw = g.standard_normal((M, C, 3, 3))
    Cb = g.standard_normal(M) if with_bias else None
    return U, Cw, Cb


def test_composed_classes_equal_the_two_conv_chain():
    for seed, (C, with_bias) in enumerate([(3, True), (3, False), (1, True), (4, True)]):
        U, Cw, Cb = _case(seed, 8, 6, C, with_bias)
        x = torch.from_numpy(np.random.default_rng(100 + seed).standard_normal((2, C, 6, 7)))
        W, b = compose(U, Cw, Cb)
        got, ref = apply_classes(W, b, x), chain(U, Cw, Cb, x)
        rel = float((got - ref).abs().max() / ref.abs().max())
        assert rel <= 1e-12, (C, with_bias, rel)


def test_border_classes_matter():
    """The interior set alone is wrong on the border ring and right inside it: the classes are not vacuous."""
    U, Cw, Cb = _case(7, 8, 6, 3, True)
    x = torch.ones(1, 3, 6, 7, dtype=torch.float64)
    W, b = compose(U, Cw, Cb)
    ref = chain(U, Cw, Cb, x)
    plain = F.conv2d(x, torch.from_numpy(W[4]), torch.from_numpy(b[4]), padding=2)
    err = (plain - ref).abs()
    assert float(err[:, :, 1:-1, 1:-1].max()) <= 1e-12 * float(ref.abs().max())
    assert float(err[:, :, 0].max()) > 1e-3 and float(err[:, :, :, -1].max()) > 1e-3

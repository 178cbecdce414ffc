"""Plain torch restatements of the training steps' non-GEMM kernels (train.hip, train_dwg.hip,
train_small.hip, train_s.hip), one short function each: no tiling, no tricks.  Every function
computes in the dtype of its arguments, so tests/test_train_kernels_gpu.py evaluates the same formula
in float64 (the reference) and in float32 (the measure of what fp32 rounding alone costs);
tests/test_train_kernel_refs.py proves the closed-form backwards against float64 autograd.

Activations are channels-last like the kernels' views: [B, H, W, C] (KDLAE-T) and [B, F, H, W, C]
(KDLAE-S), here without any row padding.
"""
import math

import torch
import torch.nn.functional as F

# F.normalize's eps as the kernels hold it (a float32 constant)
NORM_EPS = float(torch.tensor(1e-12, dtype=torch.float32))


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


# ------------------------------------------------------------------ depthwise 3x3 and the GDFN gate
def dwconv(x, w, b=None, flip=False):
    """out[p, c] = sum_t w[c, t] x[p + off_t, c] (+ b[c]), zero padding 1; flip: w[c, 8 - t].
    x [B, H, W, C], w [C, 9] (taps row-major)."""
    C = x.shape[-1]
    k = w.reshape(C, 1, 3, 3)
    if flip:
        k = k.flip(2, 3)
    return _nhwc(F.conv2d(_nchw(x), k, b, padding=1, groups=C))


def gate(yd):
    """g = gelu_erf(x1) * x2 with x1, x2 the two channel halves of yd."""
    x1, x2 = yd.chunk(2, dim=-1)
    return F.gelu(x1, approximate="none") * x2


def gate_bwd(dg, yd):
    """d(yd) of g = gelu(x1) * x2 for an upstream dg: [dg x2 gelu'(x1) | dg gelu(x1)]."""
    x1, x2 = yd.chunk(2, dim=-1)
    cdf = 0.5 * (1 + torch.erf(x1 / math.sqrt(2.0)))
    pdf = torch.exp(-0.5 * x1 * x1) / math.sqrt(2.0 * math.pi)
    return torch.cat([dg * x2 * (cdf + x1 * pdf), dg * x1 * cdf], dim=-1)


def dwconv_bwd(dyd, yin, w):
    """Backward of yd = dwconv(yin, w, b): (d yin, dw [C, 9], db [C])."""
    B, H, W, C = yin.shape
    dy = dwconv(dyd, w, flip=True)
    xp = F.pad(yin, (0, 0, 1, 1, 1, 1))
    dw = torch.stack([(dyd * xp[:, t // 3:t // 3 + H, t % 3:t % 3 + W]).sum((0, 1, 2)) for t in range(9)], dim=1)
    return dy, dw, dyd.sum((0, 1, 2))


def conv3_weight_grad(dy, x, dil):
    """dW [Cout, Cin, 3, 3] of a dense 3x3 conv (dilation = padding = dil): dy [B, H, W, Cout], x [B, H, W, Cin]."""
    shape = (dy.shape[-1], x.shape[-1], 3, 3)
    return torch.nn.grad.conv2d_weight(_nchw(x).contiguous(), shape, _nchw(dy).contiguous(), padding=dil, dilation=dil)


# ------------------------------------------------------------------ MDTA core
def _norms(sumsq, heads, Ch, eps):
    B, C = sumsq.shape[0], heads * Ch
    nq = sumsq[:, :C].reshape(B, heads, Ch).sqrt().clamp_min(eps)
    nk = sumsq[:, C:].reshape(B, heads, Ch).sqrt().clamp_min(eps)
    return nq[..., :, None] * nk[..., None, :]


def attn_core(G, sumsq, temp, eps=NORM_EPS):
    """A = softmax(t G / (max(sqrt(sq), eps) max(sqrt(sk), eps)^T)): G [B, heads, Ch, Ch], sumsq [B, 2 C]
    (q then k), temp [heads]."""
    heads, Ch = G.shape[1], G.shape[2]
    return torch.softmax(temp[None, :, None, None] * G / _norms(sumsq, heads, Ch, eps), dim=-1)


def attn_core_bwd(G, sumsq, temp, A, dA, eps=NORM_EPS):
    """(Mq, cq, ck, dtemp_part) as train_kernels.h defines them: Mq = dL/dG, cq / ck = 2 dL/dsumsq
    (0 where the norm was clamped), dtemp_part [B, heads] the per-image temperature gradient."""
    B, heads, Ch, _ = G.shape
    C = heads * Ch
    nn_ = _norms(sumsq, heads, Ch, eps)
    Gh = G / nn_
    dS = A * (dA - (A * dA).sum(-1, keepdim=True))
    dGh = temp[None, :, None, None] * dS
    E = dGh * Gh
    sq = sumsq[:, :C].reshape(B, heads, Ch)
    sk = sumsq[:, C:].reshape(B, heads, Ch)
    zero = torch.zeros((), dtype=G.dtype)
    cq = torch.where(sq.sqrt() >= eps, -E.sum(-1) / sq, zero)
    ck = torch.where(sk.sqrt() >= eps, -E.sum(-2) / sk, zero)
    return dGh / nn_, cq, ck, (dS * Gh).sum((-1, -2))


# ------------------------------------------------------------------ layout
def unshuffle(x):
    """PixelUnshuffle(2): [B, 2h, 2w, C] -> [B, h, w, 4 C]."""
    return _nhwc(F.pixel_unshuffle(_nchw(x), 2))


def shuffle(x):
    """PixelShuffle(2): [B, h, w, 4 C] -> [B, 2h, 2w, C]."""
    return _nhwc(F.pixel_shuffle(_nchw(x), 2))


def pack_w3(W, mode):
    """[9 Cg, N] implicit-GEMM operand of a 3x3 OIHW weight: mode 2 B(t Cg + c, n) = W[n][c][t] (W [N, Cg, 3, 3]);
    mode 3 B(t Cg + c, n) = W[c][n][8 - t] (W [Cg, N, 3, 3])."""
    if mode == 2:
        N, Cg = W.shape[:2]
        return W.reshape(N, Cg, 9).permute(2, 1, 0).reshape(9 * Cg, N)
    Cg, N = W.shape[:2]
    return W.reshape(Cg, N, 9).flip(-1).permute(2, 0, 1).reshape(9 * Cg, N)


# ------------------------------------------------------------------ KDLAE-S
def maxpool2_bwd(inp, dout, dskip=None):
    """MaxPool3d (1, 2, 2) backward: dout [B, F, h, w, C] goes to the first maximum (row, column order) of
    each 2 x 2 window of inp [B, F, 2h, 2w, C]; + dskip."""
    win = [inp[:, :, i::2, j::2] for i in (0, 1) for j in (0, 1)]
    mx, am = win[0], torch.zeros_like(win[0], dtype=torch.long)
    for k in (1, 2, 3):
        up = win[k] > mx
        mx = torch.where(up, win[k], mx)
        am = torch.where(up, torch.full_like(am, k), am)
    din = torch.zeros_like(inp) if dskip is None else dskip.clone()
    for k, (i, j) in enumerate([(0, 0), (0, 1), (1, 0), (1, 1)]):
        din[:, :, i::2, j::2] += dout * (am == k)
    return din


_TAPS = [(t // 9, (t // 3) % 3, t % 3) for t in range(27)]


def im2col3d(x):
    """Xcol[p, tap * C + c] = x[p + off(tap), c], zero padding 1 in frames, rows and columns:
    [B, F, H, W, C] -> [B, F, H, W, 27 C]."""
    B, Fr, H, W, C = x.shape
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 1, 1))
    return torch.cat([xp[:, a:a + Fr, b:b + H, c:c + W] for a, b, c in _TAPS], dim=-1)


def col2im3d(dcol):
    """The adjoint of im2col3d: dx[q, c] = sum_tap dcol[q - off(tap), tap * C + c]."""
    B, Fr, H, W, K = dcol.shape
    C = K // 27
    dxp = torch.zeros(B, Fr + 2, H + 2, W + 2, C, dtype=dcol.dtype)
    for t, (a, b, c) in enumerate(_TAPS):
        dxp[:, a:a + Fr, b:b + H, c:c + W] += dcol[..., t * C:(t + 1) * C]
    return dxp[:, 1:-1, 1:-1, 1:-1]


def wperm(w):
    """Conv3d weight [O, C, 27] -> [O, 27, C] (the column order)."""
    return w.transpose(1, 2).contiguous()


def relu_mask(dy, y):
    return dy * (y > 0)


def upshuffle_add(U, bias, skip):
    """ConvTranspose3d (1, 2, 2) stride (1, 2, 2) scatter: D[b, f, 2y + i, 2x + j, o] = U[b, f, y, x, 4 o + 2 i + j]
    (+ bias[o]) + skip."""
    B, Fr, h, w, C4 = U.shape
    C = C4 // 4
    D = U.reshape(B, Fr, h, w, C, 2, 2).permute(0, 1, 2, 5, 3, 6, 4).reshape(B, Fr, 2 * h, 2 * w, C)
    if bias is not None:
        D = D + bias
    return D + skip

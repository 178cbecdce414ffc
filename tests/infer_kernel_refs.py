"""Plain torch restatements of the inference kernels that kdlae_debug_infer launches (gdfn.hip, ffn.hip,
mdta_fused.hip, mdta.hip's fold and gate, conv_lds.hip, conv_small.hip, conv3d_c16.hip,
asdqe_kernels.hip), one short function each: no tiling, no tricks.  Every function computes in the
dtype of its arguments, so tests/test_infer_kernels_gpu.py evaluates the same formula in float64 (the
reference) and, where a bound has to be measured, in float32; tests/test_infer_kernel_refs.py proves
them against the oracles and round-trips the layout helpers.

Activations are channels-last like the kernels' views: [B, H, W, C] ([B, F, H, W, C] for the 3-D
convs), without row padding.  Gate-family tensors of 2 hid channels are in natural order [x1 | x2]
unless a helper says "interleaved".
"""
import torch
import torch.nn.functional as F

# F.normalize's eps as the fold kernel holds it (a float32 constant)
NORM_EPS = float(torch.tensor(1e-12, dtype=torch.float32))


def _nchw(x):
    return x.permute(0, 3, 1, 2)


def _nhwc(x):
    return x.permute(0, 2, 3, 1)


# ------------------------------------------------------------------ layouts
def chunk_interleave(t, dim=-1):
    """Natural [x1 (hid) | x2 (hid)] along `dim` -> chunk-interleaved (gdfn.hip): chunk g of 16 hidden
    channels holds x1 at [32 g, 32 g + 16) and x2 at [32 g + 16, 32 g + 32)."""
    t = t.movedim(dim, -1)
    hid = t.shape[-1] // 2
    out = t.reshape(*t.shape[:-1], 2, hid // 16, 16).transpose(-3, -2).reshape(*t.shape[:-1], 2 * hid)
    return out.movedim(-1, dim)


def chunk_deinterleave(t, dim=-1):
    t = t.movedim(dim, -1)
    hid = t.shape[-1] // 2
    out = t.reshape(*t.shape[:-1], hid // 16, 2, 16).transpose(-3, -2).reshape(*t.shape[:-1], 2 * hid)
    return out.movedim(-1, dim)


def dw_blocks(wdw, bdw=None):
    """Depthwise weights [2 hid][9] (natural channel order, taps row-major) and bias [2 hid] -> the per-chunk
    blocks [hid / 16][512] of gdfn.hip: weight of tap t, half h, channel c at 32 t + 16 h + c, bias at
    288 + 16 h + c, zero pad."""
    hid = wdw.shape[0] // 2
    blk = wdw.new_zeros(hid // 16, 512)
    w = wdw.reshape(2, hid // 16, 16, 9).permute(1, 3, 0, 2)            # [g][t][h][c]
    blk[:, :288] = w.reshape(hid // 16, 288)
    if bdw is not None:
        blk[:, 288:320] = bdw.reshape(2, hid // 16, 16).transpose(0, 1).reshape(hid // 16, 32)
    return blk


def dw_blocks_decode(blk):
    """Inverse of dw_blocks: (wdw [2 hid][9], bdw [2 hid])."""
    n = blk.shape[0]
    w = blk[:, :288].reshape(n, 9, 2, 16).permute(2, 0, 3, 1).reshape(2 * n * 16, 9)
    b = blk[:, 288:320].reshape(n, 2, 16).transpose(0, 1).reshape(2 * n * 16)
    return w, b


def pack_fragments(Wmat, ntiles, kgroups):
    """[N][K] -> the f32 fragment order (runtime.h pack_fragments): element (l, e) of record (t, g) is
    W(16 t + l % 16, 16 g + 4 (l / 16) + e); zero past N / K."""
    Wp = Wmat.new_zeros(ntiles * 16, kgroups * 16)
    Wp[:Wmat.shape[0], :Wmat.shape[1]] = Wmat
    return Wp.view(ntiles, 16, kgroups, 4, 4).permute(0, 2, 3, 1, 4).contiguous().view(-1)


def unpack_fragments(flat, ntiles, kgroups):
    return flat.view(ntiles, kgroups, 4, 16, 4).permute(0, 3, 1, 2, 4).reshape(ntiles * 16, kgroups * 16)


def gram_to_acc(G):
    """Gram [..., Ch, Ch] -> the MFMA accumulator order of `reduced` (kdlae.h kdlae_debug_gram): element
    (i CT + j) 256 + 4 l + e = G[16 i + 4 (l / 16) + e][16 j + l % 16]."""
    Ch = G.shape[-1]
    CT = Ch // 16
    lead = G.shape[:-2]
    t = G.reshape(*lead, CT, 4, 4, CT, 16)                              # [i][lq][e][j][li]
    n = len(lead)
    return t.permute(*range(n), n, n + 3, n + 1, n + 4, n + 2).reshape(*lead, Ch * Ch)


def acc_to_gram(acc, Ch):
    CT = Ch // 16
    lead = acc.shape[:-1]
    t = acc.reshape(*lead, CT, CT, 4, 16, 4)                            # [i][j][lq][li][e]
    n = len(lead)
    return t.permute(*range(n), n, n + 2, n + 4, n + 1, n + 3).reshape(*lead, Ch, Ch)


def pack_reduced(G, nq, nk):
    """[..., Ch, Ch], [..., Ch], [..., Ch] -> reduced [..., Ch^2 + 2 Ch]."""
    return torch.cat([gram_to_acc(G), nq, nk], dim=-1)


def unpack_reduced(red, Ch):
    return acc_to_gram(red[..., :Ch * Ch], Ch), red[..., Ch * Ch:Ch * Ch + Ch], red[..., Ch * Ch + Ch:]


def split_records_decode(rec, ntiles, kgroups):
    """Split records (mfma3.h) as a float32 tensor of ntiles * ceil(kgroups / 2) * 768 floats -> float64
    [16 ntiles][32 ceil(kgroups / 2)]: element (n, k) is bf16 j = 4 (kk >> 4) + (kk & 3) of lane
    (n & 15) + 16 ((kk & 15) >> 2), kk = k & 31, summed over the three planes of record (n >> 4, k >> 5)."""
    kpt = (kgroups + 1) // 2
    p = rec.contiguous().view(torch.bfloat16).view(ntiles, kpt, 3, 4, 16, 2, 4).double().sum(2)
    return p.permute(0, 3, 1, 4, 2, 5).reshape(16 * ntiles, 32 * kpt)   # [t][nl][G][hi][q][e]


def split_records_encode(M, ntiles, kgroups):
    """float32 [16 ntiles][<= 16 kgroups] -> split records (float32 carrier), an odd last k-group paired with
    zeros: x = h + m + l with h = bf16(x), m = bf16(x - h), l = bf16(x - h - m)."""
    kpt = (kgroups + 1) // 2
    x = M.new_zeros(16 * ntiles, 32 * kpt, dtype=torch.float32)
    x[:, :M.shape[1]] = M.float()
    h = x.bfloat16()
    r1 = x - h.float()
    m = r1.bfloat16()
    lo = (r1 - m.float()).bfloat16()
    planes = torch.stack([h, m, lo])                                    # [3][n][k]
    t = planes.view(3, ntiles, 16, kpt, 2, 4, 4)                        # [pl][t][nl][G][hi][q][e]
    t = t.permute(1, 3, 0, 5, 2, 4, 6).contiguous()                     # [t][G][pl][q][nl][hi][e]
    return t.view(-1).view(torch.float32)


# ------------------------------------------------------------------ operations
def layer_norm(x, mode):
    """Unit-weight LayerNorm over channels: mode 1 BiasFree x / sqrt(var + eps), 2 WithBias (x - mean) / ..."""
    mu = x.mean(-1, keepdim=True)
    var = ((x - mu) ** 2).mean(-1, keepdim=True)
    return (x - mu) / torch.sqrt(var + 1e-5) if mode == 2 else x / torch.sqrt(var + 1e-5)


def dwconv(x, w, b=None):
    """out[p, c] = sum_t w[c, t] x[p + off_t, c] (+ b[c]), zero padding 1.  x [B, H, W, C], w [C, 9]."""
    C = x.shape[-1]
    return _nhwc(F.conv2d(_nchw(x), w.reshape(C, 1, 3, 3), b, padding=1, groups=C))


def gate(yd):
    x1, x2 = yd.chunk(2, dim=-1)
    return F.gelu(x1, approximate="none") * x2


def gdfn_tail(y, wdw, bdw, Wout, bout=None, R=None):
    """R + project_out(gelu(dw(y1)) * dw(y2)): y [B, H, W, 2 hid], wdw [2 hid][9], Wout [C][hid]."""
    out = gate(dwconv(y, wdw, bdw)) @ Wout.t()
    if bout is not None:
        out = out + bout
    return out if R is None else out + R


def ffn_half(x, ln, Win, bin_, wdw, bdw, Wout, bout=None):
    """x + gdfn(LN(x)) (KDLAE_model.py:161, :95-106): Win [2 hid][C] (LN weight folded in), bin_ [2 hid]."""
    y = layer_norm(x, ln) @ Win.t()
    if bin_ is not None:
        y = y + bin_
    return gdfn_tail(y, wdw, bdw, Wout, bout, x)


def mdta_pass1(x, ln, Wqkv, bqkv, wdw, bdw):
    """[q | k | v] = dwconv(qkv(LN(x))); single head: v [B, H, W, C], G = q k^T [B, C, C] over the pixels,
    |q_c|^2, |k_c|^2 [B, C]."""
    B, H, W, C = x.shape
    y = layer_norm(x, ln) @ Wqkv.t()
    if bqkv is not None:
        y = y + bqkv
    y = dwconv(y, wdw, bdw)
    q, k, v = (t.reshape(B, H * W, C) for t in y.chunk(3, dim=-1))
    return v.reshape(B, H, W, C), q.transpose(1, 2) @ k, (q * q).sum(1), (k * k).sum(1)


def attn_fold(G, nq, nk, proj, temp):
    """Softmax of the normalised Gram folded into project_out (KDLAE_model.py:137-144): G [B, heads, Ch, Ch],
    nq / nk [B, heads, Ch] squared norms, proj [C][C], temp [heads] -> M [B][C][C] with
    M[n][h Ch + c2] = sum_c1 proj[n][h Ch + c1] A_h[c1][c2]."""
    B, heads, Ch, _ = G.shape
    iq = 1.0 / nq.sqrt().clamp_min(NORM_EPS)
    ik = 1.0 / nk.sqrt().clamp_min(NORM_EPS)
    A = torch.softmax(G * iq[..., :, None] * ik[..., None, :] * temp.view(1, heads, 1, 1), dim=-1)
    Wh = proj.reshape(proj.shape[0], heads, Ch)
    return torch.einsum("nhc,bhcd->bnhd", Wh, A).reshape(B, proj.shape[0], heads * Ch)


def dwconv_gate(x, w, b=None):
    """x [B, H, W, 2 hid] natural order, w [9][2 hid] tap-major (mdta.hip dwconv_gate) -> [B, H, W, hid]."""
    return gate(dwconv(x, w.t(), b))


def conv_nhwc(x, w, bias=None, relu=False):
    """3x3 / 1x1 Conv2d (x [B, H, W, Cin], w [Cout, Cin, k, k]) or 3x3x3 / 1x3x3 Conv3d (x [B, F, H, W, Cin],
    w [Cout, Cin, kt, 3, 3]), zero padding 'same'."""
    if x.dim() == 4:
        y = _nhwc(F.conv2d(_nchw(x), w, bias, padding=w.shape[-1] // 2))
    else:
        y = F.conv3d(x.permute(0, 4, 1, 2, 3), w, bias, padding=(w.shape[2] // 2, 1, 1)).permute(0, 2, 3, 4, 1)
    return torch.relu(y) if relu else y


def pixel_unshuffle(y):
    """[B, H, W, N] -> [B, H/2, W/2, 4 N], channel 4 n + 2 (y & 1) + (x & 1) (KDLAE_model.py:186-187)."""
    return _nhwc(F.pixel_unshuffle(_nchw(y), 2))


def pixel_shuffle(y):
    """[B, H, W, N] -> [B, 2H, 2W, N/4]: output n -> pixel (2y + (n >> 1 & 1), 2x + (n & 1)), channel n >> 2."""
    return _nhwc(F.pixel_shuffle(_nchw(y), 2))


def conv_transposed_weight(w):
    """The [Cin][Cout][3][3] weight of the conv whose transpose a `wt` launch computes -> the equivalent
    forward weight [Cout][Cin][3][3] (taps flipped)."""
    return w.transpose(0, 1).flip(2, 3)


def maxpool2(x):
    """[N, H, W, C] -> [N, H // 2, W // 2, C] (floor)."""
    return _nhwc(F.max_pool2d(_nchw(x), 2))


def gap_head(y, wo, bo, w1, b1, w2, b2, w3, b3):
    """ASDQE regressor with outc folded ahead of the pool (ASDQE_model.py:109, :144-154): y [B, HW, C]."""
    f = F.linear(y.mean(1), wo, bo)
    h = torch.relu(F.linear(f, w1, b1))
    h = torch.relu(F.linear(h, w2, b2))
    return torch.tanh(F.linear(h, w3.view(1, -1), b3)).view(-1)

"""Structured operands, bounds and a CPU model for the precision tests of the split-bf16 matrix
products (csrc/mfma3.h).  Needs no GPU; imported by tests/test_gemm_precision_inputs.py (which proves
on the model that the bounds separate the six-term scheme from every five-term one) and by
tests/test_gemm_precision_gpu.py (which holds the shipped kernels to the same bounds).

The contract under test: every fp32 operand is split exactly into three bf16 planes x = h + m + l, and
per 32-deep k pair six of the nine plane products are accumulated into an fp32 accumulator in the
order (l,h) (m,m) (m,h) (h,l) (h,m) (h,h) (weight plane first).

Two input classes make the low-order terms visible:

* one-hot: every output element receives at most one nonzero product, so nothing can cancel or hide
  a wrong plane: a lost (h,l) / (l,h) / (m,m) term moves the result by ~2^-18 of the product;
* coherent: dense operands whose every plane is positive, so the low-order terms of all K products
  add up instead of cancelling.

All errors are measured as max |got - ref| / den, where den is the reference function applied to the
absolute values of every operand (sum |a||w| + |bias| + |rs R|).
"""
import math

import torch

# (weight plane, activation plane) in mfma6's order
SIX = (("l", "h"), ("m", "m"), ("m", "h"), ("h", "l"), ("h", "m"), ("h", "h"))

U = 2.0 ** -24                      # unit roundoff of fp32
# One product: six accumulator roundings of at most 2^-24 each, the three dropped plane products total
# less than 2^-25, bias / residual / store add at most a few more of the same size: 8 u.  A lost kept
# term is ~2^-18.
ONE_HOT_BOUND = 2.0 ** -21


# the contraction lengths of the coherent class: tests/test_gemm_precision_inputs.py proves for each
# that the model separates, and coherent_bound refuses any other, so no GPU case can use an unproven K
COHERENT_KS = (32, 40, 48, 64, 80, 96)


def coherent_bound(K, chunks=1):
    """Six accumulator roundings per 32-deep pair, one per partial sum a chunked / split-K kernel
    adds, and 4 for bias, residual, per-column scale and the final store."""
    assert K in COHERENT_KS, f"coherent class at K = {K}: separation not proven"
    return (6 * math.ceil(K / 32) + chunks + 4) * U


def f32_bound(K, chunks=1):
    """The f32-MFMA kernels: an fp32 fma chain rounds once per k."""
    return (K + chunks + 4) * U


# ------------------------------------------------------------------------------------- the split
def split3_ref(x):
    """The planes of fp32 `x` exactly as mfma3.h split1 computes them (bf16 round to nearest even of
    the fp32 remainders), as float64."""
    assert x.dtype == torch.float32
    h = x.to(torch.bfloat16).float()
    r1 = x - h
    m = r1.to(torch.bfloat16).float()
    r2 = r1 - m
    l = r2.to(torch.bfloat16).float()
    return h.double(), m.double(), l.double()


# ------------------------------------------------------------------------------------- operands
def piece_operand(shape, seed, positive):
    """fp32-exact values (h + m + l) 2^e: h in [1, 2) with 8 significant bits, |m| in [2^-10, 2^-8)
    with 8, |l| in [2^-19, 2^-17) with at most 4 (below half an ulp of m, so split1 finds these very
    planes when all are positive), e in [-3, 3].  positive: every piece and value positive; else
    random signs on m, l and the value."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    shape = tuple(shape) if isinstance(shape, (tuple, list, torch.Size)) else (shape,)

    def ri(lo, hi):
        return torch.randint(lo, hi, shape, generator=g, dtype=torch.int64).double()

    h = 1 + ri(0, 128) / 128
    em = ri(-10, -8)
    m = (1 + ri(0, 128) / 128) * torch.exp2(em)
    # e_m = -10: ulp(m) = 2^-17, so l stays below 2^-18; e_m = -9: l in [2^-19, 2^-17)
    el = torch.where(em == -10, torch.full_like(em, -19), ri(-19, -17))
    l = (1 + ri(0, 8) / 8) * torch.exp2(el)
    e = ri(-3, 4)
    if positive:
        s = torch.ones(shape, dtype=torch.float64)
    else:
        m = m * (2 * ri(0, 2) - 1)
        l = l * (2 * ri(0, 2) - 1)
        s = 2 * ri(0, 2) - 1
    x = (h + m + l) * torch.exp2(e) * s
    out = x.float()
    assert torch.equal(out.double(), x), "piece_operand: not exact in fp32"
    return out


def one_hot_rows(P, K, seed, positive=False):
    """[P][K] activations with exactly one nonzero piece operand per row, at column p mod K: with
    P >= K every k index is hit — both halves of every 32-deep pair and the last, odd k-group."""
    assert P >= K
    A = torch.zeros(P, K)
    p = torch.arange(P)
    A[p, p % K] = piece_operand(P, seed, positive)
    return A


def one_hot_pixels(P, M, N, seed):
    """For a contraction over pixels, C(m, n) = sum_p A[p][m] B[p][n]: [P][M] and [P][N] operands such
    that every (m, n) meets exactly one pixel where both are nonzero.  With P = a b, A[p][m] != 0 iff
    m % a == p % a and B[p][n] != 0 iff n % b == p // a."""
    a = 16
    assert P % a == 0
    b = P // a
    p = torch.arange(P)
    A = piece_operand((P, M), seed, False) * (torch.arange(M)[None, :] % a == (p % a)[:, None])
    B = piece_operand((P, N), seed + 1, False) * (torch.arange(N)[None, :] % b == (p // a)[:, None])
    both = (A != 0).double().T @ (B != 0).double()
    assert bool((both == 1).all())
    return A, B


def conv_taps(kt):
    """(dt, dy, dx) of the k order tap * Cin + c."""
    return [(dt, dy, dx) for dt in (range(-1, 2) if kt == 3 else (0,)) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]


def conv_lattice(Bn, Fr, H, W, Cin, dil, kt, seed, positive=False, cover=None):
    """[Bn][Fr][H][W][Cin] activations for the implicit 3x3 (kt 1) / 3x3x3 (kt 3) convs: nonzero pixels
    on a spatial (kt 3: and temporal, pitch 3) lattice of pitch 2 dil + 1, one nonzero channel each,
    the channel stepping through 0 .. Cin - 1.  Two lattice points are further apart than a filter
    reaches, so every output pixel receives at most one nonzero product; the taps and channels hit
    inside the image cover all 9 kt Cin k indices (asserted; `cover` = a smaller number of k indices
    that an image too small for Cin lattice points must still reach)."""
    pitch = 2 * dil + 1
    x = torch.zeros(Bn, Fr, H, W, Cin)
    frames = range(1, Fr, 3) if kt == 3 else range(Fr)
    pts = [(b, f, y, xx) for b in range(Bn) for f in frames for y in range(dil, H, pitch) for xx in range(dil, W, pitch)]
    vals = piece_operand(len(pts), seed, positive)
    hit = torch.zeros(9 * kt, Cin, dtype=torch.bool)
    for i, (b, f, y, xx) in enumerate(pts):
        c = i % Cin
        x[b, f, y, xx, c] = vals[i]
        for t, (dt, dy, dx) in enumerate(conv_taps(kt)):
            # the output pixel that sees this point through tap t
            if 0 <= f - dt < Fr and 0 <= y - dy * dil < H and 0 <= xx - dx * dil < W:
                hit[t, c] = True
    assert int(hit.sum()) >= (hit.numel() if cover is None else cover), \
        f"lattice covers {int(hit.sum())} of {hit.numel()} k indices"
    return x


def im2col(x, dil, kt):
    """[Bn][Fr][H][W][Cin] -> [pixels][9 kt Cin] with k = tap * Cin + c and zero padding (padding =
    dilation spatially, 1 temporally for kt 3; kt 1: every frame on its own)."""
    Bn, Fr, H, W, Cin = x.shape
    xp = torch.nn.functional.pad(x, (0, 0, dil, dil, dil, dil, 1, 1))
    cols = [xp[:, 1 + dt:1 + dt + Fr, dil + dy * dil:dil + dy * dil + H, dil + dx * dil:dil + dx * dil + W, :]
            for dt, dy, dx in conv_taps(kt)]
    return torch.stack(cols, dim=4).reshape(Bn * Fr * H * W, 9 * kt * Cin)


# ------------------------------------------------------------------------------------- reference
def ref_den(A, Wt, bias=None, R=None, rs=None):
    """float64 A Wt^T + bias + rs R, and the same function of the absolute values."""
    def f(a, w, b, r, s):
        y = a @ w.T
        if b is not None:
            y = y + b
        if r is not None:
            y = y + (r if s is None else s * r)
        return y
    d = lambda t: None if t is None else t.double()
    a = lambda t: None if t is None else t.double().abs()
    return f(d(A), d(Wt), d(bias), d(R), d(rs)), f(a(A), a(Wt), a(bias), a(R), a(rs))


def rel_err(got, ref, den):
    """max |got - ref| / den over the elements with den > 0; an element with den == 0 must be 0."""
    got = got.double()
    nz = den > 0
    assert bool((got[~nz] == 0).all()), "nonzero output where every operand is zero"
    if not bool(nz.any()):
        return 0.0
    return ((got - ref).abs()[nz] / den[nz]).max().item()


# ------------------------------------------------------------------------------------- the model
def emulate_mfma6(A, Wt, terms=SIX, bias=None, R=None, rs=None):
    """The contract on the CPU: out[p][n] = sum_k A[p][k] Wt[n][k].  Per 32-deep k pair (K padded with
    zeros) and per term of `terms` in order, one plane product (exact, in float64) is added to the
    accumulator, which is rounded to fp32 once per MFMA.  bias, then rs R, are added in fp32.
    `terms` with one entry left out is the model of a kernel that drops that term."""
    A, Wt = A.float(), Wt.float()
    K = A.shape[1]
    Kp = (K + 31) // 32 * 32
    Ap = dict(zip("hml", (torch.nn.functional.pad(t, (0, Kp - K)) for t in split3_ref(A))))
    Wp = dict(zip("hml", (torch.nn.functional.pad(t, (0, Kp - K)) for t in split3_ref(Wt))))
    acc = torch.zeros(A.shape[0], Wt.shape[0], dtype=torch.float64)
    for G in range(Kp // 32):
        k = slice(32 * G, 32 * G + 32)
        for wp, ap in terms:
            acc = (acc + Ap[ap][:, k] @ Wp[wp][:, k].T).float().double()
    out = acc.float()
    if bias is not None:
        out = out + bias.float()
    if R is not None:
        out = out + (R.float() if rs is None else rs.float() * R.float())
    return out


# ------------------------------------------------------------------------------------- cases
def coherent_case(P, K, N, seed, with_r=True):
    """Dense all-positive A [P][K], Wt [N][K], bias [N] and (with_r) residual R [P][N]: every plane
    product, the bias and the residual have the same sign."""
    A = piece_operand((P, K), seed, True)
    Wt = piece_operand((N, K), seed + 1, True)
    bias = piece_operand(N, seed + 2, True)
    R = piece_operand((P, N), seed + 3, True) if with_r else None
    return A, Wt, bias, R


def one_hot_case(P, K, N, seed, with_r=True):
    """One-hot A [P][K] (column p mod K), dense random-sign Wt [N][K], bias and residual."""
    A = one_hot_rows(P, K, seed)
    Wt = piece_operand((N, K), seed + 1, False)
    bias = piece_operand(N, seed + 2, False)
    R = piece_operand((P, N), seed + 3, False) if with_r else None
    return A, Wt, bias, R

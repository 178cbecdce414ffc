"""The shipped matrix-product kernels held to the accuracy csrc/mfma3.h claims for the split-bf16
scheme (as accurate as an fp32 fma chain), on inputs where a lost or misplaced low-order term shows.

The loose kernel-level bound of the variant tests (1e-5 (max|ref| + 1) sqrt(K) / 4 on dense uniform
data) lets a kernel that drops one of the six plane products, reads the l plane of a wrong record or
mis-splits one weight plane pass.  Here every case uses one of the two structured input classes of
tests/gemm_precision_inputs.py and err = max |got - ref| / den <= c, with ref the float64 product
plus bias and residual, den the same function of the absolute values of every operand, and c derived
from the number formats alone:

* one-hot / conv lattice (at most one nonzero product per output): c = 2^-21;
* coherent (dense, every plane positive, K <= 96): c = (6 ceil(K / 32) + chunks + 4) 2^-24, chunks =
  the partial sums a split-K kernel adds;
* the f32-MFMA kernels (tiled training GEMM, MDTA Gram), one-hot only: c = (K + chunks + 4) 2^-24
  with K = 1, the one nonzero product (adding exact zeros does not round).

tests/test_gemm_precision_inputs.py proves on a CPU model that the six-term scheme meets these
bounds and every five-term scheme misses them, for each class and K used here.

Covered: every entry of the four variant tables of the inference implicit-GEMM family
(kdlae_debug_gemm), the training rows / cols / tiled kernels (kdlae_debug_tgemm), conv_lds and
conv3d_c16 (kdlae_debug_infer ops 5 and 7), the MDTA Gram (kdlae_debug_gram), and bit-exact
invariance under scaling the operands by 2^40 and 2^-40.

Out of scope: the inner products of the fused kernels (ffn.hip, gdfn.hip, mdta_fused.hip) and the
attn_fold records.  Their activation operand is produced inside the kernel by fp32 elementwise code,
so it cannot be constructed piece by piece.
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_precision_inputs as G
from test_infer_kernels_gpu import _call as _infer, _conv_lds_weights
from test_kernel_variants_gpu import _run as _tgemm
from test_kernel_variants_infer_gpu import (ATTN, CHUNK2, CONV, RES2, GemmDesc, GramDesc, _call, _res2_hasr_ok,
                                            _resident_group, pack_fragments)

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAD = 7.0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _dev(t):
    return None if t is None else t.to(DEV)


def _check(name, got, ref, den, bound):
    """err = max |got - ref| / den <= bound; prints the ratio before it asserts."""
    got = got.detach().cpu()
    assert torch.isfinite(got).all(), f"{name}: non-finite output"
    err = G.rel_err(got, ref, den)
    print(f"RATIO {name} {err / bound:.4f}")
    assert err <= bound, f"{name}: max |err| / den {err:.3e} > {bound:.3e}"


def _wide(t, pad, fill=0.0):
    """t [..., C] as the first C columns of a [..., C + pad] buffer."""
    buf = torch.full((*t.shape[:-1], t.shape[-1] + pad), fill, dtype=t.dtype)
    buf[..., :t.shape[-1]] = t
    return buf


def _live_groups(kgroups):
    """The coherent class keeps K <= 96: with more k-groups only the last 6 (5 when kgroups is odd, the
    last one then pairs with zeros) carry nonzero activations — three 32-deep pairs either way."""
    n = kgroups if kgroups <= 6 else (5 if kgroups % 2 else 6)
    return list(range(kgroups - n, kgroups))


# =========================================================================== inference implicit GEMM
BN, H_, W_ = 2, 16, 32


def _gemm(name, NT, KG, c3, out_mode, route, cls, kgroups, ntiles, group_tiles=0, with_r=False, dil=1, kt=1,
          seed=0):
    """One kdlae_debug_gemm launch (ln 0, bias, optional residual) of the forced tile shape on one of
    the structured classes: 'onehot' (1x1), 'coherent' (1x1) or 'lattice' (3x3 / 3x3x3)."""
    Fr = 3 if kt == 3 else 1
    HW = Fr * H_ * W_
    P = BN * HW
    K = 16 * kgroups
    cg = kgroups // (9 * kt) if c3 else 0
    Cin = 16 * cg if c3 else K
    N = 16 * ntiles - (4 if out_mode == 2 else 0)
    pos = cls == "coherent"
    if cls == "onehot":
        A = G.one_hot_rows(P, K, seed)
        cols, bound = A, G.ONE_HOT_BOUND
    elif cls == "coherent":
        live = _live_groups(kgroups)
        A = torch.zeros(P, K)
        A[:, 16 * live[0]:] = G.piece_operand((P, 16 * len(live)), seed, True)
        cols, bound = A, G.coherent_bound(16 * len(live))
    else:
        x = G.conv_lattice(BN, Fr, H_, W_, Cin, dil, kt, seed)
        A = x.reshape(P, Cin)
        cols, bound = G.im2col(x, dil, kt), G.ONE_HOT_BOUND
    Wt = G.piece_operand((N, K), seed + 1, pos)
    bias = G.piece_operand(N, seed + 2, pos)
    ref, den = G.ref_den(cols, Wt, bias)

    def geo(y):   # [P][N] -> the store geometry, NHWC rows
        if out_mode == 0:
            return y
        y = y.view(BN * Fr, H_, W_, N).permute(0, 3, 1, 2)
        y = F.pixel_unshuffle(y, 2) if out_mode == 1 else F.pixel_shuffle(y, 2)
        return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])
    ref, den = geo(ref), geo(den)
    Nout = ref.shape[1]
    ldo = Nout + 4
    Rd = None
    if with_r:
        R = G.piece_operand((ref.shape[0], Nout), seed + 3, pos)
        ref, den = ref + R.double(), den + R.double().abs()
        Rd = _wide(R, 4).to(DEV)
    lda = Cin + (3 if route == 1 else 4)     # route 1: the ld % 4 != 0 view of the production fallback
    Ad = _wide(A, lda - Cin, 3.0).to(DEV)
    biasd = torch.zeros(16 * ntiles, device=DEV)
    biasd[:N] = bias.to(DEV)
    Wp = pack_fragments(Wt.to(DEV), ntiles, kgroups)
    out = torch.full((ref.shape[0], ldo), PAD, device=DEV)
    _call("kdlae_debug_gemm", GemmDesc, A=_ptr(Ad), lda=lda, Bn=BN, F=Fr, H=H_, W=W_, ksize=3 if c3 else 1, kt=kt,
          dil=dil, cg_per_tap=cg, kgroups=kgroups, Wp=_ptr(Wp), ntiles=ntiles, N=N, bias=_ptr(biasd), out=_ptr(out),
          ldo=ldo, R=_ptr(Rd), ldr=ldo, ln=0, ln_C=K, relu=0, out_mode=out_mode, NT=NT, KG=KG, wpe=2,
          group_tiles=group_tiles, route=route)
    _check(name, out[:, :Nout], ref, den, bound)
    assert bool((out[:, Nout:] == PAD).all()), f"{name}: wrote past its {Nout} columns"


def _chunked_kgroups(KG, cls):
    """1x1, chunked schedule.  An odd KG runs K in one chunk (split pairs may not straddle k-chunks);
    an even KG takes two chunks with an odd, ragged total (the last k-group pairs with zeros).  The
    coherent class keeps K <= 96: the largest odd count <= 5 that still needs its schedule."""
    if KG % 2:
        return KG
    return 2 * KG - 1 if cls == "onehot" else min(2 * KG - 1, 5)


def _c3_kgroups(kt, dil):
    """3x3 / 3x3x3: 32 channels at dilation 1, 16 at dilation 2 (the lattice of pitch 5 has 36 points)."""
    return 9 * kt * (2 if dil == 1 else 1)


@pytest.mark.parametrize("v", CONV, ids=[f"nt{v[0]}_kg{v[1]}_c{v[2]}_o{v[3]}_pf{v[4]}_res{v[6]}" for v in CONV])
def test_conv_gemm_precision(v):
    """route 1, conv_gemm_kernel<NT, KG, CONV3, OUT, PF, WPE, RES>, bias + residual.  1x1: one-hot over
    1024 pixels (every k hit) and coherent; resident variants over two weight groups, chunked ones over
    two k-chunks with an odd k-group total.  3x3: the lattice at dilation 1 and 2 through the variant's
    store mode; the (2, 4) plain variant also as 3x3x3."""
    NT, KG, c3, out_mode, pf, wpe, res = v
    i = CONV.index(v)
    tag = f"conv_gemm nt{NT} kg{KG} c{c3} o{out_mode}"
    if res:
        gt = _resident_group(NT, KG)
        nt = 2 * gt - 1 if gt > 1 else 2
        for cls in ("onehot", "coherent"):
            _gemm(f"{tag} res {cls}", NT, KG, False, 0, 1, cls, KG, nt, group_tiles=gt, with_r=True, seed=10 * i)
    elif c3:
        for dil in (1, 2):
            _gemm(f"{tag} lattice dil{dil}", NT, KG, True, out_mode, 1, "lattice", _c3_kgroups(1, dil), 2 * NT + 1,
                  with_r=True, dil=dil, seed=10 * i + dil)
        if (NT, KG, out_mode) == (2, 4, 0):
            _gemm(f"{tag} lattice 3d", NT, KG, True, 0, 1, "lattice", _c3_kgroups(3, 1), 2 * NT + 1, kt=3, seed=10 * i + 3)
    else:
        for cls in ("onehot", "coherent"):
            _gemm(f"{tag} {cls}", NT, KG, False, out_mode, 1, cls, _chunked_kgroups(KG, cls), 2 * NT + 1,
                  with_r=out_mode == 0, seed=10 * i)


@pytest.mark.parametrize("v", RES2, ids=[f"nt{v[0]}_kg{v[1]}_nch{v[2]}" for v in RES2])
def test_gemm_res_precision(v):
    """route 0, gemm_res_kernel<NT, KG, NCH, 2, HASR, PF>: (NCH - 1) NT + 1 tiles per group, two weight
    groups; with the residual where the variant has that instance.  One-hot and coherent."""
    NT, KG, NCH = v[:3]
    i = RES2.index(v)
    gt = (NCH - 1) * NT + 1
    nt = 2 * gt - 1 if gt > 1 else 2
    for cls in ("onehot", "coherent"):
        _gemm(f"gemm_res nt{NT} kg{KG} nch{NCH} {cls}", NT, KG, False, 0, 0, cls, KG, nt, group_tiles=gt,
              with_r=_res2_hasr_ok(NT, KG, NCH), seed=1000 + 10 * i)


@pytest.mark.parametrize("v", CHUNK2, ids=[f"nt{v[0]}_kg{v[1]}_c{v[2]}_o{v[3]}" for v in CHUNK2])
def test_gemm_chunk_precision(v):
    """route 0, gemm_chunk_kernel<NT, KG, CONV3, OUT, HASR>: as test_conv_gemm_precision; the residual
    on the plain 1x1 store where the instance exists (NT KG < 36) and on the shuffled 3x3 stores."""
    NT, KG, c3, out_mode = v[:4]
    i = CHUNK2.index(v)
    tag = f"gemm_chunk nt{NT} kg{KG} c{c3} o{out_mode}"
    if c3:
        for dil in (1, 2):
            _gemm(f"{tag} lattice dil{dil}", NT, KG, True, out_mode, 0, "lattice", _c3_kgroups(1, dil), 2 * NT + 1,
                  with_r=out_mode != 0, dil=dil, seed=2000 + 10 * i + dil)
        if (NT, KG, out_mode) == (2, 4, 0):
            _gemm(f"{tag} lattice 3d", NT, KG, True, 0, 0, "lattice", _c3_kgroups(3, 1), 2 * NT + 1, kt=3,
                  seed=2000 + 10 * i + 3)
    else:
        for cls in ("onehot", "coherent"):
            _gemm(f"{tag} {cls}", NT, KG, False, out_mode, 0, cls, _chunked_kgroups(KG, cls), 2 * NT + 1,
                  with_r=out_mode == 0 and NT * KG < 36, seed=2000 + 10 * i)


@pytest.mark.parametrize("cls", ["onehot", "coherent"])
@pytest.mark.parametrize("v", ATTN, ids=[f"nt{v[0]}_kg{v[1]}_nch{v[2]}" for v in ATTN])
def test_gemm_attn_in_precision(v, cls):
    """gemm_attn_in_kernel<NT, KG, NCH>: the per-image M GEMM probed with structured v, out1 = x + M v +
    bias_m.  The kernel normalises x1 before the second GEMM whatever `ln` says (it has no LN-free
    form), so its operand cannot be built piece by piece: out1 only is checked, and the project_in
    weights are covered by the resident kernels that share mfma_chunk3."""
    NT, KG, NCH = v[:3]
    seed = 3000 + 10 * ATTN.index(v)
    K, HW = 16 * KG, H_ * W_
    ntiles = (NCH - 1) * NT + 1
    N = 16 * ntiles
    pos = cls == "coherent"
    if pos:
        vv, bound = G.piece_operand((BN * HW, K), seed, True), G.coherent_bound(K)
    else:
        vv, bound = G.one_hot_rows(BN * HW, K, seed), G.ONE_HOT_BOUND
    M = G.piece_operand((BN, K, K), seed + 1, pos)
    bm = G.piece_operand(K, seed + 2, pos)
    X = G.piece_operand((BN * HW, K), seed + 3, pos)
    parts = [G.ref_den(vv[b * HW:(b + 1) * HW], M[b], bm, X[b * HW:(b + 1) * HW]) for b in range(BN)]
    ref, den = torch.cat([p[0] for p in parts]), torch.cat([p[1] for p in parts])
    Wp = pack_fragments(G.piece_operand((N, K), seed + 4, False).to(DEV), ntiles, KG)
    Mp = torch.cat([pack_fragments(M[b].to(DEV), KG, KG) for b in range(BN)])
    vd, Xd, bmd = _wide(vv, 4, 3.0).to(DEV), _wide(X, 4, 3.0).to(DEV), bm.to(DEV)
    out = torch.full((BN * HW, N + 4), PAD, device=DEV)
    out1 = torch.full((BN * HW, K + 4), PAD, device=DEV)
    _call("kdlae_debug_gemm", GemmDesc, A=_ptr(vd), lda=K + 4, Bn=BN, F=1, H=H_, W=W_, ksize=1, kt=1, dil=1,
          kgroups=KG, Wp=_ptr(Wp), ntiles=ntiles, N=N, out=_ptr(out), ldo=N + 4, R=_ptr(Xd), ldr=K + 4, ln=1, ln_C=K,
          Wm=_ptr(Mp), wm_img_stride=K * K, bias_m=_ptr(bmd), out1=_ptr(out1), ldo1=K + 4, NT=NT, KG=KG, wpe=2,
          group_tiles=ntiles, route=0)
    _check(f"gemm_attn_in nt{NT} kg{KG} nch{NCH} {cls} out1", out1[:, :K], ref, den, bound)
    assert bool((out1[:, K:] == PAD).all()) and bool((out[:, N:] == PAD).all())
    assert torch.isfinite(out[:, :N]).all()


# =========================================================================== training GEMM family
@pytest.mark.parametrize("cls", ["onehot", "coherent"])
@pytest.mark.parametrize("K", [40, 96])
@pytest.mark.parametrize("transposed", [False, True])
@pytest.mark.parametrize("nt", [1, 4, 8])
def test_rows_kernel_precision(nt, transposed, K, cls):
    """tgemm_rows_kernel<NT>: C = A W^T + bias (+ rs R, NT <= 4) with the weights split inside the
    kernel from either orientation (B(k, n) = Wt[n][k] or W[k][n]); K = 40: a ragged last pair (8 valid
    k in the third k-group, NaN in the A pad columns), K = 96: three whole pairs."""
    M, N = 304, 16 * nt
    lda, ldc = (K + 3) // 4 * 4 + 4, N + 4
    seed = 4000 + 100 * nt + K + transposed
    hasr = nt <= 4
    A, Wt, bias, R = (G.coherent_case if cls == "coherent" else G.one_hot_case)(M, K, N, seed, hasr)
    rs = G.piece_operand(N, seed + 4, cls == "coherent") if hasr else None
    ref, den = G.ref_den(A, Wt, bias, R, rs)
    Ad = _wide(A, lda - K, float("nan")).to(DEV)
    Bd = (Wt.t().contiguous() if transposed else Wt).to(DEV)
    Rd = None if R is None else _wide(R, 4).to(DEV)
    C = torch.full((M, ldc), PAD, device=DEV)
    biasd, rsd = _dev(bias), _dev(rs)
    _tgemm(A=_ptr(Ad), sam=lda, sak=1, B=_ptr(Bd), sbk=N if transposed else 1, sbn=1 if transposed else K,
           C=_ptr(C), scm=ldc, scn=1, bias=_ptr(biasd), R=_ptr(Rd), srm=ldc, srn=1, rs=_ptr(rsd), M=M, N=N, K=K, route=1)
    bound = G.coherent_bound(K) if cls == "coherent" else G.ONE_HOT_BOUND
    _check(f"tgemm_rows nt{nt} K{K} t{int(transposed)} {cls}", C[:, :N], ref, den, bound)
    assert bool((C[:, N:] == PAD).all()), "wrote past N"


def _cols(name, dY, X, bound, **kw):
    """dW = dY^T X through route 2; returns nothing, checks against float64."""
    P, M = dY.shape
    ref, den = G.ref_den(dY.t().contiguous(), kw.pop("cols", X).t().contiguous())
    N = ref.shape[1]
    dYd, Xd = _wide(dY, 4, 3.0).to(DEV), _wide(X, 4, 3.0).to(DEV)
    C = torch.zeros(M, N, device=DEV)
    part = torch.empty(1 << 20, device=DEV)
    _tgemm(A=_ptr(dYd), sam=1, sak=M + 4, B=_ptr(Xd), sbk=X.shape[1] + 4, sbn=1, C=_ptr(C), scm=N, scn=1, M=M, N=N,
           K=P, partial=_ptr(part), partial_floats=part.numel(), route=2, **kw)
    _check(name, C, ref, den, bound)


def test_cols_kernel_precision_one_hot():
    """tgemm_cols_kernel<2, 2>: the contraction index is the pixel, so one-hot = exactly one pixel per
    (m, n) where both operands are nonzero; P = 512 (at most ceil(512 / 256) = 2 split-K partials, all
    but one of which are zero for every output), ragged M = 29, N = 31."""
    dY, X = G.one_hot_pixels(512, 29, 31, 5000)
    _cols("tgemm_cols onehot", dY, X, G.ONE_HOT_BOUND)


def test_cols_kernel_precision_coherent():
    """Dense positive operands over P = 96 pixels: one chunk (chunks of at least 256 pixels), three
    32-pixel MFMA steps."""
    dY, X = G.piece_operand((96, 29), 5001, True), G.piece_operand((96, 31), 5002, True)
    _cols("tgemm_cols coherent", dY, X, G.coherent_bound(96, chunks=1))


def test_cols_kernel_precision_implicit_conv3d():
    """bmode 4, tgemm_cols_kernel<2, 3, implicit>: dW'[o][tap * 16 + c] = sum_p dZ[p][o] X[p + off(tap)][c]
    with X on the 3x3x3 lattice (B 1, F 3, 10 x 16: 480 pixels, at most 2 partials) and dense dZ.  The
    15 lattice points of this image carry 15 distinct channels, so every (o, tap, c) receives at most one
    product, and 27 x 15 of the 27 x 16 columns receive one."""
    Fr, H, W, cin, cout = 3, 10, 16, 16, 16
    x = G.conv_lattice(1, Fr, H, W, cin, 1, 3, 5003, cover=27 * 15)
    assert int((x != 0).sum()) <= cin          # distinct channels: no (tap, c) is hit twice
    dZ = G.piece_operand((Fr * H * W, cout), 5004, False)
    _cols("tgemm_cols conv3d", dZ, x.reshape(-1, cin), G.ONE_HOT_BOUND, cols=G.im2col(x, 1, 3), bmode=4, Bn=1, F=Fr,
          H=H, W=W, Cg=cin)


@pytest.mark.parametrize("kind", ["lean", "generic"])
def test_tiled_kernel_precision_one_hot(kind):
    """The f32-MFMA tiled kernels (route 3, no split-K without a partial buffer): one product per
    output, so one fp32 rounding — (1 + 1 + 4) 2^-24.  lean: aligned operands; generic: strides that
    rule out float4 loads, K = 41, N = 50."""
    M, K, N, lda, ldb, ldc = (304, 72, 64, 72, 64, 64) if kind == "lean" else (304, 41, 50, 43, 53, 51)
    A = G.one_hot_rows(M, K, 6000)
    B = G.piece_operand((K, N), 6001, False)
    ref, den = G.ref_den(A, B.t().contiguous())
    Ad, Bd = _wide(A, lda - K, 3.0).to(DEV), _wide(B, ldb - N, 3.0).to(DEV)
    C = torch.full((M, ldc), PAD, device=DEV)
    _tgemm(A=_ptr(Ad), sam=lda, sak=1, B=_ptr(Bd), sbk=ldb, sbn=1, C=_ptr(C), scm=ldc, scn=1, M=M, N=N, K=K, route=3)
    _check(f"tgemm_tiled {kind}", C[:, :N], ref, den, G.f32_bound(1, 1))
    assert bool((C[:, N:] == PAD).all())


# =========================================================================== conv_lds, conv3d_c16
def _conv_case(name, op, kt, ntiles, cin, cls, seed, wp3=0):
    """conv_lds (op 5) / conv3d_c16 (op 7) on the lattice, or on dense positive data with the weights
    of the first 96 / cin taps only (K = 96: three tap pairs, or three (tap, 32-channel) pairs)."""
    Fr = 3 if kt == 3 else 1
    N, taps = 16 * ntiles, 9 * kt
    if cls == "lattice":
        x = G.conv_lattice(BN, Fr, H_, W_, cin, 1, kt, seed)
        Wm = G.piece_operand((N, taps * cin), seed + 1, False)
        bound = G.ONE_HOT_BOUND
    else:
        x = G.piece_operand((BN, Fr, H_, W_, cin), seed, True)
        Wm = torch.zeros(N, taps * cin)
        Wm[:, :96] = G.piece_operand((N, 96), seed + 1, True)
        bound = G.coherent_bound(96)
    bias = G.piece_operand(N, seed + 2, cls != "lattice")
    ref, den = G.ref_den(G.im2col(x, 1, kt), Wm, bias)
    Wt = Wm.view(N, taps, cin).transpose(1, 2).reshape(N, cin, kt, 3, 3)
    wp, wt = _conv_lds_weights(Wt.to(DEV), ntiles, cin, kt)
    out = torch.full((BN * Fr * H_ * W_, N + 4), PAD, device=DEV)
    xd = _wide(x, 4, 3.0).to(DEV)
    kw = dict(ntiles=ntiles, cin_pad=cin, use_wp3=wp3) if op == 5 else {}
    _infer(op=op, inp=[(xd, cin + 4)], out=[(out, N + 4)], w=[wp, wt] if (op == 5 and kt == 3) else [wp],
           bias=[bias.to(DEV)], kt=kt, relu=0, Bn=BN, F=Fr, H=H_, W=W_, **kw)
    _check(name, out[:, :N], ref, den, bound)
    assert bool((out[:, N:] == PAD).all()), f"{name}: wrote past its columns"


@pytest.mark.parametrize("cls", ["lattice", "coherent"])
@pytest.mark.parametrize("wp3", [0, 1])
@pytest.mark.parametrize("kt,ntiles,cin", [(1, 3, 32), (3, 2, 16)])
def test_conv_lds_precision(kt, ntiles, cin, wp3, cls):
    """conv_lds_kernel, both weight-split paths against one reference: use_wp3 0 splits the fp32
    fragments in the kernel, use_wp3 1 reads pre-split records (kt 1, cin 32: pre-split halo as well;
    kt 3: tap-pair records)."""
    _conv_case(f"conv_lds kt{kt} wp3{wp3} {cls}", 5, kt, ntiles, cin, cls, 7000 + 10 * kt + wp3, wp3=wp3)


@pytest.mark.parametrize("cls", ["lattice", "coherent"])
@pytest.mark.parametrize("kt", [1, 3])
def test_conv3d_c16_precision(kt, cls):
    """conv3d_c16_kernel: 9 / 27 taps of 16 channels, the odd last tap paired with zeros."""
    _conv_case(f"conv3d_c16 kt{kt} {cls}", 7, kt, 1, 16, cls, 7100 + kt)


# =========================================================================== MDTA Gram (f32 MFMA)
@pytest.mark.parametrize("route,ct", [(0, 3), (1, 6), (2, 2)])
def test_gram_precision_one_hot(route, ct):
    """dwconv_gram ring / sweep / generic kernel + gram_reduce, one head width each: the depthwise weight
    is the centre tap = 1 with no bias, so q and k are the inputs themselves, one-hot in the pixel index
    (one pixel per (c1, c2) where both are nonzero).  One product per Gram entry, every other partial an
    exact zero: (1 + 1 + 4) 2^-24.  v passes through unchanged."""
    Bn, H, W, heads = 2, 40, 48, 1 if ct > 4 else 2
    Ch = 16 * ct
    C, P = Ch * heads, H * W
    ops = [[G.one_hot_pixels(P, Ch, Ch, 8000 + 100 * route + 10 * b + h) for h in range(heads)] for b in range(Bn)]
    q = torch.stack([torch.cat([ops[b][h][0] for h in range(heads)], dim=1) for b in range(Bn)])     # [Bn][P][C]
    k = torch.stack([torch.cat([ops[b][h][1] for h in range(heads)], dim=1) for b in range(Bn)])
    v = G.piece_operand((Bn, P, C), 8100 + route, False)
    qkvd = _wide(torch.cat([q, k, v], dim=-1), 4, 3.0).to(DEV)
    wdw = torch.zeros(9, 3 * C)
    wdw[4] = 1.0
    wdwd = wdw.to(DEV)
    v_out = torch.full((Bn, P, C), PAD, device=DEV)
    sf = ct * ct * 256 + 2 * Ch
    partial = torch.empty(Bn * heads * 64 * 8 * sf, device=DEV)
    reduced = torch.empty(Bn * heads, sf, device=DEV)
    zeros = torch.zeros(64, device=DEV)
    _call("kdlae_debug_gram", GramDesc, qkv=_ptr(qkvd), ld=3 * C + 4, wdw=_ptr(wdwd), v_out=_ptr(v_out), ldv=C,
          partial=_ptr(partial), partial_floats=partial.numel(), reduced=_ptr(reduced), zeros=_ptr(zeros), C=C,
          heads=heads, Bn=Bn, H=H, W=W, route=route)
    assert torch.equal(v_out.cpu(), v)
    for b in range(Bn):
        for h in range(heads):
            qa, ka = ops[b][h]
            ref, den = G.ref_den(qa.t().contiguous(), ka.t().contiguous())          # [Ch][Ch]
            got = reduced[b * heads + h, :ct * ct * 256].cpu().view(ct, ct, 4, 16, 4).permute(0, 2, 4, 1, 3)
            _check(f"gram route{route} ct{ct} b{b} h{h}", got.reshape(Ch, Ch), ref, den, G.f32_bound(1, 1))


# =========================================================================== scale invariance, bit-exact
SCALES = [(2.0 ** 40, 2.0 ** -40), (2.0 ** -40, 2.0 ** 40)]


def test_gemm_scale_invariance_bits():
    """Resident 1x1 (route 0, gemm_res_kernel<6, 3, 1>), dense random-sign piece operands, no bias, no LN:
    scaling A by 2^40 and W by 2^-40 (and the reverse) leaves every output bit unchanged — a power of two
    commutes with the round-to-nearest split, the exact plane products and the fp32 accumulator while
    every plane stays normal."""
    KG, ntiles = 3, 6
    K, N, P = 16 * KG, 16 * ntiles, BN * H_ * W_
    A = G.piece_operand((P, K), 9000, False)
    Wt = G.piece_operand((N, K), 9001, False)

    def run(sa, sw):
        Ad = (A * sa).to(DEV)
        Wp = pack_fragments((Wt * sw).to(DEV), ntiles, KG)
        out = torch.zeros(P, N, device=DEV)
        _call("kdlae_debug_gemm", GemmDesc, A=_ptr(Ad), lda=K, Bn=BN, F=1, H=H_, W=W_, ksize=1, kt=1, dil=1, kgroups=KG,
              Wp=_ptr(Wp), ntiles=ntiles, N=N, out=_ptr(out), ldo=N, ln=0, ln_C=K, NT=6, KG=KG, wpe=2,
              group_tiles=ntiles, route=0)
        return out
    base = run(1.0, 1.0)
    assert bool((base != 0).any())
    for sa, sw in SCALES:
        assert torch.equal(run(sa, sw), base), f"A x {sa}, W x {sw} changed the bits"


def test_rows_kernel_scale_invariance_bits():
    """The same for tgemm_rows_kernel<4> (weights split inside the kernel), K = 96."""
    M, K, N = 304, 96, 64
    A = G.piece_operand((M, K), 9002, False)
    Wt = G.piece_operand((N, K), 9003, False)

    def run(sa, sw):
        Ad, Bd = (A * sa).to(DEV), (Wt * sw).to(DEV)
        C = torch.zeros(M, N, device=DEV)
        _tgemm(A=_ptr(Ad), sam=K, sak=1, B=_ptr(Bd), sbk=1, sbn=K, C=_ptr(C), scm=N, scn=1, M=M, N=N, K=K, route=1)
        return C
    base = run(1.0, 1.0)
    assert bool((base != 0).any())
    for sa, sw in SCALES:
        assert torch.equal(run(sa, sw), base), f"A x {sa}, W x {sw} changed the bits"

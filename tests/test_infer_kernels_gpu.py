"""The forward paths' kernels that no kernel-level test reached, one launch each through
kdlae_debug_infer (include/kdlae.h) against the float64 references of tests/infer_kernel_refs.py:
fused GDFN tail (odd chunk counts, every nsplit), fused feed-forward half and fused MDTA pass 1 (their
persistent tile loops included), softmax + fold (Ch up to 128, zero / tiny norms, peaked logits), the
unfused gate, conv_lds stores, conv_small_out (tiled and generic), conv3d_c16, max-pool, ASDQE pool +
head.

Every case: Bn >= 2 different images (a halo must not read the neighbouring image), seeded uniform
[-1, 1] inputs with weights scaled by 1 / sqrt(K), output views wider than their used columns with
the rest pre-filled with 7.0 and checked untouched, input views wider than their used columns where
the launcher takes one.  Tolerance: the rule of tests/test_kernel_variants_infer_gpu.py,
1e-5 (max|ref| + 1) sqrt(K) / 4 with K the longest reduction of the chain.
"""
import ctypes

import pytest
import torch

import infer_kernel_refs as R
from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd._lib import InferDesc

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
PAD = 7.0


def _ptr(t):
    return None if t is None else t.data_ptr()


def _run(**kw):
    """One kdlae_debug_infer call; returns the error code (0 = OK)."""
    d = InferDesc()
    for k, v in kw.items():
        if k in ("inp", "out"):
            for i, (t, ld) in enumerate(v):
                getattr(d, k)[i] = _ptr(t)
                (d.ldi if k == "inp" else d.ldo)[i] = ld
        elif k in ("w", "bias"):
            for i, t in enumerate(v):
                getattr(d, k)[i] = _ptr(t)
        else:
            setattr(d, k, _ptr(v) if isinstance(v, torch.Tensor) else v)
    rc = _lib.lib().kdlae_debug_infer(ctypes.byref(d), None)
    torch.cuda.synchronize()
    return rc


def _call(**kw):
    _lib.check(_run(**kw), "kdlae_debug_infer")


def _rand(*shape, seed=0, scale=1.0):
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1) * scale).float().to(DEV)


def _wide(t, pad, seed=99):
    """t [..., C] as the first C columns of a buffer [..., C + pad] whose other columns hold other data."""
    buf = _rand(*t.shape[:-1], t.shape[-1] + pad, seed=seed)
    buf[..., :t.shape[-1]] = t
    return buf


def _out(pixels, width, pad=4):
    return torch.full((pixels, width + pad), PAD, device=DEV)


def _close(got, ref, K, what):
    err = (got.double() - ref).abs().max().item()
    tol = 1e-5 * (ref.abs().max().item() + 1) * max(1.0, K ** 0.5) / 4
    print(f"RATIO {what.split()[0]} {err / tol:.4f} ({what})")
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    assert err <= tol, f"{what} max |err| {err:.3e} > {tol:.3e}"


def _untouched(buf, width, what):
    assert bool((buf[..., width:] == PAD).all()), f"{what}: wrote past its {width} columns"


def _cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ------------------------------------------------------------------ fused GDFN tail
GDFN = ([(48, 25, 20, h) for h in (16, 48, 112, 128)] + [(96, 17, 33, h) for h in (80, 256)] +
        [(192, 17, 33, 96), (192, 17, 33, 272), (384, 17, 33, 32), (96, 5, 7, 48)])


@pytest.mark.parametrize("rmode", ["nores", "res", "inplace"])
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("C,H,W,hid", GDFN)
def test_gdfn_out(C, H, W, hid, bias, rmode):
    """gdfn_out_kernel: tiles 16 x 12 (C = 48) / 16 x 8, ragged in both directions; odd hid / 16 (the last
    chunk paired with zeros, hid = 16: a single chunk), nsplit 1 / 2 / 4; R null, separate, and R == out
    on a channel slice of a [P][2 C] buffer."""
    Bn, seed = 2, C + hid
    y = _rand(Bn, H, W, 2 * hid, seed=seed)
    wdw = _rand(2 * hid, 9, seed=seed + 1, scale=1 / 3)
    bdw = _rand(2 * hid, seed=seed + 2)
    Wout = _rand(C, hid, seed=seed + 3, scale=hid ** -0.5)
    bo = _rand(C, seed=seed + 4) if bias else None
    res = _rand(Bn, H, W, C, seed=seed + 5)
    x = R.chunk_interleave(y).contiguous()
    ldo = 2 * C
    out = torch.full((Bn * H * W, ldo), PAD, device=DEV)
    Rv, ldr = None, 0
    if rmode == "res":
        Rv, ldr = _wide(res, 4).contiguous(), C + 4
    elif rmode == "inplace":
        out[:, :C] = res.view(-1, C)
        Rv, ldr = out, ldo
    _call(op=0, inp=[(x, 2 * hid)], out=[(out, ldo)], w=[R.dw_blocks(wdw, bdw).contiguous(), R.pack_fragments(Wout, C // 16, hid // 16)],
          bias=[bo], R=Rv, ldr=ldr, zeros=torch.zeros(64, device=DEV), C=C, hidS=hid, Bn=Bn, H=H, W=W)
    ref = R.gdfn_tail(y.double(), wdw.double(), bdw.double(), Wout.double(), None if bo is None else bo.double(),
                      None if rmode == "nores" else res.double())
    _close(out[:, :C], ref.reshape(-1, C), hid, f"gdfn C{C} hid{hid}")
    _untouched(out, C, "gdfn")


# ------------------------------------------------------------------ fused feed-forward half
def _ffn_case(C, hid, ln, bias, Bn, H, W):
    seed = 3 * C + hid + ln
    xs = _rand(Bn, H, W, C, seed=seed)
    Win = _rand(2 * hid, C, seed=seed + 1, scale=C ** -0.5)
    bi = _rand(2 * hid, seed=seed + 2) if bias else None
    wdw = _rand(2 * hid, 9, seed=seed + 3, scale=1 / 3)
    bdw = _rand(2 * hid, seed=seed + 4)
    Wout = _rand(C, hid, seed=seed + 5, scale=hid ** -0.5)
    bo = _rand(C, seed=seed + 6) if bias else None
    x = _wide(xs, 4)
    out = _out(Bn * H * W, C)
    _call(op=1, inp=[(x, C + 4)], out=[(out, C + 4)], ln=ln, hidS=hid, C=C, Bn=Bn, H=H, W=W,
          w=[R.pack_fragments(R.chunk_interleave(Win, 0).contiguous(), 2 * hid // 16, C // 16),
             R.dw_blocks(wdw, bdw).contiguous(), R.pack_fragments(Wout, C // 16, hid // 16)],
          bias=[None if bi is None else R.chunk_interleave(bi).contiguous(), bo])
    d = lambda t: None if t is None else t.double()
    ref = R.ffn_half(xs.double(), ln, Win.double(), d(bi), wdw.double(), bdw.double(), Wout.double(), d(bo))
    _close(out[:, :C], ref.reshape(-1, C), max(C, hid), f"ffn C{C} hid{hid} ln{ln} Bn{Bn}")
    _untouched(out, C, "ffn")


@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("ln", [1, 2])
@pytest.mark.parametrize("C,hid", [(48, 32), (48, 96), (48, 128), (96, 64), (96, 256)])
def test_ffn_fused(C, hid, ln, bias):
    """ffn_fused_kernel, one tile per block: LN + project_in on the halo, gate, project_out, residual."""
    _ffn_case(C, hid, ln, bias, 2, 13, 21)


@pytest.mark.parametrize("C,hid", [(48, 128), (96, 256)])
def test_ffn_fused_persistent(C, hid):
    """More tiles than compute units (9 per image), so some blocks run two tiles and others one: the state
    the persistent loop carries from tile to tile."""
    _ffn_case(C, hid, 2, 1, _cus() // 9 + 2, 24, 40)


# ------------------------------------------------------------------ fused MDTA pass 1
def _mdta_case(C, ln, Bn, H, W, nseg, seg_rows):
    seed = 5 * C + ln + H
    xs = _rand(Bn, H, W, C, seed=seed)
    Wq = _rand(3 * C, C, seed=seed + 1, scale=C ** -0.5)
    bq = _rand(3 * C, seed=seed + 2)
    wdw = _rand(3 * C, 9, seed=seed + 3, scale=1 / 3)
    bdw = _rand(3 * C, seed=seed + 4)
    x = _wide(xs, 4)
    v = _out(Bn * H * W, C)
    sf = C * C + 2 * C
    nslots = (W // 16) * nseg
    scratch = torch.empty(Bn * nslots * sf, device=DEV)
    red = torch.empty(Bn, sf, device=DEV)
    _call(op=2, inp=[(x, C + 4)], out=[(v, C + 4), (red, 0)], ln=ln, C=C, Bn=Bn, H=H, W=W, nseg=nseg, seg_rows=seg_rows,
          w=[R.pack_fragments(Wq, 3 * C // 16, C // 16), wdw.t().contiguous()], bias=[bq, bdw],
          scratch=scratch, scratch_floats=scratch.numel())
    rv, G, nq, nk = R.mdta_pass1(xs.double(), ln, Wq.double(), bq.double(), wdw.double(), bdw.double())
    tag = f"C{C} ln{ln} {H}x{W} Bn{Bn}"
    _close(v[:, :C], rv.reshape(-1, C), C, f"mdta_v {tag}")
    _untouched(v, C, "mdta v")
    Gk, nqk, nkk = R.unpack_reduced(red, C)
    for b in range(Bn):   # per image, as each image's Gram has its own magnitude
        _close(Gk[b], G[b], H * W, f"mdta_gram {tag} b{b}")
        _close(nqk[b], nq[b], H * W, f"mdta_norm {tag} q b{b}")
        _close(nkk[b], nk[b], H * W, f"mdta_norm {tag} k b{b}")


@pytest.mark.parametrize("H,W,nseg,seg_rows", [(24, 32, 1, 24), (40, 32, 2, 24)])
@pytest.mark.parametrize("ln", [1, 2])
@pytest.mark.parametrize("C", [48, 96])
def test_mdta_fused(C, ln, H, W, nseg, seg_rows):
    """mdta_fused_kernel + gram_reduce: v, the Gram and both squared norms; one segment, and two with a short
    last one."""
    _mdta_case(C, ln, 2, H, W, nseg, seg_rows)


@pytest.mark.parametrize("C", [48, 96])
def test_mdta_fused_persistent(C):
    """More units (8 per image) than compute units: blocks that run two units after one another."""
    _mdta_case(C, 2, _cus() // 8 + 1, 32, 64, 2, 16)


# ------------------------------------------------------------------ softmax + fold
@pytest.mark.parametrize("C,heads", [(16, 1), (48, 1), (80, 5), (96, 2), (128, 1), (192, 4), (256, 2), (384, 8)])
def test_attn_fold(C, heads):
    """attn_fold_kernel: `reduced` built from the Gram of random q, k in which q channel 0 and k channel 2 of
    every head are zero over the image (norm 0: the 1e-12 clamp), q channel 1 is tiny (norm ~1e-8: above the
    clamp, below a wrong one), and the last head has k channel 5 = q channel 4 with temperature 100 (a
    logit of 100: exp overflows without the max subtraction).  Ch = 128 needs more than 64 KiB of LDS."""
    Bn, Ch, npix = 2, C // heads, 64
    q = _rand(Bn, heads, Ch, npix, seed=C).double()
    k = _rand(Bn, heads, Ch, npix, seed=C + 1).double()
    q[:, :, 0] = 0
    q[:, :, 1] *= 1e-9
    k[:, :, 2] = 0
    k[:, -1, 5] = q[:, -1, 4]
    temp = _rand(heads, seed=C + 2) + 2
    temp[-1] = 100.0
    proj = _rand(C, C, seed=C + 3, scale=C ** -0.5)
    # the kernel's inputs are float32: the reference starts from the rounded values
    G = (q @ k.transpose(-1, -2)).float()
    nq, nk = (q * q).sum(-1).float(), (k * k).sum(-1).float()
    assert (G[:, -1] * nq[:, -1].rsqrt()[..., :, None] * nk[:, -1].rsqrt()[..., None, :])[:, 4, 5].min() * 100 > 80
    red = R.pack_reduced(G, nq, nk).view(Bn * heads, -1).contiguous()
    kg = C // 16
    kpt = (kg + 1) // 2
    Mp = torch.full((Bn, kg * kpt * 768), PAD, device=DEV)
    _call(op=3, inp=[(red, 0)], out=[(Mp, 0)], w=[proj, temp], C=C, heads=heads, Bn=Bn)
    ref = R.attn_fold(G.double(), nq.double(), nk.double(), proj.double(), temp.double())
    for b in range(Bn):
        M = R.split_records_decode(Mp[b], kg, kg)
        assert torch.isfinite(M).all()
        _close(M[:, :C], ref[b], Ch, f"fold C{C} heads{heads} b{b}")
        if kg & 1:
            assert bool((M[:, C:] == 0).all()), "upper half of the last pair must be zero"


# ------------------------------------------------------------------ unfused gate
@pytest.mark.parametrize("bias", [0, 1])
@pytest.mark.parametrize("hid", [16, 208, 1024, 1040])
def test_dwconv_gate(hid, bias):
    """dwconv_gate_kernel: several columns per block (hid 16, 208), one (1024), and the second channel-quad
    group (1040); H = 33: a second row segment one row tall; W = 5."""
    Bn, H, W = 2, 33, 5
    xs = _rand(Bn, H, W, 2 * hid, seed=hid)
    w = _rand(9, 2 * hid, seed=hid + 1, scale=1 / 3)
    b = _rand(2 * hid, seed=hid + 2) if bias else None
    x = _wide(xs, 4)
    out = _out(Bn * H * W, hid)
    _call(op=4, inp=[(x, 2 * hid + 4)], out=[(out, hid + 4)], w=[w], bias=[b], hidS=hid, Bn=Bn, H=H, W=W)
    ref = R.dwconv_gate(xs.double(), w.double(), None if b is None else b.double())
    _close(out[:, :hid], ref.reshape(-1, hid), 9, f"gate hid{hid}")
    _untouched(out, hid, "gate")


# ------------------------------------------------------------------ conv_lds
def _conv_lds_weights(Wt, ntiles, cin_pad, kt):
    """[N][Cin][kt][3][3] -> fragments with k = tap cin_pad + c, and (kt 3) the tap-pair block in k-group
    order c-group * 28 + tap (tap 27 zero)."""
    N, Cin = Wt.shape[:2]
    taps = 9 * kt
    Wk = torch.zeros(N, taps, cin_pad, device=DEV)
    Wk[:, :, :Cin] = Wt.reshape(N, Cin, taps).transpose(1, 2)
    wp = R.pack_fragments(Wk.reshape(N, -1), ntiles, taps * cin_pad // 16)
    wt = None
    if kt == 3:
        cg = cin_pad // 16
        Wg = torch.zeros(N, cg, 28, 16, device=DEV)
        Wg[:, :, :27] = Wk.view(N, 27, cg, 16).permute(0, 2, 1, 3)
        wt = R.pack_fragments(Wg.reshape(N, -1), ntiles, 28 * cg)
    return wp, wt


@pytest.mark.parametrize("out_mode", [0, 1, 2])
@pytest.mark.parametrize("wp3", [0, 1])
@pytest.mark.parametrize("ntiles,cin_pad", [(2, 16), (3, 32), (4, 48), (5, 64), (9, 32)])
def test_conv_lds_2d(ntiles, cin_pad, wp3, out_mode):
    """conv_lds_kernel<1, ...>: fp32-staged and (cin_pad % 32 == 0 with split records) pre-split staging; plain,
    PixelUnshuffle and PixelShuffle stores with a ragged nout; ReLU on the plain store; W = 70: two column
    tiles, the second 6 wide; H = 6: a 2-row last tile."""
    Bn, H, W = 2, 6, 70
    Cin, N = cin_pad - 3, 16 * ntiles - 8
    seed = 16 * ntiles + cin_pad
    xs = _rand(Bn, H, W, Cin, seed=seed)
    x = torch.zeros(Bn, H, W, cin_pad + 4, device=DEV)     # channels Cin .. cin_pad meet zero weights
    x[..., :Cin] = xs
    x[..., cin_pad:] = 3.0
    Wt = _rand(N, Cin, 3, 3, seed=seed + 1, scale=(9 * Cin) ** -0.5)
    bias = torch.zeros(16 * ntiles, device=DEV)
    bias[:N] = _rand(N, seed=seed + 2)
    wp, _ = _conv_lds_weights(Wt, ntiles, cin_pad, 1)
    relu = out_mode == 0
    y = R.conv_nhwc(xs.double(), Wt.double(), bias[:N].double(), relu)
    if out_mode == 0:
        width, pixels, ref = 16 * ntiles, Bn * H * W, torch.cat([y, torch.zeros(Bn, H, W, 8, device=DEV, dtype=y.dtype)], -1)
    elif out_mode == 1:
        width, pixels, ref = 4 * N, Bn * H * W // 4, R.pixel_unshuffle(y)
    else:
        width, pixels, ref = N // 4, Bn * H * W * 4, R.pixel_shuffle(y)
    pad = 4 + (-width) % 4                                 # the launcher wants ldo % 4 == 0
    out = _out(pixels, width, pad)
    _call(op=5, inp=[(x, cin_pad + 4)], out=[(out, width + pad)], w=[wp], bias=[bias], ntiles=ntiles, cin_pad=cin_pad,
          kt=1, relu=int(relu), out_mode=out_mode, nout=N, use_wp3=wp3, Bn=Bn, H=H, W=W)
    _close(out[:, :width], ref.reshape(-1, width), 9 * cin_pad, f"conv_lds nt{ntiles} cin{cin_pad} wp3{wp3} mode{out_mode}")
    _untouched(out, width, "conv_lds")


@pytest.mark.parametrize("wp3", [0, 1])
@pytest.mark.parametrize("ntiles,cin_pad", [(2, 16), (4, 32)])
def test_conv_lds_3d(ntiles, cin_pad, wp3):
    """conv_lds_kernel<3, ...>: 3x3x3 over F = 3 frames (zero frames before the first and after the last),
    fragment weights and tap-pair split records."""
    Bn, Fr, H, W = 2, 3, 6, 66
    Cin, N = cin_pad - 2, 16 * ntiles
    seed = 7 * ntiles + cin_pad
    xs = _rand(Bn, Fr, H, W, Cin, seed=seed)
    x = torch.zeros(Bn, Fr, H, W, cin_pad + 4, device=DEV)
    x[..., :Cin] = xs
    x[..., cin_pad:] = 3.0
    Wt = _rand(N, Cin, 3, 3, 3, seed=seed + 1, scale=(27 * Cin) ** -0.5)
    bias = _rand(N, seed=seed + 2)
    wp, wt = _conv_lds_weights(Wt, ntiles, cin_pad, 3)
    out = _out(Bn * Fr * H * W, N)
    _call(op=5, inp=[(x, cin_pad + 4)], out=[(out, N + 4)], w=[wp, wt], bias=[bias], ntiles=ntiles, cin_pad=cin_pad,
          kt=3, relu=1, use_wp3=wp3, Bn=Bn, F=Fr, H=H, W=W)
    ref = R.conv_nhwc(xs.double(), Wt.double(), bias.double(), True)
    _close(out[:, :N], ref.reshape(-1, N), 27 * cin_pad, f"conv_lds3d nt{ntiles} cin{cin_pad} wp3{wp3}")
    _untouched(out, N, "conv_lds 3d")


# ------------------------------------------------------------------ conv_small_out
@pytest.mark.parametrize("mode", ["nchw_res", "nhwc_extra", "nhwc_inplace"])
@pytest.mark.parametrize("Fr", [1, 2])
@pytest.mark.parametrize("ks", [1, 3])
@pytest.mark.parametrize("Cin", [20, 36, 48, 272])
def test_conv_small_out(Cin, ks, Fr, mode):
    """conv_small_out_tiled_kernel (ks 3, one frame, Cin <= 256) and conv_small_out_kernel (the rest); Cout
    1, 3, 4 over the cases; W = 35: three column tiles, the last 3 wide; H = 18 < one tile.  Both kernels
    move 16 input channels a step (SmallOutParams: Cin % 16 == 0), so Cin = 20 / 36 must be refused with an
    error code before any launch, the output left as it was."""
    Bn, H, W = 2, 18, 35
    Cout = (1, 3, 4)[(Cin // 4 + ks + Fr + len(mode)) % 3]
    seed = Cin + 10 * ks + Fr
    P = Bn * Fr * H * W
    xs = _rand(Bn * Fr, H, W, Cin, seed=seed)
    x = _wide(xs, 4)
    Wt = _rand(Cout, Cin, ks, ks, seed=seed + 1, scale=(ks * ks * Cin) ** -0.5)
    bias = _rand(Cout, seed=seed + 2)
    res = _rand(Bn * Fr, H, W, Cout, seed=seed + 3)
    extra = _rand(P, seed=seed + 4)
    y = R.conv_nhwc(xs.double(), Wt.double(), bias.double()) + res.double()       # [Bn Fr][H][W][Cout]
    kw = dict(op=6, inp=[(x, Cin + 4)], w=[Wt], bias=[bias], C=Cin, C2=Cout, ks=ks, Bn=Bn, F=Fr, H=H, W=W)
    if mode == "nchw_res":
        resn = res.view(Bn, Fr * H * W, Cout).transpose(1, 2).contiguous()
        out = torch.full((Bn * Cout * Fr * H * W + 16,), PAD, device=DEV)
        kw.update(inp=[(x, Cin + 4), (resn, 0)], out=[(out, 0)], out_nchw=1)
        got = lambda: out[:-16].view(Bn, Cout, Fr * H * W).transpose(1, 2).reshape(P, Cout)
        pad_ok = lambda: bool((out[-16:] == PAD).all())
    else:
        out = _out(P, Cout + 1)
        if mode == "nhwc_extra":
            kw.update(inp=[(x, Cin + 4), (None, 0), (extra, 0)], out=[(out, Cout + 5)], R=_wide(res, 4), ldr=Cout + 4)
        else:
            out[:, :Cout] = res.view(P, Cout)
            kw.update(out=[(out, Cout + 5)], R=out, ldr=Cout + 5)
        got = lambda: out[:, :Cout]
        pad_ok = lambda: bool((out[:, Cout + 1:] == PAD).all())
    if Cin % 16:
        before = out.clone()
        assert _run(**kw) == 1 and "Cin % 16" in _lib.last_error()
        assert torch.equal(out, before)
        return
    _call(**kw)
    _close(got(), y.reshape(P, Cout), ks * ks * Cin, f"small_out Cin{Cin} ks{ks} F{Fr} {mode} Cout{Cout}")
    assert pad_ok(), "conv_small_out wrote past its output"
    if mode == "nhwc_extra":
        assert torch.equal(out[:, Cout], extra)
    elif mode == "nhwc_inplace":
        assert bool((out[:, Cout] == PAD).all())


@pytest.mark.parametrize("Cin", [48, 272])
def test_conv_small_out_transposed(Cin):
    """wt = 1: the weight of the conv this one transposes, [Cin][Cout][3][3] with flipped taps, on the tiled
    (Cin 48) and the generic (Cin 272) kernel."""
    Bn, H, W, Cout = 2, 18, 35, 3
    xs = _rand(Bn, H, W, Cin, seed=Cin)
    Wt = _rand(Cin, Cout, 3, 3, seed=Cin + 1, scale=(9 * Cin) ** -0.5)
    out = _out(Bn * H * W, Cout)
    _call(op=6, inp=[(_wide(xs, 4), Cin + 4)], out=[(out, Cout + 4)], w=[Wt], C=Cin, C2=Cout, ks=3, wt=1, Bn=Bn, H=H, W=W)
    ref = R.conv_nhwc(xs.double(), R.conv_transposed_weight(Wt.double()))
    _close(out[:, :Cout], ref.reshape(-1, Cout), 9 * Cin, f"small_out wt Cin{Cin}")
    _untouched(out, Cout, "conv_small_out wt")


# ------------------------------------------------------------------ conv3d_c16, max-pool, pool + head
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("kt", [3, 1])
def test_conv3d_c16(kt, relu):
    """conv3d_c16_kernel: 3x3x3 over F = 3 frames and 3x3 per frame (F = 2), H = 7 (a 3-row last tile), W = 19."""
    Bn, Fr, H, W = 2, (3 if kt == 3 else 2), 7, 19
    xs = _rand(Bn, Fr, H, W, 16, seed=kt)
    Wt = _rand(16, 16, kt, 3, 3, seed=kt + 1, scale=(144 * kt) ** -0.5)
    bias = _rand(16, seed=kt + 2)
    wp, _ = _conv_lds_weights(Wt, 1, 16, kt)
    out = _out(Bn * Fr * H * W, 16)
    _call(op=7, inp=[(_wide(xs, 4), 20)], out=[(out, 20)], w=[wp], bias=[bias], kt=kt, relu=relu, Bn=Bn, F=Fr, H=H, W=W)
    ref = R.conv_nhwc(xs.double(), Wt.double(), bias.double(), bool(relu))
    _close(out[:, :16], ref.reshape(-1, 16), 144 * kt, f"conv3d_c16 kt{kt} relu{relu}")
    _untouched(out, 16, "conv3d_c16")


@pytest.mark.parametrize("C", [4, 20])
def test_maxpool2(C):
    """maxpool2_kernel on strided views, odd H and W: the last row and column are dropped (floor)."""
    N, H, W = 3, 7, 9
    xs = _rand(N, H, W, C, seed=C)
    out = _out(N * (H // 2) * (W // 2), C)
    _call(op=8, inp=[(_wide(xs, 8), C + 8)], out=[(out, C + 4)], C=C, Bn=N, H=H, W=W)
    assert torch.equal(out[:, :C], R.maxpool2(xs).reshape(-1, C))
    _untouched(out, C, "maxpool2")


@pytest.mark.parametrize("slots", [1, 7])
def test_gap_head(slots):
    """gap_partial_kernel + asdqe_head_kernel: HW = 37 * 29 is no multiple of the slot or lane counts."""
    B, H, W, C, M = 3, 37, 29, 64, 96
    ys = _rand(B, H * W, C, seed=slots)
    ws = [_rand(M, C, seed=11, scale=C ** -0.5), _rand(256, M, seed=12, scale=M ** -0.5),
          _rand(64, 256, seed=13, scale=1 / 16), _rand(64, seed=14, scale=1 / 8)]
    bs = [_rand(M, seed=15), _rand(256, seed=16), _rand(64, seed=17), _rand(1, seed=18)]
    scratch = torch.empty(B * slots * C, device=DEV)
    score = torch.full((B + 4,), PAD, device=DEV)
    _call(op=9, inp=[(_wide(ys, 4), C + 4)], out=[(score, 0)], w=ws, bias=bs, scratch=scratch, scratch_floats=scratch.numel(),
          C=C, Bn=B, H=H, W=W, slots=slots, M=M, N1=256, N2=64)
    args = [t.double() for pair in zip(ws, bs) for t in pair]
    _close(score[:B], R.gap_head(ys.double(), *args), H * W, f"gap_head slots{slots}")
    assert bool((score[B:] == PAD).all())

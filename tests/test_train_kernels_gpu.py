"""The non-GEMM kernels of the KDLAE-T / KDLAE-S training steps, one launch each through the self-test
entry points ``kdlae_debug_train`` / ``kdlae_debug_train_s`` (include/kdlae.h), against the plain
float64 references of tests/train_kernel_refs.py (themselves proven against autograd in
tests/test_train_kernel_refs.py).  The whole-model gradient tests accept 2e-3 of a tensor's largest
gradient per key; a wrong border column, dead channel lane or tie-break passes that.  Here every
kernel family is compared directly, at the shapes where it takes another path:

* MDTA softmax core and its backward: head widths on both sides of 64 (each lane owns columns
  ``lane`` and ``lane + 64``), and the clamped-norm branch (sumsq = 0);
* the buffer-descriptor depthwise / gate kernels of train_dwg.hip: 4-, 8- and 16-row blocks with ragged
  last tiles, two channel groups with a nearly dead second one, the stored-yd and the recomputing
  backward bit for bit;
* ``launch_dw_fwd``: both tile kernels, a partial last channel quad, the row kernel, ``flip``;
* the small-side 3x3 weight gradient: every instance, blocks that cross an image boundary or are empty;
* column reductions, layout kernels, and the KDLAE-S data-movement kernels (first-maximum routing of
  the max-pool backward on tie-rich input, F = 1 where both frame taps fall outside).

Every view has a leading dimension larger than its width where the case list allows it: input pad
columns hold NaN (must not leak), output pad columns a sentinel (must be unchanged).

Tolerances (two rules, no per-case constants):

* element-wise and 9- / 27-term results (forward values, dy, Mq, attention rows): the same float64
  reference formula is evaluated in float32 with torch, ``e32 = max |ref32 - ref64|``, and the kernel
  passes if ``max |got - ref64| <= 4 e32 + 2^-23 max |ref64|``.  The factor 4 allows for another
  association order and the approximate erf / exp the kernels document (A&S 7.1.26, 1.5e-7); the
  floor covers e32 = 0.  The bound comes from the reference, never from the kernel's output.
* sums over pixels (weight / bias partials, colsum, cq / ck, dtemp, col2im): the project's bound of
  tests/test_kernel_variants_gpu.py::_close with K the number of summed terms.

The worst err / tol per family is printed when the module finishes (run with ``-s`` to see it).
"""
import ctypes
import functools

import pytest
import torch

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd._lib import TrainDesc, TrainSDesc
from tests import train_kernel_refs as R

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
SENT = 7.0
NAN = float("nan")


(OP_SOFTMAX, OP_ATTN_BWD, OP_DW_FWD, OP_DWGATE_FWD, OP_DWGATE_BWD, OP_DWGATE_BWD_RC, OP_DW_BWD, OP_DW3_SMALL, OP_COLSUM,
 OP_PART_REDUCE, OP_PART_REDUCE_MULTI, OP_SHUFFLE, OP_COPY_COLS, OP_NCHW_TO_NHWC, OP_NHWC_TO_NCHW, OP_PACK_W3) = range(16)
S_IM2COL, S_COL2IM, S_WPERM, S_RELU_MASK, S_MAXPOOL_BWD, S_UPSHUFFLE = range(6)


def _ptr(t, off=0):
    return None if t is None else t.data_ptr() + 4 * off


def fill_desc(d, ins=(), outs=(), **kw):
    """ins / outs: (device tensor or None, ld[, float offset]) per slot."""
    for i, v in enumerate(ins):
        d.inp[i], d.ldi[i] = _ptr(v[0], *v[2:]), v[1]
    if isinstance(d, TrainDesc):
        for i, v in enumerate(outs):
            d.out[i], d.ldo[i] = _ptr(v[0], *v[2:]), v[1]
    elif outs:
        d.out, d.ldo = _ptr(outs[0][0], *outs[0][2:]), outs[0][1]
    for k, v in kw.items():
        setattr(d, k, _ptr(v) if isinstance(v, torch.Tensor) else v)
    return d


def _run(op, ins=(), outs=(), **kw):
    d = fill_desc(TrainDesc(), ins, outs, op=op, **kw)
    _lib.check(_lib.lib().kdlae_debug_train(ctypes.byref(d), None), f"kdlae_debug_train op {op}")
    torch.cuda.synchronize()


def _run_s(op, ins=(), outs=(), **kw):
    d = fill_desc(TrainSDesc(), ins, outs, op=op, **kw)
    _lib.check(_lib.lib().kdlae_debug_train_s(ctypes.byref(d), None), f"kdlae_debug_train_s op {op}")
    torch.cuda.synchronize()


def _rand(*shape, seed=0):
    """float32 values on the CPU (the kernels' inputs are exactly these; references widen them)"""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return (torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1).float()


def _in(x, ld):
    """[..., C] CPU tensor -> device view [pixels][ld], NaN in the pad columns"""
    C = x.shape[-1]
    buf = torch.full((x.numel() // C, ld), NAN)
    buf[:, :C] = x.reshape(-1, C)
    return buf.to(DEV)


def _out(pixels, C, ld, prefill=None):
    """device view [pixels][ld] full of the sentinel (or prefill in the used columns)"""
    buf = torch.full((pixels, ld), SENT)
    if prefill is not None:
        buf[:, :C] = prefill.reshape(-1, C)
    return buf.to(DEV)


def _take(buf, shape):
    """the used columns back on the CPU; the pad must be untouched"""
    h, C = buf.cpu(), shape[-1]
    assert torch.all(h[:, C:] == SENT), "wrote into the row pad"
    return h[:, :C].reshape(shape)


def _flat_out(n, tail=8):
    return torch.full((n + tail,), SENT, device=DEV)


def _take_flat(buf, shape, tail=8):
    h = buf.cpu()
    assert torch.all(h[-tail:] == SENT), "wrote past the end"
    return h[:-tail].reshape(shape)


def both(fn, *args):
    """the reference formula in float64 and in float32 (None arguments pass through)"""
    r64 = fn(*[a.double() if isinstance(a, torch.Tensor) else a for a in args])
    r32 = fn(*[a.float() if isinstance(a, torch.Tensor) else a for a in args])
    return r64, r32


MARGINS = {}


def _record(family, what, err, tol):
    ratio = err / tol
    MARGINS[family] = max(MARGINS.get(family, 0.0), ratio)
    print(f"[{family}] {what}: err {err:.3e} tol {tol:.3e} ratio {ratio:.3f}")
    assert err <= tol, f"{family} {what}: max |err| {err:.3e} > {tol:.3e}"


def elem_check(family, what, got, r64, r32):
    """rule 1 of the module docstring"""
    assert torch.isfinite(got).all(), f"{family} {what}: non-finite output"
    assert r64.dtype == torch.float64 and r32.dtype == torch.float32
    e32 = (r32.double() - r64).abs().max().item()
    tol = 4 * e32 + 2.0 ** -23 * r64.abs().max().item()
    _record(family, what, (got.double() - r64).abs().max().item(), tol)


def sum_check(family, what, got, ref, K):
    """rule 2: tests/test_kernel_variants_gpu.py::_close"""
    assert torch.isfinite(got).all(), f"{family} {what}: non-finite output"
    tol = 1e-5 * (ref.abs().max().item() + 1) * max(1.0, K ** 0.5) / 4
    _record(family, what, (got.double() - ref.double()).abs().max().item(), tol)


@pytest.fixture(scope="module", autouse=True)
def _print_margins():
    yield
    print("\nworst err / tol per family: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(MARGINS.items())))


# ---------------------------------------------------------------------------------------------- attention
def _attn_case(Ch, zero=None, Bn=2, heads=2, P=24):
    """G = q k^T and the squared norms of random q, k [Bn, heads, Ch, P] (cosine logits times a per-head
    temperature: order 1); zero = ((b, h, i), (b, h, j)) clears one q row and one k row."""
    C = heads * Ch
    q, k = _rand(Bn, heads, Ch, P, seed=Ch).double(), _rand(Bn, heads, Ch, P, seed=Ch + 1000).double()
    if zero:
        q[zero[0]] = 0
        k[zero[1]] = 0
    G = (q @ k.transpose(-1, -2)).float()
    sumsq = torch.cat([(q * q).sum(-1).reshape(Bn, C), (k * k).sum(-1).reshape(Bn, C)], dim=1).float()
    temp = torch.tensor([1.5, 3.0])
    A = R.attn_core(G.double(), sumsq.double(), temp.double()).float()  # the backward's input: fp32 like the engine's
    dA = _rand(Bn, heads, Ch, Ch, seed=Ch + 2000)
    return G, sumsq, temp, A, dA


def _attn_gpu(G, sumsq, temp, A, dA):
    Bn, heads, Ch, _ = G.shape
    C, n = heads * Ch, G.numel()
    dev = [t.to(DEV).contiguous() for t in (G, sumsq, temp, A, dA)]
    attn = _flat_out(n)
    _run(OP_SOFTMAX, ins=[(dev[0], 0), (dev[1], 0)], outs=[(attn, 0)], w=dev[2], C=C, heads=heads, Bn=Bn)
    mq, cq, ck, dt = _flat_out(n), _flat_out(Bn * C), _flat_out(Bn * C), _flat_out(Bn * heads)
    _run(OP_ATTN_BWD, ins=[(dev[0], 0), (dev[1], 0), (dev[3], 0), (dev[4], 0)],
         outs=[(mq, 0), (cq, 0), (ck, 0), (dt, 0)], w=dev[2], C=C, heads=heads, Bn=Bn)
    return (_take_flat(attn, G.shape), _take_flat(mq, G.shape), _take_flat(cq, (Bn, heads, Ch)),
            _take_flat(ck, (Bn, heads, Ch)), _take_flat(dt, (Bn, heads)))


@pytest.mark.parametrize("Ch", [8, 48, 64, 65, 100, 120])
def test_attention_core(Ch):
    G, sumsq, temp, A, dA = _attn_case(Ch)
    attn, mq, cq, ck, dt = _attn_gpu(G, sumsq, temp, A, dA)
    a64, a32 = both(R.attn_core, G, sumsq, temp)
    elem_check("attention", f"Attn Ch={Ch}", attn, a64, a32)
    b64, b32 = both(R.attn_core_bwd, G, sumsq, temp, A, dA)
    elem_check("attention", f"Mq Ch={Ch}", mq, b64[0], b32[0])
    sum_check("attention", f"cq Ch={Ch}", cq, b64[1], Ch)
    sum_check("attention", f"ck Ch={Ch}", ck, b64[2], Ch)
    sum_check("attention", f"dtemp Ch={Ch}", dt, b64[3], Ch * Ch)


def test_attention_core_clamped_norms():
    """one q row (a ``lane`` column owner) and one k column (a ``lane + 64`` one) of sumsq = 0: everything
    finite, cq / ck exactly 0 there, Mq = dGhat / (eps nk) in the clamped row and column"""
    Ch, zq, zk = 65, (0, 1, 3), (1, 0, 64)
    G, sumsq, temp, A, dA = _attn_case(Ch, zero=(zq, zk))
    assert sumsq[0, Ch + 3] == 0 and sumsq[1, 2 * Ch + 64] == 0 and torch.all(G[zq] == 0) and torch.all(G[1, 0, :, 64] == 0)
    attn, mq, cq, ck, dt = _attn_gpu(G, sumsq, temp, A, dA)
    for t in (attn, mq, cq, ck, dt):
        assert torch.isfinite(t).all()
    assert cq[zq] == 0 and ck[zk] == 0
    a64, a32 = both(R.attn_core, G, sumsq, temp)
    elem_check("attention", "Attn clamped", attn, a64, a32)
    b64, b32 = both(R.attn_core_bwd, G, sumsq, temp, A, dA)
    # Mq is ~1e12 times larger where a norm was clamped: each region against its own scale
    row = torch.zeros_like(G, dtype=torch.bool)
    row[zq] = True
    col = torch.zeros_like(G, dtype=torch.bool)
    col[1, 0, :, 64] = True
    for name, m in (("row", row), ("column", col), ("rest", ~(row | col))):
        elem_check("attention", f"Mq clamped {name}", mq[m], b64[0][m], b32[0][m])
    sum_check("attention", "cq clamped", cq, b64[1], Ch)
    sum_check("attention", "ck clamped", ck, b64[2], Ch)
    sum_check("attention", "dtemp clamped", dt, b64[3], Ch * Ch)


# ---------------------------------------------------------------------------------------------- depthwise / gate
def _blocks(Bn, H, W):
    n = _lib.lib().kdlae_debug_train_blocks(0, Bn, H, W, 0)
    assert n > 0
    return n


def _part_sums(part, nblk, Ct):
    """[nblk][9 Ct | Ct] partials summed in block order in float64 -> (dw [Ct, 9], db [Ct])"""
    p = part.cpu().double().reshape(nblk, 10 * Ct)
    s = torch.zeros(10 * Ct, dtype=torch.float64)
    for b in range(nblk):
        s += p[b]
    return s[:9 * Ct].reshape(Ct, 9), s[9 * Ct:]


# (hid, H, W, bias): rows_per_block 4 / 8 / 16 at Bn = 2; hid = 67: two channel groups, 3 live lanes in the second
DWG = [(67, 19, 21, True), (67, 19, 21, False), (5, 19, 21, True), (5, 19, 21, False), (5, 125, 128, True),
       (5, 125, 128, False), (5, 250, 128, True), (5, 250, 128, False)]


@functools.lru_cache(maxsize=None)
def _dwgate(hid, H, W, has_bias):
    Bn, C2 = 2, 2 * hid
    px = Bn * H * W
    y, w, dg = _rand(Bn, H, W, C2, seed=hid + H), _rand(C2, 9, seed=hid + 1), _rand(Bn, H, W, hid, seed=hid + 2)
    b = _rand(C2, seed=hid + 3) if has_bias else None
    ldi, ldg, ldyd, lddy = C2 + 3, hid + 1, C2 + 5, C2 + 2
    yv, dgv, wd = _in(y, ldi), _in(dg, ldg), w.to(DEV)
    bd = b.to(DEV) if has_bias else None
    geo = dict(C=hid, Bn=Bn, H=H, W=W)
    ydb, gb, gb2 = _out(px, C2, ldyd), _out(px, hid, ldg), _out(px, hid, ldg)
    _run(OP_DWGATE_FWD, ins=[(yv, ldi)], outs=[(gb, ldg), (ydb, ldyd)], w=wd, bias=bd, **geo)
    _run(OP_DWGATE_FWD, ins=[(yv, ldi)], outs=[(gb2, ldg), (None, 0)], w=wd, bias=bd, **geo)
    yd, g = _take(ydb, y.shape), _take(gb, dg.shape)
    nblk = _blocks(Bn, H, W)
    ydv = _in(yd, ldyd)  # the stored yd as the backward reads it (NaN pads again)
    dyb, dyb2 = _out(px, C2, lddy), _out(px, C2, lddy)
    part, part2 = _flat_out(nblk * 10 * C2), _flat_out(nblk * 10 * C2)
    _run(OP_DWGATE_BWD, ins=[(dgv, ldg), (ydv, ldyd), (yv, ldi)], outs=[(dyb, lddy)], w=wd, part=part,
         part_floats=nblk * 10 * C2, **geo)
    _run(OP_DWGATE_BWD_RC, ins=[(dgv, ldg), (yv, ldi)], outs=[(dyb2, lddy)], w=wd, bias=bd, part=part2,
         part_floats=nblk * 10 * C2, **geo)
    return dict(y=y, w=w, b=b, dg=dg, yd=yd, g=g, g_noyd=_take(gb2, dg.shape), dy=_take(dyb, y.shape),
                dy_rc=_take(dyb2, y.shape), part=_take_flat(part, (nblk, 10 * C2)),
                part_rc=_take_flat(part2, (nblk, 10 * C2)), nblk=nblk, K=px)


@pytest.mark.parametrize("case", DWG)
def test_dwgate_forward(case):
    o = _dwgate(*case)
    yd64, yd32 = both(R.dwconv, o["y"], o["w"], o["b"])
    elem_check("dwgate", f"yd {case}", o["yd"], yd64, yd32)
    elem_check("dwgate", f"g {case}", o["g"], R.gate(yd64), R.gate(yd32))
    assert torch.equal(o["g_noyd"], o["g"]), "g differs when yd is not stored"


@pytest.mark.parametrize("case", DWG)
def test_dwgate_backward(case):
    """dy and the weight / bias partials of the stored-yd kernel, from the yd the forward stored"""
    o = _dwgate(*case)

    def ref(dg, yd, y, w):
        return R.dwconv_bwd(R.gate_bwd(dg, yd), y, w)

    r64, r32 = both(ref, o["dg"], o["yd"], o["y"], o["w"])
    elem_check("dwgate", f"dy {case}", o["dy"], r64[0], r32[0])
    dw, db = _part_sums(o["part"], o["nblk"], 2 * case[0])
    sum_check("dwgate", f"dw {case}", dw, r64[1], o["K"])
    sum_check("dwgate", f"db {case}", db, r64[2], o["K"])


@pytest.mark.parametrize("case", DWG)
def test_dwgate_backward_recompute_equals_stored(case):
    o = _dwgate(*case)
    assert torch.equal(o["dy_rc"], o["dy"]), "dy: recomputed yd differs from stored yd"
    assert torch.equal(o["part_rc"], o["part"]), "partials: recomputed yd differs from stored yd"


@pytest.mark.parametrize("C", [48, 70])
def test_dw_bwd(C):
    Bn, H, W = 2, 19, 21
    px = Bn * H * W
    dyd, yin, w = _rand(Bn, H, W, C, seed=C), _rand(Bn, H, W, C, seed=C + 1), _rand(C, 9, seed=C + 2)
    ldd, ldi, lddy = C + 1, C + 2, C + 3
    nblk = _blocks(Bn, H, W)
    dyb, part = _out(px, C, lddy), _flat_out(nblk * 10 * C)
    _run(OP_DW_BWD, ins=[(_in(dyd, ldd), ldd), (_in(yin, ldi), ldi)], outs=[(dyb, lddy)], w=w.to(DEV), part=part,
         part_floats=nblk * 10 * C, C=C, Bn=Bn, H=H, W=W)
    r64, r32 = both(R.dwconv_bwd, dyd, yin, w)
    elem_check("dw_bwd", f"dy C={C}", _take(dyb, yin.shape), r64[0], r32[0])
    dw, db = _part_sums(_take_flat(part, (nblk, 10 * C)), nblk, C)
    sum_check("dw_bwd", f"dw C={C}", dw, r64[1], px)
    sum_check("dw_bwd", f"db C={C}", db, r64[2], px)


# (C, ldi, ldo).  The issue's six (ld == C but for one): tile<16>, tile<8>, tile<8> over several groups, a
# partial quad in the tile kernel, the row kernel twice.  Then the same kernels with real pad columns
# (NaN in, sentinel out) and ldi != ldo: tile<16>, tile<8> with a partial quad, the row kernel through
# ld % 4 != 0 on either side and with ld > C on both.
DW_FWD = [(48, 48, 48), (24, 24, 24), (144, 144, 144), (30, 32, 32), (30, 30, 30), (7, 7, 7),
          (48, 52, 56), (30, 36, 32), (30, 33, 33), (30, 32, 35), (7, 9, 10)]


@pytest.mark.parametrize("C,ldi,ldo", DW_FWD)
def test_dw_fwd(C, ldi, ldo):
    Bn, H, W = 2, 19, 37
    x, w, b = _rand(Bn, H, W, C, seed=C), _rand(C, 9, seed=C + 1), _rand(C, seed=C + 2)
    xv, wd, bd = _in(x, ldi), w.to(DEV), b.to(DEV)
    for flip in (0, 1):
        for bias in (None, b):
            ob = _out(Bn * H * W, C, ldo)
            _run(OP_DW_FWD, ins=[(xv, ldi)], outs=[(ob, ldo)], w=wd, bias=None if bias is None else bd, flag=flip, C=C,
                 Bn=Bn, H=H, W=W)
            r64, r32 = both(R.dwconv, x, w, bias, bool(flip))
            elem_check("dw_fwd", f"C={C} ldi={ldi} ldo={ldo} flip={flip} bias={bias is not None}", _take(ob, x.shape),
                       r64, r32)


# ---------------------------------------------------------------------------------------------- dw3_small
@pytest.mark.parametrize("Cin,Cout", [(3, 3), (10, 3), (48, 3), (200, 3), (3, 48), (4, 48), (4, 10)])
@pytest.mark.parametrize("dil", [1, 2])
def test_dw3_small(Cin, Cout, dil):
    Bn, H, W = 2, 9, 11
    P, ncols = Bn * H * W, Cin * Cout * 9
    dy, x = _rand(Bn, H, W, Cout, seed=Cin + Cout), _rand(Bn, H, W, Cin, seed=Cin + Cout + 1)
    ldd, ldx = Cout + 1, Cin + 3
    dyv, xv = _in(dy, ldd), _in(x, ldx)
    ref = R.conv3_weight_grad(dy.double(), x.double(), dil)
    cap = 64 * ncols
    nq = _lib.lib().kdlae_debug_train_blocks(1, P, Cin, Cout, cap)
    assert nq == 5  # >= 48 pixels per block; block 2 (pixels 80..119) crosses the image boundary at 99
    # 120 blocks of 2 pixels: block 49 = pixels (98, 99) spans the two images, blocks 99.. are empty
    for nblk in (nq, 120):
        part = _flat_out(nblk * ncols)
        _run(OP_DW3_SMALL, ins=[(dyv, ldd), (xv, ldx)], part=part, part_floats=nblk * ncols, C=Cin, C2=Cout, Bn=Bn,
             H=H, W=W, flag=dil, nblk=nblk)
        got = _take_flat(part, (nblk, ncols)).double().sum(0).reshape(Cout, Cin, 3, 3)
        sum_check("dw3_small", f"({Cin},{Cout}) dil={dil} nblk={nblk}", got, ref, P)


# ---------------------------------------------------------------------------------------------- column reductions
@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130, 132])
def test_colsum(ncols):
    """ld % 4 both ways and a base one float off 16-byte alignment (the float4 kernel needs ncols % 4 ==
    ld % 4 == 0 and an aligned base: 64 and 132 take it only then), 3 segments, row chunks both below
    and above the row count (rows = 1000 in 3 chunks runs the unrolled main loops), and f = x and x^2
    for every one of these combinations"""
    nseg, ld4 = 3, (ncols + 3) // 4 * 4 + 4
    for rows, nblks in ((1, (1, 3)), (7, (3, 9)), (1000, (3, 1001))):
        x = _rand(nseg, rows, ncols, seed=ncols + rows)
        ref = {0: x.double().sum(1), 1: (x.double() ** 2).sum(1)}
        for ld in (ld4, ld4 + 1):
            xv = _in(x, ld).reshape(-1)
            for off in (0, 1):
                buf = torch.full((xv.numel() + 8,), NAN, device=DEV)
                buf[off:off + xv.numel()] = xv
                for nblk in nblks:
                    for square in (0, 1):
                        part = _flat_out(nseg * nblk * ncols)
                        _run(OP_COLSUM, ins=[(buf, ld, off)], part=part, part_floats=nseg * nblk * ncols, C=ncols,
                             P=rows, nseg=nseg, nblk=nblk, flag=square)
                        got = _take_flat(part, (nseg, nblk, ncols)).double().sum(1)
                        sum_check("reductions",
                                  f"colsum ncols={ncols} rows={rows} ld={ld} off={off} nblk={nblk} sq={square}",
                                  got, ref[square], rows)


@pytest.mark.parametrize("ncols", [1, 63, 64, 65, 130, 132])
def test_part_reduce(ncols):
    nseg, scale = 3, 0.37
    for nblk in (1, 17, 100):
        for pstride in (0, ncols + 5):
            for accumulate in (0, 1):
                part = _rand(nseg, nblk, ncols, seed=ncols + nblk)
                pv = part.to(DEV) if pstride == 0 else _in(part, pstride)
                prev = _rand(nseg, ncols, seed=ncols + 7)
                out = _flat_out(nseg * ncols)
                out[:nseg * ncols] = prev.reshape(-1).to(DEV)
                _run(OP_PART_REDUCE, ins=[(pv, 0)], outs=[(out, 0)], C=ncols, nblk=nblk, nseg=nseg, pstride=pstride,
                     accumulate=accumulate, scale=scale)
                ref = float(torch.tensor(scale)) * part.double().sum(1) + (prev.double() if accumulate else 0)
                sum_check("reductions", f"part_reduce ncols={ncols} nblk={nblk} pstride={pstride} acc={accumulate}",
                          _take_flat(out, (nseg, ncols)), ref, nblk)


@pytest.mark.parametrize("n", [1, 8])
def test_part_reduce_multi(n):
    shapes = [(130, 70, 135), (1, 1, 1), (64, 17, 64), (65, 3, 80), (9, 100, 12), (132, 16, 132), (63, 65, 64),
              (3, 49, 7)][:n]  # (ncols, nblk, pstride)
    d = TrainDesc()
    d.op, d.nred = OP_PART_REDUCE_MULTI, n
    keep = []
    for j, (ncols, nblk, pstride) in enumerate(shapes):
        part = _rand(nblk, ncols, seed=100 + j)
        pv, out = _in(part, pstride), _flat_out(ncols)
        keep.append((part, pv, out))
        r = d.red[j]
        r.part, r.out, r.nblk, r.ncols, r.pstride, r.scale = _ptr(pv), _ptr(out), nblk, ncols, pstride, 0.5 + j
    _lib.check(_lib.lib().kdlae_debug_train(ctypes.byref(d), None), "kdlae_debug_train op 10")
    torch.cuda.synchronize()
    for j, (ncols, nblk, pstride) in enumerate(shapes):
        part, _, out = keep[j]
        sum_check("reductions", f"part_reduce_multi {j + 1}/{n}", _take_flat(out, (ncols,)),
                  (0.5 + j) * part.double().sum(0), nblk)


# ---------------------------------------------------------------------------------------------- layout (exact)
@pytest.mark.parametrize("C", [3, 5])
def test_shuffle_exact(C):
    Bn, h, w = 2, 3, 5
    hi = _rand(Bn, 2 * h, 2 * w, C, seed=C)
    lo = R.unshuffle(hi)
    ob = _out(Bn * h * w, 4 * C, 4 * C + 3)
    _run(OP_SHUFFLE, ins=[(_in(hi, C + 2), C + 2)], outs=[(ob, 4 * C + 3)], C=C, Bn=Bn, H=h, W=w, flag=0)
    assert torch.equal(_take(ob, lo.shape), lo)
    ob = _out(Bn * 4 * h * w, C, C + 1)
    _run(OP_SHUFFLE, ins=[(_in(lo, 4 * C + 1), 4 * C + 1)], outs=[(ob, C + 1)], C=C, Bn=Bn, H=h, W=w, flag=1)
    assert torch.equal(_take(ob, hi.shape), R.shuffle(lo)) and torch.equal(R.shuffle(lo), hi)


def test_nchw_nhwc_copies_exact():
    Bn, C, HW = 2, 5, 15
    x = _rand(Bn, C, HW, seed=1)              # NCHW
    xl = x.permute(0, 2, 1).contiguous()      # [Bn, HW, C]
    prev = _rand(Bn, HW, C, seed=2)
    for accumulate in (0, 1):
        ob = _out(Bn * HW, C, C + 3, prefill=prev)
        _run(OP_NCHW_TO_NHWC, ins=[(x.to(DEV), 0)], outs=[(ob, C + 3)], C=C, Bn=Bn, P=HW, accumulate=accumulate)
        assert torch.equal(_take(ob, xl.shape), prev + xl if accumulate else xl)
    add = _rand(Bn, C, HW, seed=3)
    for a in (None, add):
        out = _flat_out(Bn * C * HW)
        _run(OP_NHWC_TO_NCHW, ins=[(_in(xl, C + 2), C + 2), (None if a is None else a.to(DEV), 0)], outs=[(out, 0)],
             C=C, Bn=Bn, P=HW)
        assert torch.equal(_take_flat(out, x.shape), x if a is None else x + a)


def test_copy_cols_and_pack_w3_exact():
    P, C, zero_to, ldo = 37, 5, 8, 11
    x, prev = _rand(P, C, seed=4), _rand(P, zero_to, seed=5)
    xv = _in(x, C + 2)
    for accumulate in (0, 1):
        for zt in (0, zero_to):
            width = max(C, zt)
            ob = _out(P, width, ldo, prefill=prev[:, :width])
            _run(OP_COPY_COLS, ins=[(xv, C + 2)], outs=[(ob, ldo)], C=C, P=P, accumulate=accumulate, zero_to=zt)
            ref = torch.zeros(P, width)
            ref[:, :C] = prev[:, :C] + x if accumulate else x
            assert torch.equal(_take(ob, (P, width)), ref), (accumulate, zt)
    Cg, N = 5, 7
    for mode, W in ((2, _rand(N, Cg, 3, 3, seed=6)), (3, _rand(Cg, N, 3, 3, seed=7))):
        out = _flat_out(9 * Cg * N)
        _run(OP_PACK_W3, outs=[(out, 0)], w=W.to(DEV), C=Cg, C2=N, flag=mode)
        assert torch.equal(_take_flat(out, (9 * Cg, N)), R.pack_w3(W, mode)), mode


# ---------------------------------------------------------------------------------------------- KDLAE-S
S_CASES = [(C, Fr) for C in (4, 12) for Fr in (1, 2, 3)]
SB, SH, SW = 2, 6, 10


def _tied_pool_input(C, Fr, seed):
    """[2, F, 6, 10, C] where every 2 x 2 window holds its maximum 2, 3 or 4 times (cycling over the
    windows) at random positions; the other elements are lower"""
    g = torch.Generator().manual_seed(seed)
    n = SB * Fr * (SH // 2) * (SW // 2) * C
    rank = torch.rand(n, 4, generator=g).argsort(1).argsort(1)
    m = torch.arange(n) % 3 + 2
    vals = torch.where(rank < m[:, None], 2 + torch.rand(n, 1, generator=g), torch.rand(n, 4, generator=g))
    ties = (vals == vals.max(1, keepdim=True).values).sum(1)
    assert all((ties == k).any() for k in (2, 3, 4)) and (ties >= 2).all()
    # and the first maximum is not always the window's first element
    assert (vals.argmax(1) > 0).any()
    v = vals.reshape(SB, Fr, SH // 2, SW // 2, C, 2, 2).permute(0, 1, 2, 5, 3, 6, 4)
    return v.reshape(SB, Fr, SH, SW, C).contiguous().float()


@pytest.mark.parametrize("C,Fr", S_CASES)
def test_maxpool2_bwd_first_maximum_exact(C, Fr):
    inp = _tied_pool_input(C, Fr, seed=C + Fr)
    dout, dskip = _rand(SB, Fr, SH // 2, SW // 2, C, seed=C), _rand(SB, Fr, SH, SW, C, seed=C + 1)
    px = SB * Fr * SH * SW
    iv, dv, sv = _in(inp, C + 1), _in(dout, C + 2), _in(dskip, C + 3)
    for skip in (None, dskip):
        ob = _out(px, C, C + 5)
        _run_s(S_MAXPOOL_BWD, ins=[(iv, C + 1), (dv, C + 2), (None if skip is None else sv, C + 3)], outs=[(ob, C + 5)],
               C=C, B=SB, F=Fr, H=SH // 2, W=SW // 2)
        assert torch.equal(_take(ob, inp.shape), R.maxpool2_bwd(inp, dout, skip)), skip is not None


@pytest.mark.parametrize("C,Fr", S_CASES)
def test_im2col3d_exact_and_col2im3d(C, Fr):
    px = SB * Fr * SH * SW
    x = _rand(SB, Fr, SH, SW, C, seed=C + Fr)
    ref = R.im2col3d(x)
    for ld in (C + 4, C + 1):  # the float4 and the scalar kernel
        col = _flat_out(px * 27 * C)
        _run_s(S_IM2COL, ins=[(_in(x, ld), ld)], outs=[(col, 0)], C=C, B=SB, F=Fr, H=SH, W=SW)
        assert torch.equal(_take_flat(col, ref.shape), ref), ld
    dcol, prev = _rand(SB, Fr, SH, SW, 27 * C, seed=C + Fr + 1), _rand(SB, Fr, SH, SW, C, seed=C + Fr + 2)
    dref = R.col2im3d(dcol.double())
    for accumulate in (0, 1):
        ob = _out(px, C, C + 4, prefill=prev)
        _run_s(S_COL2IM, ins=[(dcol.to(DEV), 0)], outs=[(ob, C + 4)], C=C, B=SB, F=Fr, H=SH, W=SW, accumulate=accumulate)
        sum_check("kdlae_s", f"col2im3d C={C} F={Fr} acc={accumulate}", _take(ob, x.shape),
                  dref + (prev.double() if accumulate else 0), 27)


@pytest.mark.parametrize("C,Fr", S_CASES)
def test_upshuffle_relu_mask_wperm_exact(C, Fr):
    px = SB * Fr * SH * SW
    U, bias = _rand(SB, Fr, SH // 2, SW // 2, 4 * C, seed=C + Fr), _rand(C, seed=C)
    skip = _rand(SB, Fr, SH, SW, C, seed=C + Fr + 1)
    uv, kv = _in(U, 4 * C + 3), _in(skip, C + 1)
    for b in (None, bias):
        ob = _out(px, C, C + 2)
        _run_s(S_UPSHUFFLE, ins=[(uv, 4 * C + 3), (kv, C + 1)], outs=[(ob, C + 2)], bias=None if b is None else b.to(DEV),
               C=C, B=SB, F=Fr, H=SH, W=SW)
        assert torch.equal(_take(ob, skip.shape), R.upshuffle_add(U, b, skip)), b is not None
    y = torch.relu(_rand(SB, Fr, SH, SW, C, seed=C + Fr + 2))  # about half exact zeros
    dy = _rand(SB, Fr, SH, SW, C, seed=C + Fr + 3)
    ob = _out(px, C, C + 3, prefill=dy)
    _run_s(S_RELU_MASK, ins=[(_in(y, C + 1), C + 1)], outs=[(ob, C + 3)], C=C, B=SB, F=Fr, H=SH, W=SW)
    assert torch.equal(_take(ob, dy.shape), R.relu_mask(dy, y))
    O = 6
    w = _rand(O, C, 27, seed=C + 9)
    out = _flat_out(O * C * 27)
    _run_s(S_WPERM, ins=[(w.to(DEV), 0)], outs=[(out, 0)], O=O, C=C, dir=0)
    wp = _take_flat(out, (O, 27, C))
    assert torch.equal(wp, R.wperm(w))
    out = _flat_out(O * C * 27)
    _run_s(S_WPERM, ins=[(wp.to(DEV), 0)], outs=[(out, 0)], O=O, C=C, dir=1)
    assert torch.equal(_take_flat(out, w.shape), w)

"""The operand generators of tests/gemm_precision_inputs.py have teeth: on the CPU model of the
split-bf16 contract (emulate_mfma6), the six-term scheme stays inside the bounds the GPU tests use
(tests/test_gemm_precision_gpu.py) and every scheme with one of the six terms removed falls outside
them, for each input class and contraction length those tests use.  A wrong kernel is modelled here,
on the CPU; no project code is altered."""
import pytest
import torch

import gemm_precision_inputs as G


def _five():
    return [(t, tuple(s for s in G.SIX if s != t)) for t in G.SIX]


# ------------------------------------------------------------------------------------- split identity
@pytest.mark.parametrize("scale", [0, 40, -40])
@pytest.mark.parametrize("positive", [True, False])
def test_split_planes_sum_exactly(positive, scale):
    """h + m + l == x bit for bit, for both generator modes, also scaled by 2^+-40; every plane is a
    bf16 value."""
    x = G.piece_operand((64, 96), 3, positive) * 2.0 ** scale
    h, m, l = G.split3_ref(x)
    assert torch.equal(h + m + l, x.double())
    for p in (h, m, l):
        assert torch.equal(p.float().to(torch.bfloat16).double(), p)
    # scaling by a power of two commutes with the split
    h0, m0, l0 = G.split3_ref(G.piece_operand((64, 96), 3, positive))
    assert torch.equal(h, h0 * 2.0 ** scale) and torch.equal(m, m0 * 2.0 ** scale) and torch.equal(l, l0 * 2.0 ** scale)


def test_positive_pieces_are_the_planes():
    """positive=True: every plane of every value is positive (the nine plane products share a sign),
    and the planes have the sizes the generator promises."""
    x = G.piece_operand((64, 96), 5, True)
    h, m, l = G.split3_ref(x)
    assert bool((h > 0).all() and (m > 0).all() and (l > 0).all())
    assert bool((m / h >= 2.0 ** -11).all() and (m / h < 2.0 ** -8).all())
    assert bool((l / h >= 2.0 ** -20).all() and (l / h < 2.0 ** -17).all())


def test_random_sign_operand_has_both_signs():
    x = G.piece_operand((64, 96), 6, False)
    assert bool((x > 0).any() and (x < 0).any())
    assert bool((x.abs() >= 2.0 ** -4).all() and (x.abs() < 2.0 ** 4).all())


# ------------------------------------------------------------------------------------- generators
def test_one_hot_rows_hit_every_k():
    A = G.one_hot_rows(200, 40, 1)
    assert bool(((A != 0).sum(1) == 1).all()) and bool(((A != 0).sum(0) >= 1).all())


def test_one_hot_pixels():
    A, B = G.one_hot_pixels(512, 29, 31, 2)
    assert bool(((A != 0).sum(1) >= 1).all())      # every pixel carries part of the contraction


@pytest.mark.parametrize("kt,dil,Cin", [(1, 1, 32), (1, 2, 16), (3, 1, 32), (3, 2, 16)])
def test_conv_lattice_one_product_per_output(kt, dil, Cin):
    """At most one nonzero column of the im2col matrix per output pixel, every k index in some row."""
    x = G.conv_lattice(2, 3 if kt == 3 else 1, 16, 32, Cin, dil, kt, 4)
    cols = G.im2col(x, dil, kt)
    assert int((cols != 0).sum(1).max()) == 1
    assert bool(((cols != 0).sum(0) >= 1).all())


def test_im2col_is_the_convolution():
    x = G.piece_operand((2, 3, 5, 6, 4), 8, False)
    w = G.piece_operand((7, 4, 3, 3, 3), 9, False)
    ref = torch.nn.functional.conv3d(x.double().permute(0, 4, 1, 2, 3), w.double(), padding=(1, 2, 2), dilation=(1, 2, 2))
    got = G.im2col(x, 2, 3).double() @ w.double().permute(0, 2, 3, 4, 1).reshape(7, -1).T
    torch.testing.assert_close(got, ref.permute(0, 2, 3, 4, 1).reshape(-1, 7), rtol=1e-12, atol=1e-10)


# ------------------------------------------------------------------------------------- discrimination
def _separates(A, Wt, bias, R, bound, what):
    ref, den = G.ref_den(A, Wt, bias, R)
    e6 = G.rel_err(G.emulate_mfma6(A, Wt, G.SIX, bias, R), ref, den)
    print(f"{what}: six terms {e6 / bound:.3f} of the bound")
    assert e6 <= bound, f"{what}: the correct scheme misses the bound ({e6:.3e} > {bound:.3e})"
    for t, five in _five():
        e5 = G.rel_err(G.emulate_mfma6(A, Wt, five, bias, R), ref, den)
        print(f"{what}: without {t} {e5 / bound:.3f} of the bound")
        assert e5 > bound, f"{what}: dropping {t} stays inside the bound ({e5:.3e} <= {bound:.3e})"


@pytest.mark.parametrize("K", [40, 48, 96, 256, 368])
def test_one_hot_separates(K):
    """One-hot rows with dense weights, bias and residual: 2^-21 holds for six terms, fails for five."""
    _separates(*G.one_hot_case(2 * K, K, 48, K), G.ONE_HOT_BOUND, f"one-hot K{K}")


@pytest.mark.parametrize("kt,dil,Cin", [(1, 1, 32), (1, 2, 16), (3, 1, 32), (3, 2, 16)])
def test_lattice_separates(kt, dil, Cin):
    """The conv lattice through im2col: the same one-hot bound."""
    x = G.conv_lattice(2, 3 if kt == 3 else 1, 16, 32, Cin, dil, kt, 10 + kt + dil)
    Wt = G.piece_operand((32, 9 * kt * Cin), 20 + kt + dil, False)
    bias = G.piece_operand(32, 30 + kt, False)
    _separates(G.im2col(x, dil, kt), Wt, bias, None, G.ONE_HOT_BOUND, f"lattice kt{kt} dil{dil}")


def test_one_hot_pixels_separates():
    """The pixel contraction of the weight-gradient kernel: both operands are activations."""
    A, B = G.one_hot_pixels(512, 29, 31, 40)
    _separates(A.T.contiguous(), B.T.contiguous(), None, None, G.ONE_HOT_BOUND, "one-hot pixels")


@pytest.mark.parametrize("chunks", [1, 2])
@pytest.mark.parametrize("K", G.COHERENT_KS)
def test_coherent_separates(K, chunks):
    """Dense positive operands at every K of the coherent class (chunks = 2: the widest bound in use)."""
    _separates(*G.coherent_case(96, K, 48, 100 + K), G.coherent_bound(K, chunks), f"coherent K{K}")

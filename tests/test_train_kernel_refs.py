"""The closed-form references of tests/train_kernel_refs.py against float64 torch.autograd (and
against the torch modules they restate) on small random inputs, to 1e-12 relative: the reference the
GPU kernel tests compare with is itself checked here, on any machine."""
import torch
import torch.nn.functional as F

from tests import train_kernel_refs as R

RTOL = 1e-12


def _rand(*shape, seed=0):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(*shape, generator=g, dtype=torch.float64) * 2 - 1


def _same(got, ref, what):
    err = (got - ref).abs().max().item()
    assert err <= RTOL * max(ref.abs().max().item(), 1e-300), f"{what}: {err:.3e}"


def test_dwconv_definition():
    """out[p, c] = sum_t w[c, t] x[p + off_t, c] with explicit loops, both tap orders."""
    x, w, b = _rand(2, 4, 5, 3, seed=1), _rand(3, 9, seed=2), _rand(3, seed=3)
    for flip in (False, True):
        ref = torch.zeros_like(x)
        xp = F.pad(x, (0, 0, 1, 1, 1, 1))
        for t in range(9):
            ref += w[:, 8 - t if flip else t] * xp[:, t // 3:t // 3 + 4, t % 3:t % 3 + 5]
        _same(R.dwconv(x, w, b, flip), ref + b, f"dwconv flip={flip}")


def test_gate_and_dwconv_backward_match_autograd():
    hid = 3
    y = _rand(2, 5, 6, 2 * hid, seed=4).requires_grad_()
    w = _rand(2 * hid, 9, seed=5).requires_grad_()
    b = _rand(2 * hid, seed=6).requires_grad_()
    dg = _rand(2, 5, 6, hid, seed=7)
    yd = R.dwconv(y, w, b)
    yd.retain_grad()
    (R.gate(yd) * dg).sum().backward()
    dyd = R.gate_bwd(dg, yd.detach())
    _same(dyd, yd.grad, "gate_bwd")
    dy, dw, db = R.dwconv_bwd(dyd, y.detach(), w.detach())
    _same(dy, y.grad, "dwconv dy")
    _same(dw, w.grad, "dwconv dw")
    _same(db, b.grad, "dwconv db")


def test_conv3_weight_grad_matches_autograd():
    for dil in (1, 2):
        x, dy = _rand(2, 6, 7, 4, seed=8), _rand(2, 6, 7, 3, seed=9)
        W = _rand(3, 4, 3, 3, seed=10).requires_grad_()
        out = F.conv2d(x.permute(0, 3, 1, 2), W, padding=dil, dilation=dil)
        (out * dy.permute(0, 3, 1, 2)).sum().backward()
        _same(R.conv3_weight_grad(dy, x, dil), W.grad, f"conv3 dW dil={dil}")


def _attn_inputs(B, heads, Ch, P, seed, zero_q=None, zero_k=None):
    C = heads * Ch
    q, k = _rand(B, heads, Ch, P, seed=seed), _rand(B, heads, Ch, P, seed=seed + 1)
    if zero_q is not None:
        q[zero_q] = 0
    if zero_k is not None:
        k[zero_k] = 0
    G = q @ k.transpose(-1, -2)
    sumsq = torch.cat([(q * q).sum(-1).reshape(B, C), (k * k).sum(-1).reshape(B, C)], dim=1)
    temp = 1.0 + 0.5 * torch.arange(heads, dtype=torch.float64)
    return G, sumsq, temp, _rand(B, heads, Ch, Ch, seed=seed + 2)


def test_attn_core_backward_matches_autograd():
    B, heads, Ch = 2, 2, 5
    G, sumsq, temp, dA = _attn_inputs(B, heads, Ch, 7, seed=11)
    G.requires_grad_(), sumsq.requires_grad_(), temp.requires_grad_()
    A = R.attn_core(G, sumsq, temp)
    (A * dA).sum().backward()
    Mq, cq, ck, dt = R.attn_core_bwd(G.detach(), sumsq.detach(), temp.detach(), A.detach(), dA)
    C = heads * Ch
    _same(Mq, G.grad, "Mq")
    _same(cq.reshape(B, C), 2 * sumsq.grad[:, :C], "cq")
    _same(ck.reshape(B, C), 2 * sumsq.grad[:, C:], "ck")
    _same(dt.sum(0), temp.grad, "dtemp")


def test_attn_core_backward_clamped_norms():
    """sumsq = 0 for one q row and one k column: autograd gives NaN there (0 * inf through sqrt under the
    clamp), the rule is coefficient 0; everything else still matches autograd."""
    B, heads, Ch = 2, 2, 5
    zq, zk = (0, 1, 2), (1, 0, 3)
    G, sumsq, temp, dA = _attn_inputs(B, heads, Ch, 7, seed=21, zero_q=zq, zero_k=zk)
    G.requires_grad_(), sumsq.requires_grad_(), temp.requires_grad_()
    A = R.attn_core(G, sumsq, temp)
    (A * dA).sum().backward()
    Mq, cq, ck, dt = R.attn_core_bwd(G.detach(), sumsq.detach(), temp.detach(), A.detach(), dA)
    for t in (Mq, cq, ck, dt):
        assert torch.isfinite(t).all()
    C = heads * Ch
    gq = 2 * sumsq.grad[:, :C].reshape(B, heads, Ch)
    gk = 2 * sumsq.grad[:, C:].reshape(B, heads, Ch)
    assert torch.isnan(gq[zq]) and torch.isnan(gk[zk])
    assert cq[zq] == 0 and ck[zk] == 0
    keep_q, keep_k = torch.ones_like(cq, dtype=torch.bool), torch.ones_like(ck, dtype=torch.bool)
    keep_q[zq], keep_k[zk] = False, False
    _same(cq[keep_q], gq[keep_q], "cq")
    _same(ck[keep_k], gk[keep_k], "ck")
    _same(Mq, G.grad, "Mq")
    _same(dt.sum(0), temp.grad, "dtemp")


def test_shuffle_is_inverse_of_unshuffle_and_pack_w3_definition():
    x = _rand(2, 6, 10, 3, seed=30)
    u = R.unshuffle(x)
    assert u.shape == (2, 3, 5, 12) and torch.equal(R.shuffle(u), x)
    assert u[1, 2, 4, 2 * 4 + 1 * 2 + 0] == x[1, 2 * 2 + 1, 2 * 4 + 0, 2]
    N, Cg = 4, 3
    W2, W3 = _rand(N, Cg, 3, 3, seed=31), _rand(Cg, N, 3, 3, seed=32)
    p2, p3 = R.pack_w3(W2, 2), R.pack_w3(W3, 3)
    for t in range(9):
        for c in range(Cg):
            for n in range(N):
                assert p2[t * Cg + c, n] == W2.reshape(N, Cg, 9)[n, c, t]
                assert p3[t * Cg + c, n] == W3.reshape(Cg, N, 9)[c, n, 8 - t]


def test_maxpool_backward_first_maximum_matches_torch():
    """tie-rich input (a few integer levels after a ReLU): torch's MaxPool3d backward routes to the first
    maximum of the window in (row, column) order."""
    g = torch.Generator().manual_seed(33)
    inp = torch.randint(-2, 3, (2, 3, 6, 10, 4), generator=g).double().clamp_min(0).requires_grad_()
    dout, dskip = _rand(2, 3, 3, 5, 4, seed=34), _rand(2, 3, 6, 10, 4, seed=35)
    out = F.max_pool3d(inp.permute(0, 4, 1, 2, 3), (1, 2, 2))
    (out * dout.permute(0, 4, 1, 2, 3)).sum().backward()
    assert torch.equal(R.maxpool2_bwd(inp.detach(), dout), inp.grad)
    assert torch.equal(R.maxpool2_bwd(inp.detach(), dout, dskip), inp.grad + dskip)


def test_im2col3d_is_the_conv3d_operand_and_col2im3d_its_adjoint():
    for Fr in (1, 2, 3):
        x = _rand(2, Fr, 4, 5, 3, seed=36).requires_grad_()
        W = _rand(6, 3, 3, 3, 3, seed=37)
        col = R.im2col3d(x)
        # Conv3d forward = Xcol . W'^T with W' = wperm(W)
        out = col @ R.wperm(W.reshape(6, 3, 27)).reshape(6, 81).t()
        ref = F.conv3d(x.permute(0, 4, 1, 2, 3), W, padding=1).permute(0, 2, 3, 4, 1)
        _same(out, ref, "im2col conv3d")
        d = _rand(*col.shape, seed=38)
        (col * d).sum().backward()
        _same(R.col2im3d(d), x.grad, f"col2im F={Fr}")


def test_upshuffle_add_is_the_transposed_conv():
    x, Wt = _rand(2, 2, 3, 5, 6, seed=39), _rand(6, 4, 1, 2, 2, seed=40)
    bias, skip = _rand(4, seed=41), _rand(2, 2, 6, 10, 4, seed=42)
    U = x @ Wt.reshape(6, 16)  # U[p, 4 o + 2 i + j]
    ref = F.conv_transpose3d(x.permute(0, 4, 1, 2, 3), Wt, bias, stride=(1, 2, 2)).permute(0, 2, 3, 4, 1) + skip
    _same(R.upshuffle_add(U, bias, skip), ref, "upshuffle_add")
    assert torch.equal(R.relu_mask(skip, ref), torch.where(ref > 0, skip, torch.zeros_like(skip)))

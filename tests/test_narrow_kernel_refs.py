"""The references of tests/narrow_kernel_refs.py against torch's own functions, and proof that the GPU
tests of tests/test_narrow_kernels_gpu.py can see the mistakes their kernels could make: every mutant
below, applied to an explicit model of the operation on the GPU test's own inputs, moves a compared
quantity by more than that quantity's tolerance.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import narrow_kernel_refs as R

D = torch.float64


def _same(a, b, tol=1e-12):
    err = (a - b).abs().max().item()
    assert err <= tol * (1 + b.abs().max().item()), err


# ------------------------------------------------------------------ narrow-input 3x3 conv
def _small_in_explicit(x, sub, w, bias, dil, vh, vw, relu, wt, mutant=None):
    """The conv as a sum over taps of shifted images times a [Cout][Cin][9] weight block, with the mistakes
    the kernel could make switched in by name."""
    x = x.to(D)
    if sub is not None and mutant != "sub_ignored":
        x = x - sub.to(D)
    Bn, Cin, H, W = x.shape
    if (vh or vw) and mutant != "extent_ignored":
        x = x.clone()
        x[:, :, vh or H:, :] = 0
        x[:, :, :, vw or W:] = 0
    w = w.to(D)
    if wt:
        Cout = w.shape[1]
        blk = w.permute(1, 0, 2, 3).reshape(Cout, Cin, 9)
        if mutant == "wt_pass2_offset":  # the second 128-channel pass reads the first pass's weights
            blk = torch.cat([blk[:128], blk[:Cout - 128]])
        if mutant != "wt_taps_not_flipped":
            blk = blk.flip(-1)
    else:
        Cout = w.shape[0]
        blk = w.reshape(Cout, Cin, 9)
    if mutant == "k_tap_major":  # the gather walks k = tap Cin + ci while the weights stay k = ci 9 + tap
        blk = blk.reshape(Cout, 9, Cin).permute(0, 2, 1)
    dil_x = 1 if mutant == "dilation_one_axis" else dil
    xp = F.pad(x, (dil_x, dil_x, dil, dil))
    out = x.new_zeros(Bn, Cout, H, W)
    for tap in range(9):
        ky, kx = tap // 3, tap % 3
        out += torch.einsum("bchw,nc->bnhw", xp[:, :, ky * dil:ky * dil + H, kx * dil_x:kx * dil_x + W], blk[:, :, tap])
    if bias is not None:
        b = bias.to(D)
        if mutant == "pass2_bias_from_0":
            b = torch.cat([b[:128], b[:Cout - 128]])
        out += b.view(1, -1, 1, 1)
    return out.clamp_min(0) if relu else out


def _applies(mutant, c):
    return {"wt_taps_not_flipped": c["wt"], "k_tap_major": c["Cin"] > 1, "dilation_one_axis": c["dil"] > 1,
            "extent_ignored": c["vh"] > 0, "sub_ignored": c["sub"], "pass2_bias_from_0": c["Cout"] > 128 and c["bias"],
            "wt_pass2_offset": c["wt"] and c["Cout"] > 128}[mutant]


SMALL_IN_MUTANTS = ("wt_taps_not_flipped", "k_tap_major", "dilation_one_axis", "extent_ignored", "sub_ignored",
                    "pass2_bias_from_0", "wt_pass2_offset")


def _args(c):
    x, sub, w, bias = R.small_in_inputs(c)
    return x, sub, w, bias, c["dil"], c["vh"], c["vw"], c["relu"], c["Cout"] if c["wt"] else 0


def test_small_in_cases_cover_every_axis_per_cin():
    cases = R.small_in_cases()
    assert 40 <= len(cases) <= 52 and len({R.small_in_id(c) for c in cases}) == len(cases)
    for Cin in (1, 2, 3, 4):
        mine = [c for c in cases if c["Cin"] == Cin and not c["wt"]]
        for key, values in (("Cout", (16, 48, 96, 144)), ("dil", (1, 2)), ("layout", ("nchw", "nhwc")),
                            ("bias", (0, 1)), ("relu", (0, 1)), ("sub", (0, 1))):
            assert {c[key] for c in mine} >= set(values), (Cin, key)
    wt = {(c["Cin"], c["Cout"], c["dil"]) for c in cases if c["wt"]}
    assert wt == {(ci, co, d) for ci in (3, 4) for co in (48, 96, 144) for d in (1, 2)}
    assert any(c["H"] == 2 and c["W"] == 3 and c["dil"] == 2 for c in cases)


@pytest.mark.parametrize("c", R.small_in_cases(), ids=R.small_in_id)
def test_small_in_reference_and_mutants(c):
    """The reference equals the explicit tap sum; for wt it equals autograd's input gradient of the conv
    being transposed; every applicable mutant moves the result past the GPU test's tolerance."""
    a = _args(c)
    ref = R.small_in_2d(*a)
    _same(_small_in_explicit(*a), ref)
    x, sub, w, bias = a[:4]
    if c["wt"]:
        # forward conv Cout -> Cin of weight w [Cin][Cout][3][3]; its dX for upstream gradient x
        z = torch.zeros(c["Bn"], c["Cout"], c["H"], c["W"], dtype=D, requires_grad=True)
        F.conv2d(z, w.to(D), padding=c["dil"], dilation=c["dil"]).backward(x.to(D))
        _same(z.grad + (0 if bias is None else bias.to(D).view(1, -1, 1, 1)), ref)
    t = R.tol(ref, 9 * c["Cin"])
    for m in SMALL_IN_MUTANTS:
        if _applies(m, c):
            moved = (_small_in_explicit(*a, mutant=m) - ref).abs().max().item()
            assert moved > 10 * t, (m, moved, t)


def test_small_in_every_mutant_is_exercised():
    cases = R.small_in_cases()
    for m in SMALL_IN_MUTANTS:
        assert sum(bool(_applies(m, c)) for c in cases) >= 2, m


# ------------------------------------------------------------------ regressor head
def _head_explicit(t, inv_hw, mutant=None):
    """The head's forward and hand-derived backward in float64, with the kernels' possible mistakes
    switched in by name.  (The reference itself uses autograd; this model exists to carry the mutants.)"""
    d = lambda v: None if v is None else v.to(D)
    p = {k: d(v) for k, v in t.items()}
    B = p["partial"].shape[0]
    one = lambda n: torch.ones(B, n, dtype=D)
    m1 = p["mask1"] if p["mask1"] is not None else one(p["w1"].shape[0])
    m2 = p["mask2"] if p["mask2"] is not None else one(p["w2"].shape[0])
    g = p["partial"].sum(1) * (1.0 if mutant == "inv_hw_dropped" else inv_hw)
    f = g @ p["wo"].t() + p["bo"]
    a1 = f @ p["w1"].t() + p["b1"]
    h1 = a1.clamp_min(0) * m1
    a2 = h1 @ p["w2"].t() + p["b2"]
    h2 = a2.clamp_min(0) * m2
    score = torch.tanh(h2 @ p["w3"] + p["b3"])
    da3 = p["dscore"] * (1.0 if mutant == "tanh_derivative_dropped" else 1 - score * score)
    up2 = da3[:, None] * p["w3"][None, :]
    if mutant == "gate_on_masked_h_keeps_mask":      # equivalent: m >= 0, so [relu(a) m > 0] m = [a > 0] m
        da2 = (h2 > 0).to(D) * up2 * m2
    elif mutant == "gate_on_masked_h":               # the gate taken from h = relu(a) m in place of the mask factor
        da2 = (h2 > 0).to(D) * up2
    elif mutant == "mask2_missing":
        da2 = (a2 > 0).to(D) * up2
    else:
        da2 = (a2 > 0).to(D) * up2 * m2
    da1 = (a1 > 0).to(D) * (da2 @ p["w2"]) * m1
    df = da1 @ p["w1"]
    out = {"score": score, "dgap": df @ p["wo"]}
    h1w = a1.clamp_min(0) if mutant == "mask1_missing_in_dw2" else h1
    rows = slice(B - 1, B) if mutant == "last_image_only" else slice(0, B)
    outer = lambda a, b: a[rows].t() @ b[rows]
    out.update(gwo=outer(df, g), gbo=df[rows].sum(0), gw1=outer(da1, f), gb1=da1[rows].sum(0),
               gw2=outer(da2, h1w), gb2=da2[rows].sum(0), gw3=(da3[rows, None] * h2[rows]).sum(0),
               gb3=da3[rows].sum().view(1))
    return out


HEAD_MUTANTS = ("mask1_missing_in_dw2", "mask2_missing", "gate_on_masked_h", "tanh_derivative_dropped",
                "inv_hw_dropped", "last_image_only")
_NEEDS_MASK = ("mask1_missing_in_dw2", "mask2_missing", "gate_on_masked_h")


@pytest.mark.parametrize("case", R.head_cases(), ids=lambda c: "-".join(map(str, c)))
def test_head_reference_and_mutants(case):
    C, M, N1, N2, slots, masks = case
    t = R.head_inputs(*case)
    ref = R.head_train(inv_hw=R.HEAD_INV_HW, **t)
    got = _head_explicit(t, R.HEAD_INV_HW)
    assert set(ref) == {"score", "dgap", *R.HEAD_GRADS}
    for k in ref:
        _same(got[k], ref[k].view(got[k].shape))
    # the inputs hold what the GPU test relies on
    assert t["dscore"][1] == 0 and (t["dscore"] != 0).sum() == R.HEAD_B - 1
    assert ref["gw1"][3].abs().max() == 0 and ref["gb1"][3] == 0
    assert ref["gw2"][N2 - 1].abs().max() == 0 and ref["gb2"][N2 - 1] == 0
    if masks:
        for m in (t["mask1"], t["mask2"]):
            assert set(m.unique().tolist()) == {0.0, 2.0}
    # every compared quantity is many tolerances large, so the rule's absolute term hides no gradient
    for k in ref:
        assert ref[k].abs().max().item() > 50 * R.tol(ref[k], R.head_K(k, C, M, N1, N2)), k
    # with the mask factor kept, gating on the masked activation is the same function: no input separates them
    eq = _head_explicit(t, R.HEAD_INV_HW, mutant="gate_on_masked_h_keeps_mask")
    assert all(torch.equal(eq[k], got[k]) for k in got)
    for m in HEAD_MUTANTS:
        if m in _NEEDS_MASK and not masks:
            continue
        mut = _head_explicit(t, R.HEAD_INV_HW, mutant=m)
        ratio = max((mut[k] - got[k]).abs().max().item() / R.tol(ref[k], R.head_K(k, C, M, N1, N2)) for k in got)
        assert ratio > 10, (m, ratio)


def test_head_fp32_order_error_is_inside_the_rule():
    """The fp32 evaluation of the same reference, an equally valid fp32 order, stays inside each quantity's
    tolerance on the GPU test's inputs: the rule leaves room for a correct fp32 kernel."""
    worst = 0.0
    for case in R.head_cases():
        C, M, N1, N2, slots, masks = case
        t = R.head_inputs(*case)
        ref = R.head_train(inv_hw=R.HEAD_INV_HW, **t)
        f32 = _head_explicit_f32(t)
        for k in ref:
            r = (f32[k].to(D) - ref[k].view(f32[k].shape)).abs().max().item() / R.tol(ref[k], R.head_K(k, C, M, N1, N2))
            worst = max(worst, r)
    print(f"RATIO head_fp32_torch {worst:.4f}")
    assert worst < 0.25


def _head_explicit_f32(t):
    g = (t["partial"].sum(1) * torch.tensor(R.HEAD_INV_HW, dtype=torch.float32)).requires_grad_()
    P = {k: t[k].clone().requires_grad_() for k in ("wo", "bo", "w1", "b1", "w2", "b2", "w3", "b3")}
    h1 = F.relu(F.linear(F.linear(g, P["wo"], P["bo"]), P["w1"], P["b1"]))
    h1 = h1 if t["mask1"] is None else h1 * t["mask1"]
    h2 = F.relu(F.linear(h1, P["w2"], P["b2"]))
    h2 = h2 if t["mask2"] is None else h2 * t["mask2"]
    score = torch.tanh(F.linear(h2, P["w3"].view(1, -1), P["b3"]).view(-1))
    score.backward(t["dscore"])
    out = {"score": score.detach(), "dgap": g.grad}
    out.update({"g" + k: v.grad for k, v in P.items()})
    return out


# ------------------------------------------------------------------ fragment-order conv weights
PACK_CASES = [(16, 16), (32, 16), (16, 48), (20, 8)]


@pytest.mark.parametrize("cout,cin", PACK_CASES)
def test_pack_conv_means_the_conv_and_its_input_gradient(cout, cin):
    B, Fr, H, W = 2, 3, 4, 5
    w = torch.rand(cout, cin, 27, dtype=D) * 2 - 1
    x = (torch.rand(B, cin, Fr, H, W, dtype=D) * 2 - 1).requires_grad_()
    y = F.conv3d(x, w.view(cout, cin, 3, 3, 3), padding=1)
    nout, nin, in_pad, ntiles, kgroups = R.pack_conv_geometry(cout, cin, 0)
    assert (nout, nin) == (cout, cin) and in_pad % 16 == 0 and in_pad - 16 < nin <= in_pad
    Wm = R.pack_conv(w, 0)
    assert Wm.shape == (16 * ntiles, 16 * kgroups)
    _same(R.conv3d_by_matrix(x.detach(), Wm, in_pad)[:, :cout], y.detach())
    dz = torch.rand_like(y) * 2 - 1
    y.backward(dz)
    nout, nin, in_pad, ntiles, kgroups = R.pack_conv_geometry(cout, cin, 1)
    assert (nout, nin) == (cin, cout)
    Wt = R.pack_conv(w, 1)
    assert Wt.shape == (16 * ntiles, 16 * kgroups)
    _same(R.conv3d_by_matrix(dz, Wt, in_pad)[:, :cin], x.grad)
    for Wx, no, ni, ip in ((Wm, cout, cin, (cin + 15) // 16 * 16), (Wt, cin, cout, (cout + 15) // 16 * 16)):
        v = Wx.view(-1, 27, ip)
        assert v[no:].abs().max().item() == 0 if v[no:].numel() else True
        assert v[:, :, ni:].abs().max().item() == 0 if v[:, :, ni:].numel() else True


def test_unpack_fragments_is_the_documented_rule():
    import infer_kernel_refs as IR

    ntiles, kgroups = 3, 5
    Wm = torch.arange(16 * ntiles * 16 * kgroups, dtype=D).view(16 * ntiles, 16 * kgroups)
    flat = IR.pack_fragments(Wm, ntiles, kgroups)
    assert torch.equal(R.unpack_fragments(flat, ntiles, kgroups), Wm)
    # spelled out for a few elements
    f4 = flat.view(ntiles, kgroups, 64, 4)
    for t, g, lane, e in ((0, 0, 0, 0), (2, 4, 63, 3), (1, 3, 17, 2), (2, 0, 48, 1)):
        assert f4[t, g, lane, e] == Wm[16 * t + lane % 16, 16 * g + 4 * (lane // 16) + e]


# ------------------------------------------------------------------ one-liners
def test_helpers():
    lq, gt = torch.rand(2, 3, 5, 7), torch.rand(2, 3, 5, 7)
    x = R.asdqe_pack_inputs(lq, gt, 8, 8)
    assert x.shape == (2, 8, 8, 12)
    assert torch.equal(x[:, :5, :7, 0:3], lq.permute(0, 2, 3, 1)) and torch.equal(x[:, :5, :7, 4:7], gt.permute(0, 2, 3, 1))
    assert torch.equal(x[:, :5, :7, 8:11], (lq - gt).permute(0, 2, 3, 1))
    assert x[..., 3::4].abs().max() == 0 and x[:, 5:].abs().max() == 0 and x[:, :, 7:].abs().max() == 0
    src = torch.rand(16, 4, 9)
    assert torch.equal(R.narrow_w_copy(src, 2), src[:, :2]) and R.narrow_w_copy(src, 2).is_contiguous()
    v = torch.rand(2, 8)
    b = R.bcast_rows(v, 35, 1 / 35)
    assert b.shape == (2, 35, 8) and torch.equal(b[1, 34], v[1] * torch.tensor(1 / 35, dtype=torch.float32))
    g, grad = torch.rand(8), torch.rand(8)
    assert torch.equal(R.grad_commit(g, grad, 1), grad + g) and torch.equal(R.grad_commit(g, grad * float("nan"), 0), g)
    y = torch.tensor([-1.0, -0.0, 0.0, 2.0])
    assert torch.equal(R.relu(y), F.relu(y))

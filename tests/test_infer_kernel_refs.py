"""The references of tests/infer_kernel_refs.py against the oracles (float64, 1e-12), and the layout
helpers against their inverses and against an element-by-element restatement of the kernels' index
formulas.  No GPU."""
import torch
import torch.nn.functional as F

import infer_kernel_refs as R
from oracle import kdlae_oracle as KO

torch.manual_seed(0)
D = torch.float64


def _rnd(*s):
    return torch.rand(*s, dtype=D) * 2 - 1


def _close(a, b, tol=1e-12):
    err = (a - b).abs().max().item()
    assert err <= tol * (1 + b.abs().max().item()), err


def _nchw(x):
    return x.permute(0, 3, 1, 2).contiguous()


def test_ffn_half_matches_oracle():
    B, H, W, C, hid = 2, 5, 7, 48, 32
    for ln, name in ((1, "BiasFree"), (2, "WithBias")):
        sd = {"n.body.weight": _rnd(C) + 2, "n.body.bias": _rnd(C),
              "f.project_in.weight": _rnd(2 * hid, C, 1, 1), "f.project_in.bias": _rnd(2 * hid),
              "f.dwconv.weight": _rnd(2 * hid, 1, 3, 3), "f.dwconv.bias": _rnd(2 * hid),
              "f.project_out.weight": _rnd(C, hid, 1, 1), "f.project_out.bias": _rnd(C)}
        x = _rnd(B, H, W, C)
        xn = _nchw(x)
        ref = xn + KO.gdfn(KO.layer_norm(xn, sd, "n", name), sd, "f")
        # the kernels take a unit LayerNorm: its weight / bias fold into project_in
        Win = sd["f.project_in.weight"].view(2 * hid, C)
        bin_ = sd["f.project_in.bias"] + (Win @ sd["n.body.bias"] if ln == 2 else 0)
        got = R.ffn_half(x, ln, Win * sd["n.body.weight"], bin_, sd["f.dwconv.weight"].view(-1, 9),
                         sd["f.dwconv.bias"], sd["f.project_out.weight"].view(C, hid), sd["f.project_out.bias"])
        _close(_nchw(got), ref)
        # the tail alone, through the interleaved layout and the dw blocks and back
        y = R.layer_norm(x, ln) @ (Win * sd["n.body.weight"]).t() + bin_
        wdw, bdw = R.dw_blocks_decode(R.dw_blocks(sd["f.dwconv.weight"].view(-1, 9), sd["f.dwconv.bias"]))
        tail = R.gdfn_tail(R.chunk_deinterleave(R.chunk_interleave(y)), wdw, bdw,
                           sd["f.project_out.weight"].view(C, hid), sd["f.project_out.bias"], x)
        _close(_nchw(tail), ref)
        # the unfused gate kernel's tap-major weights
        g = R.dwconv_gate(y, sd["f.dwconv.weight"].view(-1, 9).t().contiguous(), sd["f.dwconv.bias"])
        _close(g @ sd["f.project_out.weight"].view(C, hid).t() + sd["f.project_out.bias"] + x, got)


def test_mdta_pass1_and_fold_match_oracle():
    B, H, W = 2, 6, 5
    for C, heads in ((32, 2), (48, 1)):
        Ch = C // heads
        sd = {"n.body.weight": _rnd(C) + 2, "n.body.bias": _rnd(C),
              "a.qkv.weight": _rnd(3 * C, C, 1, 1), "a.qkv.bias": _rnd(3 * C),
              "a.qkv_dwconv.weight": _rnd(3 * C, 1, 3, 3), "a.qkv_dwconv.bias": _rnd(3 * C),
              "a.temperature": _rnd(heads, 1, 1) + 2,
              "a.project_out.weight": _rnd(C, C, 1, 1), "a.project_out.bias": _rnd(C)}
        x = _rnd(B, H, W, C)
        xn = _nchw(x)
        ref = KO.mdta(KO.layer_norm(xn, sd, "n", "WithBias"), sd, "a", heads)
        Wq = sd["a.qkv.weight"].view(3 * C, C)
        v, G, nq, nk = R.mdta_pass1(x, 2, Wq * sd["n.body.weight"], sd["a.qkv.bias"] + Wq @ sd["n.body.bias"],
                                    sd["a.qkv_dwconv.weight"].view(-1, 9), sd["a.qkv_dwconv.bias"])
        # per-head diagonal blocks of the full Gram, through the accumulator layout and back
        Gh = torch.stack([G[:, h * Ch:(h + 1) * Ch, h * Ch:(h + 1) * Ch] for h in range(heads)], 1)
        red = R.pack_reduced(Gh, nq.view(B, heads, Ch), nk.view(B, heads, Ch))
        Gd, nqd, nkd = R.unpack_reduced(red, Ch)
        M = R.attn_fold(Gd, nqd, nkd, sd["a.project_out.weight"].view(C, C), sd["a.temperature"].view(heads))
        got = v.reshape(B, H * W, C) @ M.transpose(1, 2) + sd["a.project_out.bias"]
        _close(_nchw(got.view(B, H, W, C)), ref)


def test_gap_head_matches_asdqe_oracle_statements():
    B, H, W, C, M = 3, 5, 4, 64, 96
    y = _rnd(B, H, W, C)
    sd = {"unet.outc.conv.weight": _rnd(M, C, 1, 1), "unet.outc.conv.bias": _rnd(M),
          "regressor.2.weight": _rnd(256, M), "regressor.2.bias": _rnd(256),
          "regressor.5.weight": _rnd(64, 256) / 16, "regressor.5.bias": _rnd(64),
          "regressor.8.weight": _rnd(1, 64) / 8, "regressor.8.bias": _rnd(1)}
    # oracle/asdqe_oracle.py: unet()'s last line, then asdqe_features' regressor
    feat = F.conv2d(_nchw(y), sd["unet.outc.conv.weight"], sd["unet.outc.conv.bias"])
    g = feat.mean(dim=(2, 3))
    h = torch.relu(F.linear(g, sd["regressor.2.weight"], sd["regressor.2.bias"]))
    h = torch.relu(F.linear(h, sd["regressor.5.weight"], sd["regressor.5.bias"]))
    ref = torch.tanh(F.linear(h, sd["regressor.8.weight"], sd["regressor.8.bias"])).view(-1)
    got = R.gap_head(y.view(B, H * W, C), sd["unet.outc.conv.weight"].view(M, C), sd["unet.outc.conv.bias"],
                     sd["regressor.2.weight"], sd["regressor.2.bias"], sd["regressor.5.weight"],
                     sd["regressor.5.bias"], sd["regressor.8.weight"].view(-1), sd["regressor.8.bias"])
    _close(got, ref)


def test_conv_helpers():
    x = _rnd(2, 4, 6, 8)
    w = _rnd(8, 3, 3, 3)          # [Cin][Cout][3][3]: the conv whose transpose is computed
    ref = F.conv_transpose2d(_nchw(x), w, padding=1).permute(0, 2, 3, 1)
    _close(R.conv_nhwc(x, R.conv_transposed_weight(w)), ref)
    y = _rnd(2, 4, 6, 8)
    u = R.pixel_unshuffle(y)
    for n, yy, xx in ((0, 1, 0), (1, 2, 5), (1, 3, 3)):
        assert u[0, yy >> 1, xx >> 1, 4 * n + 2 * (yy & 1) + (xx & 1)] == y[0, yy, xx, n]
    s = R.pixel_shuffle(y)
    for n, yy, xx in ((0, 1, 0), (5, 2, 5), (7, 3, 3), (2, 0, 1)):
        assert s[1, 2 * yy + (n >> 1 & 1), 2 * xx + (n & 1), n >> 2] == y[1, yy, xx, n]
    assert R.maxpool2(_rnd(2, 5, 7, 4)).shape == (2, 2, 3, 4)


def test_layout_round_trips():
    # chunk interleave: natural h hid + 16 g + c <-> 32 g + 16 h + c
    hid = 48
    nat = torch.arange(2 * hid, dtype=D)
    il = R.chunk_interleave(nat)
    for h in range(2):
        for g in range(hid // 16):
            for c in (0, 7, 15):
                assert il[32 * g + 16 * h + c] == h * hid + 16 * g + c
    assert torch.equal(R.chunk_deinterleave(il), nat)
    t = _rnd(3, 2 * hid, 5)
    assert torch.equal(R.chunk_deinterleave(R.chunk_interleave(t, 1), 1), t)
    # dw blocks
    wdw, bdw = _rnd(2 * hid, 9), _rnd(2 * hid)
    blk = R.dw_blocks(wdw, bdw)
    assert blk.shape == (hid // 16, 512)
    for h, g, c, tp in ((0, 0, 0, 0), (1, 2, 5, 8), (0, 1, 15, 4)):
        assert blk[g, 32 * tp + 16 * h + c] == wdw[h * hid + 16 * g + c, tp]
        assert blk[g, 288 + 16 * h + c] == bdw[h * hid + 16 * g + c]
    assert torch.all(blk[:, 320:] == 0) and torch.all(R.dw_blocks(wdw)[:, 288:] == 0)
    w2, b2 = R.dw_blocks_decode(blk)
    assert torch.equal(w2, wdw) and torch.equal(b2, bdw)
    # fragment order
    Wm = _rnd(40, 44)
    fr = R.pack_fragments(Wm, 3, 3)
    for tt, g, l, e in ((0, 0, 0, 0), (2, 2, 63, 3), (1, 2, 37, 2)):
        n, k = 16 * tt + l % 16, 16 * g + 4 * (l // 16) + e
        assert fr[((tt * 3 + g) * 64 + l) * 4 + e] == (Wm[n, k] if n < 40 and k < 44 else 0)
    assert torch.equal(R.unpack_fragments(fr, 3, 3)[:40, :44], Wm)
    # accumulator order of `reduced`
    Ch = 48
    G = _rnd(2, 3, Ch, Ch)
    acc = R.gram_to_acc(G)
    CT = Ch // 16
    for i, j, l, e in ((0, 0, 0, 0), (2, 1, 63, 3), (1, 2, 21, 2)):
        assert acc[1, 2, (i * CT + j) * 256 + 4 * l + e] == G[1, 2, 16 * i + 4 * (l // 16) + e, 16 * j + l % 16]
    assert torch.equal(R.acc_to_gram(acc, Ch), G)
    nq, nk = _rnd(2, 3, Ch), _rnd(2, 3, Ch)
    Gd, a, b = R.unpack_reduced(R.pack_reduced(G, nq, nk), Ch)
    assert torch.equal(Gd, G) and torch.equal(a, nq) and torch.equal(b, nk)


def test_split_records_round_trip():
    for ntiles, kgroups in ((3, 3), (2, 4), (1, 1)):
        M = (_rnd(16 * ntiles, 16 * kgroups) * torch.tensor(10.0, dtype=D) ** torch.randint(-6, 3, (16 * ntiles, 1))).float()
        rec = R.split_records_encode(M, ntiles, kgroups)
        kpt = (kgroups + 1) // 2
        assert rec.numel() == ntiles * kpt * 768
        dec = R.split_records_decode(rec, ntiles, kgroups)
        # 8 + 8 + 8 significand bits: the three planes sum to the float32 value itself
        assert torch.equal(dec[:, :16 * kgroups], M.double())
        assert torch.all(dec[:, 16 * kgroups:] == 0)
        # the kernel's own index formula (mdta.hip attn_fold_kernel `put`), element by element
        bf = rec.view(torch.bfloat16)
        for n, k in ((0, 0), (16 * ntiles - 1, 16 * kgroups - 1), (5, 9), (17 % (16 * ntiles), 7)):
            kk = k & 31
            lane, j = (n & 15) + 16 * ((kk & 15) >> 2), 4 * (kk >> 4) + (kk & 3)
            slot = ((n >> 4) * kpt + (k >> 5)) * 3 * 64 + lane
            v = sum(bf[(slot + 64 * pl) * 8 + j].double() for pl in range(3))
            assert v == M[n, k].double()

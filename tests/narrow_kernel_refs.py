"""Float64 references of the kernels that tests/test_narrow_kernels_gpu.py launches alone, in the
operations' own terms (torch's convolutions, autograd, array slicing), and the seeded inputs of those
tests.  The inputs are built on the CPU, so tests/test_narrow_kernel_refs.py can show without a GPU that
the mistakes these kernels could make move the results by more than the GPU tests allow.

  small_in_2d      the 2-D narrow-input 3x3 conv (conv_small.hip conv_small_in_kernel<1, NTO>), forward and
                   transposed (wt)
  head_train       the ASDQE train-mode regressor head (bn_train.hip), gradients by autograd
  pack_conv        KDLAE-S fragment-order Conv3d weights (train_s.hip pack_conv_kernel), dx 0 and 1
  asdqe_pack_inputs, narrow_w_copy, bcast_rows, grad_commit, relu
"""
import torch
import torch.nn.functional as F

D = torch.float64


def rand(*shape, seed=0, scale=1.0):
    """Seeded uniform [-scale, scale] float32 on the CPU (drawn in float64, as the other kernel tests do)."""
    g = torch.Generator(device="cpu").manual_seed(seed)
    return ((torch.rand(*shape, generator=g, dtype=D) * 2 - 1) * scale).float()


def tol(ref, K):
    """The kernel tests' rule: 1e-5 (max|ref| + 1) sqrt(K) / 4."""
    return 1e-5 * (float(ref.abs().max()) + 1) * max(1.0, K ** 0.5) / 4


# ------------------------------------------------------------------ narrow-input 3x3 conv
def small_in_2d(x, sub, w, bias, dil, vh, vw, relu, wt):
    """x, sub [Bn][Cin][H][W]; out [Bn][Cout][H][W] in float64.  The conv input is (x - sub), zero outside
    the top-left vh x vw (0: all of it); padding = dilation.  wt 0: w [Cout][Cin][3][3], a Conv2d.
    wt > 0: w [Cin][wt][3][3] is the weight of the wt -> Cin conv this one transposes (its input
    gradient): a ConvTranspose2d."""
    x = x.to(D)
    if sub is not None:
        x = x - sub.to(D)
    if vh or vw:
        keep = torch.zeros_like(x)
        keep[..., :vh or x.shape[-2], :vw or x.shape[-1]] = 1
        x = x * keep
    b = None if bias is None else bias.to(D)
    if wt:
        y = F.conv_transpose2d(x, w.to(D), b, padding=dil, dilation=dil)
    else:
        y = F.conv2d(x, w.to(D), b, padding=dil, dilation=dil)
    return y.clamp_min(0) if relu else y


def nhwc_rows(y):
    """[Bn][C][H][W] -> the kernels' output rows [Bn H W][C]."""
    return y.permute(0, 2, 3, 1).reshape(-1, y.shape[1])


# general cases: one table for every Cin, so each value of Cout, dil, layout, bias and relu meets each Cin
_SMALL_IN_TABLE = [  # Cout, dil, layout, bias, relu
    (16, 1, "nchw", 1, 0), (48, 2, "nhwc", 1, 1), (96, 1, "nhwc", 0, 1), (144, 2, "nchw", 1, 0),
    (16, 2, "nhwc", 0, 1), (48, 1, "nchw", 0, 0), (96, 2, "nchw", 1, 0), (144, 1, "nhwc", 0, 1),
]


def small_in_cases():
    """The GPU test's cases as dicts: Cin, Cout, dil, layout, bias, relu, Bn, H, W, sub (in_sub given),
    vh, vw (0 = whole), wt (transposed)."""
    base = dict(Bn=2, H=7, W=9, sub=0, vh=0, vw=0, wt=0)
    cases = []
    for Cin in (1, 2, 3, 4):
        for Cout, dil, layout, bias, relu in _SMALL_IN_TABLE:
            cases.append(dict(base, Cin=Cin, Cout=Cout, dil=dil, layout=layout, bias=bias, relu=relu))
    # most taps outside the image
    cases.append(dict(base, Cin=3, Cout=48, dil=2, layout="nchw", bias=1, relu=0, H=2, W=3))
    # ASDQE's extractors: lq - gt, a 5 x 7 image on the padded 8 x 8 grid
    for Cin in (1, 2, 3, 4):
        cases.append(dict(base, Cin=Cin, Cout=(16, 48)[Cin % 2], dil=1, layout="nchw", bias=1, relu=Cin // 2 % 2,
                          H=8, W=8, sub=1, vh=5, vw=7))
    # the training dX of the image heads
    for Cin in (3, 4):
        for Cout in (48, 96, 144):
            for dil in (1, 2):
                cases.append(dict(base, Cin=Cin, Cout=Cout, dil=dil, layout="nhwc", bias=dil - 1, relu=0, wt=1))
    return cases


def small_in_id(c):
    return (f"ci{c['Cin']}-co{c['Cout']}-d{c['dil']}-{c['layout']}-b{c['bias']}-r{c['relu']}-{c['H']}x{c['W']}"
            + ("-sub" if c["sub"] else "") + ("-wt" if c["wt"] else ""))


def small_in_inputs(c):
    """(x, sub, w, bias) of a case, float32 on the CPU; x and sub cover the whole H x W grid (what lies
    outside vh x vw is other data that the conv must not see)."""
    Cin, Cout = c["Cin"], c["Cout"]
    seed = 1000 * Cin + Cout + 7 * c["dil"] + 13 * c["H"] + (1 if c["layout"] == "nhwc" else 0)
    x = rand(c["Bn"], Cin, c["H"], c["W"], seed=seed)
    sub = rand(c["Bn"], Cin, c["H"], c["W"], seed=seed + 1) if c["sub"] else None
    wshape = (Cin, Cout, 3, 3) if c["wt"] else (Cout, Cin, 3, 3)
    w = rand(*wshape, seed=seed + 2, scale=(9 * Cin) ** -0.5)
    bias = rand(Cout, seed=seed + 3) if c["bias"] else None
    return x, sub, w, bias


# ------------------------------------------------------------------ ASDQE train-mode regressor head
HEAD_GRADS = ("gwo", "gbo", "gw1", "gb1", "gw2", "gb2", "gw3", "gb3")


def head_train(partial, inv_hw, wo, bo, w1, b1, w2, b2, w3, b3, mask1, mask2, dscore):
    """partial [B][slots][C] -> dict of float64 tensors: score [B], dgap [B][C] (the gradient of the pooled
    features g = inv_hw sum_slots partial) and the eight parameter gradients, all by autograd of
    sum_b dscore[b] score[b].  masks [B][N1] / [B][N2] or None."""
    d = lambda t: None if t is None else t.detach().to(D)
    g = (d(partial).sum(1) * inv_hw).requires_grad_()
    P = {k: d(v).requires_grad_() for k, v in dict(wo=wo, bo=bo, w1=w1, b1=b1, w2=w2, b2=b2, w3=w3, b3=b3).items()}
    f = F.linear(g, P["wo"], P["bo"])
    h1 = F.relu(F.linear(f, P["w1"], P["b1"]))
    if mask1 is not None:
        h1 = h1 * d(mask1)
    h2 = F.relu(F.linear(h1, P["w2"], P["b2"]))
    if mask2 is not None:
        h2 = h2 * d(mask2)
    score = torch.tanh(F.linear(h2, P["w3"].view(1, -1), P["b3"]).view(-1))
    score.backward(d(dscore))
    out = {"score": score.detach(), "dgap": g.grad}
    out.update({"g" + k: v.grad for k, v in P.items()})
    return out


def head_cases():
    """(C, M, N1, N2, slots, masks): ASDQE's own head (M = 3 dim = 48) and one whose dimensions cross the
    256-thread stride and are no multiples of 4."""
    return [(C, M, N1, N2, slots, masks) for C, M, N1, N2 in ((64, 48, 256, 64), (20, 300, 513, 7))
            for slots in (1, 5) for masks in (0, 1)]


HEAD_B = 3


HEAD_HW = 35
HEAD_INV_HW = 1.0 / HEAD_HW


def head_inputs(C, M, N1, N2, slots, masks):
    """Seeded inputs of a head case (float32, CPU).  Hidden unit 3 of layer 1 and the last unit of layer 2
    have zero weights and bias, so their pre-activation is exactly 0; dscore[1] = 0; masks hold 0 or 2.
    Sized so that the checks bite under the tolerance rule's absolute term: the slot partials are sums
    over HW / slots pixels (the pooled g is O(1) and differs between the images), b3 = +-0.6 puts tanh on
    its curved part, and dscore is 16 x uniform so that the smallest gradient (gwo) is many tolerances large."""
    B, seed = HEAD_B, C + M + N1 + N2 + 17 * slots + masks
    t = dict(partial=rand(B, slots, C, seed=seed, scale=HEAD_HW / slots),
             wo=rand(M, C, seed=seed + 1, scale=C ** -0.5), bo=rand(M, seed=seed + 2),
             w1=rand(N1, M, seed=seed + 3, scale=M ** -0.5), b1=rand(N1, seed=seed + 4),
             w2=rand(N2, N1, seed=seed + 5, scale=N1 ** -0.5), b2=rand(N2, seed=seed + 6),
             w3=rand(N2, seed=seed + 7, scale=N2 ** -0.5), b3=torch.tensor([0.6 if seed % 2 else -0.6]),
             dscore=rand(B, seed=seed + 9, scale=16.0), mask1=None, mask2=None)
    t["w1"][3] = 0
    t["b1"][3] = 0
    t["w2"][N2 - 1] = 0
    t["b2"][N2 - 1] = 0
    t["dscore"][1] = 0
    if masks:
        t["mask1"] = (rand(B, N1, seed=seed + 10) > 0).float() * 2
        t["mask2"] = (rand(B, N2, seed=seed + 11) > 0).float() * 2
    return t


def head_K(name, C, M, N1, N2, B=HEAD_B):
    """The longest dot product feeding a compared quantity: the widest layer, times B for the sums over images."""
    K = max(C, M, N1, N2)
    return K if name in ("score", "dgap") else K * B


# ------------------------------------------------------------------ KDLAE-S fragment-order conv weights
def pack_conv_geometry(cout, cin, dx):
    """(nout, nin, in_pad, ntiles, kgroups) of launch_pack_conv: the packed conv has nout outputs and nin
    inputs (swapped for the input-gradient conv), inputs padded to 16 per tap, outputs to whole 16-row tiles."""
    nout, nin = (cin, cout) if dx else (cout, cin)
    in_pad = (nin + 15) // 16 * 16
    return nout, nin, in_pad, (nout + 15) // 16, 27 * in_pad // 16


def pack_conv(w, dx):
    """w [cout][cin][27] -> the matrix Wm [16 ntiles][27 in_pad] with out[p][n] = sum_k Xcol[p][k] Wm[n][k],
    Xcol[p][tap in_pad + c] = x[p + off(tap)][c]: dx 0 the Conv3d itself, dx 1 its input gradient as a conv
    of dZ (taps reversed, channel roles swapped).  Zero in the padding."""
    cout, cin = w.shape[:2]
    nout, nin, in_pad, ntiles, _ = pack_conv_geometry(cout, cin, dx)
    m = w.flip(-1).permute(1, 2, 0) if dx else w.permute(0, 2, 1)  # [nout][27][nin]
    Wm = w.new_zeros(16 * ntiles, 27, in_pad)
    Wm[:nout, :, :nin] = m
    return Wm.reshape(16 * ntiles, 27 * in_pad)


def unpack_fragments(flat, ntiles, kgroups):
    """The documented fragment rule, element by element: (t, g, lane, e) -> W(16 t + lane % 16,
    16 g + 4 (lane / 16) + e)."""
    t, g, lane, e = torch.meshgrid(torch.arange(ntiles), torch.arange(kgroups), torch.arange(64), torch.arange(4),
                                   indexing="ij")
    W = flat.new_zeros(16 * ntiles, 16 * kgroups)
    W[16 * t + lane % 16, 16 * g + 4 * (lane // 16) + e] = flat.view(ntiles, kgroups, 64, 4)
    return W


def conv3d_by_matrix(x, Wm, in_pad):
    """x [B][C][F][H][W] -> [B][rows of Wm][F][H][W]: the 3x3x3 conv (padding 1) as Xcol . Wm^T with
    k = tap in_pad + c, tap = (dt, dy, dx) row-major."""
    B, C, Fr, H, W = x.shape
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    col = x.new_zeros(B, 27, in_pad, Fr, H, W)
    for tap in range(27):
        dt, dy, dxx = tap // 9, tap // 3 % 3, tap % 3
        col[:, tap, :C] = xp[:, :, dt:dt + Fr, dy:dy + H, dxx:dxx + W]
    return torch.einsum("bkfhw,nk->bnfhw", col.reshape(B, 27 * in_pad, Fr, H, W), Wm)


# ------------------------------------------------------------------ one-liners
def asdqe_pack_inputs(lq, gt, Hp, Wp):
    """lq, gt [B][ci][H][W] -> [B][Hp][Wp][12] float32: lq, gt and the fp32 difference at 4 channels each,
    zero past ci and past H x W."""
    pad = lambda t: F.pad(t, (0, Wp - t.shape[3], 0, Hp - t.shape[2], 0, 4 - t.shape[1])).permute(0, 2, 3, 1)
    return torch.cat([pad(lq), pad(gt), pad(lq - gt)], -1)


def narrow_w_copy(src, ci):
    """src [Cout][4][9] -> [Cout][ci][9]"""
    return src[:, :ci].contiguous()


def bcast_rows(v, HW, scale):
    """v [B][C] -> [B][HW][C] = v[b] * scale in fp32"""
    return (v * torch.tensor(scale, dtype=v.dtype)).unsqueeze(1).expand(-1, HW, -1).contiguous()


def grad_commit(g, grad, accumulate):
    return grad + g if accumulate else g.clone()


def relu(y):
    return y.clamp_min(0)

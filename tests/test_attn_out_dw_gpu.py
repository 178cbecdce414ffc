"""attn_out_dw_kernel (csrc/attn_out_dw.hip: out = R + bias + M_img . dw3x3(v), v read from the qkv
buffer) and the Gram ring without v (kdlae_debug_gram route 3), which together replace the v-writing
ring + the per-image-weight attention-output GEMM on the C = 48 / 96 blocks.

Shapes: Bn = 2 (the per-image M differs; a halo must not read the neighbouring image), 40 x 32 pixels
(two 16-column strips, row segments of 32 + 8 rows, all four borders).  Inputs are hash-uniform in
[-1, 1] with non-zero biases.
"""
import pytest
import torch
import torch.nn.functional as F

import gemm_precision_inputs as G
import infer_kernel_refs as R
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, load_hash_weights
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_teacher
from test_infer_kernels_gpu import _run as _infer_rc
from test_kernel_variants_infer_gpu import GemmDesc, GramDesc, _call, pack_fragments

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
BN, H, W = 2, 40, 32
CASES = [(48, 1), (96, 1), (96, 2)]
IDS = [f"C{c}_h{h}" for c, h in CASES]
EINVAL_SHAPE = 1


def _ptr(t):
    return None if t is None else t.data_ptr()


def _hash(name, *shape, scale=1.0):
    return ((torch.from_numpy(hash_images(name, shape)).double() * 2 - 1) * scale).float().to(DEV)


_cache = {}


def _case(C, heads):
    """Inputs of one configuration, the v-writing ring's outputs and the fold's M records; computed once."""
    key = (C, heads)
    if key in _cache:
        return _cache[key]
    t = f"aod{C}_{heads}"
    Ch = C // heads
    CT = Ch // 16
    kg = C // 16
    d = dict(C=C, heads=heads, Ch=Ch, kg=kg)
    d["qkv"] = _hash(t + "qkv", BN, H, W, 3 * C)
    d["wdw"] = _hash(t + "wdw", 9, 3 * C, scale=1 / 3)
    d["bdw"] = _hash(t + "bdw", 3 * C, scale=0.5)
    d["proj"] = _hash(t + "proj", C, C, scale=C ** -0.5)
    d["temp"] = _hash(t + "temp", heads) + 2
    d["pbias"] = _hash(t + "pb", C, scale=0.5)
    d["x"] = _hash(t + "x", BN * H * W, C)
    d["zeros"] = torch.zeros(64, device=DEV)
    sf = CT * CT * 256 + 2 * Ch
    d["sf"] = sf
    partial = torch.empty(BN * heads * 64 * 8 * sf, device=DEV)

    def gram(route, v_out):
        red = torch.empty(BN * heads, sf, device=DEV)
        _call("kdlae_debug_gram", GramDesc, qkv=_ptr(d["qkv"]), ld=3 * C, wdw=_ptr(d["wdw"]), bdw=_ptr(d["bdw"]),
              v_out=_ptr(v_out), ldv=C, partial=_ptr(partial), partial_floats=partial.numel(), reduced=_ptr(red),
              zeros=_ptr(d["zeros"]), C=C, heads=heads, Bn=BN, H=H, W=W, route=route)
        return red

    d["gram"] = gram
    d["vbuf"] = torch.full((BN * H * W, C), 7.0, device=DEV)
    d["red"] = gram(0, d["vbuf"])
    kpt = (kg + 1) // 2
    d["Mp"] = torch.zeros(BN, kg * kpt * 768, device=DEV)
    assert _infer_rc(op=3, inp=[(d["red"], 0)], out=[(d["Mp"], 0)], w=[d["proj"], d["temp"]], C=C, heads=heads,
                     Bn=BN) == 0
    _cache[key] = d
    return d


def _new(d, out, R_, ldv=None, v=None, ldo=None, **kw):
    """One launch of the new kernel on v = the qkv buffer's third part; returns the error code."""
    C = d["C"]
    args = dict(op=10, inp=[(d["qkv"].view(-1)[2 * C:] if v is None else v, 3 * C if ldv is None else ldv)],
                out=[(out, out.shape[-1] if ldo is None else ldo)], w=[d["wdw"], d["Mp"]], bias=[d["bdw"], d["pbias"]], R=R_,
                ldr=R_.shape[-1], zeros=d["zeros"], C=C, Bn=BN, H=H, W=W)
    args.update(kw)
    return _infer_rc(**args)


def _old_pair(d):
    """Today's pair: the v-writing ring's v' through the per-image-weight gemm_res path (kdlae_debug_gemm,
    production dispatch, resident, NT = KG = C / 16).  M goes in as f32 fragments: the records' three
    planes sum to the f32 value exactly, and the entry splits it again into the same records."""
    C, kg = d["C"], d["kg"]
    Mf = torch.cat([pack_fragments(R.split_records_decode(d["Mp"][b], kg, kg)[:, :C].float().to(DEV), kg, kg)
                    for b in range(BN)])
    out = torch.empty(BN * H * W, C, device=DEV)
    _call("kdlae_debug_gemm", GemmDesc, A=_ptr(d["vbuf"]), lda=C, Bn=BN, F=1, H=H, W=W, ksize=1, kt=1, dil=1,
          cg_per_tap=0, kgroups=kg, Wp=_ptr(Mf), w_img_stride=Mf.numel() // BN, ntiles=kg, N=C, bias=_ptr(d["pbias"]),
          out=_ptr(out), ldo=C, R=_ptr(d["x"]), ldr=C, ln=0, ln_C=C, relu=0, out_mode=0, NT=kg, KG=kg, wpe=2,
          group_tiles=kg, route=0)
    return out


@pytest.mark.parametrize("C,heads", CASES, ids=IDS)
def test_equals_ring_plus_gemm_bit_for_bit(C, heads):
    d = _case(C, heads)
    ref = _old_pair(d)
    out = torch.full((BN * H * W, C + 4), 7.0, device=DEV)
    assert _new(d, out, d["x"]) == 0
    assert torch.equal(out[:, :C], ref)
    assert bool((out[:, C:] == 7.0).all()), "wrote past its C columns"
    inplace = d["x"].clone()
    assert _new(d, inplace, inplace) == 0     # R aliasing out
    assert torch.equal(inplace, ref)


@pytest.mark.parametrize("C,heads", CASES, ids=IDS)
def test_against_float64(C, heads):
    """ref = R + bias + M . conv2d(v) in float64 on the CPU, M decoded from the attn_fold records.
    Tolerance per output n: the product part is mfma3.h's claim as tests/test_gemm_precision_gpu.py applies
    it, coherent_bound(C) x den with den the same expression over absolute values; the stencil part is the
    depthwise rule of tests/test_infer_kernels_gpu.py, ts = 1e-5 (max|v'| + 1) sqrt(9) / 4 per element of v',
    which reaches the output through M as ts x sum_k |M[n][k]|."""
    d = _case(C, heads)
    kg = d["kg"]
    out = torch.empty(BN * H * W, C, device=DEV)
    assert _new(d, out, d["x"]) == 0
    v = d["qkv"][..., 2 * C:].double().cpu().permute(0, 3, 1, 2)
    w = d["wdw"][:, 2 * C:].double().cpu().T.reshape(C, 1, 3, 3)
    vp = F.conv2d(v, w, d["bdw"][2 * C:].double().cpu(), padding=1, groups=C).flatten(2).permute(0, 2, 1)  # [Bn][HW][C]
    ts = 1e-5 * (vp.abs().max().item() + 1) * 3 / 4
    x = d["x"].double().cpu().view(BN, H * W, C)
    pb = d["pbias"].double().cpu()
    got = out.double().cpu().view(BN, H * W, C)
    for b in range(BN):
        M = R.split_records_decode(d["Mp"][b], kg, kg)[:, :C].cpu()
        ref = x[b] + pb + vp[b] @ M.T
        den = x[b].abs() + pb.abs() + vp[b].abs() @ M.abs().T
        tol = G.coherent_bound(C) * den + ts * M.abs().sum(1)
        ratio = ((got[b] - ref).abs() / tol).max().item()
        print(f"RATIO attn_out_dw C{C} heads{heads} b{b} {ratio:.4f}")
        assert torch.isfinite(got[b]).all() and ratio <= 1.0, ratio


@pytest.mark.parametrize("C,heads", CASES, ids=IDS)
def test_ring_without_v(C, heads):
    d = _case(C, heads)
    sentinel = torch.full((BN * H * W, C), -3.0, device=DEV)
    red = d["gram"](3, sentinel)
    assert torch.equal(red, d["red"])
    assert bool((sentinel == -3.0).all()), "the no-v ring wrote v_out"


KW = dict(inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4,
          heads=[1, 2, 4, 8], ffn_expansion_factor=2.66, bias=False, LayerNorm_type="BiasFree",
          dual_pixel_task=False, static="train", params="cat")   # bench.py's KW


@pytest.mark.parametrize("shape", [(1, 3, 48, 80), (2, 3, 64, 64)], ids=["1x48x80", "2x64x64"])
def test_whole_model_equals_old_path(shape, monkeypatch):
    """The default path against KDLAE_DEBUG=no_attn_out_dw (the v-writing ring + the M GEMM), bit for bit; a
    HIP-graph replay equals a launch-by-launch call."""
    img = torch.from_numpy(hash_images("aodm", shape)).to(DEV)
    rate = torch.from_numpy(hash_images("aodmr", (shape[0], 1) + shape[2:])).to(DEV)

    def model():
        m = KDLAE_teacher(**KW)
        load_hash_weights(m)
        return m.to(DEV).eval()

    def run(m):
        with torch.no_grad():
            o = m({"img": img, "denoise_rate": rate})
        torch.cuda.synchronize()
        return o["hq"].clone(), o["sr"].clone()

    m = model()
    m.hip_graphs = False
    new = run(m)
    m.hip_graphs = True
    for _ in range(3):       # the second call of a shape captures, the third replays
        rep = run(m)
    assert torch.equal(rep[0], new[0]) and torch.equal(rep[1], new[1])
    monkeypatch.setenv("KDLAE_DEBUG", "no_attn_out_dw")  # read when a new handle builds its blocks
    m_old = model()
    m_old.hip_graphs = False
    old = run(m_old)
    assert torch.equal(new[0], old[0]) and torch.equal(new[1], old[1])


def test_preconditions():
    """Each returns KDLAE_EINVAL_SHAPE before any launch: the output keeps its fill."""
    d = _case(48, 1)
    C = 48
    out = torch.full((BN * H * W, C), 7.0, device=DEV)
    assert _new(d, out, d["x"], ldv=3 * C + 2) == EINVAL_SHAPE          # misaligned ldv
    assert _new(d, out, d["x"], C=192) == EINVAL_SHAPE                   # C = 192
    assert _new(d, out, d["x"], W=24, H=40) == EINVAL_SHAPE              # W % 16 != 0
    q = d["qkv"].view(-1, 3 * C)
    before = q.clone()
    assert _new(d, q[:, C:], d["x"], ldo=3 * C) == EINVAL_SHAPE          # out overlaps v
    assert bool((out == 7.0).all()) and torch.equal(q, before)

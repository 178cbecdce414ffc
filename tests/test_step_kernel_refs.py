"""tests/step_kernel_refs.py on the CPU, two halves.

1. The float64 models say what the reference says: ``clip_adamw`` against
   ``torch.nn.utils.clip_grad_norm_`` + ``torch.optim.AdamW`` / ``Adam`` on float64 tensors, ``l1sr`` /
   ``l1frames`` against the oracle's losses under float64 autograd, ``mixup`` / ``ema`` / ``mse``
   against their one-line torch statements, all to 1e-12 relative.
2. The bounds tests/test_step_kernels_gpu.py applies can fail: on every input class the fp32
   emulation of the kernel's arithmetic meets them, and each mutant misses at least one.  Which class
   exposes which mutant is stated per test; a mutant that no class exposed would fail here.

The worst ratio of the emulation to each bound is printed when the module finishes (``-s``).
"""
import math

import numpy as np
import pytest
import torch

from oracle.train_oracle import l1_video_frames, l1sr_loss
from tests import step_kernel_refs as R

RTOL = 1e-12
U = R.U
MARGINS = {}


def _same(got, ref, what):
    got, ref = np.asarray(got, dtype=np.float64), np.asarray(ref, dtype=np.float64)
    err = float(np.abs(got - ref).max())
    assert err <= RTOL * max(float(np.abs(ref).max()), 1e-300), f"{what}: {err:.3e}"


def _note(name, ratio):
    MARGINS[name] = max(MARGINS.get(name, 0.0), float(ratio))
    return ratio


def teardown_module(module):
    for k in sorted(MARGINS):
        print(f"[emulation / bound] {k}: {MARGINS[k]:.3f}")


# ===================================================================== 1. models against torch
@pytest.mark.parametrize("opt_cls,wd", [("AdamW", 0.0), ("AdamW", 0.5e-4), ("Adam", 0.0)])
@pytest.mark.parametrize("betas", [(0.9, 0.999), (0.2, 0.999)])
@pytest.mark.parametrize("max_norm", [0.01, 0.0])
def test_clip_adamw_model_matches_torch(opt_cls, wd, betas, max_norm):
    """Four steps over three parameters in one flat buffer; the middle one has grad = None from the
    second step on (the optimizer skips it, `ranges` leaves it out), while clip_grad_norm_ ran over
    all three before the gradient was dropped: the norm covers all n.  Adam is AdamW without decay
    (its own weight_decay is L2, another operation, and is not run)."""
    sizes, n = (5, 7, 4), 16
    offs = np.cumsum((0,) + sizes)
    lr, eps, max_norm = R.f32(1e-3), R.f32(1e-8), R.f32(max_norm)
    b1, b2, wdf = R.f32(betas[0]), R.f32(betas[1]), R.f32(wd)
    theta = R.spread(n, 1e-4, 1.0, 3).astype(np.float64)
    params = [torch.tensor(theta[offs[i]:offs[i + 1]], requires_grad=True) for i in range(3)]
    opt = getattr(torch.optim, opt_cls)(params, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wdf)
    th, m, v = theta.copy(), np.zeros(n), np.zeros(n)
    for step in range(1, 5):
        g = R.spread(n, 1e-3, 1.0, 10 + step).astype(np.float64)
        for i, p in enumerate(params):
            p.grad = torch.tensor(g[offs[i]:offs[i + 1]])
        norm = float(torch.nn.utils.clip_grad_norm_(params, max_norm)) if max_norm > 0 else math.sqrt((g * g).sum())
        ranges = None
        if step >= 2:
            params[1].grad = None
            ranges = [(0, 5), (12, 16)]
        opt.step()
        r = R.clip_adamw(th, g, m, v, 1.0, max_norm, lr, b1, b2, eps, wdf, step, ranges)
        th, m, v = r["theta"], r["m"], r["v"]
        _same(r["norm"], norm, f"norm step {step}")
        _same(th, torch.cat([p.detach() for p in params]).numpy(), f"theta step {step}")
        want = torch.cat([p.detach() for p in params]).numpy()     # and element by element: theta spans 1e-4 .. 1
        assert np.all(np.abs(th - want) <= RTOL * np.abs(want)), f"theta step {step}, per element"
        for i in (0, 2):
            st = opt.state[params[i]]
            _same(m[offs[i]:offs[i + 1]], st["exp_avg"].numpy(), f"exp_avg[{i}] step {step}")
            _same(v[offs[i]:offs[i + 1]], st["exp_avg_sq"].numpy(), f"exp_avg_sq[{i}] step {step}")
    # the skipped parameter saw exactly one update
    assert int(opt.state[params[1]]["step"]) == 1


def test_clip_adamw_model_gscale_is_a_prescaled_gradient():
    x = R.adamw_inputs(257, "gscale")
    a = R.clip_adamw(x["theta"], x["grad"], x["m"], x["v"], 0.125, 0.01, step=3, **R.HYPER)
    b = R.clip_adamw(x["theta"], x["grad"].astype(np.float64) * 0.125, x["m"], x["v"], 1.0, 0.01, step=3, **R.HYPER)
    for k in ("norm", "theta", "m", "v"):
        _same(a[k], b[k], k)


@pytest.mark.parametrize("with_sr", [True, False])
def test_l1sr_model_matches_oracle(with_sr):
    p0, t0 = R.loss_generic((2, 3, 9, 13), 1)
    p1, t1 = R.loss_generic((2, 3, 18, 26), 5)
    pred = {"hq": torch.tensor(p0, dtype=torch.float64, requires_grad=True)}
    tgt = {"hq": torch.tensor(t0, dtype=torch.float64)}
    if with_sr:
        pred["sr"] = torch.tensor(p1, dtype=torch.float64, requires_grad=True)
        tgt["sr"] = torch.tensor(t1, dtype=torch.float64)
    ref = l1sr_loss(pred, tgt)
    ref.backward()
    loss, dhq, dsr = R.l1sr(p0, t0, p1 if with_sr else None, t1 if with_sr else None)
    _same(loss, float(ref.detach()), "loss")
    _same(dhq, pred["hq"].grad.numpy().ravel(), "dhq")
    assert (dhq == 0).sum() >= dhq.size // 7          # the ties
    if with_sr:
        _same(dsr, pred["sr"].grad.numpy().ravel(), "dsr")


@pytest.mark.parametrize("frames", [1, 2, 3, 4])
@pytest.mark.parametrize("red", ["mean", "sum"])
def test_l1frames_model_matches_oracle(frames, red):
    p, t = R.loss_generic((2, frames, 9 * 13), 20 + frames)
    binary = R.f32(0.3)
    pr = torch.tensor(p, dtype=torch.float64, requires_grad=True)
    ref = l1_video_frames(pr, torch.tensor(t, dtype=torch.float64), l1loss_weight=R.f32(0.7), reduction=red,
                          temporal_weight=R.f32(0.3), binary=binary)
    ref.backward()
    loss, g = R.l1frames(p, t, 0.7, 0.3, binary, int(red == "sum"))
    _same(loss, float(ref.detach()), "loss")
    _same(g, pr.grad.numpy(), "dpred")


def test_mixup_ema_mse_models_match_torch():
    x = torch.tensor(R.spread(4 * 5, 1e-3, 1.0, 1).reshape(4, 5), dtype=torch.float64)
    perm, lam = [2, 1, 3, 0], R.f32(0.3)
    _same(R.mixup(x.numpy(), perm, 0.3), (lam * x + (1 - lam) * x[perm]).numpy(), "mixup")
    e = torch.tensor(R.spread(20, 1e-3, 1.0, 2), dtype=torch.float64)
    d = R.f32(0.999)
    _same(R.ema(e.numpy(), x.numpy().ravel(), 0.999), (e * d + x.reshape(-1) * (1 - d)).numpy(), "ema")
    s = x.reshape(-1).clone().requires_grad_(True)
    sc = R.f32(1 / 32)
    loss = torch.nn.functional.mse_loss(s, e)
    (loss * sc).backward()
    ds, l0, l1 = R.mse(s.detach().numpy(), e.numpy(), 1 / 32)
    _same(ds, s.grad.numpy(), "dscore")
    _same(l0, float(loss.detach()), "mse")
    _same(l1, float((s.detach() - e).abs().mean()), "mae")


# ===================================================================== 2. emulation meets, mutants miss
L1_SIZES = R.SMALL_SIZES + (R.three_trip(R.T_L1),)     # 2 * 262144 + 257 = 524545


def _l1sr_grad_ok(got, p, t, w):
    c = np.float32(w / p.size)
    return np.array_equal(got, (np.sign(p.astype(np.float64) - t) * c).astype(np.float32).ravel())


def test_l1sr_gradient_class():
    """Gradient = sign c exactly, 0.0 on the tied block.  Exposes: sign0."""
    for n in L1_SIZES:
        p, t = R.loss_generic((n,), n)
        q, s = R.loss_generic((n + 3,), n + 7)
        _, dhq, dsr = R.emu_l1sr(p, t, q, s)
        assert _l1sr_grad_ok(dhq, p, t, 0.5) and _l1sr_grad_ok(dsr, q, s, 0.25), n
        _, mh, ms = R.emu_l1sr(p, t, q, s, mutant="sign0")
        assert not _l1sr_grad_ok(mh, p, t, 0.5), n


def _rel(got, ref):
    err = abs(float(got) - ref)
    return err / abs(ref) if err else 0.0


def test_l1sr_one_hot_class():
    """One untied element at j: a dropped or doubled thread, block or tail element changes the loss
    by all of it.  L1 term (0.875 / 0.125) and shadow term (0.125 / 0.0625).  Exposes: drop_block."""
    n = R.three_trip(R.T_L1)
    for j in R.one_hot_positions(n, R.T_L1):
        for pv, tv in ((0.875, 0.125), (0.125, 0.0625)):
            p, t = R.loss_one_hot((n,), j, pv, tv, 3)
            ref = R.l1sr(p, t)[0]
            assert _note("l1sr one-hot loss / 2u", _rel(R.emu_l1sr(p, t)[0], ref) / (2 * U)) <= 1
            assert _rel(R.emu_l1sr(p, t, mutant="drop_block")[0], ref) > 2 * U


def test_l1sr_threshold_class():
    """Exposes: ge (the elements exactly on float32(0.1))."""
    for n in (6, 257, 1000):
        p, t, count = R.loss_threshold(n)
        a, s, _ = R.l1sr_parts(p, t)
        assert s * n == count
        ref = R.l1sr(p, t)[0]
        tol = 2 * U * 0.25 * s + R.loss_dense_bound(n) * 0.5 * a
        assert _note("l1sr threshold loss", abs(float(R.emu_l1sr(p, t)[0]) - ref) / tol) <= 1
        assert abs(float(R.emu_l1sr(p, t, mutant="ge")[0]) - ref) > tol


def test_l1sr_dense_class_and_the_final_sum():
    """(ceil(n/T) + 13) u with 2x room for the double final sum.  Exposes: drop_block.  The serial
    fp32 final sum l1sr_final_kernel used to have is measured beside it (reported, not asserted: its
    worst case is 1023 u more, its typical error is not)."""
    for n in L1_SIZES:
        p, t = R.loss_dense((n,), n)
        q, s = R.loss_dense((n + 5,), n + 1)
        ref = R.l1sr(p, t, q, s)[0]
        bound = R.loss_dense_bound(n + 5)
        assert _note("l1sr dense loss", _rel(R.emu_l1sr(p, t, q, s)[0], ref) / bound) <= 0.5
        _note("l1sr dense loss, fp32 final sum (not asserted)",
              _rel(R.emu_l1sr(p, t, q, s, final_double=False)[0], ref) / bound)
        assert _rel(R.emu_l1sr(p, t, q, s, mutant="drop_block")[0], ref) > bound


L1F_SHAPES = [(1, 1, 1), (1, 3, 21), (1, 1, 64), (1, 5, 13), (3, 1, 85), (1, 2, 128), (1, 1, 257), (2, 4, 125),
              (1, 3, 174849)]     # n = 1, 63, 64, 65, 255, 256, 257, 1000, 524547 >= 2 T + 257


def test_l1frames_gradient_class():
    """Within 2u (|g1| + 2 |gt|) of float64; exactly 0.0 on ties.  Exposes: sign0, swap_t."""
    for shape in L1F_SHAPES:
        for red in (0, 1):
            p, t = R.loss_generic(shape, shape[2] + red)
            _, g64 = R.l1frames(p, t, 0.9, 0.1, 0.1, red)
            n, n2 = p.size, shape[0] * (shape[1] - 1) * shape[2]
            tol = 2 * U * (R.f32(0.9) * (1 if red else 1 / n) + 2 * R.f32(0.1) * (1 if red or not n2 else 1 / n2))
            _, g = R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red)
            assert _note("l1frames gradient", np.abs(g - g64).max() / tol) <= 1
            assert np.abs(R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red, mutant="sign0")[1] - g64).max() > tol
            if shape[1] > 1:
                assert np.abs(R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red, mutant="swap_t")[1] - g64).max() > tol


def test_l1frames_tie_classes():
    """pred == target on a block: gradient exactly 0.0 there; pred = target + c(pixel), constant over
    frames: temporal term and temporal gradient exactly 0."""
    p, t = R.loss_generic((2, 3, 300), 4)
    p[:, :, :256] = t[:, :, :256]
    _, g = R.emu_l1frames(p, t, 0.9, 0.1, 0.1, 0)
    assert np.all(g[:, :, :256] == 0.0) and np.count_nonzero(g[:, :, 256:]) > 200
    t = R.dyadic((2, 3, 300), 9)
    p = t + (R.dyadic((2, 1, 300), 10) + np.float32(2.0 ** -10))
    loss, g = R.emu_l1frames(p, t, 0.9, 0.1, 0.1, 0)
    assert np.all(g == np.float32(R.f32(0.9) / p.size))
    assert R.l1frames_parts(p, t, 0.1)[2] == 0.0


def test_l1frames_one_hot_threshold_and_dense_classes():
    """One differing pixel in one frame (L1, binary and temporal terms at once: 0.875 / 0.125 crosses
    no threshold, 0.125 / 0.0625 does), the threshold triples at `binary`, dense all-positive.
    Exposes: drop_block (one-hot, dense), ge (threshold)."""
    shape = (1, 3, 174849)
    n = shape[0] * shape[1] * shape[2]
    for j in R.one_hot_positions(n, R.T_L1):
        for pv, tv in ((0.875, 0.125), (0.125, 0.0625)):
            p, t = R.loss_one_hot(shape, j, pv, tv, 5)
            for red in (0, 1):
                ref = R.l1frames(p, t, 0.9, 0.1, 0.1, red)[0]
                got = R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red)[0]
                assert _note("l1frames one-hot loss / 2u", _rel(got, ref) / (2 * U)) <= 1
                assert _rel(R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red, mutant="drop_block")[0], ref) > 2 * U
    for binary in (0.1, 0.3):
        p, t, count = R.loss_threshold(2 * 3 * 50, R.f32(binary))
        p, t = p.reshape(2, 3, 50), t.reshape(2, 3, 50)
        s1, sb, st, _, _ = R.l1frames_parts(p, t, binary)
        assert sb == count
        ref = R.l1frames(p, t, 0.9, 0.1, binary, 0)[0]
        tol = 2 * U * R.f32(0.9) * sb / p.size + R.loss_dense_bound(p.size) * (ref - R.f32(0.9) * sb / p.size)
        assert _note("l1frames threshold loss", abs(float(R.emu_l1frames(p, t, 0.9, 0.1, binary, 0)[0]) - ref) / tol) <= 1
        assert abs(float(R.emu_l1frames(p, t, 0.9, 0.1, binary, 0, mutant="ge")[0]) - ref) > tol
    for shape in L1F_SHAPES:
        p, t = R.loss_dense(shape, shape[2])
        for red in (0, 1):
            ref = R.l1frames(p, t, 0.9, 0.1, 0.1, red)[0]
            bound = R.loss_dense_bound(p.size)
            assert _note("l1frames dense loss", _rel(R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red)[0], ref) / bound) <= 0.5
            assert _rel(R.emu_l1frames(p, t, 0.9, 0.1, 0.1, red, mutant="drop_block")[0], ref) > bound


# ------------------------------------------------------------------ clip + AdamW
def _three_steps(x, hyper, step0, ranges=None, **emu_kw):
    """Three consecutive updates from the class's nonzero moments, the emulation fed its own state and
    the model fed the same fp32 state (so each step is judged on its own roundings).  -> worst ratios"""
    n = x["theta"].size
    th, m, v = x["theta"], x["m"], x["v"]
    worst = {}
    for i in range(3):
        g = x["grad"] if i == 0 else (x["grad"] * np.float32(1 - 0.25 * i)).astype(np.float32)[::-1].copy()
        args = (th, g, m, v, x["gscale"], x["max_norm"])
        ref = R.clip_adamw(*args, step=step0 + i, ranges=ranges, **hyper)
        got = R.emu_clip_adamw(*args, step=step0 + i, ranges=ranges, **hyper, **emu_kw)
        for k, r in R.check_adamw(got, ref, th, n, hyper["beta1"], hyper["beta2"]).items():
            worst[k] = max(worst.get(k, 0.0), r)
        outside = ~ref["mask"]
        for k, old in (("theta", th), ("m", m), ("v", v)):
            assert np.array_equal(got[k][outside], old[outside])
        th, m, v = got["theta"], got["m"], got["v"]
    return worst


ADAMW_N = (1, 257, 1000)


@pytest.mark.parametrize("cls", R.ADAMW_CLASSES)
@pytest.mark.parametrize("hyper", [R.HYPER, R.HYPER_T], ids=["b0.9", "b0.2"])
def test_adamw_emulation_meets_every_bound(cls, hyper):
    for n in ADAMW_N:
        for step0 in (1, 2, 1000, 300000):
            w = _three_steps(R.adamw_inputs(n, cls, n), hyper, step0)
            for k, r in w.items():
                assert _note(f"adamw {k}", r) <= 1, (cls, n, step0, k, r)


def test_adamw_norm_at_the_three_trip_size():
    n = R.three_trip(R.T_SUMSQ)                       # 2 * 524288 + 257 = 1048833
    g = R.spread(n, 0.25, 1.0, 1, signed=False)
    z = np.zeros(n, dtype=np.float32)
    got = R.emu_clip_adamw(z, g, z, z, 1.0, 0.01, step=1, **R.HYPER)
    ref = R.clip_adamw(z, g, z, z, 1.0, 0.01, step=1, **R.HYPER)
    assert _note("adamw norm", _rel(got["norm"], ref["norm"]) / R.norm_dense_bound(n)) <= 1
    assert _note("adamw scale", _rel(got["scale"], ref["scale"]) / R.scale_bound(n, True)) <= 1
    for j in R.one_hot_positions(n, R.T_SUMSQ):
        got = R.emu_clip_adamw(z, R.one_hot_grad(n, j), z, z, 0.125, 0.01, step=1, **R.HYPER)
        assert _rel(got["norm"], 0.75 * 0.125) <= 2 * U


def test_adamw_zero_gradient():
    x = R.adamw_inputs(257, "clip")
    z = np.zeros(257, dtype=np.float32)
    got = R.emu_clip_adamw(x["theta"], z, z, z, 0.125, 0.01, step=1, **R.HYPER)
    assert got["norm"] == 0 and got["scale"] == np.float32(0.125)
    assert not got["m"].any() and not got["v"].any()
    f = np.float32(1) - np.float32(R.HYPER["lr"]) * np.float32(R.HYPER["weight_decay"])
    assert np.array_equal(got["theta"], x["theta"] * f)


# which class exposes which mutant (steps 1..3, both beta pairs, n = 1000)
MUTANT_CLASS = {"eps_in_sqrt": "tiny", "no_bc1": "clip", "no_bc2": "clip", "l2_wd": "clip", "no_1e6": "tiny",
                "no_clamp": "noclip"}


@pytest.mark.parametrize("mutant", sorted(MUTANT_CLASS))
@pytest.mark.parametrize("hyper", [R.HYPER, R.HYPER_T], ids=["b0.9", "b0.2"])
def test_adamw_mutants_miss(mutant, hyper):
    w = _three_steps(R.adamw_inputs(1000, MUTANT_CLASS[mutant], 1), hyper, 1, mutant=mutant)
    assert max(w.values()) > 1, w


RANGES3 = [(3, 130), (131, 131), (257, 999)]      # an empty one, unaligned begins


def test_adamw_ranges_and_the_norm_over_ranges_mutant():
    """theta / m / v outside the ranges keep their bits (_three_steps asserts it), the norm covers
    all n: the mutant that sums the updated ranges only misses the norm bound."""
    x = R.adamw_inputs(1000, "clip", 2)
    for ranges in (None, RANGES3, [(517, 518)]):
        assert max(_three_steps(x, R.HYPER, 1, ranges=ranges).values()) <= 1
    w = _three_steps(x, R.HYPER, 1, ranges=RANGES3, mutant="norm_ranges")
    assert w["norm"] > 1, w


def test_fp32_bias_corrections_miss_the_theta_bound():
    """launch_adamw's earlier 1.f - powf(beta2, step): at step 2 with beta2 = 0.999 the subtraction
    cancels and the rounding of powf's result sits on 2e-3.  The double route meets the bound on the
    same input, so the difference is the bias correction alone."""
    bc_d = R.bias_corrections(0.9, 0.999, 2)
    bc_f = R.bias_corrections(0.9, 0.999, 2, fp32_pow=True)
    exact = math.sqrt(1 - R.f32(0.999) ** 2)
    print(f"bc2s at step 2: double route {abs(float(bc_d[1]) - exact) / exact / U:.2f} u, "
          f"fp32 route {abs(float(bc_f[1]) - exact) / exact / U:.1f} u")
    x = R.adamw_inputs(1000, "clip", 1)
    x["theta"] = R.spread(1000, 1e-4, 2e-4, 5)
    args = (x["theta"], x["grad"], x["m"], x["v"], 1.0, 0.01)
    ref = R.clip_adamw(*args, step=2, **R.HYPER)
    good = R.check_adamw(R.emu_clip_adamw(*args, step=2, **R.HYPER), ref, x["theta"], 1000, 0.9, 0.999)
    old = R.check_adamw(R.emu_clip_adamw(*args, step=2, fp32_pow=True, **R.HYPER), ref, x["theta"], 1000, 0.9, 0.999)
    _note("adamw theta, fp32 powf route at step 2 (not a bound the kernel keeps)", old["theta"])
    assert good["theta"] <= 1 < old["theta"], (good, old)


# ------------------------------------------------------------------ mixup, EMA, MSE
PERMS = {"identity": [0, 1, 2, 3, 4], "reversal": [4, 3, 2, 1, 0], "fixed points": [0, 3, 2, 4, 1]}


def test_mixup_emulation_and_mutants():
    """Exposes: perm_first and swapped on every perm but the identity, at every lam but 0.5 / 1 / 0
    respectively; lam = 0.3 exposes both."""
    for per in (1, 3, 1000):
        x = R.spread(5 * per, 1e-3, 1.0, per).reshape(5, per)
        for name, perm in PERMS.items():
            for lam in (0.0, 1.0, 0.5, 0.3):
                ref, tol = R.mixup(x, perm, lam), R.mixup_bound(x, perm, lam)
                assert _note("mixup", np.max(np.abs(R.emu_mixup(x, perm, lam) - ref) / (tol + 1e-300))) <= 1
                if name != "identity" and lam == 0.3:
                    for mutant in ("perm_first", "swapped"):
                        assert np.any(np.abs(R.emu_mixup(x, perm, lam, mutant) - ref) > tol)
        one = x[:1]
        assert np.all(np.abs(R.emu_mixup(one, [0], 0.3) - R.mixup(one, [0], 0.3)) <= R.mixup_bound(one, [0], 0.3))


def test_ema_emulation_and_mutant():
    """Exposes: swapped at every decay but 0.5."""
    for n in R.SMALL_SIZES:
        e, th = R.spread(n, 1e-4, 1.0, n), R.spread(n, 1e-4, 1.0, n + 1)
        for decay in (0.999, 0.9, 0.0, 1.0):
            ref, tol = R.ema(e, th, decay), R.ema_bound(e, th)
            assert _note("ema", np.max(np.abs(R.emu_ema(e, th, decay) - ref) / tol)) <= 1
            assert np.any(np.abs(R.emu_ema(e, th, decay, "swapped") - ref) > tol)
            same = R.emu_ema(e, e, decay)
            assert np.all(np.abs(same - e) <= np.spacing(np.abs(e)))


def test_mse_emulation_and_mutants():
    """Exposes: no2 always, no_scale at scale 1/32."""
    for n in (1, 63, 64, 65, 200):
        s, t = R.spread(n, 0.05, 1.0, n), R.spread(n, 0.05, 1.0, n + 1)
        for scale in (1.0, 1 / 32):
            ds64, l0, l1 = R.mse(s, t, scale)
            ds, a, m = R.emu_mse(s, t, scale)
            tol = 3 * U * np.abs(ds64) + 1e-300
            assert _note("mse dscore", np.max(np.abs(ds - ds64) / tol)) <= 1
            assert _note("mse loss[0]", _rel(a, l0) / ((n + 2) * U)) <= 1
            assert _note("mse loss[1]", _rel(m, l1) / ((n + 1) * U)) <= 1
            assert np.any(np.abs(R.emu_mse(s, t, scale, "no2")[0] - ds64) > tol)
            if scale != 1.0:
                assert np.any(np.abs(R.emu_mse(s, t, scale, "no_scale")[0] - ds64) > tol)

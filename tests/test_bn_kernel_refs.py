"""The references of tests/bn_kernel_refs.py, checked without a GPU:

* the float64 models against torch in float64 (F.batch_norm(training=True) + relu and its autograd, the
  running statistics, F.interpolate(bilinear, align_corners=True) and its autograd) to 1e-12;
* the fp32 emulations of the kernels (operation order and thread / lane / block partition re-derived in
  Python) meet every bound on every input of tests/test_bn_kernels_gpu.py; the worst error / bound per
  quantity is printed (``EMU`` lines).  The element-wise bounds (y, dz) and the two-term sums count at most
  a handful of roundings at u each and take no constant on top, so over millions of elements the emulation
  comes within a few per cent of them (0.9 - 0.97 measured): that is the bound being sharp, not loose
  headroom lost; a contracted multiply-add on the GPU only removes roundings;
* every mutant misses a bound on those same inputs; the factor is printed (``MUTANT`` lines) and must be
  >= 10 unless the mutation is a rounding-level one.

Two mutations the issue lists turn out to be equivalent to the kernel, and the tests say so instead of
pretending to catch them:

* the backward window one candidate short on either side.  Low index i receives from output o only when
  i - 1 < o (n - 1) / (2n - 1) < i + 1, i.e. 2i - 2 + (i - 1) / (n - 1) < o < 2i + 2 + (i + 1) / (n - 1),
  and o <= 2n - 1: only the candidates k = 2 .. 5 of o = 2i - 3 + k can carry weight; k = 0, 1, 6, 7 are
  slack.  ``window_1short_*`` is asserted bit-identical; ``window_short_*`` (the first / last live
  candidate cut) is the mutant that must miss.
* the second neighbour not clamped at the last row.  fl(fl((n - 1) / (2n - 1)) (2n - 1)) <= n - 1 for every
  n tried (2 .. 4100), so the last row has l1 = 0 whenever i0 = n - 1, and the unclamped read is multiplied by
  zero: it shows only when the memory after the tensor is not finite.  The GPU test therefore puts +inf
  behind the forward input, and the mutant is run that way here.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as TF

import bn_kernel_refs as R

F = np.float32


def _t(a):
    return torch.from_numpy(np.asarray(a, dtype=np.float64))


# ------------------------------------------------------------------ float64 models against torch
@pytest.mark.parametrize("C,P,mom", [(12, 70, 0.1), (4, 2, 0.3), (64, 259, 0.1)])
def test_models_against_torch(C, P, mom):
    t = R.bn_inputs(C, P)
    z = _t(t["z"]).requires_grad_(True)
    gamma, beta = _t(t["gamma"]).requires_grad_(True), _t(t["beta"]).requires_grad_(True)
    rm, rv = _t(t["rm"]).clone(), _t(t["rv"]).clone()
    m = R.f32(mom)
    # [P][C] -> N = P, C: batch statistics over the P rows
    pre = TF.batch_norm(z, rm, rv, gamma, beta, training=True, momentum=m, eps=R.EPS)
    y = torch.relu(pre)
    st = R.bn_stats(t["z"], t["rm"], t["rv"], mom)
    assert np.abs(st["rm"] - rm.numpy()).max() <= 1e-12 and np.abs(st["rv"] - rv.numpy()).max() <= 1e-12
    ym = R.bn_apply_relu(t["z"], st["mean"], st["rstd"], t["gamma"], t["beta"])
    assert np.abs(ym - y.detach().numpy()).max() <= 1e-12
    dy = _t(t["dy"])
    y.backward(dy)
    # the model gates on the y it is handed: hand it torch's own
    dg, db = R.bn_bwd_reduce(t["dy"], ym, t["z"], st["mean"], st["rstd"])
    assert np.abs(dg - gamma.grad.numpy()).max() <= 1e-11 and np.abs(db - beta.grad.numpy()).max() <= 1e-11
    dz = R.bn_bwd_dx(t["dy"], ym, t["z"], st["mean"], st["rstd"], t["gamma"], dg, db)
    assert np.abs(dz - z.grad.numpy()).max() <= 1e-10   # rstd = 316 on the constant channel scales the error


def test_model_single_pixel_rule():
    """P = 1: torch refuses to train on one value per channel; the kernel takes mean = x, var = 0 and feeds
    the biased variance (0) to the running update."""
    t = R.bn_inputs(8, 1)
    st = R.bn_stats(t["z"], t["rm"], t["rv"], 0.1)
    assert np.array_equal(st["mean"], t["z"][0].astype(np.float64)) and not st["var"].any()
    assert np.allclose(st["rstd"], 1 / np.sqrt(R.EPS), rtol=1e-15)
    assert np.abs(st["rv"] - (1 - R.f32(0.1)) * t["rv"].astype(np.float64)).max() <= 1e-15


@pytest.mark.parametrize("h,w", R.UP_SIZES[:-1] + ((9, 4),))
def test_upsample_matrices_against_torch(h, w):
    N, C = 2, 3
    x, v = R.up_inputs(N, C, h, w)
    xt = _t(x).permute(0, 3, 1, 2).clone().requires_grad_(True)
    ref = TF.interpolate(xt, scale_factor=2, mode="bilinear", align_corners=True)
    Uy, Ux = R.up_matrix(h), R.up_matrix(w)
    assert np.abs(R.up_fwd(x, Uy, Ux) - ref.detach().permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    ref.backward(_t(v).permute(0, 3, 1, 2))
    assert np.abs(R.up_bwd(v, Uy, Ux) - xt.grad.permute(0, 2, 3, 1).numpy()).max() <= 1e-12
    # the fp32-weight matrices are within the stated weight error of the exact ones, and rows sum to ~1
    for n, Um in ((h, Uy), (w, Ux)):
        V = R.up_matrix_f32(n)
        assert np.abs(V - Um).max() <= R.up_weight_err(n)
        assert np.abs(V.sum(1) - 1).max() <= R.U and np.abs(Um.sum(1) - 1).max() <= 1e-15


def test_last_row_never_overshoots():
    assert not any(R.last_overshoots(n) for n in range(1, 4101))


# ------------------------------------------------------------------ geometry
def test_case_grid_reaches_every_class():
    """Each lanes class meets each P class; the cap case is past both caps with a ragged last block."""
    seen = {}
    for C, P in R.bn_cases():
        k = R.case_class(C, P)
        assert (R.ew_cover(C, P) == 1).all(), (C, P)
        s = seen.setdefault(k["lanes"], set())
        s.add("P1" if P == 1 else "P2" if P == 2 else "")
        if P < k["lanes"]:
            s.add("below_a_run")
        if k["nblk"] == 1 and P == 16 * k["lanes"] - 1:
            s.add("one_block_full")
        if k["nblk"] == 2 and P == 16 * k["lanes"] + 1:
            s.add("two_blocks")
        if 2 <= k["nblk"] < 16 and k["ragged"]:
            s.add("few_ragged")
        if k["nblk"] >= 17 and k["nblk"] % 16:
            s.add("many")
    assert sorted(seen) == [1, 4, 8, 16, 21, 51, 85, 256]
    for lanes, s in seen.items():
        need = {"P1", "P2", "one_block_full", "two_blocks", "few_ragged", "many"} | ({"below_a_run"} if lanes > 2 else set())
        assert need <= s, (lanes, need - s)
    C, P = R.CAP_CASE
    k = R.case_class(C, P)
    assert (P + 15) // 16 > R.BN_MAX_BLOCKS and k["per"] == 17 and k["ragged"] and k["nblk"] < R.BN_MAX_BLOCKS
    assert (P + R.KU - 1) // R.KU > R.EW_CAP and k["ew"] == R.EW_CAP
    N, C, h, w = R.BWD_CAP_CASE
    assert N * h * w * (C // 4) > R.BWD_CAP * 256
    N, C, h, w = R.FWD_CAP_CASE
    assert R.FWD_CAP * 256 < N * 4 * h * w * (C // 4) <= (R.FWD_CAP + 64) * 256


def test_onehot_rounds_visit_every_lane_block_and_tail():
    for C, P in R.ONEHOT_CASES:
        lanes = R.lanes_of(C)
        nblk, per = R.red_geom(C, P)
        hit = set()
        for dy in R.onehot_rounds(C, P):
            assert ((dy != 0).sum(0) == 1).all()
            hit |= set(np.nonzero(dy)[0].tolist())
        assert {p // per for p in hit} == set(range(nblk))
        assert {(p % per) % lanes for p in hit} >= set(range(min(lanes, per)))
        assert 0 in hit and P - 1 in hit


# ------------------------------------------------------------------ emulations meet the bounds
def _worst(into, r, tag):
    for k, v in r.items():
        if v >= into.get(k, (-1.0, None))[0]:
            into[k] = (v, tag)


def test_emulation_meets_every_bound():
    worst = {}
    for C, P in R.bn_cases():
        t = R.bn_inputs(C, P)
        for mom in (R.MOMENTUM, 0.3):
            _worst(worst, R.bn_ratios(t, C, P, R.emu_all(t, C, P, mom, only="stats"), mom), (C, P))
        _worst(worst, R.bn_ratios(t, C, P, {k: v for k, v in R.emu_all(t, C, P).items() if k in ("y", "dgamma", "dbeta", "dz")}),
               (C, P))
    for C, P in ((64, 4097), (12, 1000)):
        t = R.bn_inputs(C, P, "bigmean")
        _worst(worst, R.bn_ratios(t, C, P, R.emu_all(t, C, P)), (C, P, "bigmean"))
    for k, (v, tag) in sorted(worst.items()):
        print(f"EMU {k}: worst error / bound {v:.3f} at {tag}")
        assert v <= 1.0, (k, v, tag)


def test_emulation_onehot_sums():
    """One nonzero per channel: dbeta is exact and dgamma within 3 u |g xhat| (its bound with depth 0)."""
    worst = 0.0
    for C, P in R.ONEHOT_CASES:
        t = R.bn_inputs(C, P)
        ones = np.ones((P, C), F)
        for dy in R.onehot_rounds(C, P):
            dg, db = R.emu_bwd_reduce(dy, ones, t["z"], t["mean"], t["rstd"], C, P)
            assert np.array_equal(db, dy.sum(0))
            rg, rb = R.bn_bwd_reduce(dy, ones, t["z"], t["mean"], t["rstd"])
            bg, bb = R.reduce_bounds(dy, ones, t["z"], t["mean"], t["rstd"], C, P)
            assert not bb.any()
            worst = max(worst, R.ratio(dg - rg, bg))
    print(f"EMU onehot dgamma: worst error / bound {worst:.3f}")
    assert worst <= 1.0


def test_emulation_upsample():
    w_t = w_w = b_t = b_w = 0.0
    for N, C, h, w in R.up_cases():
        x, v = R.up_inputs(N, C, h, w)
        Uy, Ux, Vy, Vx = R.up_matrix(h), R.up_matrix(w), R.up_matrix_f32(h), R.up_matrix_f32(w)
        tight, wide = R.up_fwd_bounds(x, h, w)
        got = R.emu_up_fwd(x, after=np.inf)
        w_t, w_w = max(w_t, R.ratio(got - R.up_fwd(x, Vy, Vx), tight)), max(w_w, R.ratio(got - R.up_fwd(x, Uy, Ux), wide))
        tight, wide = R.up_bwd_bounds(v, h, w)
        got = R.emu_up_bwd(v)
        b_t, b_w = max(b_t, R.ratio(got - R.up_bwd(v, Vy, Vx), tight)), max(b_w, R.ratio(got - R.up_bwd(v, Uy, Ux), wide))
        for m in ("window_1short_lo", "window_1short_hi"):   # equivalent: candidates 0, 1, 6, 7 never carry weight
            assert np.array_equal(R.emu_up_bwd(v, mutant=m), got), (m, h, w)
    print(f"EMU upsample fwd: fp32 weights {w_t:.3f}, exact weights {w_w:.3f}; bwd: {b_t:.3f}, {b_w:.3f}")
    assert max(w_t, w_w, b_t, b_w) <= 1.0


# ------------------------------------------------------------------ mutants
_BN_MUTANTS = [  # mutant, op, quantity it must break, cases to look at
    ("biased_running", "stats", "rv", "all"), ("unbiased_rstd", "stats", "rstd", "all"),
    ("eps_outside", "stats", "rstd", "all"), ("momentum_old", "stats", "rm", "all"),
    ("ragged_full", "stats", "mean", "all"), ("segment_skipped", "stats", "mean", "all"),
    ("lane_dropped", "stats", "mean", "all"), ("idle_garbage", "stats", "mean", "all"),
    ("subtractive", "stats", "rstd", "bigmean"),
    ("gate_ge", "reduce", "dbeta", "all"), ("gate_z", "reduce", "dbeta", "all"),
    ("lane_dropped", "reduce", "dbeta", "all"), ("idle_garbage", "reduce", "dgamma", "all"),
    ("block_dropped", "reduce", "dbeta", "all"),
    ("gate_ge", "dx", "dz", "all"), ("gate_z", "dx", "dz", "all"), ("no_dbeta", "dx", "dz", "all"),
    ("no_dgamma", "dx", "dz", "all"), ("no_gamma", "dx", "dz", "all"), ("wrong_P", "dx", "dz", "all"),
]
_MUTANT_CASES = [(C, P) for C, P in R.bn_cases() if C * P <= 40000]


@pytest.mark.parametrize("mutant,op,what,where", _BN_MUTANTS, ids=lambda v: v if isinstance(v, str) else None)
def test_bn_mutant_misses(mutant, op, what, where):
    """The largest miss over the GPU test's own inputs, and in how many of them the mutant misses at all."""
    cases = [(64, 4097, "bigmean"), (12, 1000, "bigmean")] if where == "bigmean" else [c + ("plain",) for c in _MUTANT_CASES]
    best, hit = (0.0, None), 0
    for C, P, kind in cases:
        t = R.bn_inputs(C, P, kind)
        r = R.bn_ratios(t, C, P, R.emu_all(t, C, P, mutant=mutant, only=op)).get(what, 0.0)
        hit += r > 1
        if r > best[0]:
            best = (r, (C, P))
    print(f"MUTANT {op} {mutant}: {what} misses its bound by a factor {best[0]:.3g} at {best[1]}; "
          f"missed in {hit} of {len(cases)} cases")
    assert best[0] >= 10


@pytest.mark.parametrize("mutant", ["half_pixel", "swap", "no_clamp"])
def test_upsample_fwd_mutant_misses(mutant):
    best = 0.0
    for N, C, h, w in R.up_cases()[:-1]:
        x, _ = R.up_inputs(N, C, h, w)
        tight, _ = R.up_fwd_bounds(x, h, w)
        with np.errstate(invalid="ignore"):
            got = R.emu_up_fwd(x, mutant=mutant, after=np.inf)
            err = np.where(np.isfinite(got), got - R.up_fwd(x, R.up_matrix_f32(h), R.up_matrix_f32(w)), np.inf)
        best = max(best, R.ratio(err, tight))
    print(f"MUTANT upsample2x {mutant}: misses the fp32-weight bound by a factor {best:.3g}")
    assert best >= 10


@pytest.mark.parametrize("mutant", ["half_pixel", "swap", "window_short_lo", "window_short_hi"])
def test_upsample_bwd_mutant_misses(mutant):
    best = 0.0
    for N, C, h, w in R.up_cases()[:-1]:
        _, v = R.up_inputs(N, C, h, w)
        tight, _ = R.up_bwd_bounds(v, h, w)
        best = max(best, R.ratio(R.emu_up_bwd(v, mutant=mutant) - R.up_bwd(v, R.up_matrix_f32(h), R.up_matrix_f32(w)), tight))
    print(f"MUTANT upsample2x_bwd {mutant}: misses the fp32-weight bound by a factor {best:.3g}")
    assert best >= 10

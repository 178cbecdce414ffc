"""Float64 model, fp32 emulation, mutants, inputs and the judge for ``kdlae_train_l1sonar`` (L1LossSonar,
Train/basicsr/models/losses/losses.py:25-65).  Needs no GPU.  tests/test_restormer.py proves the model against
values recorded from the reference (tests/golden/restormer_loss.npz), shows that the emulation of the kernel's
operation order meets every check below and that each mutant misses one; tests/test_restormer_gpu.py holds the
shipped kernel to the same checks on the same inputs (``CASES`` / ``judge``).

Bounds are those of tests/step_kernel_refs.py, derived there by counting roundings: gradients exact
(``sign(p - t) float32(w / n)`` or ``float32(w)``, 0.0 on a tie), a one-hot loss within 2u (every partial sum is
exact; the double final product and the cast round once), a dense loss within (ceil(n / T) + 13) u with
T = 1024 blocks * 256 threads."""
import math

import numpy as np

from tests import step_kernel_refs as R

F = np.float32
U = R.U
SONAR_BLOCKS = 1024            # train.hip kSonarBlocks (min with ceil(n / 256))
T = SONAR_BLOCKS * 256
SIZES = (1, T - 1, T + 1, 2 * T + 257)
REDUCTIONS = ("mean", "sum")
MUTANTS = ("ge", "bin_grad", "sign0", "w_drop", "drop_block", "sum_div_n")


def l1sonar(pred, tgt, loss_weight, binary, reduction):
    """loss_weight (red|p - t| + red|[p > binary] - [t > binary]|), red = 'mean' / 'sum'; the gradient is
    loss_weight sign(p - t) (/ n for 'mean'): the binarised term carries none.  -> (loss, dpred), float64."""
    p, t = np.asarray(pred, np.float64).ravel(), np.asarray(tgt, np.float64).ravel()
    w, b = R.f32(loss_weight), R.f32(binary)
    inv = 1.0 / p.size if reduction == "mean" else 1.0
    d = p - t
    sb = np.abs((p > b).astype(np.float64) - (t > b))
    return w * (np.abs(d).sum() * inv + sb.sum() * inv), w * inv * np.sign(d)


def grad_exact(pred, tgt, loss_weight, reduction):
    """The gradient the kernel must give bit for bit."""
    p, t = np.asarray(pred, np.float64).ravel(), np.asarray(tgt, np.float64).ravel()
    w = R.f32(loss_weight)
    c = F(w / p.size) if reduction == "mean" else F(w)
    return (np.sign(p - t) * c).astype(F)


def emu_l1sonar(pred, tgt, loss_weight, binary, reduction, mutant=None):
    """l1sonar_kernel + l1sonar_final_kernel in fp32, in the kernel's operation order (grid-stride chain per
    thread, block_sum_256, double final sum in block order, one cast)."""
    p, t = np.asarray(pred, dtype=F).ravel(), np.asarray(tgt, dtype=F).ravel()
    n = p.size
    w, b = R.f32(loss_weight), F(R.f32(binary))
    mean = reduction == "mean"
    inv = 1.0 / n if (mean or mutant == "sum_div_n") else 1.0
    c = F(w / n) if (mean or mutant == "sum_div_n") else F(w)
    d = p - t
    gt_ = np.greater_equal if mutant == "ge" else np.greater
    bp, bt = gt_(p, b).astype(F), gt_(t, b).astype(F)
    sb = np.abs(bp - bt)
    pos = d >= 0 if mutant == "sign0" else d > 0
    sg = np.where(pos, F(1), np.where(d < 0, F(-1), F(0))).astype(F)
    if mutant == "bin_grad":
        sg = sg + (bp - bt)
    grad = (sg * c).astype(F)
    blocks = min(SONAR_BLOCKS, math.ceil(n / 256))
    pa = R._block_sum_256(R._thread_partials(np.abs(d), blocks))
    if mutant == "drop_block" and np.any(pa):      # the last block that saw data never reaches the final sum
        pa = R._drop(pa, mutant)
    ps = R._block_sum_256(R._thread_partials(sb, blocks))
    a, s = float(np.asarray(pa, np.float64).sum()), float(np.asarray(ps, np.float64).sum())
    loss = F(w * (a * inv) + s * inv) if mutant == "w_drop" else F(w * ((a + s) * inv))
    return loss, grad


# ------------------------------------------------------------------------------------------------ inputs
def _plant(p, t, binary):
    """Elements exactly at ``binary`` and one ulp above it, in pred (against a target of 0: two at, one above)
    and in target (against a pred of 0.5: one at, one above).  Under the strict `>` the ones at ``binary``
    binarise to 0; a `>=` moves two pred-side and one target-side element, so the count changes."""
    if p.size < 16:
        return
    b = F(R.f32(binary))
    up = np.nextafter(b, F(1), dtype=F)
    p[1:6] = [b, up, 0.5, 0.5, b]
    t[1:6] = [0, 0, b, up, 0]


def generic(n, binary):
    p, t = R.loss_generic((n,), n)
    _plant(p, t, binary)
    return p, t


def dense(n, binary):
    p, t = R.loss_dense((n,), n)
    _plant(p, t, binary)
    return p, t


def _cases():
    out = []
    for red in REDUCTIONS:
        for n in SIZES:
            out.append(dict(kind="generic", n=n, red=red, w=0.7, binary=0.1))
            out.append(dict(kind="dense", n=n, red=red, w=1.0, binary=0.3))
        n = SIZES[-1]
        for pv, tv in ((0.875, 0.125), (0.125, 0.0625)):
            for j in R.one_hot_positions(n, T):
                out.append(dict(kind="one_hot", n=n, red=red, w=0.7, binary=0.1, j=j, pv=pv, tv=tv))
    return out


CASES = _cases()


def case_id(c):
    return "-".join(str(c[k]) for k in ("kind", "n", "red", "j", "pv") if k in c)


def inputs(c):
    if c["kind"] == "one_hot":
        return R.loss_one_hot((c["n"],), c["j"], c["pv"], c["tv"], 3)
    return (generic if c["kind"] == "generic" else dense)(c["n"], c["binary"])


def judge(c, p, t, loss, grad):
    """Ratios to the bounds of one result (emulation or GPU) for case ``c``; every ratio <= 1 passes.
    'grad' is 0 when the gradient has the exact bits, inf otherwise."""
    ref, _ = l1sonar(p, t, c["w"], c["binary"], c["red"])
    g = np.asarray(grad, F).ravel()
    ok = np.array_equal(g.view(np.int32) & 0x7FFFFFFF == 0, grad_exact(p, t, c["w"], c["red"]) == 0) and \
        np.array_equal(g, grad_exact(p, t, c["w"], c["red"]))
    if c["kind"] == "one_hot":
        ok = ok and np.count_nonzero(g) == 1
        bound = 2 * U
    else:
        bound = R.loss_dense_bound(c["n"], T)
    err = abs(float(loss) - ref)
    return {"grad": 0.0 if ok else math.inf, "loss": (err / abs(ref) if err else 0.0) / bound}

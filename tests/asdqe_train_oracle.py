"""TEST INFRASTRUCTURE ONLY — CPU restatement of one ASDQE training micro-batch.

DenoiseRatePredictor in train mode (ASDQE/ASDQE_model.py:123-171 under Train/ASDQE.py:95-122), in
the functional style of ``oracle/asdqe_oracle.py``: BatchNorm with batch statistics and the running
update (``F.batch_norm(training=True, momentum=0.1)`` on cloned buffers), Dropout as a multiply by
an explicit, already scaled mask, ``F.mse_loss``; gradients from torch autograd.  Works in fp32 and
fp64.  ``tests/golden/atrain_*.npz`` (from the imported reference, ``make_golden_asdqe_train.py``)
pin it; the GPU tests and ``tools/asdqe_train_bench.py`` use it.  The product package never imports it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle.asdqe_oracle import AsdqeCfg, asdqe_param_shapes, pad_to_multiple
from rethink_acoustic_image_enhancement_amd.hashweights import hash_images, hash_normal, hash_uniform

# name: (ctor kwargs, input shape, dropout masks active)
CASES = {
    "atrain_b2_24x40": (dict(in_channels=3, dim=16), (2, 3, 24, 40), True),
    "atrain_g1_d32_16": (dict(in_channels=1, dim=32), (3, 1, 16, 16), True),
    "atrain_b4_64_nodrop": (dict(in_channels=3, dim=16), (4, 3, 64, 64), False),
}
SUB = 32  # the goldens keep every SUB-th element of the packed gradient vector
SMALL = 256  # ... and every key of at most SMALL elements in full


def case_tensors(name, shape, suffix, use_masks):
    """Inputs, target and masks of a golden case, regenerated from the hash streams (not stored).
    ``suffix`` is the input key's suffix the generator settled on (stored in the fixture)."""
    B = shape[0]
    key = f"{name}#{suffix}"
    scale = (0.3 + 0.7 * np.arange(1, B + 1) / B).reshape(B, 1, 1, 1)
    sigma = (0.02 + 0.2 * np.arange(B) / max(B - 1, 1)).reshape(B, 1, 1, 1)
    gt = (hash_images(f"gt:{key}", shape) * scale).astype(np.float32)
    lq = np.clip(gt + sigma * hash_normal(f"noise:{key}", shape), 0, 1).astype(np.float32)
    target = (0.5 * hash_uniform(f"target:{name}", B)).astype(np.float32).reshape(B, 1)
    m1 = m2 = None
    if use_masks:
        m1 = ((hash_uniform(f"mask1:{name}", B * 256) >= 0.0) * 2.0).astype(np.float32).reshape(B, 256)
        m2 = (((hash_uniform(f"mask2:{name}", B * 64) + 1.0) * 0.5 >= 0.3) / 0.7).astype(np.float32).reshape(B, 64)
    t = torch.from_numpy
    return t(lq), t(gt), t(target), (t(m1) if use_masks else None), (t(m2) if use_masks else None)


def param_keys(cfg: AsdqeCfg):
    """named_parameters() order: the state_dict keys without the BatchNorm buffers."""
    return [k for k in asdqe_param_shapes(cfg)
            if not k.endswith(("running_mean", "running_var", "num_batches_tracked"))]


def buffer_keys(cfg: AsdqeCfg):
    return [k for k in asdqe_param_shapes(cfg) if k.endswith(("running_mean", "running_var"))]


def bn_fed_bias_keys(cfg: AsdqeCfg):
    """Conv biases that feed a BatchNorm (true gradient 0) -> the following BatchNorm's bias key."""
    out = {}
    for k in param_keys(cfg):
        if k.endswith(".double_conv.0.bias"):
            out[k] = k[:-len("0.bias")] + "1.bias"
        elif k.endswith(".double_conv.3.bias"):
            out[k] = k[:-len("3.bias")] + "4.bias"
    return out


def _double_conv(x, P, Bf, p):
    for i in (0, 3):
        x = F.conv2d(x, P[f"{p}.{i}.weight"], P[f"{p}.{i}.bias"], padding=1)
        bn = f"{p}.{i + 1}"
        x = F.batch_norm(x, Bf[bn + ".running_mean"], Bf[bn + ".running_var"], P[bn + ".weight"], P[bn + ".bias"],
                         training=True, momentum=0.1, eps=1e-5)
        x = torch.relu(x)
    return x


def _down(x, P, Bf, p):
    return _double_conv(F.max_pool2d(x, 2), P, Bf, p + ".maxpool_conv.1.double_conv")


def _up(x1, x2, P, Bf, p):
    x1 = F.interpolate(x1, scale_factor=2, mode="bilinear", align_corners=True)
    dy, dx = x2.shape[2] - x1.shape[2], x2.shape[3] - x1.shape[3]
    x1 = F.pad(x1, [dx // 2, dx - dx // 2, dy // 2, dy - dy // 2])
    return _double_conv(torch.cat([x2, x1], dim=1), P, Bf, p + ".conv.double_conv")


def train_forward(P, Bf, lq, gt, cfg: AsdqeCfg, m1=None, m2=None):
    """Train-mode forward on parameter dict P; the running statistics in Bf are updated in place."""
    lq = pad_to_multiple(lq, cfg.dim)
    gt = pad_to_multiple(gt, cfg.dim)
    merged = torch.cat([_double_conv(lq, P, Bf, "lq_extractor.double_conv"),
                        _double_conv(gt, P, Bf, "gt_extractor.double_conv"),
                        _double_conv(lq - gt, P, Bf, "diff_extractor.double_conv")], dim=1)
    x1 = _double_conv(merged, P, Bf, "unet.inc.double_conv")
    x2 = _down(x1, P, Bf, "unet.down1")
    x3 = _down(x2, P, Bf, "unet.down2")
    x4 = _down(x3, P, Bf, "unet.down3")
    y = _up(x4, x3, P, Bf, "unet.up1")
    y = _up(y, x2, P, Bf, "unet.up2")
    y = _up(y, x1, P, Bf, "unet.up3")
    feat = F.conv2d(y, P["unet.outc.conv.weight"], P["unet.outc.conv.bias"])
    h = torch.relu(F.linear(feat.mean(dim=(2, 3)), P["regressor.2.weight"], P["regressor.2.bias"]))
    if m1 is not None:
        h = h * m1
    h = torch.relu(F.linear(h, P["regressor.5.weight"], P["regressor.5.bias"]))
    if m2 is not None:
        h = h * m2
    return torch.tanh(F.linear(h, P["regressor.8.weight"], P["regressor.8.bias"]))


def train_step(sd, lq, gt, target, cfg: AsdqeCfg, m1=None, m2=None, dtype=torch.float32, device="cpu"):
    """One forward + MSE + backward.  Returns score, loss, per-key gradients (named_parameters order)
    and the updated running statistics; ``sd`` is not modified."""
    cv = lambda t: None if t is None else t.to(device=device, dtype=dtype)  # noqa: E731
    P = {k: sd[k].detach().to(device=device, dtype=dtype).clone().requires_grad_(True) for k in param_keys(cfg)}
    Bf = {k: sd[k].detach().to(device=device, dtype=dtype).clone() for k in buffer_keys(cfg)}
    score = train_forward(P, Bf, cv(lq), cv(gt), cfg, cv(m1), cv(m2))
    loss = F.mse_loss(score, cv(target))
    grads = torch.autograd.grad(loss, list(P.values()))
    return {"score": score.detach(), "loss": loss.detach(), "grads": dict(zip(P.keys(), grads)), "buffers": Bf}


def packed(grads, keys):
    return torch.cat([grads[k].reshape(-1) for k in keys])


def key_of_subsample(cfg: AsdqeCfg):
    """For every element of packed(...)[::SUB]: the index of its key in param_keys(cfg)."""
    shapes = asdqe_param_shapes(cfg)
    sizes = np.array([int(np.prod(shapes[k])) if shapes[k] else 1 for k in param_keys(cfg)])
    ends = np.cumsum(sizes)
    idx = np.arange(0, int(ends[-1]), SUB)
    return np.searchsorted(ends, idx, side="right")

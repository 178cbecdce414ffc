"""KDLAE-T training on the MI355X HIP path.

Three layers, all backed by ``libkdlae.so`` (``kdlae_tt_*`` / ``kdlae_train_*`` in include/kdlae.h):

* ``TrainEngine`` — one training handle per (model, device): forward with saved activations and the
  hand-sequenced backward of every KDLAE_teacher layer over flat parameter / gradient buffers.
* Drop-in autograd: ``KDLAE_teacher.forward`` under grad mode routes through ``TeacherTrainFn`` and
  ``L1LossSr`` here is an autograd-aware HIP loss, so the reference's own loop
  (``preds = net_g(lq); l_pix = cri_pix(preds, gt); l_pix.backward(); clip_grad_norm_; opt.step()``,
  Train/basicsr/models/image_restoration_model.py:198-218) runs unchanged with any torch optimizer.
* ``KDLAETrainer`` — the fast path of that same loop: flat buffers end to end, the HIP L1LossSr, one
  RCCL all-reduce of the flat gradient for DDP (base_model.py:76-82), and the fused
  clip_grad_norm_ + AdamW kernel.  The model's parameters become views of the trainer's flat
  buffer, so ``state_dict()``/checkpoints and the inference path always see the trained weights.

There is no CPU fallback: every entry point raises on CPU tensors or a missing library.
"""
from __future__ import annotations

import ctypes
import math
import random

import torch
import torch.distributed as dist

from . import _lib

__all__ = ["TrainEngine", "TeacherTrainFn", "L1LossSr", "KDLAETrainer", "MixingAugment", "sync_gradients",
           "grad_buckets", "sync_gradients_bucketed", "StudentTrainEngine", "StudentTrainFn",
           "L1LossForVideoFrames", "KDLAESTrainer", "AsdqeTrainEngine", "AsdqeTrainFn", "asdqe_train_forward",
           "asdqe_dropout_masks", "ASDQETrainer", "flat_to_optim_state", "optim_state_to_flat",
           "freeze_except_patch_embed_and_enhance", "RestormerTrainEngine", "L1LossSonar", "RestormerTrainer",
           "CosineAnnealingRestartCyclicLR"]


def _vp(t):
    return ctypes.c_void_p(t.data_ptr() if t is not None else 0)


def _stream(dev):
    return ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)


# ------------------------------------------------------------------ training state (BaseModel.save_training_state)
def _group_template(hyper):
    """The one ``param_groups`` entry this torch writes for AdamW (Adam when ``hyper['optimizer'] == 'Adam'``),
    taken from a throw-away optimizer so every key this torch version knows is there with its default."""
    cls = torch.optim.Adam if hyper.get("optimizer", "AdamW") == "Adam" else torch.optim.AdamW
    opt = cls([torch.nn.Parameter(torch.zeros(1))], lr=float(hyper["lr"]), betas=tuple(hyper["betas"]),
              eps=float(hyper["eps"]), weight_decay=float(hyper["weight_decay"]), amsgrad=False)
    return opt.state_dict()["param_groups"][0]


def flat_to_optim_state(keys, exp_avg, exp_avg_sq, step, hyper, shapes=None) -> dict:
    """The trainers' flat AdamW moments as ``torch.optim.AdamW(...).state_dict()`` (what
    BaseModel.save_training_state stores under ``'optimizers'``, Train/basicsr/models/base_model.py:311-330).

    ``keys``: the engine's ``(name, numel, offset)`` list in ``model.parameters()`` order, the order BasicSR
    hands to the optimizer, so parameter i of the dict is ``keys[i]``.  ``shapes``: the parameters' shapes
    (default: flat ``[numel]``).  ``hyper``: ``lr, betas, eps, weight_decay`` (+ ``optimizer='Adam'`` for the
    Adam layout).  ``state[i] = {'step', 'exp_avg', 'exp_avg_sq'}`` with copies of the moments; one param group."""
    state = {}
    for i, (_, n, off) in enumerate(keys):
        shape = tuple(shapes[i]) if shapes is not None else (n,)
        state[i] = {"step": torch.tensor(float(int(step)), dtype=torch.float32),
                    "exp_avg": exp_avg[off:off + n].detach().clone().view(shape),
                    "exp_avg_sq": exp_avg_sq[off:off + n].detach().clone().view(shape)}
    group = _group_template(hyper)
    group["params"] = list(range(len(keys)))
    return {"state": state, "param_groups": [group]}


def optim_state_to_flat(state, keys, out_exp_avg, out_exp_avg_sq, shapes=None) -> int:
    """Inverse of ``flat_to_optim_state``: an AdamW / Adam ``state_dict()`` (from here or from stock PyTorch)
    into the flat moment buffers; returns the step count.  The pad floats between the 16-byte-aligned keys
    are zeroed.  A parameter torch holds no state for (its ``.grad`` was always None) gets zero moments.
    Raises ValueError on more than one param group, ``amsgrad=True``, a wrong number of parameters, a shape
    (or element count) mismatch at any index, or parameters at different steps."""
    groups = state.get("param_groups", [])
    if len(groups) != 1:
        raise ValueError(f"expected an optimizer state with one param group, got {len(groups)}")
    group = groups[0]
    if group.get("amsgrad", False):
        raise ValueError("amsgrad=True optimizer state cannot be resumed: the HIP AdamW keeps no max_exp_avg_sq")
    params = list(group["params"])
    if len(params) != len(keys):
        raise ValueError(f"optimizer state has {len(params)} parameters, the model has {len(keys)}")
    st = state.get("state", {})
    for i, (pid, (name, n, off)) in enumerate(zip(params, keys)):
        ent = st.get(pid)
        if ent is None:
            continue
        want = tuple(shapes[i]) if shapes is not None else None
        for k in ("exp_avg", "exp_avg_sq"):
            t = ent[k]
            if t.numel() != n or (want is not None and tuple(t.shape) != want):
                raise ValueError(f"parameter {i} ({name}): {k} has shape {tuple(t.shape)}, expected "
                                 f"{want if want is not None else (n,)}")
    steps = {int(float(st[pid]["step"])) for pid in params if pid in st}
    if len(steps) > 1:
        raise ValueError(f"parameters are at different steps {sorted(steps)}: the HIP AdamW keeps one step count")
    out_exp_avg.zero_()
    out_exp_avg_sq.zero_()
    for pid, (name, n, off) in zip(params, keys):
        ent = st.get(pid)
        if ent is None:
            continue
        out_exp_avg[off:off + n].copy_(ent["exp_avg"].detach().reshape(-1))
        out_exp_avg_sq[off:off + n].copy_(ent["exp_avg_sq"].detach().reshape(-1))
    return steps.pop() if steps else 0


class _TrainingState:
    """``BaseModel.save_training_state`` / ``resume_training`` (base_model.py:311-351) for the flat-buffer
    trainers: ``{'epoch', 'iter', 'optimizers': [AdamW state_dict], 'schedulers': [...]}``.  The network
    weights travel separately (``model.state_dict()`` / checkpoint.py), as in BasicSR."""

    _optimizer_name = "AdamW"

    def _hyper(self):
        return dict(lr=self.lr, betas=self.betas, eps=self.eps, weight_decay=self.weight_decay,
                    optimizer=self._optimizer_name)

    def _state_keys(self):
        """The engine's ``(name, numel, offset)`` entries the optimizer holds: the parameters with
        ``requires_grad``, in ``named_parameters()`` order (what ImageCleanModel.setup_optimizers hands to
        AdamW, image_restoration_model.py:139-160); all of them for an engine without a trainable mask."""
        tr = getattr(self.engine, "trainable", None)
        return list(self.engine.keys) if tr is None else [k for k, t in zip(self.engine.keys, tr) if t]

    def _shapes(self):
        tr = getattr(self.engine, "trainable", None)
        shapes = [tuple(p.shape) for p in self.model.parameters()]
        return shapes if tr is None else [sh for sh, t in zip(shapes, tr) if t]

    def training_state(self, epoch: int, current_iter: int) -> dict:
        """The dict ``torch.save`` writes as ``{current_iter}.state``.  Call it after iteration
        ``current_iter``'s ``optimize_parameters``; it copies the moments (later steps do not change it)."""
        opt = flat_to_optim_state(self._state_keys(), self.exp_avg, self.exp_avg_sq, self.step_count, self._hyper(),
                                  self._shapes())
        scheds = []
        if getattr(self, "scheduler", None) is not None:
            # BaseModel.update_learning_rate steps the scheduler from iteration 2 on (:186-188)
            scheds.append({"last_epoch": max(int(current_iter) - 1, 0)})
            opt["param_groups"][0]["initial_lr"] = self.init_lr   # what a torch scheduler adds to its group
        return {"epoch": epoch, "iter": current_iter, "optimizers": [opt], "schedulers": scheds}

    def resume_training(self, state: dict) -> None:
        """Inverse of ``training_state``; also takes a bare ``optimizer.state_dict()`` of stock AdamW / Adam.
        Restores the moments, the step count, lr and the hyperparameters; with a scheduler set, lr is then
        re-derived through ``update_learning_rate``.  Load the network weights first (``load_state_dict``)."""
        if "optimizers" in state:
            if len(state["optimizers"]) != 1:
                raise ValueError(f"expected one optimizer in the training state, got {len(state['optimizers'])}")
            opt = state["optimizers"][0]
        elif "param_groups" in state:
            opt = state
        else:
            raise ValueError("not a training state: neither 'optimizers' nor 'param_groups'")
        keys = self._state_keys()
        if len(opt["param_groups"]) == 1 and len(opt["param_groups"][0]["params"]) != len(keys):
            raise ValueError(f"optimizer state has {len(opt['param_groups'][0]['params'])} parameters, the trainer "
                             f"has {len(keys)} trainable parameters (of {len(self.engine.keys)}): resume under the "
                             "trainable mask the state was saved with")
        self.step_count = optim_state_to_flat(opt, keys, self.exp_avg, self.exp_avg_sq, self._shapes())
        g = opt["param_groups"][0]
        self.lr, self.betas = float(g["lr"]), tuple(float(b) for b in g["betas"])
        self.eps, self.weight_decay = float(g["eps"]), float(g["weight_decay"])
        if hasattr(self, "init_lr"):
            self.init_lr = float(g.get("initial_lr", self.init_lr))
        scheds = state.get("schedulers", [])
        if getattr(self, "scheduler", None) is not None and scheds:
            self.update_learning_rate(int(scheds[0]["last_epoch"]) + 1)


def _inference_flat(trainer, vec):
    """``vec`` (theta or theta_ema, the training handle's aligned layout) as the flat vector the module's
    inference handle packs from: every key back to back in state_dict order."""
    dev = vec.device
    infer_keys = [k for k, _ in trainer.model.engine(dev).keys]
    if infer_keys != [k for k, _, _ in trainer.engine.keys]:
        raise RuntimeError("the inference handle's state_dict layout differs from the training handle's")
    return trainer.engine.packed(vec)


def _reflect_pad(t, multiple):
    """pad_test (image_restoration_model.py:226-234): reflect-pad right and bottom to a multiple."""
    h, w = t.shape[-2:]
    ph = (multiple - h % multiple) % multiple if multiple else 0
    pw = (multiple - w % multiple) % multiple if multiple else 0
    if ph or pw:
        t = torch.nn.functional.pad(t, (0, pw, 0, ph), "reflect")
    return t


def _val_metrics(metrics):
    """``validate(metrics=...)``: the names of the reference's val.metrics block this build has
    (calculate_psnr, calculate_ssim), checked -> (want PSNR, want SSIM)."""
    names = (metrics,) if isinstance(metrics, str) else tuple(metrics)
    for m in names:
        if m not in ("psnr", "ssim"):
            raise ValueError(f"validate: unknown metric {m!r} (expected 'psnr' and / or 'ssim')")
    if not names:
        raise ValueError("validate: no metrics")
    return "psnr" in names, "ssim" in names


class _FlatEngine:
    """A ``{prefix}_*`` training handle for one model config on one device: the flat parameter layout
    (``keys``: ``(name, numel, offset)`` in ``named_parameters()`` order, every key 16-byte aligned; ``numel``:
    floats of the flat buffer) and the workspace ``ws``, grown on demand."""

    def __init__(self, prefix, model, device: torch.device, what, create="create"):
        L = _lib.lib()
        self._L, self._prefix, self.device = L, prefix, device
        h = ctypes.c_void_p()
        idx = device.index if device.index is not None else torch.cuda.current_device()
        _lib.check(self._fn(create)(ctypes.byref(model._c_config()), idx, ctypes.byref(h)), f"{prefix}_{create}")
        self.handle = h
        self._dtor = self._fn("destroy")
        self.keys = []
        for i in range(self._fn("num_params")(h)):
            name, numel, off = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
            _lib.check(self._fn("param_info")(h, i, ctypes.byref(name), ctypes.byref(numel), ctypes.byref(off)),
                       prefix + "_param_info")
            self.keys.append((name.value.decode(), int(numel.value), int(off.value)))
        self.numel = int(self._fn("num_floats")(h))
        if [k for k, _, _ in self.keys] != [k for k, _ in model.named_parameters()]:
            raise RuntimeError(f"{what} parameters do not match the training handle's state_dict layout")
        self.ws = None
        self.generation = 0

    def _fn(self, name):
        return getattr(self._L, f"{self._prefix}_{name}")

    def __del__(self):
        try:
            if self.handle:
                self._dtor(self.handle)
        except Exception:
            pass

    def used_ranges(self):
        """[begin, end) float ranges of the flat buffer that receive gradients: all of it."""
        return [[0, self.numel]]

    def flatten(self, tensors) -> torch.Tensor:
        """Parameters -> the handle's flat layout (state_dict order, each key 16-byte aligned, pads zero)."""
        tensors = list(tensors)
        flat = torch.zeros(self.numel, dtype=torch.float32, device=tensors[0].device)
        for (k, n, off), t in zip(self.keys, tensors):
            flat[off:off + n] = t.detach().reshape(-1).to(torch.float32)
        return flat

    def packed(self, flat) -> torch.Tensor:
        """The flat layout without its pad floats: torch.cat of the keys in state_dict order."""
        return torch.cat([flat[off:off + n] for _, n, off in self.keys])

    def _workspace(self, *shape):
        nbytes = int(self._fn("workspace_bytes")(self.handle, *shape))
        if nbytes < 0:
            _lib.check(1, self._prefix + "_workspace_bytes")
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(nbytes, dtype=torch.uint8, device=self.device)
        return self.ws


class TrainEngine(_FlatEngine):
    """``kdlae_tt_*`` handle for one KDLAE_teacher config on one device."""

    def __init__(self, model, device: torch.device, what="KDLAE_teacher", create="create"):
        super().__init__("kdlae_tt", model, device, what, create)
        cfg = model._cfg
        self.static_train = cfg["static"] == "train"
        self.params_cat = cfg["params"] == "cat"
        self.out_channels = cfg["out_channels"]
        # parameters the reference forward never touches (KDLAE_model.py:315-319 when params != 'cat'):
        # autograd leaves their .grad None and torch.optim skips them
        unused = ("output_param.", "refinement_out.") if not self.params_cat else ()
        self.used = [not k.startswith(unused) for k, _, _ in self.keys]
        # kdlae_tt_set_trainable's mask, one bool per key (all True: no mask set on the handle)
        self.trainable = [True] * len(self.keys)

    def set_trainable(self, mask=None):
        """Freeze parameters (``kdlae_tt_set_trainable``): ``mask`` holds one truth value per key in
        ``named_parameters()`` order, True = trainable; ``None`` = all.  The backward then computes a layer's
        weight gradient only for a trainable key and stops at the first layer that holds one; the forward keeps
        no activations before it.  Frozen keys get exactly zero in ``grad``.  Not between a forward and its
        backward; holds until changed."""
        if mask is None:
            rc = self._L.kdlae_tt_set_trainable(self.handle, None, 0)
            new = [True] * len(self.keys)
        else:
            new = [bool(v) for v in mask]
            buf = (ctypes.c_ubyte * len(new))(*[int(v) for v in new])
            rc = self._L.kdlae_tt_set_trainable(self.handle, buf, len(new))
        _lib.check(rc, "kdlae_tt_set_trainable")
        self.trainable = new

    def backward_launches(self) -> int:
        """Launches the last backward issued (``kdlae_tt_debug_backward_launches``)."""
        return int(self._L.kdlae_tt_debug_backward_launches(self.handle))

    def used_ranges(self):
        """[begin, end) float ranges of the flat buffer that receive gradients (merged): the keys the forward
        uses that are trainable."""
        out = []
        for (k, n, off), u, t in zip(self.keys, self.used, self.trainable):
            if not (u and t):
                continue
            end = off + ((n + 3) & ~3)  # keys are 16-byte aligned; the zero pad floats ride along
            if out and out[-1][1] == off:
                out[-1][1] = end
            else:
                out.append([off, end])
        return out

    def forward(self, theta, img, rate):
        """KDLAE_teacher.forward (KDLAE_model.py:270-336) with activations kept for ``backward``."""
        if img.device.type != "cuda":
            raise RuntimeError("KDLAE training runs on ROCm devices only; there is no CPU fallback")
        img = img.detach().to(torch.float32).contiguous()
        B, _, H, W = img.shape
        if H % 8 or W % 8:
            raise RuntimeError(f"KDLAE_teacher needs H and W divisible by 8, got {H}x{W}")
        rate = rate.detach().to(device=img.device, dtype=torch.float32).contiguous() if self.params_cat else None
        oc = self.out_channels
        hq = torch.empty((B, oc, H, W), device=img.device, dtype=torch.float32)
        sr = torch.empty((B, oc, 2 * H, 2 * W), device=img.device, dtype=torch.float32) if self.static_train else None
        ws = self._workspace(B, H, W)
        rc = self._L.kdlae_tt_forward(self.handle, _vp(theta), _vp(img), _vp(rate), B, H, W, _vp(hq), _vp(sr),
                                      _vp(ws), ws.numel(), _stream(img.device))
        _lib.check(rc, "kdlae_tt_forward")
        self.generation += 1
        return hq, sr

    def backward(self, theta, dhq, dsr, grad, marked=False):
        """d loss / d theta into ``grad`` (flat, overwritten) from the output gradients.

        ``marked``: also record the gradient-ready events of ``kdlae_tt_backward_marked``; returns
        their suffix offsets (decreasing: the backward runs deepest-first, i.e. from the buffer's end)."""
        dhq = dhq.detach().to(torch.float32).contiguous() if dhq is not None else None
        dsr = dsr.detach().to(torch.float32).contiguous() if (dsr is not None and self.static_train) else None
        fn = self._L.kdlae_tt_backward_marked if marked else self._L.kdlae_tt_backward
        rc = fn(self.handle, _vp(theta), _vp(dhq), _vp(dsr), _vp(grad), _vp(self.ws), self.ws.numel(),
                _stream(grad.device))
        _lib.check(rc, "kdlae_tt_backward_marked" if marked else "kdlae_tt_backward")
        if not marked:
            return grad
        return [int(self._L.kdlae_tt_mark_lo(self.handle, j)) for j in range(self._L.kdlae_tt_mark_count(self.handle))]


class RestormerTrainEngine(TrainEngine):
    """``kdlae_tt_*`` handle made by ``kdlae_tt_create_restormer`` for one ``KDLAE_model.Restormer`` on one device:
    Restormer's own key list, the teacher's no-cat / no-sr launches; ``forward(theta, x, None) -> (out, None)``."""

    def __init__(self, model, device: torch.device):
        super().__init__(model, device, "Restormer", "create_restormer")


class TeacherTrainFn(torch.autograd.Function):
    """Autograd node for one KDLAE_teacher (or Restormer: ``rate`` None, one output) forward on the training
    engine."""

    @staticmethod
    def forward(ctx, engine, img, rate, *params):
        # frozen parameters (requires_grad False, e.g. after freeze_except_patch_embed_and_enhance): the
        # engine skips their gradients and every layer before the first trainable one
        mask = [bool(g) for g in ctx.needs_input_grad[3:]]
        if mask != engine.trainable:
            engine.set_trainable(None if all(mask) else mask)
        theta = engine.flatten(params)
        hq, sr = engine.forward(theta, img, rate)
        # an output the loss ignores arrives as None (not zeros), so the branch that produced only it
        # gets None gradients and torch.optim skips those parameters, as with the reference module
        ctx.set_materialize_grads(False)
        ctx.engine = engine
        ctx.generation = engine.generation
        ctx.theta = theta
        ctx.shapes = [p.shape for p in params]
        ctx.mask = mask
        if sr is None:
            return hq
        return hq, sr

    @staticmethod
    def backward(ctx, dhq, dsr=None):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("KDLAE_teacher: a second training forward ran before this graph's backward; "
                               "the HIP engine keeps one set of saved activations per model and device")
        if dhq is None and dsr is None:
            return (None, None, None, *[None] * len(ctx.shapes))
        grad = torch.empty(eng.numel, dtype=torch.float32, device=ctx.theta.device)
        eng.backward(ctx.theta, dhq, dsr, grad)  # a None output gradient is read as zero
        # sr = enhance(cen(hq)) (KDLAE_model.py:324-329): with no sr gradient that branch is untouched
        skip = ("cen.", "upen.", "enhance.", "outputen.") if dsr is None else None
        grads = []
        for (k, n, off), shape, used, train in zip(eng.keys, ctx.shapes, eng.used, ctx.mask):
            live = used and train and not (skip and k.startswith(skip))
            grads.append(grad[off:off + n].view(shape) if live else None)
        return (None, None, None, *grads)


def freeze_except_patch_embed_and_enhance(model):
    """The reference's fine-tuning freeze (Train/basicsr/train.py:24-55, used by 01_sures_param_fintune.yml,
    03_param_fintue.yml, 05_sures_fintue.yml): every parameter's ``requires_grad`` becomes False except those of
    ``patch_embed`` and, when ``model.static == "train"``, of the sr head ``cen``, ``upen``, ``enhance``,
    ``outputen``.  Returns the model.  The training forward reads ``requires_grad``, so the drop-in and a
    ``KDLAETrainer`` built afterwards get the cheaper backward."""
    for p in model.parameters():
        p.requires_grad = False
    mods = [model.patch_embed]
    if model.static == "train":
        mods += [model.cen, model.upen, model.enhance, model.outputen]
    for m in mods:
        for p in m.parameters():
            p.requires_grad = True
    return model


class _L1LossSrFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, hq, gt_hq, sr, gt_sr, loss_weight):
        L = _lib.lib()
        dev = hq.device
        hq = hq.detach().contiguous()
        gt_hq = gt_hq.detach().to(torch.float32).contiguous()
        dhq = torch.empty_like(hq)
        dsr = None
        if sr is not None:
            sr = sr.detach().contiguous()
            gt_sr = gt_sr.detach().to(torch.float32).contiguous()
            dsr = torch.empty_like(sr)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty(int(L.kdlae_train_l1sr_scratch_floats()), dtype=torch.float32, device=dev)
        rc = L.kdlae_train_l1sr(_vp(hq), _vp(gt_hq), hq.numel(), _vp(sr), _vp(gt_sr),
                                sr.numel() if sr is not None else 0, _vp(dhq), _vp(dsr), _vp(loss), _vp(scratch),
                                _stream(dev))
        _lib.check(rc, "kdlae_train_l1sr")
        ctx.save_for_backward(dhq, dsr if dsr is not None else torch.empty(0, device=dev))
        ctx.has_sr = sr is not None
        ctx.w = loss_weight
        return loss * loss_weight

    @staticmethod
    def backward(ctx, g):
        dhq, dsr = ctx.saved_tensors
        s = g * ctx.w
        return dhq * s, None, (dsr * s if ctx.has_sr else None), None, None


class L1LossSr(torch.nn.Module):
    """L1LossSr (Train/basicsr/models/losses/losses.py:135-194) on the HIP path, autograd-aware.

    loss = loss_weight * (0.5 l1(hq) + 0.25 l1(sr) + 0.25 (shadow(hq) + shadow(sr))), reduction 'mean'.
    """

    def __init__(self, loss_weight=1.0, reduction="mean"):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['none', 'mean', 'sum']")
        if reduction != "mean":
            raise NotImplementedError("the HIP L1LossSr implements reduction='mean' (the KDLAET.yml setting)")
        self.loss_weight = loss_weight
        self.reduction = reduction

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("element-wise loss weights are not used by the reference configs")
        if pred["hq"].device.type != "cuda":
            raise RuntimeError("L1LossSr (MI355X build) runs on ROCm devices only")
        return _L1LossSrFn.apply(pred["hq"], target["hq"], pred.get("sr"), target.get("sr") if pred.get("sr")
                                 is not None else None, float(self.loss_weight))


_REDUCTIONS = {"mean": 0, "sum": 1}


def _l1sonar(pred, target, loss_weight, binary, reduction, dpred, loss, scratch):
    """``kdlae_train_l1sonar`` over contiguous fp32 tensors; ``dpred`` None = loss only."""
    rc = _lib.lib().kdlae_train_l1sonar(_vp(pred), _vp(target), pred.numel(), float(loss_weight), float(binary),
                                        _REDUCTIONS[reduction], None, _vp(dpred), _vp(loss), _vp(scratch),
                                        _stream(pred.device))
    _lib.check(rc, "kdlae_train_l1sonar")


class _L1LossSonarFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, loss_weight, binary, reduction):
        dev = pred.device
        p = pred.detach().to(torch.float32).contiguous()
        t = target.detach().to(device=dev, dtype=torch.float32).contiguous()
        dp = torch.empty_like(p) if ctx.needs_input_grad[0] else None
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty(int(_lib.lib().kdlae_train_l1sonar_scratch_floats()), dtype=torch.float32, device=dev)
        _l1sonar(p, t, loss_weight, binary, reduction, dp, loss, scratch)
        ctx.dp = dp
        return loss

    @staticmethod
    def backward(ctx, g):
        # g == 1 (l_pix.backward()) leaves the kernel's bits: x * 1.0f is exact
        return (ctx.dp * g if ctx.dp is not None else None), None, None, None, None


class L1LossSonar(torch.nn.Module):
    """L1LossSonar (Train/basicsr/models/losses/losses.py:25-65, Restomer.yml's pixel_opt) on the HIP path,
    autograd-aware: loss_weight * (red|p - t| + red|[p > binary] - [t > binary]|), red = 'mean' or 'sum'; the
    binarised term carries no gradient (``kdlae_train_l1sonar``)."""

    def __init__(self, loss_weight=1.0, reduction='mean', binary=0.1):
        super().__init__()
        if reduction not in ("none", "mean", "sum"):
            raise ValueError(f"Unsupported reduction mode: {reduction}. Supported ones are: ['none', 'mean', 'sum']")
        if reduction == "none":
            raise NotImplementedError("the HIP L1LossSonar implements reduction='mean' and 'sum'")
        self.loss_weight = loss_weight
        self.reduction = reduction
        self.binary = binary

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("element-wise loss weights are not used by the reference configs")
        if pred.device.type != "cuda":
            raise RuntimeError("L1LossSonar (MI355X build) runs on ROCm devices only")
        if pred.shape != target.shape:
            raise RuntimeError(f"L1LossSonar: pred {tuple(pred.shape)} and target {tuple(target.shape)} differ")
        return _L1LossSonarFn.apply(pred, target, float(self.loss_weight), float(self.binary), self.reduction)


# ------------------------------------------------------------------ KDLAE-S (KDLAES.yml)
class StudentTrainEngine(_FlatEngine):
    """``kdlae_st_*`` handle for one KDLAE_student config on one device (KDLAE_model.py:340-431)."""

    def __init__(self, model, device: torch.device):
        super().__init__("kdlae_st", model, device, "KDLAE_student")

    def forward(self, theta, x):
        """KDLAE_student.forward with activations kept for ``backward``: x [B, F, H, W] -> [B, F, H, W]."""
        if x.device.type != "cuda":
            raise RuntimeError("KDLAE training runs on ROCm devices only; there is no CPU fallback")
        x = x.detach().to(torch.float32).contiguous()
        B, F, H, W = x.shape
        self._workspace(B, F, H, W)
        out = torch.empty_like(x)
        self._x = x  # the residual input must outlive the backward
        rc = self._L.kdlae_st_forward(self.handle, _vp(theta), _vp(x), B, F, H, W, _vp(out), _vp(self.ws),
                                      self.ws.numel(), _stream(x.device))
        _lib.check(rc, "kdlae_st_forward")
        self.generation += 1
        return out

    def backward(self, theta, dout, grad):
        dout = dout.detach().to(torch.float32).contiguous()
        rc = self._L.kdlae_st_backward(self.handle, _vp(theta), _vp(dout), _vp(grad), _vp(self.ws), self.ws.numel(),
                                       _stream(grad.device))
        _lib.check(rc, "kdlae_st_backward")
        return grad


class StudentTrainFn(torch.autograd.Function):
    """Autograd node for one KDLAE_student forward on the training engine (the input gets no gradient)."""

    @staticmethod
    def forward(ctx, engine, x, *params):
        theta = engine.flatten(params)
        out = engine.forward(theta, x)
        ctx.engine = engine
        ctx.generation = engine.generation
        ctx.theta = theta
        ctx.shapes = [p.shape for p in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("KDLAE_student: a second training forward ran before this graph's backward; "
                               "the HIP engine keeps one set of saved activations per model and device")
        grad = torch.empty(eng.numel, dtype=torch.float32, device=ctx.theta.device)
        eng.backward(ctx.theta, dout, grad)
        return (None, None, *[grad[off:off + n].view(shape) for (k, n, off), shape in zip(eng.keys, ctx.shapes)])


class _L1FramesFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target, l1w, tw, binary, red):
        L = _lib.lib()
        dev = pred.device
        p = pred.detach().to(torch.float32).contiguous()
        t = target.detach().to(device=dev, dtype=torch.float32).contiguous()
        N, Cf = p.shape[0], p.shape[1]
        hw = p.numel() // max(1, N * Cf)
        dp = torch.empty_like(p)
        loss = torch.empty((), dtype=torch.float32, device=dev)
        scratch = torch.empty(int(L.kdlae_train_l1frames_scratch_floats()), dtype=torch.float32, device=dev)
        rc = L.kdlae_train_l1frames(_vp(p), _vp(t), N, Cf, hw, float(l1w), float(tw), float(binary), red, _vp(dp),
                                    _vp(loss), _vp(scratch), _stream(dev))
        _lib.check(rc, "kdlae_train_l1frames")
        ctx.save_for_backward(dp)
        return loss

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None, None, None, None, None


class L1LossForVideoFrames(torch.nn.Module):
    """L1LossForVideoFrames (Train/basicsr/models/losses/losses.py:409-526) on the HIP path, autograd-aware:
    l1loss_weight * reduce(|p - t| + |bin(p) - bin(t)|) + temporal_weight * reduce(|dp - dt|) over the
    frame axis (dim 1) of [N, frames, H, W] tensors.  The reference's 'max' / 'mix' reductions (and
    element weights) are not used by its configs and raise NotImplementedError here."""

    def __init__(self, l1loss_weight=0.64, reduction="mean", sigma=2.0, weight=[1.5, 1.0], invert=False,
                 temporal_weight=0.36, binary=0.1):
        super().__init__()
        if reduction not in ["none", "mean", "sum", "max", "mix"]:
            raise ValueError(f"Unsupported reduction mode: {reduction}. "
                             f'Supported ones are: ["none", "mean", "sum", "max", "mix"]')
        self.l1loss_weight = l1loss_weight
        self.reduction = reduction
        self.temporal_weight = temporal_weight
        self.binary = binary

    def forward(self, pred, target, weight=None, **kwargs):
        if weight is not None:
            raise NotImplementedError("element-wise loss weights are not used by the reference configs")
        if self.reduction not in ("mean", "sum"):
            raise NotImplementedError(f"L1LossForVideoFrames reduction {self.reduction!r} on the HIP path "
                                      "(KDLAES.yml uses 'mean')")
        if pred.device.type != "cuda":
            raise RuntimeError("L1LossForVideoFrames (MI355X build) runs on ROCm devices only")
        return _L1FramesFn.apply(pred, target, self.l1loss_weight, self.temporal_weight, self.binary,
                                 0 if self.reduction == "mean" else 1)


class KDLAESTrainer(_TrainingState):
    """ImageCleanModel.optimize_parameters for KDLAE_student with KDLAES.yml (AdamW lr 3e-4 wd 1e-4 betas
    (0.9, 0.999); use_grad_clip -> clip_grad_norm_(0.01); L1LossForVideoFrames(0.9, mean, temporal 0.1);
    mixup): flat buffers end to end, one RCCL all-reduce of the flat gradient for DDP."""

    def __init__(self, model, lr=3e-4, weight_decay=1e-4, betas=(0.9, 0.999), eps=1e-8, use_grad_clip=True,
                 max_norm=0.01, loss_kw=None, group=None, mixing_augs=None):
        params = list(model.parameters())
        if not params or params[0].device.type != "cuda":
            raise RuntimeError("KDLAESTrainer: move the model to a ROCm device first (no CPU fallback)")
        dev = params[0].device
        self.model = model
        self.engine = StudentTrainEngine(model, dev)
        eng = self.engine
        self.theta = eng.flatten(params).contiguous()
        with torch.no_grad():
            for (k, n, off), p in zip(eng.keys, params):
                p.data = self.theta[off:off + n].view(p.shape)
        self.grad = torch.zeros(eng.numel, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.lr, self.weight_decay, self.betas, self.eps = lr, weight_decay, tuple(betas), eps
        self.max_norm = max_norm if use_grad_clip else 0.0
        kw = dict(l1loss_weight=0.9, temporal_weight=0.1, reduction="mean")
        kw.update(loss_kw or {})
        self.loss_fn = L1LossForVideoFrames(**kw)
        self.group = group
        self.step_count = 0
        self.loss = None
        L = _lib.lib()
        self._opt_scratch = torch.empty(int(L.kdlae_train_adamw_scratch_floats()), dtype=torch.float32, device=dev)
        self._l1_scratch = torch.empty(int(L.kdlae_train_l1frames_scratch_floats()), dtype=torch.float32,
                                       device=dev)
        self._loss = torch.zeros((), dtype=torch.float32, device=dev)
        m = mixing_augs or {}
        self.mixing = (MixingAugment(m.get("mixup_beta", 1.2), m.get("use_identity", False), dev)
                       if m.get("mixup", False) else None)

    def feed_train_data(self, lq, gt):
        if self.mixing is not None:
            gt, lq = self.mixing(gt, lq)
        return lq, gt

    def forward_backward(self, lq, gt):
        eng, L = self.engine, _lib.lib()
        out = eng.forward(self.theta, lq)
        self.output = out
        dout = torch.empty_like(out)
        # the same device move as _L1FramesFn: the loss kernel dereferences gt on the GPU
        gt = gt.to(device=out.device, dtype=torch.float32).contiguous()
        if gt.shape != out.shape:
            raise ValueError(f"gt shape {tuple(gt.shape)} != output shape {tuple(out.shape)}")
        N, Cf = out.shape[0], out.shape[1]
        lf = self.loss_fn
        if lf.reduction not in ("mean", "sum"):
            raise NotImplementedError(f"reduction {lf.reduction!r}")
        rc = L.kdlae_train_l1frames(_vp(out), _vp(gt), N, Cf, out.numel() // (N * Cf), float(lf.l1loss_weight),
                                    float(lf.temporal_weight), float(lf.binary), 0 if lf.reduction == "mean" else 1,
                                    _vp(dout), _vp(self._loss), _vp(self._l1_scratch), _stream(out.device))
        _lib.check(rc, "kdlae_train_l1frames")
        eng.backward(self.theta, dout, self.grad)
        self.loss = self._loss
        return self.loss

    def step(self, gscale: float = 1.0):
        self.step_count += 1
        b1, b2 = self.betas
        rc = _lib.lib().kdlae_train_clip_adamw(
            _vp(self.theta), _vp(self.grad), _vp(self.exp_avg), _vp(self.exp_avg_sq), self.engine.numel,
            float(gscale), float(self.max_norm), float(self.lr), float(b1), float(b2), float(self.eps),
            float(self.weight_decay), self.step_count, None, 0, _vp(self._opt_scratch), _stream(self.theta.device))
        _lib.check(rc, "kdlae_train_clip_adamw")

    def optimize_parameters(self, lq, gt):
        loss = self.forward_backward(lq, gt)
        self.step(sync_gradients(self.grad, self.group))
        return loss

    def grad_norm(self) -> torch.Tensor:
        return self._opt_scratch[2048]

    @torch.no_grad()
    def validate(self, batches, window_size=8, crop_border=0, use_image=False, metrics=("psnr",), niqe=False,
                 niqe_params=None):
        """ImageCleanModel.nondist_validation (image_restoration_model.py:264-348) for ``(lq, gt)`` pairs of
        [B, F, H, W] tensors: reflect-pad to the multiple the student needs (2^levels, and ``window_size``),
        the inference engine, PSNR of the top-left H x W window against ``gt``.  Returns ``{'psnr': mean}``
        over all images; with ``"ssim"`` in ``metrics`` also ``{'ssim': mean}`` (``calculate_ssim`` over the
        same window, 1 <= F <= 4 frames).  ``niqe=True`` adds ``{'niqe': mean}``: ``calculate_niqe`` of the
        output's window (F = 1 or 3; at least 96 x 96 pixels after ``crop_border``), always on ``tensor2img``'s
        uint8 image, which is what the reference's function takes; ``niqe_params`` is the reference's pristine
        model (``metrics.load_niqe_params``).  The trainer's state is untouched."""
        from .metrics import load_niqe_params, niqe_batch, psnr_batch, ssim_batch
        want_psnr, want_ssim = _val_metrics(metrics)
        niqe_p, niqes = (load_niqe_params(niqe_params) if niqe else None), []
        need = 1 << self.model.num_levels
        mult = math.lcm(need, int(window_size)) if window_size else need
        flat = _inference_flat(self, self.theta)
        vals, ssims, seen = [], [], False
        for lq, gt in batches:
            if lq.device.type != "cuda":
                raise RuntimeError("KDLAE validation runs on ROCm devices only; there is no CPU fallback")
            h, w = lq.shape[-2:]
            out = self.model._forward_eager(_reflect_pad(lq.to(torch.float32), mult), flat=flat)
            self.val_output = out[..., :h, :w]  # the last item's cropped output (pad_test's self.output)
            seen = True
            if want_psnr:
                vals.append(psnr_batch(out, gt.to(out.device), (h, w), crop_border, use_image))
            if want_ssim:
                ssims.append(ssim_batch(out, gt.to(out.device), (h, w), crop_border, use_image))
            if niqe:
                niqes.append(niqe_batch(out, (h, w), crop_border, True, "y", niqe_p))
        if not seen:
            raise ValueError("validate: no batches")
        res = {}
        if want_psnr:
            res["psnr"] = float(torch.cat(vals).mean())
        if want_ssim:
            res["ssim"] = float(torch.cat(ssims).mean())
        if niqe:
            res["niqe"] = float(torch.cat(niqes).mean())
        return res


class DistillTrainer(KDLAESTrainer):
    """``KDLAESTrainer`` whose targets are computed by a teacher on the device inside the step
    (``distill.teacher_labels``) instead of being read from the folder of saved teacher outputs that KDLAES.yml's
    ``dataroot_gt`` names.  ``teacher``: a ``KDLAE_teacher`` or ``Restormer`` in eval mode on the student's device;
    its parameters are read, never written, and it is not part of the training state (``validate``,
    ``training_state`` and ``resume_training`` are the parent's).  ``denoise_rate``, ``label_mode`` (``"mean"``:
    no quantisation; ``"file"``: the saved-image round trip) and ``teacher_batch`` are ``teacher_labels``'
    arguments; everything else is ``KDLAESTrainer``'s."""

    def __init__(self, student, teacher, denoise_rate, label_mode="mean", teacher_batch=16, **kwargs):
        from . import distill
        if label_mode not in distill.MODES:
            raise RuntimeError(f"label_mode must be one of {sorted(distill.MODES)}, got {label_mode!r}")
        if teacher.training:
            raise RuntimeError("DistillTrainer: the teacher must be in eval mode (call .eval() first)")
        super().__init__(student, **kwargs)
        self.teacher, self.denoise_rate = teacher, denoise_rate
        self.label_mode, self.teacher_batch = label_mode, int(teacher_batch)
        self.labels = None

    def make_labels(self, frames):
        """The teacher's targets for ``frames`` (u8 [B,F,h,w(,C)] or f32 [B,F,H,W]) in a buffer kept across steps."""
        from . import distill
        shape = tuple(frames.shape[:4])
        if self.labels is None or tuple(self.labels.shape) != shape or self.labels.device != frames.device:
            self.labels = torch.empty(shape, dtype=torch.float32, device=frames.device)
        return distill.teacher_labels(self.teacher, frames, self.denoise_rate, self.label_mode, self.teacher_batch,
                                      out=self.labels)

    def optimize_parameters(self, lq, clean=None):
        """One step against the teacher's labels of ``clean`` (default: of ``lq`` itself; ``clean`` lets ``lq`` be
        degraded by ``augment.train_inputs`` / ``mask_frames`` while the teacher sees the undegraded frames).
        Mixup, if configured, is applied after the labels are made; then the parent's forward_backward and step."""
        gt = self.make_labels(clean if clean is not None else lq)
        lq, gt = self.feed_train_data(lq, gt)
        return super().optimize_parameters(lq, gt)


# ------------------------------------------------------------------ ASDQE (Train/ASDQE.py)
def _bn_modules(model):
    return [m for m in model.modules() if isinstance(m, torch.nn.BatchNorm2d)]


def asdqe_dropout_masks(B, device, generator=None):
    """The regressor's two Dropout masks (p = 0.5 / 0.3, ASDQE_model.py:148,151), already scaled: 0 or
    1 / (1 - p), [B, 256] and [B, 64].  Drawn on the device with ``torch.rand(generator=...)``: NOT the
    bits ``nn.Dropout`` would draw from torch's global stream."""
    m1 = (torch.rand(B, 256, device=device, generator=generator) >= 0.5).to(torch.float32) * 2.0
    m2 = (torch.rand(B, 64, device=device, generator=generator) >= 0.3).to(torch.float32) * (1.0 / 0.7)
    return m1, m2


class AsdqeTrainEngine(_FlatEngine):
    """``asdqe_train_*`` handle for one DenoiseRatePredictor config on one device (ASDQE_model.py:123-171
    in train mode: batch-statistics BatchNorm with the running update, Dropout by explicit masks)."""

    def __init__(self, model, device: torch.device):
        super().__init__("asdqe_train", model, device, "DenoiseRatePredictor")
        self.num_stats = int(self._L.asdqe_train_num_stat_floats(self.handle))
        self.in_channels = int(model._cfg["in_channels"])
        # per BatchNorm2d, in state_dict order: [running_mean | running_var] at this offset
        self.stat_slots, off = [], 0
        for bn in _bn_modules(model):
            self.stat_slots.append((off, bn.num_features))
            off += 2 * bn.num_features
        if off != self.num_stats:
            raise RuntimeError("DenoiseRatePredictor BatchNorm buffers do not match the training handle's layout")

    def flatten_stats(self, model) -> torch.Tensor:
        bns = _bn_modules(model)
        flat = torch.empty(self.num_stats, dtype=torch.float32, device=self.device)
        for (off, c), bn in zip(self.stat_slots, bns):
            flat[off:off + c] = bn.running_mean.detach().to(torch.float32)
            flat[off + c:off + 2 * c] = bn.running_var.detach().to(torch.float32)
        return flat

    def forward(self, theta, stats, lq, gt, mask1=None, mask2=None):
        """Train-mode forward with activations kept for ``backward``; ``stats`` is updated in place."""
        if lq.device.type != "cuda" or gt.device != lq.device:
            raise RuntimeError("ASDQE training runs on ROCm devices only; there is no CPU fallback")
        ci = self.in_channels  # the kernels index the images with the handle's channel count
        if lq.dim() != 4 or lq.shape[1] != ci or lq.shape != gt.shape:
            raise RuntimeError(f"expected lq, gt [B,{ci},H,W] of equal shape, got {tuple(lq.shape)}, {tuple(gt.shape)}")
        lq = lq.detach().to(torch.float32).contiguous()
        gt = gt.detach().to(torch.float32).contiguous()
        B, _, H, W = lq.shape
        for m, n in ((mask1, 256), (mask2, 64)):
            if m is not None and (tuple(m.shape) != (B, n) or m.device != lq.device):
                raise RuntimeError(f"dropout mask must be a [{B}, {n}] tensor on {lq.device}")
        mask1 = mask1.detach().to(torch.float32).contiguous() if mask1 is not None else None
        mask2 = mask2.detach().to(torch.float32).contiguous() if mask2 is not None else None
        self._workspace(B, H, W)
        score = torch.empty((B, 1), dtype=torch.float32, device=lq.device)
        rc = self._L.asdqe_train_forward(self.handle, _vp(theta), _vp(stats), _vp(lq), _vp(gt), B, H, W, _vp(mask1),
                                         _vp(mask2), _vp(score), _vp(self.ws), self.ws.numel(), _stream(lq.device))
        _lib.check(rc, "asdqe_train_forward")
        self.generation += 1
        return score

    def backward(self, theta, dscore, grad, accumulate=False):
        if self.ws is None:
            raise RuntimeError("ASDQE training: backward without a preceding forward")
        dscore = dscore.detach().to(torch.float32).contiguous()
        rc = self._L.asdqe_train_backward(self.handle, _vp(theta), _vp(dscore), _vp(grad), 1 if accumulate else 0,
                                          _vp(self.ws), self.ws.numel(), _stream(grad.device))
        _lib.check(rc, "asdqe_train_backward")
        return grad


class AsdqeTrainFn(torch.autograd.Function):
    """Autograd node for one train-mode DenoiseRatePredictor forward (the images get no gradient)."""

    @staticmethod
    def forward(ctx, engine, stats, lq, gt, mask1, mask2, *params):
        theta = engine.flatten(params)
        score = engine.forward(theta, stats, lq, gt, mask1, mask2)
        ctx.engine = engine
        ctx.generation = engine.generation
        ctx.theta = theta
        ctx.shapes = [p.shape for p in params]
        return score

    @staticmethod
    def backward(ctx, dscore):
        eng = ctx.engine
        if eng.generation != ctx.generation:
            raise RuntimeError("DenoiseRatePredictor: a second training forward ran before this graph's backward; "
                               "the HIP engine keeps one set of saved activations per model and device")
        grad = torch.empty(eng.numel, dtype=torch.float32, device=ctx.theta.device)
        eng.backward(ctx.theta, dscore, grad)
        return (None, None, None, None, None, None,
                *[grad[off:off + n].view(shape) for (k, n, off), shape in zip(eng.keys, ctx.shapes)])


def _asdqe_engine(model, device):
    engines = model.__dict__.setdefault("_train_engines", {})
    idx = device.index if device.index is not None else torch.cuda.current_device()
    eng = engines.get(idx)
    if eng is None:
        eng = engines[idx] = AsdqeTrainEngine(model, torch.device("cuda", idx))
    return eng


def asdqe_train_forward(model, lq, gt, masks=None, generator=None):
    """``model(lq, gt)`` as ``model.train()`` computes it in the reference (batch-statistics BatchNorm,
    Dropout), on the HIP path, for users who write their own loop: the returned score [B, 1] carries an
    autograd graph into ``model.parameters()``, so ``loss.backward()`` and any torch optimizer work.
    The BatchNorm buffers are updated as ``nn.BatchNorm2d`` updates them (momentum 0.1, unbiased running
    variance, ``num_batches_tracked += 1``).  One forward per backward: the engine keeps one set of saved
    activations per model and device, and a second training forward before the first graph's backward
    raises at that backward.

    ``masks=(mask1 [B, 256], mask2 [B, 64])`` fixes the two Dropout masks (values 0 or 1 / (1 - p);
    ``None`` entries = no dropout); by default they are drawn with ``asdqe_dropout_masks(generator=...)``,
    which are not the bits ``nn.Dropout`` would draw from torch's global stream.  fp32 throughout."""
    if lq.device.type != "cuda":
        raise RuntimeError("ASDQE training runs on ROCm devices only; there is no CPU fallback")
    eng = _asdqe_engine(model, lq.device)
    m1, m2 = masks if masks is not None else asdqe_dropout_masks(lq.shape[0], lq.device, generator)
    stats = eng.flatten_stats(model)
    score = AsdqeTrainFn.apply(eng, stats, lq, gt, m1, m2, *model.parameters())
    with torch.no_grad():
        for (off, c), bn in zip(eng.stat_slots, _bn_modules(model)):
            bn.running_mean.copy_(stats[off:off + c])
            bn.running_var.copy_(stats[off + c:off + 2 * c])
            bn.num_batches_tracked += 1
    return score


class ASDQETrainer(_TrainingState):
    """``train_epoch``'s inner loop (Train/ASDQE.py:95-122) on flat buffers: train-mode forward, MSE /
    ``accumulation_steps``, backward accumulating into ``grad``, and every ``accumulation_steps``-th
    micro-batch one Adam step (``kdlae_train_clip_adamw`` without clipping; with ``weight_decay=0`` that is
    ``torch.optim.Adam``) followed by zeroing the gradient.  The model's parameters and BatchNorm buffers
    become views of the trainer's flat buffers, so ``model.state_dict()`` (what ``torch.save`` writes at
    :210 and ASDQE_test.py:79 loads) and the eval forward always see the trained values.

    fp32 throughout: the reference's ``autocast`` + ``GradScaler`` (fp16 on CUDA) is not needed and this
    path is not narrower arithmetic.  Dropout masks come from ``asdqe_dropout_masks`` with a generator
    seeded by ``seed`` (not the bits ``nn.Dropout`` would draw).  ``lr`` is a plain attribute: drive it
    with any plateau rule."""

    def __init__(self, model, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, accumulation_steps=32,
                 group=None, seed=None):
        params = list(model.parameters())
        if not params or params[0].device.type != "cuda":
            raise RuntimeError("ASDQETrainer: move the model to a ROCm device first (no CPU fallback)")
        if accumulation_steps < 1:
            raise ValueError("accumulation_steps must be >= 1")
        dev = params[0].device
        self.model = model
        self.engine = eng = _asdqe_engine(model, dev)
        self.theta = eng.flatten(params).contiguous()
        self.stats = eng.flatten_stats(model)
        with torch.no_grad():
            for (k, n, off), p in zip(eng.keys, params):
                p.data = self.theta[off:off + n].view(p.shape)
            for (off, c), bn in zip(eng.stat_slots, _bn_modules(model)):
                bn.running_mean.data = self.stats[off:off + c]
                bn.running_var.data = self.stats[off + c:off + 2 * c]
        self.grad = torch.zeros(eng.numel, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.lr, self.betas, self.eps, self.weight_decay = lr, tuple(betas), eps, weight_decay
        self.accumulation_steps = int(accumulation_steps)
        self.group = group
        self.step_count = 0
        self.micro = 0  # micro-batches accumulated since the last step
        self.generator = torch.Generator(device=dev)
        if seed is not None:
            self.generator.manual_seed(int(seed))
        L = _lib.lib()
        self._opt_scratch = torch.empty(int(L.kdlae_train_adamw_scratch_floats()), dtype=torch.float32, device=dev)
        self._loss = torch.zeros(2, dtype=torch.float32, device=dev)

    def _target(self, target, B, dev):
        t = target.detach().to(device=dev, dtype=torch.float32).reshape(-1).contiguous()
        if t.numel() != B:
            raise ValueError(f"target has {t.numel()} scores for a batch of {B}")
        return t

    def train_batch(self, lq, gt, target, masks=None):
        """One micro-batch: returns ``(loss * accumulation_steps, mae)`` as the reference logs them, i.e.
        the unscaled MSE and the mean absolute error, as 0-d device tensors."""
        eng, L = self.engine, _lib.lib()
        if lq.device.type != "cuda" or gt.device != lq.device:
            raise RuntimeError("ASDQE training runs on ROCm devices only; there is no CPU fallback")
        self.model.train()
        m1, m2 = masks if masks is not None else asdqe_dropout_masks(lq.shape[0], lq.device, self.generator)
        score = eng.forward(self.theta, self.stats, lq, gt, m1, m2)
        with torch.no_grad():
            for bn in _bn_modules(self.model):
                bn.num_batches_tracked += 1
        B = score.shape[0]
        t = self._target(target, B, score.device)
        dscore = torch.empty_like(score)
        loss = torch.empty(2, dtype=torch.float32, device=score.device)
        rc = L.kdlae_train_mse(_vp(score), _vp(t), B, 1.0 / self.accumulation_steps, _vp(dscore), _vp(loss),
                               _stream(score.device))
        _lib.check(rc, "kdlae_train_mse")
        eng.backward(self.theta, dscore, self.grad, accumulate=True)
        self.score = score
        self.micro += 1
        if self.micro == self.accumulation_steps:
            self.step()
        return loss[0], loss[1]

    def step(self):
        """Adam on the accumulated gradient (all-reduced over ``group`` first), then ``grad = 0``."""
        gscale = sync_gradients(self.grad, self.group)
        self.step_count += 1
        b1, b2 = self.betas
        rc = _lib.lib().kdlae_train_clip_adamw(
            _vp(self.theta), _vp(self.grad), _vp(self.exp_avg), _vp(self.exp_avg_sq), self.engine.numel,
            float(gscale), 0.0, float(self.lr), float(b1), float(b2), float(self.eps), float(self.weight_decay),
            self.step_count, None, 0, _vp(self._opt_scratch), _stream(self.theta.device))
        _lib.check(rc, "kdlae_train_clip_adamw")
        self.grad.zero_()
        self.micro = 0

    def flush(self):
        """Step on a partial accumulation window (the reference's ``len(loader) % accumulation_steps``
        tail, Train/ASDQE.py:114-118); a no-op when nothing is accumulated."""
        if self.micro:
            self.step()

    @torch.no_grad()
    def validate_batch(self, lq, gt, target):
        """The validation pass (Train/ASDQE.py:124-146): the eval HIP forward; returns ``(mse, mae)``."""
        was = self.model.training
        self.model.eval()
        try:
            score = self.model(lq, gt)
        finally:
            self.model.train(was)
        t = self._target(target, score.shape[0], score.device).view_as(score)
        d = score - t
        return (d * d).mean(), d.abs().mean()

    def state_dict(self):
        return self.model.state_dict()

    _optimizer_name = "Adam"

    def training_state(self, epoch: int, current_iter: int) -> dict:
        """``_TrainingState.training_state`` plus what a bit-identical continuation inside an accumulation
        window needs, under keys stock BasicSR ignores: ``asdqe_micro``, the partial ``asdqe_grad`` (when
        ``micro > 0``) and the dropout generator's ``asdqe_generator_state``."""
        state = super().training_state(epoch, current_iter)
        state["asdqe_micro"] = int(self.micro)
        if self.micro > 0:
            state["asdqe_grad"] = self.grad.detach().clone()
        state["asdqe_generator_state"] = self.generator.get_state()
        return state

    def resume_training(self, state: dict) -> None:
        """Without the extra keys the accumulation window restarts empty and the generator keeps its state."""
        super().resume_training(state)
        self.micro = int(state.get("asdqe_micro", 0))
        if self.micro < 0 or self.micro >= self.accumulation_steps:
            raise ValueError(f"asdqe_micro {self.micro} does not fit accumulation_steps {self.accumulation_steps}")
        g = state.get("asdqe_grad")
        if self.micro > 0:
            if g is None or g.numel() != self.grad.numel():
                raise ValueError("asdqe_micro > 0 needs the partial gradient 'asdqe_grad' of the engine's size")
            self.grad.copy_(g)
        else:
            self.grad.zero_()
        if state.get("asdqe_generator_state") is not None:
            self.generator.set_state(state["asdqe_generator_state"].cpu())


def _mix(t, perm, lam):
    t = t.to(torch.float32).contiguous()
    out = torch.empty_like(t)
    per = t.numel() // t.shape[0]
    rc = _lib.lib().kdlae_train_mixup(_vp(t), _vp(out), t.shape[0], per, _vp(perm), float(lam), _stream(t.device))
    _lib.check(rc, "kdlae_train_mixup")
    return out


class MixingAugment:
    """Mixing_Augment (Train/basicsr/models/image_restoration_model.py:25-61), blend on the GPU.

    lam ~ Beta(mixup_beta, mixup_beta) and the batch permutation are drawn on the host exactly as the
    reference draws them (torch.distributions / torch.randperm / random.randint), so a seeded run
    picks the same mixes; the blend lam * x + (1 - lam) * x[perm] is ``kdlae_train_mixup``."""

    def __init__(self, mixup_beta=1.2, use_identity=False, device=None):
        self.dist = torch.distributions.beta.Beta(torch.tensor([mixup_beta]), torch.tensor([mixup_beta]))
        self.device = device
        self.use_identity = use_identity
        self.augments = [self.mixup]

    def mixup(self, target, input_):
        lam = self.dist.rsample((1, 1)).item()
        first = next(iter(target.values())) if isinstance(target, dict) else target
        if first.device.type != "cuda":
            raise RuntimeError("MixingAugment (MI355X build) blends ROCm tensors only")
        r_index = torch.randperm(first.size(0))
        perm = r_index.to(device=first.device, dtype=torch.int32)

        def blend(v):
            return _mix(v, perm, lam) if v is not None else None

        mixed_target = {k: blend(v) for k, v in target.items()} if isinstance(target, dict) else blend(target)
        mixed_input = {k: blend(v) for k, v in input_.items()} if isinstance(input_, dict) else blend(input_)
        return mixed_target, mixed_input

    def __call__(self, target, input_):
        if self.use_identity:
            augment_idx = random.randint(0, len(self.augments))  # includes "no augmentation"
        else:
            augment_idx = random.randint(0, len(self.augments) - 1)
        if augment_idx < len(self.augments):
            target, input_ = self.augments[augment_idx](target, input_)
        return target, input_


def sync_gradients(grad: torch.Tensor, group=None) -> float:
    """DDP gradient averaging (base_model.py:76-82) as ONE all-reduce over the flat gradient buffer.

    Sums in place over the process group (RCCL on ROCm, gloo on CPU) and returns the scale
    (1 / world size) that the clip + AdamW kernel folds in, so the mean never costs a pass."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1.0
    ws = dist.get_world_size(group)
    if ws == 1:
        return 1.0
    if grad.is_cuda and dist.get_backend(group) != "nccl":
        host = grad.cpu()  # gloo reduces host memory (multi-process tests sharing one GPU)
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        grad.copy_(host)
    else:
        dist.all_reduce(grad, op=dist.ReduceOp.SUM, group=group)
    return 1.0 / ws


def grad_buckets(mark_los, numel: int, cap_floats: int):
    """DDP-style gradient buckets over the flat buffer from the backward's gradient-ready marks.

    ``mark_los[j]``: the suffix [lo, numel) is final at mark j (decreasing).  Consecutive marks are
    merged until a bucket holds ``cap_floats`` (DistributedDataParallel's bucket_cap_mb, 25 MB by
    default); returns [(mark or None, lo, hi)] covering [0, numel) exactly, back to front.  A bucket
    waits on its mark's event; None = after the whole backward."""
    out, hi = [], numel
    for j, lo in enumerate(mark_los):
        if lo < hi and hi - lo >= cap_floats:
            out.append((j, lo, hi))
            hi = lo
    if hi > 0:
        last = len(mark_los) - 1 if mark_los and mark_los[-1] == 0 else None
        out.append((last, 0, hi))
    return out


def allreduce_buckets_rccl(grad: torch.Tensor, buckets, handle, group=None) -> None:
    """RCCL leg of ``sync_gradients_bucketed``: each bucket's SUM all-reduce is enqueued on the
    communication stream behind its gradient-ready event; the current stream waits for all of them."""
    L = _lib.lib()
    comm = _comm_stream(grad.device)
    cur = torch.cuda.current_stream(grad.device)
    works = []
    for j, lo, hi in buckets:
        if j is None:
            comm.wait_stream(cur)
        else:
            _lib.check(L.kdlae_tt_mark_wait(handle, j, ctypes.c_void_p(comm.cuda_stream)), "kdlae_tt_mark_wait")
        with torch.cuda.stream(comm):
            works.append(dist.all_reduce(grad[lo:hi], op=dist.ReduceOp.SUM, group=group, async_op=True))
    for w in works:
        w.wait()
    cur.wait_stream(comm)


def sync_gradients_bucketed(grad: torch.Tensor, buckets, handle=None, group=None) -> float:
    """The DDP all-reduce overlapped with the backward: bucket (j, lo, hi) of ``grad`` is all-reduced on
    a communication stream as soon as the backward has recorded gradient-ready event j
    (``kdlae_tt_mark_wait``), while the backward's later layers still run; the current stream then
    waits for every bucket.  Returns the 1 / world-size scale, like ``sync_gradients``.  On gloo
    (host collectives: the multi-process tests) each bucket waits for its event on the host."""
    if not (dist.is_available() and dist.is_initialized()):
        return 1.0
    ws = dist.get_world_size(group)
    if ws == 1:
        return 1.0
    L = _lib.lib()
    if grad.is_cuda and dist.get_backend(group) == "nccl":
        allreduce_buckets_rccl(grad, buckets, handle, group)
        return 1.0 / ws
    if not grad.is_cuda:
        for _, lo, hi in buckets:
            dist.all_reduce(grad[lo:hi], op=dist.ReduceOp.SUM, group=group)
        return 1.0 / ws
    # gloo on device gradients: the same event-ordered schedule as RCCL, with each bucket staged
    # through pinned host memory by a stream-ordered copy on the communication stream (so a bucket
    # leaves the device when its event fires, not after the whole backward)
    comm = _comm_stream(grad.device)
    cur = torch.cuda.current_stream(grad.device)
    staged = []
    for j, lo, hi in buckets:
        if j is None:
            comm.wait_stream(cur)
        else:
            _lib.check(L.kdlae_tt_mark_wait(handle, j, ctypes.c_void_p(comm.cuda_stream)), "kdlae_tt_mark_wait")
        host = torch.empty(hi - lo, dtype=grad.dtype, pin_memory=True)
        with torch.cuda.stream(comm):
            host.copy_(grad[lo:hi], non_blocking=True)
        comm.synchronize()  # this bucket's event wait and copy only
        dist.all_reduce(host, op=dist.ReduceOp.SUM, group=group)
        with torch.cuda.stream(comm):
            grad[lo:hi].copy_(host, non_blocking=True)
        staged.append(host)
    cur.wait_stream(comm)
    comm.synchronize()  # the pinned staging buffers outlive their copies
    return 1.0 / ws


_COMM = {}


def _comm_stream(device):
    key = torch.device(device).index
    if key not in _COMM:
        _COMM[key] = torch.cuda.Stream(device=device)
    return _COMM[key]


def _position_from_periods(iteration: int, cumulative_period) -> int:
    """get_position_from_periods (Train/basicsr/models/lr_scheduler.py:115-133)."""
    for i, period in enumerate(cumulative_period):
        if iteration <= period:
            return i
    return None


class CosineAnnealingRestartCyclicLR:
    """The LR schedule of KDLAET.yml (train.scheduler, :95-99), lr_scheduler.py:186-233 restated
    over the trainer's single parameter group: ``lr(last_epoch)`` is what the reference's
    ``get_lr`` returns after ``last_epoch`` scheduler steps."""

    def __init__(self, base_lr: float, periods, restart_weights=(1,), eta_mins=(0,)):
        if len(periods) != len(restart_weights):
            raise ValueError("periods and restart_weights should have the same length.")
        self.base_lr = float(base_lr)
        self.periods, self.restart_weights, self.eta_mins = list(periods), list(restart_weights), list(eta_mins)
        self.cumulative_period = [sum(self.periods[:i + 1]) for i in range(len(self.periods))]

    def lr(self, last_epoch: int) -> float:
        idx = _position_from_periods(last_epoch, self.cumulative_period)
        w = self.restart_weights[idx]
        nearest_restart = 0 if idx == 0 else self.cumulative_period[idx - 1]
        eta_min = self.eta_mins[idx]
        return eta_min + w * 0.5 * (self.base_lr - eta_min) * (
            1 + math.cos(math.pi * ((last_epoch - nearest_restart) / self.periods[idx])))


class _ImageCleanTrainer(_TrainingState):
    """ImageCleanModel.optimize_parameters (image_restoration_model.py:198-218) over a ``kdlae_tt_*`` handle's
    flat buffers: everything the KDLAE-T and the Restormer trainer share.  A subclass names its engine
    (``_engine_cls``), its loss scratch (``_loss_scratch_floats``), how a batch reaches the network and the loss
    (``_forward_loss``) and how a validation pair is read (``_val_pair``)."""

    _engine_cls = None

    def __init__(self, model, lr=1e-5, weight_decay=0.5e-4, betas=(0.2, 0.999), eps=1e-8, use_grad_clip=True,
                 max_norm=0.01, loss_weight=1.0, group=None, mixing_augs=None, ema_decay=0.0, scheduler=None,
                 bucket_cap_mb=25.0, overlap_grad_reduce=True):
        params = list(model.parameters())
        if not params or params[0].device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__}: move the model to a ROCm device first (no CPU fallback)")
        dev = params[0].device
        self.model = model
        self.engine = self._engine_cls(model, dev)
        eng = self.engine
        # flat parameter buffer; the module's parameters become views of it
        self.theta = eng.flatten(params).contiguous()
        with torch.no_grad():
            for (k, n, off), p in zip(eng.keys, params):
                p.data = self.theta[off:off + n].view(p.shape)
        self.grad = torch.zeros(eng.numel, dtype=torch.float32, device=dev)
        self.exp_avg = torch.zeros_like(self.grad)
        self.exp_avg_sq = torch.zeros_like(self.grad)
        self.lr, self.weight_decay, self.betas, self.eps = lr, weight_decay, tuple(betas), eps
        self.init_lr = lr
        # train.scheduler (e.g. CosineAnnealingRestartCyclicLR for KDLAET.yml); driven by the caller
        # through update_learning_rate(current_iter) like BaseModel's, else the lr stays fixed
        self.scheduler = scheduler
        self.max_norm = max_norm if use_grad_clip else 0.0
        self.loss_weight = loss_weight
        self.group = group
        # DDP gradient buckets (DistributedDataParallel(bucket_cap_mb=25), base_model.py:76-82):
        # all-reduced while the backward still runs; overlap_grad_reduce=False = one collective after it
        self.bucket_cap_floats = max(1, int(bucket_cap_mb * 1024 * 1024 / 4))
        self.overlap_grad_reduce = overlap_grad_reduce
        self.buckets = None
        self.step_count = 0
        self.output = None
        self.loss = None
        # frozen parameters (requires_grad False at construction, or set_trainable later)
        mask = [bool(p.requires_grad) for p in params]
        if not all(mask):
            eng.set_trainable(mask)
        self._set_ranges()
        L = _lib.lib()
        self._l1_scratch = torch.empty(self._loss_scratch_floats(), dtype=torch.float32, device=dev)
        self._opt_scratch = torch.empty(int(L.kdlae_train_adamw_scratch_floats()), dtype=torch.float32, device=dev)
        self._loss = torch.zeros((), dtype=torch.float32, device=dev)
        # KDLAET.yml train.mixing_augs ({mixup, mixup_beta, use_identity}); ImageCleanModel.__init__ :83-87
        m = mixing_augs or {}
        self.mixing = (MixingAugment(m.get("mixup_beta", 1.2), m.get("use_identity", False), dev)
                       if m.get("mixup", False) else None)
        # train.ema_decay (ImageCleanModel.__init__: net_g_ema starts as a copy of net_g, model_ema(0))
        self.ema_decay = float(ema_decay)
        self.theta_ema = self.theta.clone() if self.ema_decay > 0 else None

    def _set_ranges(self):
        """The [begin, end) ranges clip + AdamW updates: the used, trainable keys (frozen weights see neither
        the update nor the weight decay, as torch.optim never holds them)."""
        ranges = self.engine.used_ranges()
        self._ranges = (ctypes.c_int64 * (2 * len(ranges)))(*[v for r in ranges for v in r])
        self._nranges = len(ranges) if len(ranges) != 1 or ranges[0] != [0, self.engine.numel] else 0

    def set_trainable(self, which=None):
        """Choose the trainable parameters: ``which`` is an iterable of parameter names, a predicate
        ``name -> bool``, or ``None`` for all.  Sets the parameters' ``requires_grad`` and the engine's mask;
        frozen ``theta``, ``exp_avg`` and ``exp_avg_sq`` then keep their bits across ``step()``.  Call it between
        iterations (not between ``forward_backward`` and ``step``)."""
        names = [k for k, _, _ in self.engine.keys]
        if which is None:
            mask = [True] * len(names)
        elif callable(which):
            mask = [bool(which(k)) for k in names]
        else:
            want = set(which)
            unknown = sorted(want - set(names))
            if unknown:
                raise ValueError(f"set_trainable: unknown parameter names {unknown[:4]}")
            mask = [k in want for k in names]
        self.engine.set_trainable(None if all(mask) else mask)
        for p, t in zip(self.model.parameters(), mask):
            p.requires_grad = t
        self._set_ranges()

    def update_learning_rate(self, current_iter: int, warmup_iter: int = -1) -> float:
        """BaseModel.update_learning_rate (Train/basicsr/models/base_model.py:183-205): the scheduler
        has stepped current_iter - 1 times by iteration current_iter (train.py calls this before
        optimize_parameters); linear warm-up below warmup_iter.  Returns the lr now in force."""
        if self.scheduler is not None:
            self.lr = self.scheduler.lr(max(current_iter - 1, 0))
        if current_iter < warmup_iter:
            self.lr = self.init_lr / warmup_iter * current_iter
        return self.lr

    def feed_train_data(self, lq, gt):
        """ImageCleanModel.feed_train_data (:161-186): the optional mixup of (gt, lq); dicts of tensors
        (KDLAE-T) or bare tensors (Restormer)."""
        if self.mixing is not None:
            gt, lq = self.mixing(gt, lq)
        return lq, gt

    def ema_state_dict(self):
        """net_g_ema's parameters (``params_ema`` in BasicSR checkpoints) as views of the EMA buffer."""
        if self.theta_ema is None:
            raise RuntimeError("ema_decay is 0: there is no EMA copy")
        return {k: self.theta_ema[off:off + n].view(p.shape)
                for (k, n, off), p in zip(self.engine.keys, self.model.parameters())}

    def load_ema_state_dict(self, sd, strict: bool = True):
        """Counterpart of ``ema_state_dict()``: copy a ``params_ema`` entry (checkpoint.py reads it) into the
        EMA buffer.  ``strict``: every parameter key must be present with its shape."""
        if self.theta_ema is None:
            raise RuntimeError("ema_decay is 0: there is no EMA copy")
        names = {k for k, _, _ in self.engine.keys}
        unexpected = [k for k in sd if k not in names]
        missing = [k for k in names if k not in sd]
        if strict and (unexpected or missing):
            raise RuntimeError(f"load_ema_state_dict: missing keys {missing[:4]}, unexpected keys {unexpected[:4]}")
        with torch.no_grad():
            for (k, n, off), p in zip(self.engine.keys, self.model.parameters()):
                if k not in sd:
                    continue
                if tuple(sd[k].shape) != tuple(p.shape):
                    raise RuntimeError(f"size mismatch for {k}: {tuple(sd[k].shape)} vs {tuple(p.shape)}")
                self.theta_ema[off:off + n].copy_(sd[k].detach().reshape(-1))

    @torch.no_grad()
    def validate(self, batches, window_size=8, crop_border=0, use_image=False, use_ema=None, metrics=("psnr",),
                 niqe=False, niqe_params=None, tile=None, tile_overlap=32, tile_batch=16, tile_window="uniform",
                 ensemble=None, ens_batch=8):
        """ImageCleanModel.nondist_validation with pad_test (image_restoration_model.py:226-348) over
        ``(lq, gt)`` pairs, ``lq = {'img', 'denoise_rate'}``, ``gt = {'hq', 'sr'}`` (RestormerTrainer: two
        tensors, and only the ``*_hq`` results): reflect-pad ``img`` and the
        rate map right and bottom to a multiple of ``window_size``, run the inference engine
        (``kdlae_t_forward``), and take the PSNR of the top-left h x w window of ``hq`` (2h x 2w of ``sr``)
        against its target.  Returns ``{'psnr_hq': mean, 'psnr_sr': mean}`` over all images (``psnr_sr`` only
        when ``static == 'train'``).  ``metrics``: ``"psnr"`` and / or ``"ssim"`` (the val.metrics names
        calculate_psnr / calculate_ssim, :324-336); with ``"ssim"`` the result also holds ``ssim_hq`` / ``ssim_sr``
        over the same windows.  ``niqe=True`` adds ``niqe_hq`` / ``niqe_sr``: ``calculate_niqe`` (the third
        val.metrics type, no target needed) of the outputs' windows, always on ``tensor2img``'s uint8 image,
        which is what the reference's function takes (at least 96 x 96 pixels after ``crop_border``);
        ``niqe_params`` is the reference's pristine model (``metrics.load_niqe_params``).

        ``tile``: validate images too large for one forward.  The padded image goes through the tiled forward
        (``KDLAE_teacher.forward_tiled``'s tiles, ``tile_overlap`` and ``tile_batch``, with the weights chosen
        below) instead of one ``kdlae_t_forward``; the padded sizes must then be multiples of 8.  A tiled output
        is a different function of the image from the untiled one (MDTA's attention is global over each tile),
        so its metrics are not comparable digit for digit with ``tile=None``, today's path.  ``tile_window``:
        the blend window of the tiled forward (``forward_tiled``'s ``window``); not read without ``tile``.

        ``ensemble``: geometric self-ensemble at evaluation, the usual setting of reported PSNR / SSIM: ``"d8"``,
        ``"flips"`` or an iterable of modes 0..7 (``forward_ensemble``'s ``modes``, ``ens_batch`` views of the batch
        a forward).  The padded image goes through the views' forwards and one merge per output (with the weights
        chosen below; the padded sizes must then be multiples of 8) instead of one ``kdlae_t_forward``.  The mean
        over the views is a different function of the image, so its metrics are not comparable digit for digit
        with ``ensemble=None``, today's path.  Not to be combined with ``tile``.

        ``use_ema=None``: the EMA weights when ``ema_decay > 0`` (net_g_ema, :242-248), else the live ones.
        The chosen flat vector is packed straight into the module's inference handle; the trainer's buffers,
        the training engine and the module's parameters are not written, so training continues bit for bit."""
        from .metrics import load_niqe_params, niqe_batch, psnr_batch, ssim_batch
        want_psnr, want_ssim = _val_metrics(metrics)
        if ensemble is not None and tile is not None:
            raise RuntimeError("validate: ensemble= and tile= cannot be combined")
        niqe_p, n_hqs, n_srs = (load_niqe_params(niqe_params) if niqe else None), [], []
        if use_ema is None:
            use_ema = self.theta_ema is not None
        if use_ema and self.theta_ema is None:
            raise RuntimeError("ema_decay is 0: there is no EMA copy to validate")
        flat = _inference_flat(self, self.theta_ema if use_ema else self.theta)
        hqs, srs, s_hqs, s_srs, seen = [], [], [], [], False
        for lq, gt in batches:
            img, rate, gt = self._val_pair(lq, gt)
            if img.device.type != "cuda":
                raise RuntimeError("KDLAE validation runs on ROCm devices only; there is no CPU fallback")
            h, w = img.shape[-2:]
            img_p = _reflect_pad(img.to(torch.float32), window_size)
            rate_p = _reflect_pad(rate.to(device=img.device, dtype=torch.float32), window_size) if rate is not None \
                else None
            if ensemble is not None:
                out = self.model._forward_ensemble(img_p, rate_p, ensemble, ens_batch, flat=flat)
            elif tile is None:
                out = self.model._forward_eager(img_p, rate_p, flat=flat)
            else:
                out = self.model._forward_tiled(img_p, rate_p, tile, tile_overlap, tile_batch, flat=flat,
                                                window=tile_window)
            # the last item's cropped outputs (pad_test's self.output, :236-237), as views
            self.val_output = {"hq": out["hq"][..., :h, :w],
                               "sr": out["sr"][..., :2 * h, :2 * w] if out["sr"] is not None else None}
            seen = True
            for want, fn, a_hq, a_sr in ((want_psnr, psnr_batch, hqs, srs), (want_ssim, ssim_batch, s_hqs, s_srs)):
                if not want:
                    continue
                a_hq.append(fn(out["hq"], gt["hq"].to(img.device), (h, w), crop_border, use_image))
                if out["sr"] is not None:
                    a_sr.append(fn(out["sr"], gt["sr"].to(img.device), (2 * h, 2 * w), crop_border, use_image))
            if niqe:
                n_hqs.append(niqe_batch(out["hq"], (h, w), crop_border, True, "y", niqe_p))
                if out["sr"] is not None:
                    n_srs.append(niqe_batch(out["sr"], (2 * h, 2 * w), crop_border, True, "y", niqe_p))
        if not seen:
            raise ValueError("validate: no batches")
        res = {}
        for name, vals in (("psnr_hq", hqs), ("psnr_sr", srs), ("ssim_hq", s_hqs), ("ssim_sr", s_srs),
                           ("niqe_hq", n_hqs), ("niqe_sr", n_srs)):
            if vals:
                res[name] = float(torch.cat(vals).mean())
        return res

    def _distributed(self) -> bool:
        return dist.is_available() and dist.is_initialized() and dist.get_world_size(self.group) > 1

    def forward_backward(self, lq, gt, marked: bool = False):
        """preds = net_g(lq); l_pix = cri_pix(preds, gt); l_pix.backward()  (:198-213).

        ``marked``: record gradient-ready marks and build ``self.buckets`` for the overlapped all-reduce."""
        eng = self.engine
        dhq, dsr, loss = self._forward_loss(lq, gt)
        if marked:
            self.buckets = grad_buckets(eng.backward(self.theta, dhq, dsr, self.grad, marked=True), eng.numel,
                                        self.bucket_cap_floats)
        else:
            eng.backward(self.theta, dhq, dsr, self.grad)
        self.loss = loss
        return self.loss

    def step(self, gscale: float = 1.0):
        """clip_grad_norm_(net_g.parameters(), 0.01) + AdamW step (:215-218) over the flat buffers."""
        self.step_count += 1
        b1, b2 = self.betas
        rc = _lib.lib().kdlae_train_clip_adamw(
            _vp(self.theta), _vp(self.grad), _vp(self.exp_avg), _vp(self.exp_avg_sq), self.engine.numel,
            float(gscale), float(self.max_norm), float(self.lr), float(b1), float(b2), float(self.eps),
            float(self.weight_decay), self.step_count, self._ranges if self._nranges else None, self._nranges,
            _vp(self._opt_scratch), _stream(self.theta.device))
        _lib.check(rc, "kdlae_train_clip_adamw")
        if self.theta_ema is not None:  # model_ema(decay) after the step (:221-222)
            rc = _lib.lib().kdlae_train_ema(_vp(self.theta_ema), _vp(self.theta), self.engine.numel,
                                            self.ema_decay, _stream(self.theta.device))
            _lib.check(rc, "kdlae_train_ema")

    def optimize_parameters(self, lq, gt):
        """One full iteration: forward, the loss, backward, DDP all-reduce, clip, AdamW.  With several
        ranks the all-reduce runs in gradient buckets overlapped with the backward (overlap_grad_reduce)."""
        if self._distributed() and self.overlap_grad_reduce:
            loss = self.forward_backward(lq, gt, marked=True)
            gscale = sync_gradients_bucketed(self.grad, self.buckets, self.engine.handle, self.group)
        else:
            loss = self.forward_backward(lq, gt)
            gscale = sync_gradients(self.grad, self.group)
        self.step(gscale)
        return loss

    def grad_norm(self) -> torch.Tensor:
        """Gradient norm of the last step (after DDP averaging, before clipping)."""
        return self._opt_scratch[2048]

    def get_current_log(self):
        return {"l_pix": float(self.loss)} if self.loss is not None else {}


class KDLAETrainer(_ImageCleanTrainer):
    """ImageCleanModel.optimize_parameters for KDLAE_teacher (image_restoration_model.py:198-218).

    Defaults follow Train/Denoising/Options/paper202508/KDLAET.yml: AdamW lr 1e-5,
    weight_decay 5e-5, betas (0.2, 0.999); use_grad_clip -> clip_grad_norm_(0.01); L1LossSr.
    ``lq = {'img', 'denoise_rate'}``, ``gt = {'hq', 'sr'}``."""

    _engine_cls = TrainEngine

    def _loss_scratch_floats(self):
        return int(_lib.lib().kdlae_train_l1sr_scratch_floats())

    def _val_pair(self, lq, gt):
        return lq["img"], (lq.get("denoise_rate") if self.engine.params_cat else None), gt

    def _forward_loss(self, lq, gt):
        hq, sr = self.engine.forward(self.theta, lq["img"], lq.get("denoise_rate"))
        self.output = {"hq": hq, "sr": sr}
        dhq = torch.empty_like(hq)
        dsr = torch.empty_like(sr) if sr is not None else None
        gt_hq = gt["hq"].to(torch.float32).contiguous()
        gt_sr = gt["sr"].to(torch.float32).contiguous() if sr is not None else None
        rc = _lib.lib().kdlae_train_l1sr(_vp(hq), _vp(gt_hq), hq.numel(), _vp(sr), _vp(gt_sr),
                                         sr.numel() if sr is not None else 0, _vp(dhq), _vp(dsr), _vp(self._loss),
                                         _vp(self._l1_scratch), _stream(hq.device))
        _lib.check(rc, "kdlae_train_l1sr")
        if self.loss_weight != 1.0:
            dhq.mul_(self.loss_weight)
            if dsr is not None:
                dsr.mul_(self.loss_weight)
        return dhq, dsr, self._loss * self.loss_weight


class RestormerTrainer(_ImageCleanTrainer):
    """ImageCleanModel.optimize_parameters for ``KDLAE_model.Restormer`` with paper202508/Restomer.yml: tensor
    ``lq`` / ``gt`` [B,C,H,W], the optional mixup, forward, ``L1LossSonar(loss_weight, reduction, binary)``
    (``kdlae_train_l1sonar``), backward, clip_grad_norm_(0.01) + AdamW (lr 1e-5, weight_decay 5e-5, betas
    (0.2, 0.999)), EMA, CosineAnnealingRestartCyclicLR.  ``validate`` returns the ``*_hq`` metrics of the
    output; ``training_state`` / ``resume_training`` / ``set_trainable`` / ``group=`` as ``KDLAETrainer``."""

    _engine_cls = RestormerTrainEngine

    def __init__(self, model, *args, reduction="mean", binary=0.1, **kwargs):
        if reduction not in _REDUCTIONS:
            raise NotImplementedError("the HIP L1LossSonar implements reduction='mean' and 'sum'")
        self.reduction, self.binary = reduction, binary
        super().__init__(model, *args, **kwargs)

    def _loss_scratch_floats(self):
        return int(_lib.lib().kdlae_train_l1sonar_scratch_floats())

    def _val_pair(self, lq, gt):
        return lq, None, {"hq": gt}

    def _forward_loss(self, lq, gt):
        out, _ = self.engine.forward(self.theta, lq, None)
        self.output = out
        dout = torch.empty_like(out)
        gt_c = gt.to(device=out.device, dtype=torch.float32).contiguous()
        if gt_c.shape != out.shape:
            raise RuntimeError(f"RestormerTrainer: gt {tuple(gt_c.shape)} does not match the output {tuple(out.shape)}")
        _l1sonar(out, gt_c, self.loss_weight, self.binary, self.reduction, dout, self._loss, self._l1_scratch)
        return dout, None, self._loss.clone()

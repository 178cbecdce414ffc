"""Drop-in KDLAE-T module whose forward runs on the MI355X HIP path (libkdlae.so).

Same public surface as ``KDLAE/KDLAE_model.py`` in the reference:
  * ``KDLAE_teacher(**ctor kwargs)`` with identical kwargs and defaults (:205-218);
  * an identical submodule tree, so ``state_dict()`` keys / shapes match the released ``.pth``
    files (``torch.load(p)['params']`` + strict ``load_state_dict``, KDLAE_T.ipynb:1074-1075) and
    the BasicSR ``RestormerSuperResolutionParam2`` checkpoints (same 483 keys);
  * ``forward({'img': [B,C,H,W], 'denoise_rate': [B,1,H,W]}) -> {'hq', 'sr'}`` (:270-336).

The submodules here only own parameters.  ``KDLAE_teacher.forward`` hands device pointers to the C
ABI (``kdlae_t_forward``), which enqueues the whole network on the current HIP stream.  There is
no CPU path: a CPU tensor or a missing library raises.  The CPU restatement used to check this
module lives in ``oracle/`` and is test infrastructure only.
"""
from __future__ import annotations

import ctypes
import numbers
import warnings
import weakref

import torch
import torch.nn as nn

from . import _lib


class BiasFree_LayerNorm(nn.Module):
    """Parameter holder for x / sqrt(var_C(x) + 1e-5) * w (KDLAE_model.py:38-52)."""

    def __init__(self, normalized_shape):
        super().__init__()
        if isinstance(normalized_shape, numbers.Integral):
            normalized_shape = (normalized_shape,)
        self.normalized_shape = torch.Size(normalized_shape)
        self.weight = nn.Parameter(torch.ones(self.normalized_shape))


class WithBias_LayerNorm(nn.Module):
    """Parameter holder for (x - mu) / sqrt(var + 1e-5) * w + b (KDLAE_model.py:54-70)."""

    def __init__(self, normalized_shape):
        super().__init__()
        if isinstance(normalized_shape, numbers.Integral):
            normalized_shape = (normalized_shape,)
        self.normalized_shape = torch.Size(normalized_shape)
        self.weight = nn.Parameter(torch.ones(self.normalized_shape))
        self.bias = nn.Parameter(torch.zeros(self.normalized_shape))


class LayerNorm(nn.Module):
    def __init__(self, dim, LayerNorm_type):
        super().__init__()
        self.body = BiasFree_LayerNorm(dim) if LayerNorm_type == "BiasFree" else WithBias_LayerNorm(dim)


class FeedForward(nn.Module):
    """GDFN parameters (KDLAE_model.py:89-99): hidden = int(dim * ffn_expansion_factor)."""

    def __init__(self, dim, ffn_expansion_factor, bias):
        super().__init__()
        hidden = int(dim * ffn_expansion_factor)
        self.project_in = nn.Conv2d(dim, 2 * hidden, kernel_size=1, bias=bias)
        self.dwconv = nn.Conv2d(2 * hidden, 2 * hidden, kernel_size=3, padding=1, groups=2 * hidden, bias=bias)
        self.project_out = nn.Conv2d(hidden, dim, kernel_size=1, bias=bias)


class Attention(nn.Module):
    """MDTA parameters (KDLAE_model.py:112-120)."""

    def __init__(self, dim, num_heads, bias):
        super().__init__()
        self.num_heads = num_heads
        self.temperature = nn.Parameter(torch.ones(num_heads, 1, 1))
        self.qkv = nn.Conv2d(dim, 3 * dim, kernel_size=1, bias=bias)
        self.qkv_dwconv = nn.Conv2d(3 * dim, 3 * dim, kernel_size=3, padding=1, groups=3 * dim, bias=bias)
        self.project_out = nn.Conv2d(dim, dim, kernel_size=1, bias=bias)


class TransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, ffn_expansion_factor, bias, LayerNorm_type):
        super().__init__()
        self.norm1 = LayerNorm(dim, LayerNorm_type)
        self.attn = Attention(dim, num_heads, bias)
        self.norm2 = LayerNorm(dim, LayerNorm_type)
        self.ffn = FeedForward(dim, ffn_expansion_factor, bias)


class OverlapPatchEmbed(nn.Module):
    def __init__(self, in_c=3, embed_dim=48, bias=False):
        super().__init__()
        self.proj = nn.Conv2d(in_c, embed_dim, kernel_size=3, padding=1, bias=bias)


class Downsample(nn.Module):
    def __init__(self, n_feat):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat // 2, kernel_size=3, padding=1, bias=False),
                                  nn.PixelUnshuffle(2))


class Upsample(nn.Module):
    def __init__(self, n_feat):
        super().__init__()
        self.body = nn.Sequential(nn.Conv2d(n_feat, n_feat * 2, kernel_size=3, padding=1, bias=False),
                                  nn.PixelShuffle(2))


def _stage(n, dim, heads, ffn, bias, ln):
    return nn.Sequential(*[TransformerBlock(dim, heads, ffn, bias, ln) for _ in range(n)])


class _Engine:
    """One C-ABI handle per (module, device).

    ``prefix`` selects the handle family: ``kdlae_t`` (teacher), ``kdlae_s`` (student) or ``asdqe``.
    The packed weights are rebuilt ON THE DEVICE from the module's live parameters at every forward
    (``<prefix>_pack_device``: one ``torch.cat`` of the state_dict into a flat fp32 buffer, then the
    handle's pack program, ~0.1 ms for KDLAE-T).  Nothing is cached across forwards, so in-place
    writes that bypass autograd's version counter (``p.data.mul_()``, BasicSR's ``model_ema``,
    base_model.py:54-62), optimizer steps and ``load_state_dict`` are always seen."""

    def __init__(self, cfg, device_index: int, prefix: str = "kdlae_t", create: str = "_create"):
        """``create``: the suffix of the create entry (``_create_restormer``: a plain-Restormer ``kdlae_t`` handle)."""
        L = _lib.lib()
        h = ctypes.c_void_p()
        self.prefix = prefix
        _lib.check(getattr(L, prefix + create)(ctypes.byref(cfg), device_index, ctypes.byref(h)),
                   prefix + create)
        self.handle = h
        self.device_index = device_index
        self.ws = None
        self.flat = None
        self._src_sig = None
        self._srcs = None
        self._fin = weakref.finalize(self, getattr(L, prefix + "_destroy"), h)
        names = []
        for i in range(getattr(L, prefix + "_num_params")(h)):
            name, numel = ctypes.c_char_p(), ctypes.c_int64()
            _lib.check(getattr(L, prefix + "_param_info")(h, i, ctypes.byref(name), ctypes.byref(numel)),
                       prefix + "_param_info")
            names.append((name.value.decode(), int(numel.value)))
        self.keys = names
        self.numel = int(getattr(L, prefix + "_params_numel")(h))
        # the pack program (device allocation + synchronous upload) is built here, so no forward —
        # and no HIP-graph capture of one — allocates or synchronises inside the library
        _lib.check(getattr(L, prefix + "_prepare")(h), prefix + "_prepare")

    def _sources(self, module: nn.Module, device) -> list:
        tensors = list(module.parameters()) + list(module.buffers())
        sig = (len(tensors),) + tuple(t.data_ptr() for t in tensors)  # identity of the storages, not values
        if sig != self._src_sig:
            if not tensors and self.keys:
                raise RuntimeError(f"{type(module).__name__}: the module has no registered parameters (an "
                                   "nn.DataParallel replica?). The MI355X build runs one process per GPU: use "
                                   "DistributedDataParallel / torchrun instead of nn.DataParallel")
            sd = module.state_dict(keep_vars=True)
            missing = [k for k, _ in self.keys if k not in sd]
            if missing:
                raise RuntimeError(f"{type(module).__name__}: state_dict lacks {missing[:4]} "
                                   f"({len(missing)} missing keys)")
            srcs = []
            for k, n in self.keys:
                t = sd[k].detach()
                if t.numel() != n:
                    raise RuntimeError(f"size mismatch for {k}: expected {n} elements, got {t.numel()}")
                if t.device != device:
                    raise RuntimeError(f"{k} is on {t.device}, the input on {device}: move the model with .to()")
                # fp32 contiguous storage: keep an aliasing view (reads the live values every forward)
                srcs.append(t.view(-1) if t.dtype == torch.float32 and t.is_contiguous() else t)
            self._srcs, self._src_sig = srcs, sig
        return [t if t.dim() == 1 and t.dtype == torch.float32 else t.reshape(-1).to(torch.float32)
                for t in self._srcs]

    def sync_params(self, module: nn.Module, stream) -> None:
        """Pack the module's current parameters into the handle's device arena (on ``stream``)."""
        device = torch.device("cuda", self.device_index)
        if self.flat is None or self.flat.device != device:
            self.flat = torch.empty(self.numel, dtype=torch.float32, device=device)
        torch.cat(self._sources(module, device), out=self.flat)
        _lib.check(getattr(_lib.lib(), self.prefix + "_pack_device")(
            self.handle, ctypes.c_void_p(self.flat.data_ptr()), self.numel, ctypes.c_void_p(stream)),
            self.prefix + "_pack_device")

    def pack_flat(self, flat: torch.Tensor, stream) -> None:
        """Pack a caller-owned flat parameter vector (every key back to back in ``self.keys`` order, fp32)
        instead of the module's live parameters: how a trainer evaluates its EMA weights."""
        if flat.dtype != torch.float32 or flat.numel() != self.numel or not flat.is_contiguous() or \
                flat.device != torch.device("cuda", self.device_index):
            raise RuntimeError(f"expected a contiguous fp32 vector of {self.numel} parameters on cuda:{self.device_index}")
        _lib.check(getattr(_lib.lib(), self.prefix + "_pack_device")(
            self.handle, ctypes.c_void_p(flat.data_ptr()), self.numel, ctypes.c_void_p(stream)),
            self.prefix + "_pack_device")

    def workspace(self, nbytes: int, device) -> torch.Tensor:
        if self.ws is None or self.ws.numel() < nbytes:
            self.ws = None
            self.ws = torch.empty(int(nbytes), dtype=torch.uint8, device=device)
        return self.ws


class KDLAE_teacher(nn.Module):
    """KDLAE-T (KDLAE/KDLAE_model.py:204-336) with the forward on the MI355X HIP path."""

    def __init__(self, inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8],
                 num_refinement_blocks=4, heads=[1, 2, 4, 8], ffn_expansion_factor=2.66, bias=False,
                 LayerNorm_type='WithBias', dual_pixel_task=False, static="train", params='cat'):
        super().__init__()
        self.params = params
        self.static = static
        self.dual_pixel_task = dual_pixel_task
        self._cfg = dict(inp_channels=inp_channels, out_channels=out_channels, dim=dim,
                         num_blocks=list(num_blocks), num_refinement_blocks=num_refinement_blocks,
                         heads=list(heads), ffn_expansion_factor=ffn_expansion_factor, bias=bias,
                         LayerNorm_type=LayerNorm_type, dual_pixel_task=dual_pixel_task, static=static,
                         params=params)
        d, nb, hd, f, ln = dim, num_blocks, heads, ffn_expansion_factor, LayerNorm_type
        self.patch_embed = OverlapPatchEmbed(inp_channels, d)
        self.encoder_level1 = _stage(nb[0], d, hd[0], f, bias, ln)
        self.down1_2 = Downsample(d)
        self.encoder_level2 = _stage(nb[1], 2 * d, hd[1], f, bias, ln)
        self.down2_3 = Downsample(2 * d)
        self.encoder_level3 = _stage(nb[2], 4 * d, hd[2], f, bias, ln)
        self.down3_4 = Downsample(4 * d)
        self.latent = _stage(nb[3], 8 * d, hd[3], f, bias, ln)
        self.up4_3 = Upsample(8 * d)
        self.reduce_chan_level3 = nn.Conv2d(8 * d, 4 * d, kernel_size=1, bias=bias)
        self.decoder_level3 = _stage(nb[2], 4 * d, hd[2], f, bias, ln)
        self.up3_2 = Upsample(4 * d)
        self.reduce_chan_level2 = nn.Conv2d(4 * d, 2 * d, kernel_size=1, bias=bias)
        self.decoder_level2 = _stage(nb[1], 2 * d, hd[1], f, bias, ln)
        self.up2_1 = Upsample(2 * d)
        self.decoder_level1 = _stage(nb[0], 2 * d, hd[0], f, bias, ln)
        self.refinement = _stage(num_refinement_blocks, 2 * d, hd[0], f, bias, ln)
        if dual_pixel_task:
            self.skip_conv = nn.Conv2d(d, 2 * d, kernel_size=1, bias=bias)
        self.output = nn.Conv2d(2 * d, out_channels, kernel_size=3, padding=1, bias=bias)
        self.output_param = nn.Conv2d(out_channels + 1, 2 * d, kernel_size=3, dilation=2, padding=2, bias=bias)
        self.refinement_out = _stage(num_refinement_blocks, 2 * d, hd[0], f, bias, ln)
        self.output2 = nn.Conv2d(2 * d, out_channels, kernel_size=3, padding=1, bias=bias)
        if static == "train":
            hc = 2 * d
            self.cen = nn.Conv2d(out_channels, hc, kernel_size=3, padding=1, bias=bias)
            self.upen = Upsample(hc)
            self.enhance = _stage(num_refinement_blocks, hc // 2, hd[0], f, bias, ln)
            self.outputen = nn.Conv2d(hc // 2, out_channels, kernel_size=3, padding=1, bias=bias)
        self._engines = {}
        self._train_engines = {}
        self._warned_grad = False

    # ------------------------------------------------------------------ HIP plumbing
    def _c_config(self) -> _lib.TConfig:
        c = self._cfg
        cfg = _lib.TConfig()
        cfg.inp_channels, cfg.out_channels, cfg.dim = c["inp_channels"], c["out_channels"], c["dim"]
        for i in range(4):
            cfg.num_blocks[i] = int(c["num_blocks"][i])
            cfg.heads[i] = int(c["heads"][i])
        cfg.num_refinement_blocks = c["num_refinement_blocks"]
        cfg.ffn_expansion_factor = float(c["ffn_expansion_factor"])
        cfg.bias = int(bool(c["bias"]))
        cfg.layernorm_biasfree = int(c["LayerNorm_type"] == "BiasFree")
        cfg.dual_pixel_task = int(bool(c["dual_pixel_task"]))
        cfg.static_train = int(c["static"] == "train")
        cfg.params_cat = int(c["params"] == "cat")
        return cfg

    def engine(self, device: torch.device) -> _Engine:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        eng = self._engines.get(idx)
        if eng is None:
            eng = _Engine(self._c_config(), idx)
            self._engines[idx] = eng
        return eng

    def forward(self, input):
        img = input["img"]
        denoise_rate = input["denoise_rate"]
        if self.dual_pixel_task:
            raise NotImplementedError("dual_pixel_task=True: the reference forward leaves out_hq undefined "
                                      "(KDLAE_model.py:305-321)")
        if img.device.type != "cuda":
            raise RuntimeError("KDLAE_teacher (MI355X build) runs on ROCm devices only; move the model "
                               "inputs to 'cuda' — there is no CPU fallback")
        if img.dim() != 4 or img.shape[1] != self._cfg["inp_channels"]:
            raise RuntimeError(f"expected img [B,{self._cfg['inp_channels']},H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if H % 8 or W % 8:
            raise RuntimeError(f"KDLAE_teacher needs H and W divisible by 8, got {H}x{W} "
                               "(pad to a multiple of 8 as KDLAE_T.ipynb does)")
        cat = self._cfg["params"] == "cat"
        if cat and tuple(denoise_rate.shape) != (B, 1, H, W):
            raise RuntimeError(f"denoise_rate must be [B,1,H,W]={B, 1, H, W}, got {tuple(denoise_rate.shape)}")
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if wants_grad and not self.training and not self._warned_grad:
            warnings.warn("KDLAE_teacher in eval mode with grad enabled: the HIP inference path returns outputs "
                          "without an autograd graph; call .train() to differentiate through the model")
            self._warned_grad = True
        if wants_grad and self.training:
            # training (BasicSR calls net_g.train()): the HIP training engine behind an autograd node
            # (train.py), so `l_pix.backward()` (image_restoration_model.py:213) runs the hand-written backward
            if img.requires_grad and not self._warned_grad:
                warnings.warn("KDLAE_teacher HIP training path: the input image receives no gradient")
                self._warned_grad = True
            from .train import TeacherTrainFn, TrainEngine
            eng = self._train_engines.get(img.device.index)
            if eng is None:
                eng = TrainEngine(self, img.device)
                self._train_engines[img.device.index] = eng
            out = TeacherTrainFn.apply(eng, img, denoise_rate if cat else None, *self.parameters())
            if self.static == "train":
                return {"hq": out[0], "sr": out[1]}
            return {"hq": out, "sr": None}
        dev = img.device
        if self.hip_graphs and not torch.cuda.is_current_stream_capturing():
            return self._forward_graphed(img, denoise_rate if cat else None)
        return self._forward_eager(img, denoise_rate if cat else None)

    # Repeated inference shapes replay a HIP graph of the whole forward (weight pack program included,
    # so parameter updates are still seen): the ~380 kernel launches of a forward cost no host time
    # and leave no gaps between kernels, which is what single-image latency is made of (bs=1 512^2:
    # 32.0 ms launched one by one, 30.6 ms replayed, profiles/r02_v4_t16_bench.json).  The first call
    # of a shape runs eagerly (it also sizes the workspace and builds the pack program); the second
    # captures.  Inputs are copied into the graph's static buffers and the outputs cloned out, so
    # callers never see aliasing between calls.  `model.hip_graphs = False` turns it off.
    hip_graphs = True
    _GRAPH_CACHE = 4  # shapes kept per module (least recently used dropped)

    def _forward_graphed(self, img, rate, out=None):
        """``out``: as in ``_forward_eager``; the replayed graph's outputs are copied there instead of cloned."""
        dev = img.device
        B, _, H, W = img.shape
        stream = torch.cuda.current_stream(dev)
        eng = self.engine(dev)
        # a graph bakes in every pointer: parameter storages, the flat pack buffer, the workspace
        # (the same tensor list _Engine._sources packs: parameters and buffers)
        key = (dev.index, B, H, W, stream.cuda_stream,
               tuple(t.data_ptr() for t in list(self.parameters()) + list(self.buffers())))
        cache = self.__dict__.setdefault("_graphs", {})
        seen = self.__dict__.setdefault("_graph_seen", {})
        ent = cache.pop(key, None)
        if ent is not None and (eng.ws is None or ent[4] != (eng.ws.data_ptr(), eng.flat.data_ptr())):
            ent = None  # the workspace was reallocated for a larger shape since the capture
        if ent is None:
            if seen.get(key, 0) != 1:  # first call of a shape (or capture failed before): eager
                if len(seen) > 64:
                    seen.clear()
                seen.setdefault(key, 1)
                return self._forward_eager(img, rate, out=out)
            s_img = img.detach().to(torch.float32).contiguous().clone()
            s_rate = rate.detach().to(device=dev, dtype=torch.float32).contiguous().clone() if rate is not None else None
            g = torch.cuda.CUDAGraph()
            torch.cuda.synchronize(dev)
            try:
                # thread_local: HIP calls other threads of the process make meanwhile (a DataLoader's
                # pin_memory thread, an async checkpoint copy) are not captured and do not fail
                with torch.cuda.graph(g, capture_error_mode="thread_local"):
                    s_out = self._forward_eager(s_img, s_rate)
            except RuntimeError:
                seen[key] = 2  # this shape stays eager
                torch.cuda.synchronize(dev)
                return self._forward_eager(img, rate, out=out)
            ent = (g, s_img, s_rate, s_out, (eng.ws.data_ptr(), eng.flat.data_ptr()))
            while len(cache) >= self._GRAPH_CACHE:
                cache.pop(next(iter(cache)))
        cache[key] = ent
        g, s_img, s_rate, s_out, _ = ent
        s_img.copy_(img.detach())
        if s_rate is not None:
            s_rate.copy_(rate.detach())
        g.replay()
        if out is not None:
            for dst, k in zip(out, ("hq", "sr")):
                if dst is not None:
                    dst.copy_(s_out[k])
            return {"hq": out[0], "sr": out[1]}
        return {k: (v.clone() if v is not None else None) for k, v in s_out.items()}

    def _forward_eager(self, img, rate, flat=None, out=None):
        """``flat``: run with this packed parameter vector (``_Engine.pack_flat``) instead of the module's own.
        ``out``: ``(hq, sr)`` contiguous fp32 destinations of the outputs' shapes (``sr`` None without the sr
        head) to write into instead of fresh tensors: how ``forward_tiled`` fills its staging."""
        dev = img.device
        B, _, H, W = img.shape
        cat = rate is not None
        denoise_rate = rate
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng = self.engine(dev)
        if flat is None:
            eng.sync_params(self, stream)
        else:
            eng.pack_flat(flat, stream)
        img_c = img.detach().to(torch.float32).contiguous()
        rate_c = denoise_rate.detach().to(device=dev, dtype=torch.float32).contiguous() if cat else None
        oc = self._cfg["out_channels"]
        if out is not None:
            hq, sr = out
        else:
            hq = torch.empty((B, oc, H, W), device=dev, dtype=torch.float32)
            sr = torch.empty((B, oc, 2 * H, 2 * W), device=dev, dtype=torch.float32) if self.static == "train" \
                else None
        L = _lib.lib()
        nbytes = L.kdlae_t_workspace_bytes(eng.handle, B, H, W)
        if nbytes < 0:
            _lib.check(1, "kdlae_t_workspace_bytes")
        ws = eng.workspace(nbytes, dev)
        rc = L.kdlae_t_forward(eng.handle, ctypes.c_void_p(img_c.data_ptr()),
                               ctypes.c_void_p(rate_c.data_ptr() if rate_c is not None else 0), B, H, W,
                               ctypes.c_void_p(hq.data_ptr()), ctypes.c_void_p(sr.data_ptr() if sr is not None else 0),
                               ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream))
        _lib.check(rc, "kdlae_t_forward")
        return {"hq": hq, "sr": sr}

    # ------------------------------------------------------------------ tiled inference
    def forward_tiled(self, input, tile=512, tile_overlap=32, tile_batch=16, window="uniform"):
        """``forward`` for images larger than one forward can hold: overlapping ``tile`` x ``tile`` tiles (clamped
        per axis to the image), ``tile_overlap`` pixels shared by neighbours, every covered pixel the plain mean of
        its tiles' outputs (tiling.py and include/kdlae.h state the plan and the sum order; it is upstream
        Restormer's ``--tile`` / ``--tile_overlap`` rule).  Tiles are gathered on the device ``tile_batch`` at a
        time and go through this module's own inference forward, so every full chunk replays one HIP graph; the
        outputs land in a staging tensor and one blend launch per output writes the result.

        Returns ``{"hq": [B,C,H,W], "sr": [B,C,2H,2W] or None}``.  Each tile's rows are bit for bit what ``forward``
        gives for that tile alone, for every ``tile_batch``; with one tile per image the result equals ``forward``.
        MDTA's channel attention is global over the pixels it is given, so with more than one tile the result is a
        different function of the image from the untiled ``forward`` (as upstream), not an approximation of it
        that carries a bound.  Inference only (eval mode, no autograd graph).

        ``window``: ``"uniform"`` (the plain mean above, the default), ``"ramp"``, ``"hann"`` or a pair of per-axis
        tables (``tiling.tile_window``): a weighted mean whose weights fall towards the tile edge, so that
        neighbouring tiles cross-fade over their overlap instead of meeting in two steps; a pixel under one tile
        keeps that tile's value bit for bit."""
        self._check_inference_input(input["img"], "forward_tiled")
        with torch.no_grad():
            return self._forward_tiled(input["img"], input.get("denoise_rate"), tile, tile_overlap, tile_batch,
                                       window=window)

    def _forward_tiled(self, img, rate, tile, tile_overlap, tile_batch, flat=None, window="uniform"):
        """``flat``: as in ``_forward_eager`` (a trainer's flat parameters; always launched one by one)."""
        from . import tiling
        ci, oc = self._cfg["inp_channels"], self._cfg["out_channels"]
        if img.dim() != 4 or img.shape[1] != ci:
            raise RuntimeError(f"expected img [B,{ci},H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if int(tile_batch) < 1:
            raise RuntimeError(f"tile_batch must be at least 1, got {tile_batch}")
        plan = tiling.tile_plan(H, W, tile, tile_overlap)   # refuses a bad shape / tile / overlap before any launch
        has_sr = self.static == "train"
        # the blend tables, once per call and before the staging is allocated: a bad window is refused here
        win_hq = tiling.tile_window(window, H, W, tile, tile_overlap, 1, img.device)
        win_sr = tiling.tile_window(window, H, W, tile, tile_overlap, 2, img.device) if has_sr else None
        cat = self._cfg["params"] == "cat"
        if cat and (rate is None or tuple(rate.shape) != (B, 1, H, W)):
            raise RuntimeError(f"denoise_rate must be [B,1,H,W]={B, 1, H, W}, got "
                               f"{tuple(rate.shape) if rate is not None else None}")
        dev = img.device
        img_c = img.detach().to(torch.float32).contiguous()
        rate_c = rate.detach().to(device=dev, dtype=torch.float32).contiguous() if cat else None
        n = B * plan.ni * plan.nj
        th, tw = plan.th, plan.tw
        st_hq = torch.empty((n, oc, th, tw), device=dev, dtype=torch.float32)
        st_sr = torch.empty((n, oc, 2 * th, 2 * tw), device=dev, dtype=torch.float32) if has_sr else None
        graphed = flat is None and self.hip_graphs and not torch.cuda.is_current_stream_capturing()
        for first in range(0, n, int(tile_batch)):
            count = min(int(tile_batch), n - first)
            t_img = tiling.tile_gather(img_c, tile, tile_overlap, first, count)
            t_rate = tiling.tile_gather(rate_c, tile, tile_overlap, first, count) if cat else None
            out = (st_hq[first:first + count], st_sr[first:first + count] if has_sr else None)
            if graphed:
                self._forward_graphed(t_img, t_rate, out=out)
            else:
                self._forward_eager(t_img, t_rate, flat=flat, out=out)
        hq = tiling.tile_blend(st_hq, B, H, W, tile, tile_overlap, 1, window=win_hq)
        sr = tiling.tile_blend(st_sr, B, H, W, tile, tile_overlap, 2, window=win_sr) if has_sr else None
        return {"hq": hq, "sr": sr}

    # ------------------------------------------------------------------ self-ensemble
    def forward_ensemble(self, input, modes="d8", ens_batch=8):
        """Geometric self-ensemble (the "x8" test-time trick): ``forward`` on the dihedral views of the image and of
        its rate map, every output turned back and the results averaged (ensemble.py and include/kdlae_ensemble.h
        state the modes, the sum order and the slot layout).  ``modes``: ``"d8"`` (all eight), ``"flips"`` (the four
        that keep the shape) or an iterable of modes 0..7.  The views of each input are gathered with one launch,
        go through this module's own inference forward ``ens_batch`` views of the whole batch at a time (runs of
        consecutive views of one shape; with H == W any views), so every full chunk replays one HIP graph, and one
        merge launch per output writes the result.

        Returns ``{"hq": [B,C,H,W], "sr": [B,C,2H,2W] or None}``, bit for bit the host loop (``torch.rot90`` /
        ``torch.flip`` of image and rate map, ``forward``, the inverse, ``E.add_`` in ascending mode order, one
        ``E.div_``) for every ``ens_batch``; ``modes=(0,)`` equals ``forward``.  The mean over the views is a
        different function of the image from ``forward``, not an approximation of it that carries a bound.
        Inference only (eval mode, no autograd graph).  A chunk is one forward at batch ``ens_batch * B`` and the
        workspace grows with it: lower ``ens_batch`` when that many images do not fit."""
        self._check_inference_input(input["img"], "forward_ensemble")
        with torch.no_grad():
            return self._forward_ensemble(input["img"], input.get("denoise_rate"), modes, ens_batch)

    def _forward_ensemble(self, img, rate, modes, ens_batch, flat=None):
        """``flat``: as in ``_forward_eager`` (a trainer's flat parameters; always launched one by one)."""
        from . import ensemble
        ci, oc = self._cfg["inp_channels"], self._cfg["out_channels"]
        if img.dim() != 4 or img.shape[1] != ci:
            raise RuntimeError(f"expected img [B,{ci},H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        mask = ensemble.mode_mask(modes)              # refuses bad modes / ens_batch / shapes before any launch
        ensemble.ens_chunks(mask, H, W, ens_batch)
        if H % 8 or W % 8:
            raise RuntimeError(f"forward_ensemble needs H and W divisible by 8, got {H}x{W}")
        cat = self._cfg["params"] == "cat"
        if cat and (rate is None or tuple(rate.shape) != (B, 1, H, W)):
            raise RuntimeError(f"denoise_rate must be [B,1,H,W]={B, 1, H, W}, got "
                               f"{tuple(rate.shape) if rate is not None else None}")
        dev = img.device
        has_sr = self.static == "train"
        g_img = ensemble.ens_gather(img.detach().to(torch.float32), mask)
        g_rate = ensemble.ens_gather(rate.detach().to(device=dev, dtype=torch.float32), mask) if cat else None
        graphed = flat is None and self.hip_graphs and not torch.cuda.is_current_stream_capturing()

        def run(ins, outs):
            if graphed:
                self._forward_graphed(ins[0], ins[1], out=tuple(outs))
            else:
                self._forward_eager(ins[0], ins[1], flat=flat, out=tuple(outs))

        st_hq, st_sr = ensemble.run_views(run, mask, B, H, W, ens_batch, [(g_img, ci), (g_rate, 1)],
                                          [oc, oc if has_sr else None], [1, 2])
        hq = ensemble.ens_merge(st_hq, B, H, W, mask)
        sr = ensemble.ens_merge(st_sr, B, 2 * H, 2 * W, mask) if has_sr else None
        return {"hq": hq, "sr": sr}

    # ------------------------------------------------------------------ rate sweep
    def _check_inference_input(self, x, what):
        if self.dual_pixel_task:
            raise NotImplementedError("dual_pixel_task=True: the reference forward leaves out_hq undefined "
                                      "(KDLAE_model.py:305-321)")
        if self.training:
            raise RuntimeError(f"KDLAE_teacher.{what} is inference-only: call .eval() first (the training path "
                               "differentiates through forward)")
        if x.device.type != "cuda":
            raise RuntimeError("KDLAE_teacher (MI355X build) runs on ROCm devices only; move the model "
                               "inputs to 'cuda' — there is no CPU fallback")

    def forward_rates(self, img, rates, sr=False):
        """R denoise rates of the same images in one call: the rate-independent trunk (everything up to the
        ``output`` conv) runs once, the rate-dependent tail at batch R*B (``kdlae_t_forward_rates``).

        ``rates``: R scalars (sequence or 1-D tensor, shared by the batch), an ``[R, B]`` tensor, or
        ``[R, B, 1, H, W]`` maps.  Returns ``{"hq": [R,B,C,H,W], "sr": [R,B,C,2H,2W] or None}``; ``hq[r]`` /
        ``sr[r]`` are bit for bit what ``forward`` gives with ``denoise_rate = rates[r]``.  Eval mode, eager."""
        self._check_inference_input(img, "forward_rates")
        ci = self._cfg["inp_channels"]
        if img.dim() != 4 or img.shape[1] != ci:
            raise RuntimeError(f"expected img [B,{ci},H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if H % 8 or W % 8:
            raise RuntimeError(f"KDLAE_teacher needs H and W divisible by 8, got {H}x{W} "
                               "(pad to a multiple of 8 as KDLAE_T.ipynb does)")
        if self._cfg["params"] != "cat":
            raise RuntimeError("forward_rates needs params='cat': with params='plus' the forward never reads "
                               "denoise_rate")
        if sr and self.static != "train":
            raise RuntimeError("forward_rates(sr=True) needs static='train': the model has no sr head")
        dev = img.device
        rt = torch.as_tensor(rates, dtype=torch.float32).detach().to(dev)
        if rt.dim() == 1:
            rt = rt[:, None].expand(-1, B)
        is_map = rt.dim() == 5
        R = rt.shape[0] if rt.dim() else 0
        if not (tuple(rt.shape) == (R, B) or tuple(rt.shape) == (R, B, 1, H, W)):
            raise RuntimeError(f"rates must be R scalars, [R,B] or [R,B,1,H,W] with B,H,W = {B, H, W}, got "
                               f"{tuple(rt.shape)}")
        if not 1 <= R <= 64:
            raise RuntimeError(f"forward_rates takes 1..64 rates, got {R}")
        rt = rt.contiguous()
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng = self.engine(dev)
        eng.sync_params(self, stream)
        img_c = img.detach().to(torch.float32).contiguous()
        oc = self._cfg["out_channels"]
        hq = torch.empty((R, B, oc, H, W), device=dev, dtype=torch.float32)
        srt = torch.empty((R, B, oc, 2 * H, 2 * W), device=dev, dtype=torch.float32) if sr else None
        L = _lib.lib()
        nbytes = L.kdlae_t_rates_workspace_bytes(eng.handle, B, R, H, W, int(bool(sr)))
        if nbytes < 0:
            _lib.check(1, "kdlae_t_rates_workspace_bytes")
        ws = eng.workspace(nbytes, dev)
        rc = L.kdlae_t_forward_rates(eng.handle, ctypes.c_void_p(img_c.data_ptr()), ctypes.c_void_p(rt.data_ptr()),
                                     int(is_map), B, R, H, W, ctypes.c_void_p(hq.data_ptr()),
                                     ctypes.c_void_p(srt.data_ptr() if srt is not None else 0),
                                     ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream))
        _lib.check(rc, "kdlae_t_forward_rates")
        return {"hq": hq, "sr": srt}

    # ------------------------------------------------------------------ tiled rate sweep
    def forward_rates_tiled(self, img, rates, sr=False, tile=512, tile_overlap=32, tile_batch=16, window="uniform"):
        """``forward_rates`` for images larger than one forward can hold: the tiles of ``forward_tiled``'s plan go
        through ``kdlae_t_forward_rates`` ``tile_batch`` at a time (the trunk runs once per tile, the rate tail at
        batch R * count), every chunk writes its block of a chunk-major staging buffer, and one
        ``kdlae_tile_blend_rates`` launch per output blends all R results (tiling.py, include/kdlae.h).

        ``rates``: R scalars, ``[R, B]`` or ``[R, B, 1, H, W]`` maps, as ``forward_rates`` takes them.  Returns
        ``{"hq": [R,B,C,H,W], "sr": [R,B,C,2H,2W] or None}``; ``hq[r]`` / ``sr[r]`` are bit for bit what
        ``forward_tiled`` gives with ``denoise_rate = rates[r]`` as a map, for every ``tile_batch``.  The staging
        holds R outputs of every tile (R * B * ni * nj tiles of C * th * tw floats, five times that with ``sr``).
        Eval mode, eager (no HIP-graph replay), no autograd graph.  ``window``: as in ``forward_tiled``, for both
        blends."""
        with torch.no_grad():
            plan, rt, st_hq, st_sr = self._sweep_tiles(img, rates, sr, tile, tile_overlap, tile_batch)
            from . import tiling
            B, _, H, W = img.shape
            R = rt.shape[0]
            hq = tiling.tile_blend_rates(st_hq, R, B, H, W, tile, tile_overlap, tile_batch, 1, window=window)
            srt = tiling.tile_blend_rates(st_sr, R, B, H, W, tile, tile_overlap, tile_batch, 2, window=window) \
                if sr else None
        return {"hq": hq, "sr": srt}

    def _sweep_tiles(self, img, rates, sr, tile, tile_overlap, tile_batch):
        """The sweep on gathered tiles -> (plan, rates as given ([R,B] or maps), hq staging, sr staging or None):
        flat fp32 buffers in ``kdlae_tile_blend_rates``' chunk-major layout.  Every refusal comes before the first
        launch and before the staging is allocated."""
        from . import tiling
        self._check_inference_input(img, "forward_rates_tiled")
        ci, oc = self._cfg["inp_channels"], self._cfg["out_channels"]
        if img.dim() != 4 or img.shape[1] != ci:
            raise RuntimeError(f"expected img [B,{ci},H,W], got {tuple(img.shape)}")
        B, _, H, W = img.shape
        if int(tile_batch) < 1:
            raise RuntimeError(f"tile_batch must be at least 1, got {tile_batch}")
        plan = tiling.tile_plan(H, W, tile, tile_overlap)   # refuses a bad shape / tile / overlap
        if self._cfg["params"] != "cat":
            raise RuntimeError("forward_rates_tiled needs params='cat': with params='plus' the forward never reads "
                               "denoise_rate")
        if sr and self.static != "train":
            raise RuntimeError("forward_rates_tiled(sr=True) needs static='train': the model has no sr head")
        dev = img.device
        rt = torch.as_tensor(rates, dtype=torch.float32).detach().to(dev)
        if rt.dim() == 1:
            rt = rt[:, None].expand(-1, B)
        is_map = rt.dim() == 5
        R = rt.shape[0] if rt.dim() else 0
        if not (tuple(rt.shape) == (R, B) or tuple(rt.shape) == (R, B, 1, H, W)):
            raise RuntimeError(f"rates must be R scalars, [R,B] or [R,B,1,H,W] with B,H,W = {B, H, W}, got "
                               f"{tuple(rt.shape)}")
        if not 1 <= R <= 64:
            raise RuntimeError(f"forward_rates_tiled takes 1..64 rates, got {R}")
        rt = rt.contiguous()
        th, tw, per = plan.th, plan.tw, plan.ni * plan.nj
        n = B * per
        tb = min(int(tile_batch), n)
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng = self.engine(dev)
        L = _lib.lib()
        eng.sync_params(self, stream)
        # sized for the largest chunk and for the tail chunk, whichever needs more
        sizes = [L.kdlae_t_rates_workspace_bytes(eng.handle, c, R, th, tw, int(bool(sr))) for c in {tb, n % tb or tb}]
        if min(sizes) < 0:
            _lib.check(1, "kdlae_t_rates_workspace_bytes")
        ws = eng.workspace(max(sizes), dev)
        img_c = img.detach().to(torch.float32).contiguous()
        T = oc * th * tw
        st_hq = torch.empty((n * R * T,), device=dev, dtype=torch.float32)
        st_sr = torch.empty((n * R * 4 * T,), device=dev, dtype=torch.float32) if sr else None
        # tile -> image, on the device: a chunk's [R, count] scalars are one index_select, no host round trip
        image_of = None if is_map else torch.arange(n, device=dev) // per
        for first in range(0, n, tb):
            count = min(tb, n - first)
            t_img = tiling.tile_gather(img_c, tile, tile_overlap, first, count)
            if is_map:
                t_rate = torch.empty((R, count, 1, th, tw), device=dev, dtype=torch.float32)
                for r in range(R):
                    tiling.tile_gather(rt[r], tile, tile_overlap, first, count, out=t_rate[r])
            else:
                t_rate = rt.index_select(1, image_of[first:first + count]).contiguous()
            hq_k = st_hq[first * R * T:]
            sr_k = st_sr[first * R * 4 * T:] if sr else None
            rc = L.kdlae_t_forward_rates(eng.handle, ctypes.c_void_p(t_img.data_ptr()),
                                         ctypes.c_void_p(t_rate.data_ptr()), int(is_map), count, R, th, tw,
                                         ctypes.c_void_p(hq_k.data_ptr()),
                                         ctypes.c_void_p(sr_k.data_ptr() if sr else 0),
                                         ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream))
            _lib.check(rc, "kdlae_t_forward_rates")
        return plan, rt, st_hq, st_sr

    def forward_sr(self, hq):
        """The sr head alone on an (unclamped) ``hq`` [B,C,H,W] -> ``sr`` [B,C,2H,2W]: the bits ``forward``
        gives for the same ``hq``.  Needs static='train'.  Eval mode, eager."""
        self._check_inference_input(hq, "forward_sr")
        oc = self._cfg["out_channels"]
        if hq.dim() != 4 or hq.shape[1] != oc:
            raise RuntimeError(f"expected hq [B,{oc},H,W], got {tuple(hq.shape)}")
        B, _, H, W = hq.shape
        if H % 8 or W % 8:
            raise RuntimeError(f"KDLAE_teacher needs H and W divisible by 8, got {H}x{W}")
        if self.static != "train":
            raise RuntimeError("forward_sr needs static='train': the model has no sr head")
        dev = hq.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng = self.engine(dev)
        eng.sync_params(self, stream)
        hq_c = hq.detach().to(torch.float32).contiguous()
        sr = torch.empty((B, oc, 2 * H, 2 * W), device=dev, dtype=torch.float32)
        L = _lib.lib()
        nbytes = L.kdlae_t_sr_workspace_bytes(eng.handle, B, H, W)
        if nbytes < 0:
            _lib.check(1, "kdlae_t_sr_workspace_bytes")
        ws = eng.workspace(nbytes, dev)
        rc = L.kdlae_t_forward_sr(eng.handle, ctypes.c_void_p(hq_c.data_ptr()), B, H, W, ctypes.c_void_p(sr.data_ptr()),
                                  ctypes.c_void_p(ws.data_ptr()), ws.numel(), ctypes.c_void_p(stream))
        _lib.check(rc, "kdlae_t_forward_sr")
        return sr


# BasicSR registers the same network under this name (Train/basicsr/models/archs/restormer_arch.py:566)
RestormerSuperResolutionParam2 = KDLAE_teacher


class Restormer(KDLAE_teacher):
    """Plain Restormer (Train/basicsr/models/archs/restormer_arch.py:471-562), the paper's baseline
    (paper202508/Restomer.yml), with the forward on the MI355X HIP path.

    The reference's constructor kwargs and submodule tree: ``state_dict()`` holds Restormer's own keys
    (``patch_embed`` ... ``refinement``, ``output``), so upstream Restormer checkpoints load and none of the
    teacher's ``output_param.*`` / ``refinement_out.*`` / ``output2.*`` is read or written.
    ``forward(x [B,C,H,W]) -> [B,C,H,W]`` = ``output(refinement(...)) + x``, H and W divisible by 8.

    The network is ``KDLAE_teacher(params != 'cat', static != 'train')``'s and runs the same kernels in the same
    order (``kdlae_t_create_restormer`` / ``kdlae_tt_create_restormer``); this class inherits the teacher's
    plumbing (HIP-graph replay with an eager fallback in eval mode, ``forward_tiled``, the training engine behind
    an autograd node in train mode, ``requires_grad`` read as the trainable mask) with tensors in place of dicts.
    ``dual_pixel_task=True`` raises NotImplementedError."""

    def __init__(self, inp_channels=3, out_channels=3, dim=48, num_blocks=[4, 6, 6, 8], num_refinement_blocks=4,
                 heads=[1, 2, 4, 8], ffn_expansion_factor=2.66, bias=False, LayerNorm_type='WithBias',
                 dual_pixel_task=False):
        nn.Module.__init__(self)
        if dual_pixel_task:
            raise NotImplementedError("Restormer dual_pixel_task=True needs a 6-channel patch embed; the MI355X "
                                      "build's narrow-input conv takes at most 4 channels")
        if inp_channels != out_channels:
            raise RuntimeError(f"Restormer: inp_channels ({inp_channels}) must equal out_channels ({out_channels}): "
                               "the residual output(...) + inp_img is undefined otherwise")
        self.params, self.static, self.dual_pixel_task = "none", "none", False
        self._cfg = dict(inp_channels=inp_channels, out_channels=out_channels, dim=dim,
                         num_blocks=list(num_blocks), num_refinement_blocks=num_refinement_blocks,
                         heads=list(heads), ffn_expansion_factor=ffn_expansion_factor, bias=bias,
                         LayerNorm_type=LayerNorm_type, dual_pixel_task=False, static="none", params="none")
        d, nb, hd, f, ln = dim, num_blocks, heads, ffn_expansion_factor, LayerNorm_type
        self.patch_embed = OverlapPatchEmbed(inp_channels, d)
        self.encoder_level1 = _stage(nb[0], d, hd[0], f, bias, ln)
        self.down1_2 = Downsample(d)
        self.encoder_level2 = _stage(nb[1], 2 * d, hd[1], f, bias, ln)
        self.down2_3 = Downsample(2 * d)
        self.encoder_level3 = _stage(nb[2], 4 * d, hd[2], f, bias, ln)
        self.down3_4 = Downsample(4 * d)
        self.latent = _stage(nb[3], 8 * d, hd[3], f, bias, ln)
        self.up4_3 = Upsample(8 * d)
        self.reduce_chan_level3 = nn.Conv2d(8 * d, 4 * d, kernel_size=1, bias=bias)
        self.decoder_level3 = _stage(nb[2], 4 * d, hd[2], f, bias, ln)
        self.up3_2 = Upsample(4 * d)
        self.reduce_chan_level2 = nn.Conv2d(4 * d, 2 * d, kernel_size=1, bias=bias)
        self.decoder_level2 = _stage(nb[1], 2 * d, hd[1], f, bias, ln)
        self.up2_1 = Upsample(2 * d)
        self.decoder_level1 = _stage(nb[0], 2 * d, hd[0], f, bias, ln)
        self.refinement = _stage(num_refinement_blocks, 2 * d, hd[0], f, bias, ln)
        self.output = nn.Conv2d(2 * d, out_channels, kernel_size=3, padding=1, bias=bias)
        self._engines = {}
        self._train_engines = {}
        self._warned_grad = False

    def engine(self, device: torch.device) -> _Engine:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        eng = self._engines.get(idx)
        if eng is None:
            eng = _Engine(self._c_config(), idx, create="_create_restormer")
            self._engines[idx] = eng
        return eng

    def forward(self, inp_img):
        x = inp_img
        if not torch.is_tensor(x):
            raise RuntimeError("Restormer.forward takes a tensor [B,C,H,W] (KDLAE_teacher takes the dict)")
        if x.device.type != "cuda":
            raise RuntimeError("Restormer (MI355X build) runs on ROCm devices only; move the model inputs to "
                               "'cuda' — there is no CPU fallback")
        if x.dim() != 4 or x.shape[1] != self._cfg["inp_channels"]:
            raise RuntimeError(f"expected x [B,{self._cfg['inp_channels']},H,W], got {tuple(x.shape)}")
        H, W = x.shape[-2:]
        if H % 8 or W % 8:
            raise RuntimeError(f"Restormer needs H and W divisible by 8, got {H}x{W}")
        wants_grad = torch.is_grad_enabled() and any(p.requires_grad for p in self.parameters())
        if wants_grad and not self.training and not self._warned_grad:
            warnings.warn("Restormer in eval mode with grad enabled: the HIP inference path returns outputs "
                          "without an autograd graph; call .train() to differentiate through the model")
            self._warned_grad = True
        if wants_grad and self.training:
            if x.requires_grad and not self._warned_grad:
                warnings.warn("Restormer HIP training path: the input image receives no gradient")
                self._warned_grad = True
            from .train import RestormerTrainEngine, TeacherTrainFn
            eng = self._train_engines.get(x.device.index)
            if eng is None:
                eng = RestormerTrainEngine(self, x.device)
                self._train_engines[x.device.index] = eng
            return TeacherTrainFn.apply(eng, x, None, *self.parameters())
        if self.hip_graphs and not torch.cuda.is_current_stream_capturing():
            return self._forward_graphed(x, None)["hq"]
        return self._forward_eager(x, None)["hq"]

    def forward_tiled(self, inp_img, tile=512, tile_overlap=32, tile_batch=16, window="uniform"):
        """``forward`` over overlapping tiles blended on the device (upstream Restormer's ``--tile`` /
        ``--tile_overlap``; ``KDLAE_teacher.forward_tiled`` states the plan and ``window``): ``[B,C,H,W] -> [B,C,H,W]``."""
        self._check_inference_input(inp_img, "forward_tiled")
        with torch.no_grad():
            return self._forward_tiled(inp_img, None, tile, tile_overlap, tile_batch, window=window)["hq"]

    def forward_ensemble(self, inp_img, modes="d8", ens_batch=8):
        """``forward`` on the dihedral views of the image, turned back and averaged on the device
        (``KDLAE_teacher.forward_ensemble`` states the rule, ``modes`` and ``ens_batch``): ``[B,C,H,W] -> [B,C,H,W]``."""
        self._check_inference_input(inp_img, "forward_ensemble")
        with torch.no_grad():
            return self._forward_ensemble(inp_img, None, modes, ens_batch)["hq"]

    def forward_rates(self, *args, **kwargs):
        raise RuntimeError("Restormer has no denoise_rate input: forward_rates is KDLAE_teacher's")

    def forward_rates_tiled(self, *args, **kwargs):
        raise RuntimeError("Restormer has no denoise_rate input: forward_rates_tiled is KDLAE_teacher's")

    def forward_sr(self, *args, **kwargs):
        raise RuntimeError("Restormer has no sr head: forward_sr is KDLAE_teacher's")


def _conv_block3d(cin, cout, k, pad):
    """KDLAE_student._create_conv_block (KDLAE_model.py:386-393): Conv3d, ReLU, Conv3d, ReLU."""
    return nn.Sequential(nn.Conv3d(cin, cout, kernel_size=k, padding=pad), nn.ReLU(inplace=True),
                         nn.Conv3d(cout, cout, kernel_size=k, padding=pad), nn.ReLU(inplace=True))


class KDLAE_student(nn.Module):
    """KDLAE-S (KDLAE/KDLAE_model.py:340-431): multi-frame 3-D U-Net, forward on the HIP path.

    ``forward(x [B, F, H, W]) -> [B, F, H, W]`` with H and W divisible by 2**(len(hidden_channels)-1).
    """

    def __init__(self, inp_channels=1, out_channels=1, residual=False, hidden_channels=[16, 32, 64], kernel_size=3):
        super().__init__()
        self.residual = residual
        self.num_levels = len(hidden_channels) - 1
        hc = list(hidden_channels)
        pad = kernel_size // 2
        self._cfg = dict(inp_channels=inp_channels, out_channels=out_channels, residual=residual,
                         hidden_channels=hc, kernel_size=kernel_size)
        self.encoders = nn.ModuleList()
        self.pooling_layers = nn.ModuleList()
        cin = inp_channels
        for i in range(self.num_levels):
            self.encoders.append(_conv_block3d(cin, hc[i], kernel_size, pad))
            self.pooling_layers.append(nn.MaxPool3d(kernel_size=(1, 2, 2)))
            cin = hc[i]
        self.st_fusion = _conv_block3d(cin, hc[-1], kernel_size, pad)
        self.upconv_layers = nn.ModuleList()
        self.decoders = nn.ModuleList()
        for i in range(self.num_levels - 1, -1, -1):
            cu = hc[-1] if i == self.num_levels - 1 else hc[i + 1]
            self.upconv_layers.append(nn.ConvTranspose3d(cu, hc[i], kernel_size=(1, 2, 2), stride=(1, 2, 2)))
            self.decoders.append(_conv_block3d(hc[i], hc[i], kernel_size, pad))
        self.out_conv = nn.Conv3d(hc[0], out_channels, kernel_size=(1, 1, 1))
        self._engines = {}
        self._warned_grad = False

    def _c_config(self) -> _lib.SConfig:
        c = self._cfg
        cfg = _lib.SConfig()
        cfg.inp_channels, cfg.out_channels = c["inp_channels"], c["out_channels"]
        cfg.residual = int(bool(c["residual"]))
        if not 2 <= len(c["hidden_channels"]) <= 8:
            raise RuntimeError("KDLAE_student (MI355X build) supports 2..8 hidden_channels entries")
        cfg.num_hidden = len(c["hidden_channels"])
        for i, v in enumerate(c["hidden_channels"]):
            cfg.hidden_channels[i] = int(v)
        cfg.kernel_size = c["kernel_size"]
        return cfg

    def engine(self, device: torch.device) -> _Engine:
        idx = device.index if device.index is not None else torch.cuda.current_device()
        eng = self._engines.get(idx)
        if eng is None:
            eng = _Engine(self._c_config(), idx, "kdlae_s")
            self._engines[idx] = eng
        return eng

    def _check_input(self, x):
        if x.device.type != "cuda":
            raise RuntimeError("KDLAE_student (MI355X build) runs on ROCm devices only; there is no CPU fallback")
        if x.dim() != 4:
            raise RuntimeError(f"expected x [B,F,H,W], got {tuple(x.shape)}")
        H, W = x.shape[-2:]
        m = 1 << self.num_levels
        if H % m or W % m:
            raise RuntimeError(f"KDLAE_student needs H and W divisible by {m}, got {H}x{W}")

    def forward(self, x):
        self._check_input(x)
        if torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.parameters())):
            if self.training and any(p.requires_grad for p in self.parameters()):
                # BasicSR's KDLAE-S training (KDLAES.yml, l_pix.backward()): the HIP training engine
                # behind an autograd node (train.py)
                from .train import StudentTrainEngine, StudentTrainFn
                if x.requires_grad and not self._warned_grad:
                    warnings.warn("KDLAE_student HIP training path: the input frames receive no gradient")
                    self._warned_grad = True
                eng = self.__dict__.setdefault("_train_engines", {}).get(x.device.index)
                if eng is None:
                    eng = StudentTrainEngine(self, x.device)
                    self._train_engines[x.device.index] = eng
                return StudentTrainFn.apply(eng, x, *self.parameters())
            if not self._warned_grad:
                warnings.warn("KDLAE_student in eval mode with grad enabled: the HIP inference path returns "
                              "outputs without an autograd graph")
                self._warned_grad = True
        return self._forward_eager(x)

    def forward_clip(self, x, frames=7, overlap=2, window_batch=8, window="uniform"):
        """``forward`` for a clip of any length: ``x [B,T,H,W] -> [B,T,H,W]`` through overlapping windows of
        ``frames`` consecutive frames (the network was trained at 7), ``overlap`` frames shared by neighbours, every
        frame the plain mean of its windows' outputs (clips.py and include/kdlae.h state the plan and the sum
        order).  Windows are gathered on the device ``window_batch`` at a time and go through this module's own
        inference forward; the outputs land in a staging tensor in window order and one blend launch writes the
        result.

        Each window's rows are bit for bit what ``forward`` gives for that window alone at batch 1, for every
        ``window_batch``, so the result equals the host loop (slice, forward, ``E[:, s:s+f].add_(y)``,
        ``W[s:s+f].add_(1)``, ``E.div_(W)``) bit for bit; ``T <= frames`` is one window and equals ``forward(x)``.
        The 3-D convolutions zero-pad along the frame axis, so with more than one window the result is a different
        function of the clip from ``forward`` over all T frames, not an approximation of it that carries a bound.
        Inference only (no autograd graph).

        ``window``: ``"uniform"`` (the plain mean, the default), ``"ramp"``, ``"hann"`` or a table of ``f`` weights
        (``clips.clip_window``): a weighted mean whose weights fall towards the window's ends, where the zero
        padding is felt, so that neighbouring windows cross-fade over their overlap; a frame under one window
        keeps that window's value bit for bit."""
        from . import clips
        self._check_input(x)
        B, T, H, W = x.shape
        if int(window_batch) < 1:
            raise RuntimeError(f"window_batch must be at least 1, got {window_batch}")
        plan = clips.clip_plan(T, frames, overlap)   # refuses a bad T / frames / overlap before any launch
        with torch.no_grad():
            # the blend table, once per call and before the staging is allocated: a bad window is refused here
            table = clips.clip_window(window, T, frames, overlap, x.device)
            return clips.clip_blend(self._clip_windows(x, plan, frames, overlap, window_batch), B, T, frames, overlap,
                                    table)

    def _clip_windows(self, x, plan, frames, overlap, window_batch):
        """Every window of ``x``'s plan through ``_forward_eager`` -> the outputs [B n, f, H, W] in window order."""
        from . import clips
        B, _, H, W = x.shape
        x_c = x.detach().to(torch.float32).contiguous()
        n = B * plan.n
        staged = torch.empty((n, plan.f, H, W), device=x.device, dtype=torch.float32)
        for first in range(0, n, int(window_batch)):
            count = min(int(window_batch), n - first)
            self._forward_eager(clips.clip_gather(x_c, frames, overlap, first, count),
                                out=staged[first:first + count])
        return staged

    def forward_ensemble(self, x, modes="d8", ens_batch=8):
        """Geometric self-ensemble of ``forward``: ``x [B,F,H,W] -> [B,F,H,W]``, the frames being the channel axis
        of the views (every frame of a window is flipped and turned alike).  The views are gathered with one
        launch, go through this module's own inference forward ``ens_batch`` views of the whole batch at a time
        (runs of consecutive views of one shape) into a staging tensor, and one merge launch writes the mean
        (ensemble.py and include/kdlae_ensemble.h state the modes, the sum order and the layout).

        Bit for bit the host loop (``torch.rot90`` / ``torch.flip``, ``forward``, the inverse, ``E.add_`` in
        ascending mode order, one ``E.div_``) for every ``ens_batch``; ``modes=(0,)`` equals ``forward``.  A
        different function of the frames from ``forward``, not an approximation of it that carries a bound.
        Inference only (eval mode, no autograd graph)."""
        from . import ensemble
        if self.training:
            raise RuntimeError("KDLAE_student.forward_ensemble is inference-only: call .eval() first")
        self._check_input(x)
        B, Fr, H, W = x.shape
        mask = ensemble.mode_mask(modes)
        ensemble.ens_chunks(mask, H, W, ens_batch)     # refuses a bad ens_batch before any launch
        with torch.no_grad():
            g_x = ensemble.ens_gather(x.detach().to(torch.float32), mask)
            staged, = ensemble.run_views(lambda ins, outs: self._forward_eager(ins[0], out=outs[0]), mask, B, H, W,
                                         ens_batch, [(g_x, Fr)], [Fr], [1])
            return ensemble.ens_merge(staged, B, H, W, mask)

    def stream(self, batch, h, w, frames=7, emit=None, channels=1, multiple=32, dtype="u8"):
        """A ``streams.StudentStream`` on this module: frames of ``batch`` parallel sources pushed one at a time,
        every frame returned enhanced from the window in which it sits at position ``emit`` (streams.py states the
        rule and the schedule), the steady state replayed as one HIP graph."""
        from .streams import StudentStream
        return StudentStream(self, batch, h, w, frames, emit, channels, multiple, dtype)

    def _forward_eager(self, x, flat=None, out=None):
        """``flat``: run with this packed parameter vector (``_Engine.pack_flat``) instead of the module's own.
        ``out``: a contiguous fp32 destination of the output's shape to write into instead of a fresh tensor: how
        ``forward_clip`` fills its staging."""
        B, Fr, H, W = x.shape
        dev = x.device
        stream = torch.cuda.current_stream(dev).cuda_stream
        eng = self.engine(dev)
        if flat is None:
            eng.sync_params(self, stream)
        else:
            eng.pack_flat(flat, stream)
        x_c = x.detach().to(torch.float32).contiguous()
        if out is None:
            out = torch.empty((B, Fr, H, W), device=dev, dtype=torch.float32)
        L = _lib.lib()
        nbytes = L.kdlae_s_workspace_bytes(eng.handle, B, Fr, H, W)
        if nbytes < 0:
            _lib.check(1, "kdlae_s_workspace_bytes")
        ws = eng.workspace(nbytes, dev)
        rc = L.kdlae_s_forward(eng.handle, ctypes.c_void_p(x_c.data_ptr()), B, Fr, H, W,
                               ctypes.c_void_p(out.data_ptr()), ctypes.c_void_p(ws.data_ptr()), ws.numel(),
                               ctypes.c_void_p(stream))
        _lib.check(rc, "kdlae_s_forward")
        return out

"""Shared helpers for the test suite (fixtures -> configs, hash weights -> modules)."""
import json
import os

import numpy as np
import torch

from rethink_acoustic_image_enhancement_amd.hashweights import hash_state_dict

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def load_fixture(name):
    d = np.load(os.path.join(GOLDEN, name + ".npz"), allow_pickle=False)
    cfg = json.loads(bytes(d["cfg"]).decode())
    return d, cfg


def hash_sd_for(shapes: dict) -> dict:
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in hash_state_dict(shapes).items()}


def mdd_input_tensor(d):
    """Rebuild the config-1 input [1,3,512,512] from the committed uint8 crop."""
    crop = d["crop_u8"]
    if crop.ndim == 2:
        crop = np.repeat(crop[..., None], 3, axis=2)
    t = torch.from_numpy(crop.astype(np.float32) / 255.0).permute(2, 0, 1).unsqueeze(0)
    return torch.nn.functional.pad(t, (0, 512 - t.shape[-1], 0, 0), mode="reflect")


def max_abs(a, b):
    return float((a.double() - b.double()).abs().max())


FAKE = 4096  # a non-null, 16-byte aligned "device pointer" for entries that must fail before they touch it


def failed(rc, code, text):
    """An entry point that refused: its KDLAE_E* code and the text it left in kdlae_last_error."""
    from rethink_acoustic_image_enhancement_amd import _lib
    assert (rc, _lib.last_error()) == (code, text), (rc, _lib.last_error())


def silent(call, want):
    """An entry point that answers `want` without touching kdlae_last_error."""
    from rethink_acoustic_image_enhancement_amd import _lib
    failed(_lib.lib().kdlae_train_ema(None, None, 0, 0.0, None), 2, "bad argument")
    assert call() == want
    assert _lib.last_error() == "bad argument"

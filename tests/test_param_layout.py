"""One state_dict key list per model: the inference handle and the training handle of KDLAE-T, KDLAE-S and
ASDQE enumerate the same keys in the same order (csrc/param_layout.cpp), the inference layout packed back
to back and the training layout with every key rounded up to 4 floats.  No call here touches the GPU."""
import ctypes

import pytest

from rethink_acoustic_image_enhancement_amd import _lib
from rethink_acoustic_image_enhancement_amd.ASDQE_model import DenoiseRatePredictor
from rethink_acoustic_image_enhancement_amd.KDLAE_model import KDLAE_student, KDLAE_teacher

# model -> (module class, inference prefix, training prefix, the configs the ABI / training-layout tests use)
MODELS = {
    "teacher": (KDLAE_teacher, "kdlae_t", "kdlae_tt", [
        dict(LayerNorm_type="BiasFree"), dict(), dict(bias=True, static="no", params="plus"),
        dict(dim=16, inp_channels=1, out_channels=1, num_blocks=[1, 2, 1, 1]),
        dict(dim=16, num_blocks=[1, 2, 1, 1], num_refinement_blocks=1, LayerNorm_type="WithBias", bias=True),
        dict(dim=16, num_blocks=[1, 1, 1, 1], num_refinement_blocks=1, static="no", params="plus")]),
    "student": (KDLAE_student, "kdlae_s", "kdlae_st", [
        dict(), dict(hidden_channels=[8, 16, 16, 32], residual=True), dict(hidden_channels=[32, 64]),
        dict(hidden_channels=[16, 32, 64], residual=True)]),
    "asdqe": (DenoiseRatePredictor, "asdqe", "asdqe_train", [
        dict(), dict(in_channels=1, dim=32), dict(in_channels=2), dict(in_channels=4)]),
}
CASES = [(model, i) for model, spec in MODELS.items() for i in range(len(spec[3]))]
BUFFERS = (".running_mean", ".running_var", ".num_batches_tracked")


def enumerate_handle(prefix, cfg):
    """[(name, numel, offset)], total floats and the open handle's extra figures of one ``prefix`` handle.
    The inference ABI reports no offsets (its flat vector is the keys back to back): offset is None there."""
    L = _lib.lib()
    train = prefix in ("kdlae_tt", "kdlae_st", "asdqe_train")
    h = ctypes.c_void_p()
    _lib.check(getattr(L, prefix + "_create")(ctypes.byref(cfg), 0, ctypes.byref(h)), prefix + "_create")
    try:
        keys = []
        for i in range(getattr(L, prefix + "_num_params")(h)):
            name, numel, off = ctypes.c_char_p(), ctypes.c_int64(), ctypes.c_int64()
            args = [h, i, ctypes.byref(name), ctypes.byref(numel)] + ([ctypes.byref(off)] if train else [])
            _lib.check(getattr(L, prefix + "_param_info")(*args), prefix + "_param_info")
            keys.append((name.value.decode(), int(numel.value), int(off.value) if train else None))
        total = int(getattr(L, prefix + ("_num_floats" if train else "_params_numel"))(h))
        nstat = int(L.asdqe_train_num_stat_floats(h)) if prefix == "asdqe_train" else None
        return keys, total, nstat
    finally:
        getattr(L, prefix + "_destroy")(h)


@pytest.mark.parametrize("model,i", CASES)
def test_inference_and_training_handles_share_one_key_list(model, i):
    cls, infer, train, kws = MODELS[model]
    cfg = cls(**kws[i])._c_config()
    ikeys, itotal, _ = enumerate_handle(infer, cfg)
    tkeys, ttotal, nstat = enumerate_handle(train, cfg)
    # the training handle holds the parameters; only ASDQE has buffers (BatchNorm statistics) to leave out
    params = [(k, n) for k, n, _ in ikeys if not k.endswith(BUFFERS)]
    assert len(params) == len(ikeys) or model == "asdqe"
    assert [(k, n) for k, n, _ in tkeys] == params
    # inference: back to back; training: each key rounded up to 4 floats (16-byte aligned, pads zero)
    assert itotal == sum(n for _, n, _ in ikeys)
    end = 0
    for k, n, off in tkeys:
        assert off == end, k
        end += (n + 3) // 4 * 4
    assert ttotal == end
    if model == "asdqe":
        assert nstat == sum(n for k, n, _ in ikeys if k.endswith(BUFFERS[:2]))
        assert nstat > 0

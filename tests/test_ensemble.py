"""The self-ensemble rule (include/kdlae_ensemble.h) on the CPU: the numpy model of tests/ensemble_model.py against
the dataset's augmentation model, the mistakes a hand-written loop makes, the Python helpers, and the header against
the binding.  No GPU."""
import os
import re

import numpy as np
import pytest

from rethink_acoustic_image_enhancement_amd import _lib, ensemble
from tests import ensemble_model as em
from tests.dataset_oracle import data_augmentation_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_MASKS = range(1, 256)


def _rng_img(shape, seed=0):
    return np.random.default_rng(seed).uniform(-1.0, 1.0, shape).astype(np.float32)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.int32)


@pytest.mark.parametrize("m", em.MODES)
def test_transform_is_the_datasets_augmentation(m):
    x = np.arange(15, dtype=np.float32).reshape(3, 5)
    want = data_augmentation_model(x, m)
    assert np.array_equal(em.transform(x, m), want)
    assert want.shape == em.view_shape(m, 3, 5) == ensemble.view_shape(m, 3, 5)
    assert ensemble.transposes(m) == (want.shape == (5, 3))
    # on a batch the last two axes are the image
    xb = _rng_img((2, 3, 3, 5))
    got = em.transform(xb, m)
    for n in range(2):
        for c in range(3):
            assert np.array_equal(got[n, c], data_augmentation_model(xb[n, c], m))


@pytest.mark.parametrize("m", em.MODES)
def test_inverse_undoes_the_transform(m):
    x = _rng_img((2, 1, 3, 5))
    assert np.array_equal(em.inverse(em.transform(x, m), m), x)
    assert np.array_equal(em.transform(em.inverse(em.transform(x, m), m), m), em.transform(x, m))


@pytest.mark.parametrize("hw", [(3, 5), (4, 4), (1, 7)])
def test_single_mode_round_trip_is_the_identity(hw):
    x = _rng_img((2, 3) + hw, 1)
    for m in em.MODES:
        mask = 1 << m
        buf = em.gather(x, mask)
        assert buf.shape == (x.size,)
        assert np.array_equal(_bits(em.merge(buf, 2, 3, *hw, mask)), _bits(x)), m


def test_slot_layout():
    N, C, H, W = 2, 3, 3, 5
    x = _rng_img((N, C, H, W), 2)
    mask = em.mask_of((1, 2, 7))
    buf = em.gather(x, mask)
    per = N * C * H * W
    assert buf.shape == (3 * per,)
    for s, m in enumerate((1, 2, 7)):
        want = np.stack([np.stack([data_augmentation_model(x[n, c], m) for c in range(C)]) for n in range(N)])
        assert np.array_equal(buf[s * per:(s + 1) * per].reshape(want.shape), want)
    assert [v.shape for v in em.views(buf, N, C, H, W, mask)] == [(N, C, H, W), (N, C, W, H), (N, C, W, H)]


def test_a_constant_image_merges_to_itself_for_every_mask():
    c = np.float32(0.3)   # k * 0.3 / k is not exact in general: the check is against the rule's own arithmetic
    for hw in ((3, 5), (4, 4)):
        x = np.full((1, 2) + hw, c, np.float32)
        for mask in ALL_MASKS:
            k = len(em.modes_of(mask))
            acc = np.float32(0)
            for _ in range(k):
                acc = np.float32(acc + c)
            want = np.float32(acc / np.float32(k))
            got = em.merge(em.gather(x, mask), 1, 2, *hw, mask)
            assert got.shape == x.shape and np.all(_bits(got) == _bits(want)), mask
    ones = np.ones((1, 1, 3, 5), np.float32)    # exactly representable sums: itself, bit for bit
    for mask in ALL_MASKS:
        assert np.array_equal(_bits(em.merge(em.gather(ones, mask), 1, 1, 3, 5, mask)), _bits(ones))


def _model(img, rate):
    """A stand-in network that is not equivariant under any flip or rotation: a ramp along both axes enters."""
    h, w = img.shape[-2:]
    ramp = (np.arange(h, dtype=np.float32)[:, None] * np.float32(0.5) + np.arange(w, dtype=np.float32)[None, :])
    return (img * rate + ramp * np.float32(0.125)).astype(np.float32)


def test_planted_mistakes_change_the_answer():
    mask = em.mask_of("d8")
    x, rate = _rng_img((1, 2, 4, 4), 3), _rng_img((1, 1, 4, 4), 4) + np.float32(1.5)
    right = em.ensemble(_model, x, rate, mask)
    assert np.array_equal(_bits(right), _bits(em.ensemble(_model, x, rate, mask)))
    wrong_inverse = em.ensemble(_model, x, rate, mask, inverse_fn=em.inverse_wrong_way)
    assert not np.array_equal(_bits(wrong_inverse), _bits(right))
    flip_first = em.ensemble(_model, x, rate, mask, transform_fn=em.transform_flip_first)
    assert not np.array_equal(_bits(flip_first), _bits(right))
    rate_as_it_came = em.ensemble(_model, x, rate, mask, transform_rate=False)
    assert not np.array_equal(_bits(rate_as_it_came), _bits(right))
    # the same on H != W for the two mistakes that can run there
    xr, rr = _rng_img((1, 2, 3, 5), 5), _rng_img((1, 1, 3, 5), 6) + np.float32(1.5)
    right_r = em.ensemble(_model, xr, rr, mask)
    assert not np.array_equal(_bits(em.ensemble(_model, xr, rr, mask, transform_fn=em.transform_flip_first)),
                              _bits(right_r))
    # the wrong-way inverse of a transposing mode still has the right shape, and the wrong content
    one = em.mask_of((2,))
    assert not np.array_equal(em.merge(em.gather(xr, one), 1, 2, 3, 5, one, inverse_fn=em.inverse_wrong_way), xr)


def test_planted_sum_order_and_divisor():
    mask, buf = em.planted_sum_order(1, 1, 3, 5)
    asc = em.merge(buf, 1, 1, 3, 5, mask)
    desc = em.merge(buf, 1, 1, 3, 5, mask, order="descending")
    assert np.all(_bits(asc) == _bits(np.float32(0.0)))
    assert np.all(_bits(desc) == _bits(np.float32(1.0) / np.float32(3.0)))
    # the divisor is the number of modes, not 8
    x = _rng_img((1, 1, 3, 5), 7)
    m3 = em.mask_of((0, 1, 5))
    by3 = em.merge(em.gather(x, m3), 1, 1, 3, 5, m3)
    by8 = em.merge(em.gather(x, m3), 1, 1, 3, 5, m3, divisor=8)
    assert not np.array_equal(_bits(by3), _bits(by8))


# ------------------------------------------------------------------ the Python helpers
def test_mode_mask_and_chunks():
    assert ensemble.MODES == em.MODES
    assert ensemble.mode_mask("d8") == 255 == em.mask_of("d8")
    assert ensemble.mode_mask("flips") == 0b00110011 == em.mask_of("flips")
    assert ensemble.mode_mask([7, 2, 5, 2]) == em.mask_of((2, 5, 7))
    assert ensemble.mask_modes(0b10100100) == [2, 5, 7] == em.modes_of(0b10100100)
    for bad in ("d4", [], [8], [-1], [1.0], [True], 3, None):
        with pytest.raises(RuntimeError):
            ensemble.mode_mask(bad)
    for bad in (0, 256, -1):
        with pytest.raises(RuntimeError):
            ensemble.mask_modes(bad)
    with pytest.raises(RuntimeError, match="ens_batch"):
        ensemble.ens_chunks(255, 8, 8, 0)
    for mask in (255, 0b00110011, 0b10100100, 1, 0b11001100):
        for hw in ((24, 40), (16, 16)):
            for eb in (1, 2, 3, 8, 16):
                got = ensemble.ens_chunks(mask, *hw, eb)
                assert got == em.chunks(mask, *hw, eb)
                modes = em.modes_of(mask)
                assert [s for s, _, _ in got] == [sum(n for _, n, _ in got[:i]) for i in range(len(got))]
                assert sum(n for _, n, _ in got) == len(modes)
                for s, n, shape in got:
                    assert 1 <= n <= eb
                    assert all(em.view_shape(m, *hw) == shape for m in modes[s:s + n])
    # a square image: one run of all eight; H != W: the shapes alternate in pairs
    assert ensemble.ens_chunks(255, 16, 16, 8) == [(0, 8, (16, 16))]
    assert ensemble.ens_chunks(255, 24, 40, 8) == [(0, 2, (24, 40)), (2, 2, (40, 24)), (4, 2, (24, 40)),
                                                    (6, 2, (40, 24))]
    assert ensemble.ens_chunks(255, 16, 16, 3) == [(0, 3, (16, 16)), (3, 3, (16, 16)), (6, 2, (16, 16))]


# ------------------------------------------------------------------ header and binding
def _declared(path):
    text = open(path).read()
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    return sorted(set(re.findall(r"\b((?:kdlae|asdqe)_\w+)\s*\(", text)))


def test_header_binding_and_library_agree():
    names = _declared(os.path.join(ROOT, "include", "kdlae_ensemble.h"))
    assert names == sorted(_lib.ENSEMBLE_EXPORTS) and len(names) == 2
    L = _lib.lib()
    for name in names:
        fn = getattr(L, name)            # AttributeError if the library does not export it
        assert len(fn.argtypes) == 8 and fn.restype is _lib.c_int
    main = open(os.path.join(ROOT, "include", "kdlae.h")).read()
    for name in names:
        assert name not in main          # not even in a comment: tests/test_abi.py reads that header whole
        assert name not in _lib.EXPORTS
    assert L.kdlae_abi_version() == 1


def test_argument_refusals_need_no_device():
    """Every refusal comes before the launch: EINVAL_SHAPE (1) and a message, with pointers never dereferenced."""
    L = _lib.lib()
    P = 0x1000
    for name in _lib.ENSEMBLE_EXPORTS:
        fn = getattr(L, name)
        for args in ((None, P, 1, 1, 4, 4, 255), (P, None, 1, 1, 4, 4, 255), (P, P, 0, 1, 4, 4, 255),
                     (P, P, 1, -1, 4, 4, 255), (P, P, 1, 1, 0, 4, 255), (P, P, 1, 1, 4, 0, 255),
                     (P, P, 1, 1, 4, 4, 0), (P, P, 1, 1, 4, 4, 256), (P, P, 1, 1, 4, 4, -1)):
            assert fn(*args, None) == 1, (name, args)
            assert name in _lib.last_error()

"""The refusals of the six per-plane goal-map analytics (csrc/map_plane.h, and the call-side helpers of ops.py), word for word: what
ynet_last_error() says after a bad call of each C entry point, and what the Python wrappers raise on host tensors.  The entries share
their checks; this pins every message, and which of several faults is reported, against the next change to the shared part."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import pkg

P = ctypes.c_void_p(4096)      # (never dereferenced: every call below is refused before anything is launched)
LEVELS = (ctypes.c_float * 2)(0.5, 0.9)
TEMP = "the temperature and its reciprocal must be positive and finite"


def _entries(lib):
    """name -> a call of the entry point with legal arguments (2 images of 3 planes of 4x4, batch stride 48), each replaceable by keyword"""
    def temps(T):
        return (ctypes.c_float * 2)(1.0, T)

    def likelihood(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_likelihood(x, bs, P, B, Cn, H, W, T, P, P, P, P, None)

    def sweep(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_likelihood_sweep(x, bs, P, B, Cn, H, W, temps(T), 2, P, P, P, None)

    def class_mass(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_class_mass(x, bs, P, 0, B, Cn, H, W, 6, T, P, None)

    def credible(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_credible(x, bs, B, Cn, H, W, LEVELS, 2, T, P, P, P, P, None)

    def occupancy(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_occupancy(x, bs, P, B, 1, Cn, H, W, 2, T, P, P, P, P, P, P, None)

    def modes(x=P, bs=48, B=2, Cn=3, H=4, W=4, T=1.0):
        return lib.ynet_map_modes(x, bs, B, Cn, H, W, 3, 2, T, P, P, P, P, P, None)

    return {"map_likelihood": likelihood, "map_likelihood_sweep": sweep, "map_class_mass": class_mass, "map_credible": credible,
            "map_occupancy": occupancy, "map_modes": modes}


# per entry: what differs from the common wording -- the null map, the temperature, H = 0, and the plane-count overflow with its call
OWN = {
    "map_likelihood": ("null map", TEMP, "bad shape B=2 C=3 0x4", dict(B=1 << 31, Cn=1, bs=16), "too many planes"),
    "map_likelihood_sweep": ("null map", "temperature 1: it and its reciprocal must be positive and finite", "bad shape B=2 C=3 0x4",
                             dict(B=1 << 31, Cn=1, bs=16), "too many planes"),
    "map_class_mass": ("null map", TEMP, "bad shape B=2 C=3 0x4", dict(bs=4, B=1 << 29, Cn=4, H=1, W=1), "too many planes"),
    "map_credible": ("null map", TEMP, "bad shape B=2 C=3 0x4", dict(bs=4, B=1 << 20, Cn=4, H=1, W=1),
                     "too many planes (1048576 x 4, at most 4194303)"),
    "map_occupancy": ("null map", TEMP, "bad shape B=2 C=3 0x4 G=1", dict(bs=4, B=1 << 29, Cn=4, H=1, W=1), "too many planes"),
    "map_modes": ("null map, xy, logit, count or status", "with mass, " + TEMP, "bad shape B=2 C=3 0x4", dict(bs=16, B=1 << 22, Cn=1),
                  "more than 4194303 planes"),
}


@pytest.mark.parametrize("name", list(OWN))
def test_c_entry_refusals_word_for_word(name):
    lib = pkg("_lib").load()
    call = _entries(lib)[name]
    null, temp, shape, overflow_call, overflow = OWN[name]

    def refused(**kw):
        assert call(**kw) != 0, kw
        return lib.ynet_last_error().decode()

    assert refused(x=None) == f"{name}: {null}"
    for T in (0.0, float("inf"), 1e-39):      # (1e-39: positive and finite, its reciprocal is not)
        assert refused(T=T) == f"{name}: {temp}", T
    assert refused(H=0) == f"{name}: {shape}"
    assert refused(bs=47) == f"{name}: batch stride 47 below the 3 planes of 4x4 of an image"
    assert refused(**overflow_call) == f"{name}: {overflow}"
    # several faults at once: the one reported is the first of the entry's own order
    first = shape if name == "map_modes" else temp
    assert refused(T=0.0, H=0, bs=47) == f"{name}: {first}"
    assert refused(H=0, bs=-1) == f"{name}: {shape}"


class _OnDevice(torch.Tensor):
    """A host tensor that says it lives on the device: what the wrappers look at before they refuse it."""
    is_cuda = property(lambda self: True)


def test_wrapper_refusals_word_for_word():
    ops = pkg("ops")
    x, gt = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2)

    def message(exc, f, *args, **kw):
        with pytest.raises(exc) as e:
            f(*args, **kw)
        return str(e.value)

    # the selection of outputs, refused before the map is looked at
    assert message(ValueError, ops.map_likelihood, x, None, want=("variance",)) == \
        "map_likelihood: want ('variance',): a non-empty selection of ('nll', 'entropy', 'hpd') is expected"
    assert message(ValueError, ops.map_likelihood, x, None, want=()) == \
        "map_likelihood: want (): a non-empty selection of ('nll', 'entropy', 'hpd') is expected"
    assert message(ValueError, ops.map_likelihood_sweep, x, gt, [1.0], want=("nll", "nll")) == \
        "map_likelihood_sweep: want ('nll', 'nll'): a non-empty selection of ('nll', 'hpd') is expected"
    assert message(ValueError, ops.map_occupancy, x, want=("mass",)) == \
        "map_occupancy: want ('mass',): a selection of ('occupancy', 'any', 'conflict', 'risk') is expected"
    # map_occupancy: want, then cell, then the temperature, then the device
    assert message(ValueError, ops.map_occupancy, x, cell=3, temperature=0.0, want=("mass",)).startswith("map_occupancy: want")
    assert message(ValueError, ops.map_occupancy, x, cell=3, temperature=0.0) == "map_occupancy: cell = 3, expected one of (1, 2, 4, 8)"
    assert message(ValueError, ops.map_occupancy, x, temperature=0.0) == "map_occupancy: temperature 0.0 must be positive and finite"
    assert message(ValueError, ops.map_occupancy, x, temperature=float("inf"), want=()) == \
        "map_occupancy: temperature inf must be positive and finite"
    assert message(RuntimeError, ops.map_occupancy, x, want=()).startswith("map_occupancy: tensor is on cpu; the MI355X path runs on HIP devices only")
    # the other wrappers look at the map first
    for f, args in ((ops.map_likelihood, (x, None)), (ops.map_class_mass, (x, torch.zeros(4, 4, dtype=torch.uint8), 6)),
                    (ops.map_credible, (x, [0.5])), (ops.map_modes, (x, 3, 2))):
        assert "HIP devices only" in message(RuntimeError, f, *args, temperature=0.0)
    # host sequences
    dev = torch.ones(2).as_subclass(_OnDevice)
    tail = " are read on the host at call time; pass a host sequence, not a device tensor"
    assert message(TypeError, ops.sweep_temperatures, dev) == "map_likelihood_sweep: the temperatures" + tail
    assert message(TypeError, ops.credible_levels, dev) == "map_credible: the levels" + tail
    assert message(TypeError, ops.occupancy_offsets, dev, 2) == "map_occupancy: the group sizes" + tail
    assert message(TypeError, ops.credible_levels, dev, "predict") == "predict: the levels" + tail
    assert message(TypeError, ops.map_likelihood_sweep, x, gt, dev) == "map_likelihood_sweep: the temperatures" + tail
    assert message(TypeError, ops.map_credible, x, dev) == "map_credible: the levels" + tail
    assert message(ValueError, ops.sweep_temperatures, [1.0, 0.0]) == \
        f"map_likelihood_sweep: temperature {np.float64(0.0)!r} (entry 1) must be positive and finite in fp32"      # (NumPy's own repr)
    assert ops.sweep_temperatures(torch.tensor([1.0, 0.5])).tolist() == [1.0, 0.5]      # a host tensor is a host sequence
    assert ops.occupancy_offsets(torch.tensor([2, 0, 1]), 3).tolist() == [0, 2, 2, 3]
    # nothing was launched: nothing to report, by any of the checks
    assert ops.check_likelihood_status() is False and ops.check_credible_status() is False
    assert ops.check_occupancy_status() is False and ops.check_modes_status() is False
    assert ops.check_patch_status() is None and ops.check_gather_status() is None

"""forward_test / saliency without a GPU: the reference's signatures (names recorded in tests/golden/forward_test_signatures.json),
the new C-ABI symbols and their argument checks, host tensors refused, saliency()'s argument validation."""
import ctypes
import inspect
import json
import os

import pytest
import torch

from conftest import GOLDEN, pkg


def test_signatures_match_the_reference():
    trn = pkg("models.trainer")
    with open(os.path.join(GOLDEN, "forward_test_signatures.json")) as f:
        want = json.load(f)
    for name, params in want.items():
        assert list(inspect.signature(getattr(trn.YNetTrainer, name)).parameters) == params, name
    sig = inspect.signature(trn.YNetTrainer._forward_batch).parameters
    assert sig["set_input"].default is None and sig["noisy_std_frac"].default is None and sig["return_pred_map"].default is False


def test_new_symbols_exported_and_validated():
    L = pkg("_lib")
    lib = L.load()
    for n in ("ynet_input_grad", "ynet_input_grad_supported", "ynet_input_grad_workspace_floats", "ynet_avgpool_pyramid_bwd",
              "ynet_add_range_noise", "ynet_range_noise_workspace_floats"):
        assert hasattr(ctypes.CDLL(L.LIB_PATH), n) and n in L.header_symbols() and n in L.SIGNATURES
    ok = lib.ynet_input_grad_supported
    assert ok(32, 256, 256, 32, 6, 8) and ok(16, 512, 512, 16, 6, 0) and ok(16, 512, 512, 16, 0, 5) and ok(1, 32, 64, 8, 16, 8)
    assert not ok(32, 250, 256, 32, 6, 8) and not ok(32, 256, 256, 48, 6, 8) and not ok(32, 256, 256, 32, 7, 8) and not ok(2, 64, 64, 32, 0, 0)
    assert lib.ynet_input_grad_workspace_floats(4, 64, 64, 6) == 0 and lib.ynet_input_grad_workspace_floats(32, 64, 64, 6) == 8 * 6 * 64 * 64
    vp = ctypes.c_void_p
    assert lib.ynet_input_grad(vp(256), None, vp(256), None, vp(256), None, 2, 64, 64, 32, 7, 8, None) != 0
    assert b"not served" in lib.ynet_last_error()
    assert lib.ynet_input_grad(vp(256), None, vp(256), None, None, None, 2, 64, 64, 32, 6, 8, None) != 0
    assert b"no destination" in lib.ynet_last_error()
    assert lib.ynet_input_grad(vp(256), None, vp(256), vp(256), None, None, 32, 64, 64, 32, 6, 8, None) != 0
    assert b"workspace" in lib.ynet_last_error()
    assert lib.ynet_add_range_noise(vp(256), vp(256), 16, -1.0, 0, vp(256), None) != 0 and b"frac" in lib.ynet_last_error()
    assert lib.ynet_range_noise_workspace_floats() > 0
    assert lib.ynet_avgpool_pyramid_bwd(None, 2, vp(256), 1, 64, 64, None) != 0


def test_new_ops_refuse_host_tensors():
    ops = pkg("ops")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.input_grad(torch.zeros(1, 32, 32, 32), torch.zeros(10), 6, 8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.add_range_noise(torch.zeros(1, 6, 32, 32), 0.1, 0)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.avgpool_pyramid_grad(torch.zeros(1, 1, 32, 32), 3)


def test_saliency_validates_its_arguments():
    trn = pkg("models.trainer")
    t = trn.YNetTrainer.__new__(trn.YNetTrainer)      # (validation happens before any model or data is touched)
    t.params = {}
    with pytest.raises(ValueError, match="target"):
        t.saliency(None, None, target="all")
    for bad in ("scene", (), ("scene", "depth"), ("traj", "traj"), ("scene", "semantic")):
        with pytest.raises(ValueError, match="set_input|exclude"):
            t.saliency(None, None, set_input=bad)

"""Likelihood scores of the goal map (ynet_map_likelihood, ops.map_likelihood, utils/likelihood.py, evaluate(return_likelihood=True)) --
everything that needs no GPU: the case table of tests/_likelihood_cases.py is self-consistent, the calibration curve on planted inputs,
the C entry point's refusals, and the signatures."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import _likelihood_cases as C
from conftest import pkg


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error(si):
    (H, W), _, recorded = C.SHAPES[si]
    measured = {k: 0.0 for k in C.OUTPUTS}
    for kind in range(len(C.KINDS)):
        x, gt, T, ref = C.case(si, kind)
        assert all(bool(torch.isfinite(ref[k]).all()) for k in C.OUTPUTS), (H, W, kind)
        for k, v in C.e32(x, gt, T).items():
            measured[k] = max(measured[k], v)
    print(f"{H}x{W}: E32 measured {measured}, recorded {recorded}")
    # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and the
    # vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two below.
    for k in C.OUTPUTS:
        assert measured[k] <= 1.25 * recorded[k] and recorded[k] <= 2.0 * measured[k] + 1e-12, (k, measured[k], recorded[k])


def test_ground_truth_visits_every_position_and_rounds_half_even():
    for si, ((H, W), _, _) in enumerate(C.SHAPES):
        pos = C.positions(H, W)
        hit = set()
        for kind in range(len(C.KINDS)):
            gt = C.ground_truth(H, W, kind)
            g = torch.round(gt.double())
            for p in range(C.B * C.C):
                want = pos[(p + 3 * kind) % len(pos)][1]
                assert (int(g[p // C.C, p % C.C, 0]), int(g[p // C.C, p % C.C, 1])) == want
                hit.add(want)
        assert hit == {px for _, px in pos}, (H, W)
    assert ((2.5, 2.5), (2, 2)) in C.positions(96, 160) and ((3.5, 3.5), (4, 4)) in C.positions(96, 160)


def test_fp64_restatement_reproduces_the_closed_forms():
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        x, gt, T, want = C.constant_plane(H, W)
        got = C.like_ref(x, gt, T)
        assert abs(float(got["nll"]) - want["nll"]) <= 1e-12 and abs(float(got["entropy"]) - want["entropy"]) <= 1e-12
        assert float(got["hpd"]) == 1.0
        if H * W < 2:
            continue
        x, gt, T, want = C.spike_planes(H, W)
        got = C.like_ref(x, gt, T)
        for k in C.OUTPUTS:
            np.testing.assert_allclose(got[k][0].numpy(), np.array(want[k]), rtol=0, atol=1e-12, err_msg=f"{k} {H}x{W}")
        assert float(got["hpd"][0, 1]) == 1.0


def test_membership_by_logits_is_membership_by_fp64_probabilities():
    for si in range(len(C.SHAPES) - 1):          # (the 512 x 512 planes add nothing here)
        for kind in range(len(C.KINDS)):
            x, gt, T, _ = C.case(si, kind)
            Bn, Cn, H, W = x.shape
            p = torch.sigmoid(x.double() / T)
            p = p / p.sum(dim=(2, 3), keepdim=True)
            g = torch.round(gt.double()).long()
            for b in range(Bn):
                for c in range(Cn):
                    xg, pg = x[b, c, g[b, c, 1], g[b, c, 0]], p[b, c, g[b, c, 1], g[b, c, 0]]
                    by_logit, by_prob = x[b, c] >= xg, p[b, c] >= pg
                    distinct = (p[b, c] != pg) | (x[b, c] == xg)      # saturated sigmoids tie in fp64 where the logits still differ
                    assert torch.equal(by_logit[distinct], by_prob[distinct]), (si, kind, b, c)


def test_edge_planes_follow_the_rules_in_fp64():
    for H, W in C.EDGE_SHAPES:
        x, gt, T = C.edge_planes(H, W)
        r = C.like_ref(x, gt, T)
        name = {n: i for i, n in enumerate(C.EDGE_PLANES)}
        for k in C.OUTPUTS:
            assert math.isnan(float(r[k][0, name["nan"]])) and math.isnan(float(r[k][0, name["all_minus_inf"]])), k
            assert math.isfinite(float(r[k][0, name["minus_inf_elsewhere"]])) and math.isfinite(float(r[k][0, name["plus_and_minus_inf"]])), k
            assert math.isfinite(float(r[k][0, name["gt_minus_0.4"]])), k
        assert float(r["nll"][0, name["gt_on_minus_inf"]]) == float("inf") and float(r["hpd"][0, name["gt_on_minus_inf"]]) == 1.0
        assert math.isfinite(float(r["entropy"][0, name["gt_on_minus_inf"]]))
        for i, outside in enumerate(C.edge_outside(H, W)):
            if outside:
                assert math.isnan(float(r["nll"][0, i])) and math.isnan(float(r["hpd"][0, i])) and math.isfinite(float(r["entropy"][0, i])), i
        assert sum(C.edge_outside(H, W)) == 4
        assert all(C.shape_e32(H, W)[k] > 0 for k in C.OUTPUTS)


# ---- 2. the calibration curve ----------------------------------------------------------------------------------------------------------
def test_calibration_curve_on_planted_inputs():
    lk = pkg("utils.likelihood")
    n = 20000
    u = np.random.default_rng(7).random(n)
    levels, cov, ece = lk.calibration_curve(u)
    assert np.array_equal(levels, np.linspace(0.05, 0.95, 19)) and cov.shape == (19,)
    # coverage[q] is a binomial frequency of n trials with success probability q: five standard deviations at q = 1/2
    assert np.abs(cov - levels).max() <= 5 * math.sqrt(0.25 / n) and ece <= 5 * math.sqrt(0.25 / n)
    exact = (np.arange(n) + 0.5) / n              # a perfect uniform grid: coverage = level up to 1 / n
    assert lk.calibration_curve(exact)[2] <= 1.0 / n
    _, cov1, ece1 = lk.calibration_curve(np.ones(50))          # the truth always in the last pixel of the region: no level covers it
    assert (cov1 == 0).all() and abs(ece1 - levels.mean()) < 1e-15
    _, cov0, ece0 = lk.calibration_curve(np.zeros(50))         # always the mode: every level covers it
    assert (cov0 == 1).all() and abs(ece0 - (1 - levels).mean()) < 1e-15
    with_nan = np.concatenate([u, np.full(100, np.nan)])
    assert np.array_equal(lk.calibration_curve(with_nan)[1], cov)
    assert np.array_equal(lk.calibration_curve(torch.from_numpy(with_nan).float().view(-1, 4))[0], levels)
    lv, cv, _ = lk.calibration_curve([0.2, 0.4, float("nan")], levels=[0.1, 0.2, 0.5])
    assert cv.tolist() == [0.0, 0.5, 1.0] and lv.tolist() == [0.1, 0.2, 0.5]
    for bad in ([], [float("nan")] * 3, np.empty((0, 2))):
        with pytest.raises(ValueError, match="no finite"):
            lk.calibration_curve(bad)
    with pytest.raises(ValueError, match="outside"):
        lk.calibration_curve([0.5, 1.5])
    with pytest.raises(ValueError, match="levels"):
        lk.calibration_curve([0.5], levels=[])
    with pytest.raises(ValueError, match="levels"):
        lk.calibration_curve([0.5], levels=[0.5, 1.2])


# ---- 3. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_likelihood_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_likelihood" in L.header_symbols() and len(L.SIGNATURES["ynet_map_likelihood"][1]) == 13
    vp = ctypes.c_void_p
    p = vp(4096)

    def call(x=p, bs=48, gt=p, B=2, Cn=3, H=4, W=4, T=1.0, nll=p, ent=p, hpd=p, status=p):
        return lib.ynet_map_likelihood(x, bs, gt, B, Cn, H, W, T, nll, ent, hpd, status, None)

    assert call(x=None) != 0 and b"null" in lib.ynet_last_error()
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert call(T=T) != 0 and b"temperature" in lib.ynet_last_error(), T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=1 << 31, B=1, Cn=1, H=32768, W=65536) != 0 and b"32-bit" in lib.ynet_last_error()
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    assert call(nll=None, ent=None, hpd=None) != 0 and b"no output" in lib.ynet_last_error()
    assert call(gt=None) != 0 and b"ground truth" in lib.ynet_last_error()
    assert call(gt=None, nll=None) != 0 and b"ground truth" in lib.ynet_last_error()          # hpd alone still needs it
    assert call(status=None) != 0 and b"status" in lib.ynet_last_error()


def test_wrappers_refuse_host_tensors_and_bad_requests():
    ops = pkg("ops")
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_likelihood(x, torch.zeros(2, 3, 2))
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_likelihood(x, None, want=("entropy",))
    with pytest.raises(TypeError):
        ops.map_likelihood(x.numpy())
    for want in ((), ("nll", "nll"), ("variance",)):
        with pytest.raises(ValueError, match="want"):
            ops.map_likelihood(x, None, want=want)
    ops.check_likelihood_status()                               # nothing launched, nothing to report
    assert ops.LIKELIHOOD_OUTPUTS == C.OUTPUTS


def test_signatures_keep_the_references_order():
    ev, P, trn = pkg("utils.evaluate"), pkg("utils.predict"), pkg("models.trainer")
    names = list(inspect.signature(ev.evaluate).parameters)
    assert names[:23] == ["model", "val_loader", "val_images", "device", "dataset_name", "homo_mat", "input_template", "waypoints", "mode",
                          "n_goal", "n_traj", "obs_len", "batch_size", "resize_factor", "temperature", "use_TTST", "use_CWS", "rel_thresh",
                          "CWS_params", "return_preds", "return_samples", "network", "swap_semantic"]          # utils/evaluate.py:37-42
    assert names[-1] == "return_likelihood" and inspect.signature(ev.evaluate).parameters["return_likelihood"].default is False
    # the entropy of a forecast: predict_with_entropy() takes predict()'s arguments, defaults included; predict_styles says it has none
    assert P._PREDICT_SIGNATURE == inspect.signature(P.predict) and "entropy" in P.predict_with_entropy.__doc__
    with pytest.raises(TypeError):
        P.predict_with_entropy(None, return_entropy=True)
    with pytest.raises(ValueError, match="observed must be"):      # the same validation, through the same body
        P.predict_with_entropy(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0)
    assert "out of scope" in P.predict_styles.__doc__
    tp = inspect.signature(trn.YNetTrainer.test).parameters
    assert list(tp)[:5] == ["self", "df_test", "image_path", "return_preds", "return_samples"] and tp["return_likelihood"].default is False

"""Goal-map marginals (ynet_map_marginals, ops.map_marginals, utils/marginals.py, evaluate(return_marginals=...),
predict_with_intervals()) -- everything that needs no GPU: the case table of tests/_marginals_cases.py is self-consistent, the restatement
against closed forms, utils/marginals.py on planted profiles, the C entry point's refusals, and the signatures."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _marginals_cases as C
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


def test_the_table_holds_what_it_says():
    assert [hw for hw, _, _ in C.SHAPES] == [(1, 1), (1, 3), (5, 4), (3, 64), (6, 16), (9, 256), (2, 1024), (7, 12), (17, 23), (2, 2048),
                                             (96, 160), (256, 256), (512, 512)]
    for (H, W), _, _ in C.SHAPES:
        assert H <= C.MAX_SIDE and W <= C.MAX_SIDE
        pos = C.positions(H, W)
        hit = set()
        for kind in range(len(C.KINDS)):
            g, valid = C.rounded(C.ground_truth(H, W, kind), H, W)
            assert bool(valid.all())
            hit |= {(int(a), int(b)) for a, b in g.view(-1, 2).tolist()}
        assert hit == {px for _, px in pos} and (-3, H + 2) in hit, (H, W)
    # which path a shape takes (csrc/marginals.hip): 16-byte vectors need a multiple of 4 pixels; the shapes whose W divides 1024 keep a
    # thread on the same four columns in every iteration
    vector = [(H, W) for (H, W), _, _ in C.SHAPES if (H * W) % 4 == 0]
    assert vector == [(5, 4), (3, 64), (6, 16), (9, 256), (2, 1024), (7, 12), (2, 2048), (96, 160), (256, 256), (512, 512)]
    assert [(H, W) for H, W in vector if 1024 % W == 0] == [(5, 4), (3, 64), (6, 16), (9, 256), (2, 1024), (256, 256), (512, 512)]
    for H, W in C.EXACT_SHAPES + list(C.RULE_SHAPES):
        C.shape_e32(H, W)
    # each marginal of the restatement sums to 1, the CDF ends are ordered
    x, gt, T, ref = C.case(8, 1)
    assert float((ref["col"].sum(-1) - 1).abs().max()) < 1e-14 and float((ref["row"].sum(-1) - 1).abs().max()) < 1e-14
    assert bool((ref["pit"][..., 0] <= ref["pit"][..., 1]).all()) and bool((ref["crps"] >= 0).all())
    only = C.marginals_ref(x, None, T)
    assert set(only) == {"col", "row"} and torch.equal(only["col"], ref["col"])


def crps_by_expectations(p, g):
    """E|X - g| - E|X - X'| / 2 of a profile p [side] (fp64) against the number g"""
    t = torch.arange(p.numel(), dtype=torch.float64)
    return float((p * (t - g).abs()).sum() - 0.5 * (p[:, None] * p[None, :] * (t[:, None] - t[None, :]).abs()).sum())


def test_the_restatement_against_closed_forms():
    # a one-hot plane at column a, row r: crps = |a - g| per axis exactly, pit (0, 1) at the mass, (1, 1) beyond it, (0, 0) before it
    x, gt, T, (a, r) = C.one_hot_planes()
    H, W = C.CLOSED_MAP
    ref = C.marginals_ref(x, gt, T)
    assert ref["col"][0, 0].tolist() == [1.0 if j == a else 0.0 for j in range(W)] and ref["row"][0, 0].tolist() == [1.0 if i == r else 0.0 for i in range(H)]
    g = torch.round(gt.double())
    assert torch.equal(ref["crps"][0, :, 0], (g[0, :, 0] - a).abs()) and torch.equal(ref["crps"][0, :, 1], (g[0, :, 1] - r).abs())
    assert ref["crps"][0, 3].tolist() == [a + 5.0, 0.0] and ref["crps"][0, 4].tolist() == [0.0, H + 3.0 - r]      # k pixels outside the map: + k
    assert ref["pit"][0].tolist() == [[[0.0, 1.0], [0.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 1.0]],
                                      [[0.0, 1.0], [1.0, 1.0]]]
    # two equal masses at a < b, a <= g <= b: (|a - g| + |b - g|) / 2 - (b - a) / 4
    x, gt, T, (a, b, r) = C.two_mass_planes()
    ref = C.marginals_ref(x, gt, T)
    for i, gx in enumerate((a, 6, b)):
        assert float(ref["crps"][0, i, 0]) == (abs(a - gx) + abs(b - gx)) / 2 - (b - a) / 4 and float(ref["crps"][0, i, 1]) == 0.0
    assert ref["pit"][0, :, 0].tolist() == [[0.0, 0.5], [0.5, 0.5], [0.5, 1.0]]
    # CRPS = E|X - g| - E|X - X'| / 2 on random profiles, ground truths inside and outside the map included
    x, gt, T, ref = C.case(8, 1)
    for b_ in range(C.B):
        for c_ in range(C.C):
            g = torch.round(gt[b_, c_].double())
            for axis, key in enumerate(("col", "row")):
                want = crps_by_expectations(ref[key][b_, c_], float(g[axis]))
                assert abs(float(ref["crps"][b_, c_, axis]) - want) <= 1e-12 * max(1.0, want), (b_, c_, axis)
    # a ground truth k pixels left of the map adds exactly k to the one on the border pixel
    base = C.marginals_ref(x, torch.tensor([0.0, 3.0]).expand(C.B, C.C, 2), T)["crps"]
    for k in (1, 7, 16384):
        moved = C.marginals_ref(x, torch.tensor([-float(k), 3.0]).expand(C.B, C.C, 2), T)
        assert float((moved["crps"][..., 0] - base[..., 0] - k).abs().max()) <= 1e-9 and torch.equal(moved["crps"][..., 1], base[..., 1])
        assert bool((moved["pit"][..., 0, :] == 0).all())
    # the plane-level rules
    for H, W in C.RULE_SHAPES:
        x, gt, T, raises = C.rule_planes(H, W)
        r = C.marginals_ref(x, gt, T)
        name = {n: i for i, n in enumerate(C.RULE_PLANES)}
        for n in ("nan_logit", "all_minus_inf"):
            assert all(bool(torch.isnan(r[k][0, name[n]]).all()) for k in C.OUTPUTS), n
        for n in ("gt_nan", "gt_inf", "gt_20000_away"):
            assert bool(torch.isnan(r["crps"][0, name[n]]).all()) and bool(torch.isnan(r["pit"][0, name[n]]).all()), n
            assert bool(torch.isfinite(r["col"][0, name[n]]).all()) and bool(torch.isfinite(r["row"][0, name[n]]).all()), n
        for n in ("plain", "gt_outside_valid", "gt_at_the_margin"):
            assert all(bool(torch.isfinite(r[k][0, name[n]]).all()) for k in C.OUTPUTS), n
        assert raises == [n in ("gt_nan", "gt_inf", "gt_20000_away") for n in C.RULE_PLANES]
    # exact inputs: the fp32 restatement of col, row and pit is the fp64 one
    x, gt, T = C.exact_planes(17, 23)
    a, b = C.marginals_ref(x, gt, T), C.marginals_ref(x, gt, T, torch.float32)
    for k in ("col", "row", "pit"):
        assert torch.equal(a[k].float(), b[k]), k


# ---- 2. utils/marginals.py on planted profiles -------------------------------------------------------------------------------------------
def test_quantiles_intervals_and_inside():
    M = pkg("utils.marginals")
    assert M.marginal_levels(False) is None and M.marginal_levels(None) is None and M.marginal_levels(True) == (0.5, 0.9)
    assert M.marginal_levels([0.1, 0.999]) == (0.1, 0.999)
    for bad in ((0.9, 0.5), (0.0,), 0.5, "0.5", ((0.5, 0.9),), (), tuple(0.1 * i for i in range(1, 10))):
        with pytest.raises((ValueError, TypeError)):
            M.marginal_levels(bad)
    nan = float("nan")
    p = torch.tensor([[0.25, 0.25, 0.0, 0.5], [0.0, 1.0, 0.0, 0.0], [nan] * 4])
    q = M.quantiles(p, (0.0, 0.25, 0.26, 0.5, 0.500001, 1.0))
    assert q.dtype == torch.int64 and q.tolist() == [[0, 0, 1, 1, 3, 3], [0, 1, 1, 1, 1, 1], [-1] * 6]      # exact ties: where the CDF reaches q
    iv = M.central_intervals(p, (0.5, 0.9))
    assert iv.shape == (3, 2, 2) and iv.tolist() == [[[0, 3], [0, 3]], [[1, 1], [1, 1]], [[-1, -1], [-1, -1]]]
    assert M.central_intervals(torch.tensor([0.125] * 8), (0.25, 0.75)).tolist() == [[2, 4], [0, 6]]      # ends exactly on CDF values
    # fp32 shares that sum to a little less than 1 still have every quantile
    assert M.quantiles(torch.tensor([0.5, 0.5 - 2.0 ** -24]), (1.0,)).tolist() == [1]
    inside = M.inside_intervals(iv, torch.tensor([2.4, 2.5, 1.0]))
    assert inside.dtype == torch.float64 and inside[0].tolist() == [1.0, 1.0] and inside[1].tolist() == [0.0, 0.0] and bool(torch.isnan(inside[2]).all())
    assert M.inside_intervals(iv[:2], torch.tensor([-1.0, 1.4])).tolist() == [[0.0, 0.0], [1.0, 1.0]]
    assert bool(torch.isnan(M.inside_intervals(iv[:2], torch.tensor([nan, float("inf")]))).all())
    assert M.profile_mean(p[:2]).tolist() == [0.25 + 1.5, 1.0]
    with pytest.raises(ValueError, match="qs"):
        M.quantiles(p, (1.5,))


def test_pit_histogram_spreads_the_mass():
    M = pkg("utils.marginals")
    nan = float("nan")
    pit = torch.tensor([[0.0, 1.0], [0.5, 0.5], [1.0, 1.0], [nan, 0.2], [0.05, 0.25], [0.0, 0.0]], dtype=torch.float64)
    h = M.pit_histogram(pit, 10)
    want = np.full(10, 0.1)
    want[5] += 1.0                      # a zero-width PIT goes whole into its bin
    want[9] += 1.0                      # ... F = 1 into the last one
    want[0] += 0.25 + 1.0               # [0.05, 0.25]: a quarter, a half, a quarter; (0, 0) into the first
    want[1] += 0.5
    want[2] += 0.25
    assert h.dtype == np.float64 and h.shape == (10,) and np.allclose(h, want, atol=1e-12) and abs(h.sum() - 5.0) < 1e-12      # the NaN row is left out
    assert M.pit_histogram(pit.numpy().reshape(2, 3, 2), 2).tolist() == [0.5 + 1.0 + 1.0, 0.5 + 1.0 + 1.0]
    assert M.pit_histogram(np.zeros((0, 2)), 4).tolist() == [0.0] * 4
    with pytest.raises(ValueError, match="n_bins"):
        M.pit_histogram(pit, 0)
    text = M.marginals_report((0.5,), [[1.0, 2.0], [3.0, 4.0], [nan, nan]], [[[1.0], [0.0]], [[1.0], [1.0]], [[nan], [nan]]],
                              [[[2.0], [4.0]], [[4.0], [8.0]], [[nan], [nan]]], fde=6.5)
    assert "n = 2" in text and "mean CRPS x + y: 5.0000 (x 2.0000, y 3.0000)" in text and "6.5000" in text
    assert "x, central 50 % interval: coverage 1.0000 | mean width 3.0000" in text and "y, central 50 % interval: coverage 0.5000 | mean width 6.0000" in text


# ---- 3. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_marginals_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_marginals" in L.header_symbols() and len(L.SIGNATURES["ynet_map_marginals"][1]) == 14
    with open(L.HEADER_PATH) as f:
        text = f.read()
    assert "#define YNET_MAP_MARGINALS_MAX_SIDE 2048" in text and "#define YNET_MAP_MARGINALS_GT_MARGIN 16384" in text
    p = ctypes.c_void_p(4096)      # (never dereferenced: every call below is refused before anything is launched)

    def refused(x=p, bs=48, gt=p, B=2, Cn=3, H=4, W=4, T=1.0, col=p, row=p, crps=p, pit=p, status=p):
        assert lib.ynet_map_marginals(x, bs, gt, B, Cn, H, W, T, col, row, crps, pit, status, None) != 0
        return lib.ynet_last_error().decode()

    assert refused(x=None) == "map_marginals: null map"
    assert refused(col=None, row=None, crps=None, pit=None) == "map_marginals: no output asked for"
    assert refused(gt=None) == "map_marginals: crps and pit need the ground truth (gt_xy)"
    assert refused(gt=None, crps=None) == "map_marginals: crps and pit need the ground truth (gt_xy)"
    assert refused(status=None) == "map_marginals: null status flag" and refused(status=None, pit=None) == "map_marginals: null status flag"
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert refused(T=T) == "map_marginals: the temperature and its reciprocal must be positive and finite", T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert "map_marginals: bad shape" in refused(**kw), kw
    assert refused(H=2049, W=1, bs=3 * 2049) == "map_marginals: a plane of 2049x1 has a side above 2048"
    assert refused(H=1, W=2049, bs=3 * 2049) == "map_marginals: a plane of 1x2049 has a side above 2048"
    assert refused(bs=47) == "map_marginals: batch stride 47 below the 3 planes of 4x4 of an image"
    assert refused(B=1 << 31, Cn=1, bs=16) == "map_marginals: too many planes"
    assert refused(T=0.0, H=0, bs=47) == "map_marginals: the temperature and its reciprocal must be positive and finite"
    # (the pixel cap of 2^22 is the side cap squared: no shape passes the side check and fails it)
    assert C.MAX_SIDE * C.MAX_SIDE == 4194304 and "#define YNET_MAP_MARGINALS_MAX_PIXELS 4194304" in text


def test_wrapper_refuses_host_tensors_and_bad_requests():
    ops = pkg("ops")
    x, gt = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_marginals(x, gt)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_marginals(x, None, want=("col", "row"))
    with pytest.raises(TypeError):
        ops.map_marginals(x.numpy(), gt)
    for want in ((), ("col", "col"), ("median",)):
        with pytest.raises(ValueError, match="want"):
            ops.map_marginals(x, gt, want=want)
    assert ops.check_marginals_status() is False                   # nothing launched, nothing to report
    assert ops.MARGINAL_OUTPUTS == C.OUTPUTS and ops.MARGINALS_MAX_SIDE == C.MAX_SIDE
    sig = inspect.signature(ops.map_marginals)
    assert list(sig.parameters) == ["x", "gt_xy", "temperature", "want"] and sig.parameters["gt_xy"].default is None
    assert sig.parameters["want"].default == ("col", "row", "crps", "pit") and sig.parameters["temperature"].default == 1.0


def test_drivers_take_the_flag_and_default_to_off():
    ev, trn, P = pkg("utils.evaluate"), pkg("models.trainer"), pkg("utils.predict")
    names = list(inspect.signature(ev.evaluate).parameters)
    assert names[names.index("forced_ttst_samples") + 1] == "return_marginals" and names[-2:] == ["return_sharpness", "return_likelihood"]
    assert names[:23] == ["model", "val_loader", "val_images", "device", "dataset_name", "homo_mat", "input_template", "waypoints", "mode", "n_goal",
                          "n_traj", "obs_len", "batch_size", "resize_factor", "temperature", "use_TTST", "use_CWS", "rel_thresh", "CWS_params",
                          "return_preds", "return_samples", "network", "swap_semantic"]
    assert inspect.signature(ev.evaluate).parameters["return_marginals"].default is False
    tp = inspect.signature(trn.YNetTrainer.test).parameters
    assert list(tp)[-1] == "return_sharpness" and list(tp)[-3:-1] == ["return_marginals", "return_radial"] and tp["return_marginals"].default is False
    for bad in ((0.9, 0.5), (0.0,), 0.5, "0.5", ((0.5, 0.9),)):      # refused before the model is touched
        with pytest.raises((ValueError, TypeError)):
            ev.evaluate(None, [], {}, "cpu", "sdd", None, None, [0], "test", 1, 1, 1, 1, return_marginals=bad)
    with pytest.raises(ValueError, match="return_marginals"):
        ev.evaluate(None, [], {}, "cpu", "sdd", None, None, [0], "test", 1, 1, 1, 1, return_marginals=(0.9, 0.5))
    # the forecast form takes predict()'s arguments, defaults included, through predict()'s own body
    assert P._PREDICT_SIGNATURE == inspect.signature(P.predict)
    assert list(inspect.signature(P.predict).parameters) == ["model", "scene_image", "observed", "input_template", "waypoints", "n_goal", "n_traj", "obs_len",
                                                             "resize_factor", "temperature", "use_TTST", "use_CWS", "rel_thresh", "CWS_params", "network",
                                                             "swap_semantic", "batch_size", "max_effective_batch", "forced_samples", "return_maps"]
    fp = list(inspect.signature(P._forecast).parameters)
    assert fp[-1] == "regions" and fp[-2] == "intervals" and inspect.signature(P._forecast).parameters["intervals"].default is None
    lv = inspect.signature(P.predict_with_intervals).parameters["levels"]
    assert lv.default == (0.5, 0.9) and lv.kind is inspect.Parameter.KEYWORD_ONLY
    for k in ("median_xy", "interval_xy", "marginal_mean_xy"):
        assert k in P.predict_with_intervals.__doc__
    with pytest.raises(TypeError):
        P.predict_with_intervals(None, intervals=(0.5,))
    with pytest.raises(ValueError, match="ascend"):
        P.predict_with_intervals(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0, levels=(0.9, 0.5))
    with pytest.raises(ValueError, match="levels"):
        P.predict_with_intervals(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0, levels=True)
    with pytest.raises(ValueError, match="observed must be"):      # the same validation, through the same body
        P.predict_with_intervals(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0)
    assert inspect.signature(trn.YNetTrainer.predict_intervals).parameters["levels"].default == (0.5, 0.9)
    # the scorer: its keys, its columns and its steps on planted batches
    S = pkg("utils.scores")
    s = S.MarginalScore((0.5, 0.9))
    assert s.on and s.levels == (0.5, 0.9) and not S.MarginalScore(False).on and S.MarginalScore(True).levels == (0.5, 0.9)
    e = s.empty(12, "cpu", "scene")
    assert set(e) == set(s.keys) and e["interval"].shape == (0, 12, 2, 2, 2) and e["width"].shape == (0, 12, 2, 2) and e["pit"].shape == (0, 12, 2, 2) and e["crps"].dtype == torch.float64
    import pandas as pd
    nan = float("nan")
    s.lists = {"crps": [np.array([[[4.0, 8.0]], [[nan, nan]]])], "pit": [np.array([[[[0.25, 0.75], [0.0, 0.5]]], [[[nan, nan], [nan, nan]]]], dtype=np.float32)],
               "interval": [np.array([[[[[2, 4], [1, 7]], [[3, 3], [0, 9]]]], [[[[-1, -1], [-1, -1]], [[-1, -1], [-1, -1]]]]])],
               "inside": [np.array([[[[1.0, 1.0], [0.0, 1.0]]], [[[nan, nan], [nan, nan]]]])],
               "width": [np.array([[[[8.0, 24.0], [0.0, 36.0]]], [[[nan, nan], [nan, nan]]]])]}
    df, td = pd.DataFrame({"metaId": [0, 1]}), {}
    s.columns(df)
    s.steps(td)
    assert list(df.columns) == ["metaId", "crps_x_goal", "crps_y_goal", "crps_goal", "pit_x_goal", "pit_y_goal", "width50_x_goal", "inside50_x_goal",
                                "width50_y_goal", "inside50_y_goal", "width90_x_goal", "inside90_x_goal", "width90_y_goal", "inside90_y_goal"]
    assert df.iloc[0].tolist() == [0, 4.0, 8.0, 12.0, 0.5, 0.25, 8.0, 1.0, 0.0, 0.0, 24.0, 1.0, 36.0, 1.0] and bool(df.iloc[1, 1:].isna().all())
    assert set(td) == {"crps_steps", "pit_steps", "interval_steps"} and td["interval_steps"].shape == (2, 1, 2, 2, 2)
    text = trn.marginals_report_of(df, (0.5, 0.9), fde=6.5)
    assert "n = 1" in text and "mean CRPS x + y: 12.0000" in text and "y, central 90 % interval: coverage 1.0000 | mean width 36.0000" in text

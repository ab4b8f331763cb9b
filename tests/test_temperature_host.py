"""Temperature scaling (ynet_map_likelihood_sweep, ops.map_likelihood_sweep, utils/likelihood.py's grid search, utils/calibrate.py,
YNetTrainer.calibrate_temperature) -- everything that needs no GPU: the case table of tests/_temperature_cases.py is self-consistent,
the planted calibration sets have their optimum where the GPU test expects it (under the fp64 reference alone), the grid search on
planted curves, every refusal that precedes a launch, and the signatures."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import _likelihood_cases as C
import _temperature_cases as T
from conftest import pkg


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error_over_the_sweeps_temperatures(si):
    (H, W), _, _ = C.SHAPES[si]
    recorded, measured = T.E32[(H, W)], T.measure_e32(si)
    print(f"{H}x{W}: E32 measured {measured}, recorded {recorded}")
    # (the headroom of tests/test_likelihood_host.py: the order of a stock-torch fp32 sum depends on the thread count and the vector width)
    for k in T.SWEEP_OUTPUTS:
        assert measured[k] <= 1.25 * recorded[k] and recorded[k] <= 2.0 * measured[k] + 1e-12, (k, measured[k], recorded[k])


def test_grids_are_unsorted_hold_one_and_one_repeat():
    assert set(T.E32) == {hw for hw, _, _ in C.SHAPES} and T.SWEEP_OUTPUTS == ("nll", "hpd")
    assert T.MASTER.dtype == np.float32 and T.MASTER.min() == 0.25 and T.MASTER.max() <= 8.0
    for n in T.N_TEMPS + [3]:
        g = T.grid(n)
        assert g.dtype == np.float32 and g.shape == (n,) and (g == 1.0).any()
        if n >= 2:
            i, j = T.repeated(n)
            assert i != j and g[i] == g[j] and np.unique(g).size == n - 1
        if n >= 8:
            assert not (np.diff(g) > 0).all() and not (np.diff(g) < 0).all()
    assert T.repeated(17)[0] // 8 != T.repeated(17)[1] // 8          # the two copies in different chunks
    for t in T.EDGE_TEMPS:
        assert t in T.temps_for(5, 4) and t in T.temps_for(17, 23)


def test_closed_forms_per_temperature_are_the_fp64_restatements():
    temps = T.grid(9)
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        x, gt, _, _ = C.constant_plane(H, W)
        got, want = T.sweep_ref(x, gt, temps), T.constant_answers(H, W, temps)
        assert float((got["nll"] - want["nll"]).abs().max()) <= 1e-12 and bool((got["hpd"] == 1.0).all())
        if H * W < 2:
            continue
        x, gt, _, _ = C.spike_planes(H, W)
        got, want = T.sweep_ref(x, gt, temps), T.spike_answers(H, W, temps)
        for k in T.SWEEP_OUTPUTS:
            assert float((got[k] - want[k]).abs().max()) <= 1e-12, (k, H, W)
    # at T = 1 the per-temperature forms are tests/_likelihood_cases.py's
    one = T.spike_answers(5, 4, [1.0])
    want = C.spike_planes(5, 4)[3]
    assert one["nll"][0, 0].tolist() == want["nll"] and one["hpd"][0, 0].tolist() == want["hpd"]


def test_the_no_mass_plane_loses_its_mass_at_the_small_temperature_only():
    for H, W in C.EDGE_SHAPES:
        x, gt = T.edge_planes(H, W)
        assert x.shape[1] == len(C.EDGE_PLANES) + 1 and gt.shape == (1, x.shape[1], 2)
        # in fp32 sigmoid(-160) is 0, so Z = 0 -- the rule the kernel follows (its entry is NaN); at the other temperatures Z > 0
        assert T.EDGE_TEMPS[0] == 0.25 and T.NO_MASS_LOGIT / 0.25 < -104
        Z32 = [float(torch.sigmoid(x[0, -1] / float(t)).sum()) for t in T.EDGE_TEMPS]
        assert Z32[0] == 0.0 and Z32[1] > 0.0 and Z32[2] > 0.0
        assert math.isnan(float(T.sweep_ref(x, gt, T.EDGE_TEMPS[:1], torch.float32)["hpd"][0, 0, -1]))          # 0 / 0
        r64 = T.sweep_ref(x, gt, T.EDGE_TEMPS[1:])
        assert float((r64["nll"][:, 0, -1] - math.log(H * W)).abs().max()) <= 1e-12 and bool((r64["hpd"][:, 0, -1] == 1.0).all())


# ---- 2. the grid search --------------------------------------------------------------------------------------------------------------
def test_temperature_grid():
    lk = pkg("utils.likelihood")
    g = lk.temperature_grid(0.25, 8.0, 16)
    assert g.dtype == np.float32 and g.shape == (16,) and g[0] == 0.25 and g[-1] == 8.0 and (np.diff(g) > 0).all()
    assert np.array_equal(g, T.cal_grid())                                              # stock NumPy says the same
    ratios = g[1:].astype(np.float64) / g[:-1].astype(np.float64)
    assert np.abs(ratios - 32.0 ** (1 / 15)).max() <= 2e-7 * 32.0 ** (1 / 15)           # log-spaced up to the fp32 rounding
    assert np.array_equal(g.astype(np.float64).astype(np.float32), g)                  # every value is an fp32 number
    # include: inserted in order, once
    gi = lk.temperature_grid(0.25, 8.0, 16, include=1.8)
    assert gi.shape == (17,) and (np.diff(gi) > 0).all() and np.float32(1.8) in gi and set(g) <= set(gi)
    assert int(np.flatnonzero(gi == np.float32(1.8))[0]) == int(np.searchsorted(g, np.float32(1.8)))
    assert np.array_equal(lk.temperature_grid(0.25, 8.0, 16, include=1.0), g)           # 1.0 is grid point 6 already
    assert np.array_equal(lk.temperature_grid(0.25, 8.0, 16, include=float(g[10])), g)  # an fp32 grid value given back as a float
    assert np.array_equal(lk.temperature_grid(0.25, 8.0, 16, include=float(g[10]) * (1 + 1e-9)), g)      # equal after the rounding to fp32
    out = lk.temperature_grid(0.25, 8.0, 4, include=20.0)                               # outside the bracket: still in order
    assert out.tolist() == [0.25, float(np.float32(0.25 * 32 ** (1 / 3))), float(np.float32(0.25 * 32 ** (2 / 3))), 8.0, 20.0]
    assert lk.temperature_grid(2.0, 3.0, 2).tolist() == [2.0, 3.0]
    for bad in ((0.0, 8.0), (-1.0, 8.0), (8.0, 0.25), (1.0, 1.0), (0.25, float("inf")), (float("nan"), 8.0)):
        with pytest.raises(ValueError, match="bracket"):
            lk.temperature_grid(bad[0], bad[1], 16)
    with pytest.raises(ValueError, match="at least 2"):
        lk.temperature_grid(0.25, 8.0, 1)
    for bad in (0.0, -2.0, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="include"):
            lk.temperature_grid(0.25, 8.0, 16, include=bad)


def test_best_temperature_and_next_bracket_on_planted_curves():
    lk = pkg("utils.likelihood")
    g = T.cal_grid()
    interior = (np.log(g.astype(np.float64)) - math.log(2.5)) ** 2                      # minimum at grid point 10
    assert lk.best_temperature(g, interior) == (float(g[10]), 10) and lk.next_bracket(g, interior) == (float(g[9]), float(g[11]))
    rising, falling = np.arange(16.0), -np.arange(16.0)
    assert lk.best_temperature(g, rising) == (0.25, 0) and lk.next_bracket(g, rising) == (0.25, float(g[1]))
    assert lk.best_temperature(g, falling) == (8.0, 15) and lk.next_bracket(g, falling) == (float(g[14]), 8.0)
    two = interior.copy()
    two[3] = two[10]                                                                    # a tie goes to the lower temperature
    assert lk.best_temperature(g, two) == (float(g[3]), 3) and lk.next_bracket(g, two) == (float(g[2]), float(g[4]))
    flat = np.zeros(16)
    assert lk.best_temperature(g, flat) == (0.25, 0)
    # no convexity assumed: the global minimum wins over a nearer local one
    bumpy = interior.copy()
    bumpy[2] = -1.0
    assert lk.best_temperature(g, bumpy)[1] == 2
    # an unsorted grid: neighbours are neighbours in temperature, the index is into the given order
    perm = np.random.default_rng(5).permutation(16)
    assert lk.best_temperature(g[perm], interior[perm]) == (float(g[10]), int(np.flatnonzero(perm == 10)[0]))
    assert lk.next_bracket(g[perm], interior[perm]) == (float(g[9]), float(g[11]))
    for bad in (float("nan"), float("inf")):
        c = interior.copy()
        c[5] = bad
        with pytest.raises(ValueError, match="non-finite"):
            lk.best_temperature(g, c)
        with pytest.raises(ValueError, match="non-finite"):
            lk.next_bracket(g, c)
    with pytest.raises(ValueError, match="curve values"):
        lk.best_temperature(g, interior[:15])
    with pytest.raises(ValueError, match="twice"):
        lk.best_temperature([1.0, 1.0], [0.0, 1.0])
    with pytest.raises(ValueError, match="one point"):
        lk.next_bracket([1.0], [0.0])


@pytest.mark.parametrize("hw,planes", T.PLANTED, ids=[f"{h}x{w}" for (h, w), _ in T.PLANTED])
def test_planted_sets_have_their_optimum_at_grid_point_10_under_the_reference_alone(hw, planes):
    lk = pkg("utils.likelihood")
    g = T.cal_grid()
    curve = T.planted_curve(hw[0], hw[1], planes, tuple(float(t) for t in g))
    k = int(np.argmin(curve))
    margin = min(curve[k - 1] - curve[k], curve[k + 1] - curve[k])
    print(f"{hw} x {planes} planes: minimum at grid point {k} (T = {g[k]}), margin {margin:.4f}; E32 bound ~ {2 * T.E32[hw]['nll']:.1e}")
    assert k == T.PLANTED_BEST and abs(float(g[k]) - T.PLANTED_T) < 0.03 and margin > 1e-3
    assert lk.best_temperature(g, curve) == (float(g[k]), k)
    x, gt = T.planted(*hw, planes)
    assert x.shape == (planes, 1, *hw) and x.dtype == torch.float32 and gt.shape == (planes, 1, 2)
    assert bool((gt[..., 0] >= 0).all() and (gt[..., 0] < hw[1]).all() and (gt[..., 1] >= 0).all() and (gt[..., 1] < hw[0]).all())


# ---- 3. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_sweep_is_declared_bound_and_exported():
    L = pkg("_lib")
    name = "ynet_map_likelihood_sweep"
    assert name in L.header_symbols() and name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 13
    assert set(L.header_symbols()) == set(L.SIGNATURES)
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    with open(L.HEADER_PATH) as f:
        text = f.read()
    decl = text.index("int " + name)
    comment = text[text.rindex("/*", 0, decl):decl]
    assert "utils/evaluate.py:128-131" in comment and "utils/image_utils.py:110-135" in comment      # every entry cites what it serves
    assert "#define YNET_SWEEP_MAX_TEMPS 32" in text and pkg("ops").SWEEP_MAX_TEMPS == 32


def test_sweep_entry_refuses_bad_arguments_before_any_launch():
    L = pkg("_lib")
    lib = L.load()
    p = ctypes.c_void_p(4096)
    fl = ctypes.c_float

    def call(x=p, bs=48, gt=p, B=2, Cn=3, H=4, W=4, temps=(1.0, 1.8), n=None, nll=p, hpd=p, status=p):
        arr = None if temps is None else (fl * max(len(temps), 1))(*temps)
        return lib.ynet_map_likelihood_sweep(x, bs, gt, B, Cn, H, W, arr, len(temps) if n is None else n, nll, hpd, status, None)

    assert call(x=None) != 0 and b"null map" in lib.ynet_last_error()
    assert call(temps=None, n=2) != 0 and b"null temperatures" in lib.ynet_last_error()
    for n in (0, -1, 33):
        assert call(temps=(1.0,) * 33, n=n) != 0 and b"1 .. 32" in lib.ynet_last_error(), n
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        for at in (0, 31):                                              # the first and the last entry of a full grid
            temps = [1.0] * 32
            temps[at] = bad
            assert call(temps=temps) != 0 and b"temperature %d" % at in lib.ynet_last_error(), (bad, at)
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=1 << 31, B=1, Cn=1, H=32768, W=65536) != 0 and b"32-bit" in lib.ynet_last_error()
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    assert call(B=1 << 31, Cn=1, bs=16) != 0 and b"too many planes" in lib.ynet_last_error()
    assert call(nll=None, hpd=None) != 0 and b"no output" in lib.ynet_last_error()
    assert call(gt=None) != 0 and b"ground truth" in lib.ynet_last_error()
    assert call(status=None) != 0 and b"status" in lib.ynet_last_error()


def test_op_refuses_bad_requests_before_the_device_check_and_host_tensors_at_it():
    ops = pkg("ops")
    x, gt = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2)
    for want in ((), ("nll", "nll"), ("entropy",), ("nll", "entropy")):          # the entropy is not part of the sweep
        with pytest.raises(ValueError, match="want"):
            ops.map_likelihood_sweep(x, gt, [1.0], want=want)
    for temps in ([], [1.0] * 33, np.empty((0,))):
        with pytest.raises(ValueError, match="1 .. 32"):
            ops.map_likelihood_sweep(x, gt, temps)
    for bad in (0.0, -1.0, float("inf"), float("nan"), 1e-39, 1e39):            # (1e39 is +inf in fp32, 1e-39 has no fp32 reciprocal)
        with pytest.raises(ValueError, match="positive and finite"):
            ops.map_likelihood_sweep(x, gt, [1.0, bad, 2.0])
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_likelihood_sweep(x, gt, [1.0, 1.8])
    with pytest.raises(TypeError):
        ops.map_likelihood_sweep(x.numpy(), gt, [1.0])
    t = ops.sweep_temperatures((1, 1.8, np.float64(0.3)))                         # any host sequence, converted to fp32
    assert t.dtype == np.float32 and t.flags["C_CONTIGUOUS"] and t.tolist() == [1.0, float(np.float32(1.8)), float(np.float32(0.3))]
    assert ops.sweep_temperatures(torch.tensor([2.0, 0.5])).tolist() == [2.0, 0.5]
    ops.check_likelihood_status()                                               # nothing launched, nothing to report
    assert ops.SWEEP_OUTPUTS == T.SWEEP_OUTPUTS


# ---- 4. calibrate_temperature and the trainer ---------------------------------------------------------------------------------------------
def test_calibrate_temperature_refuses_before_touching_the_device():
    cal = pkg("utils.calibrate")
    base = dict(model=None, val_loader=None, val_images=None, device=None, input_template=None, waypoints=[11], obs_len=8, batch_size=4,
                resize_factor=0.25, temperature=1.0)

    def refused(match, **kw):
        with pytest.raises(ValueError, match=match):
            cal.calibrate_temperature(**{**base, **kw})

    refused("rounds", rounds=0)
    refused("rounds", rounds=-2)
    for n in (1, 0, 32, 100):
        refused("n_temps", n_temps=n)
    for r in ((0.0, 8.0), (-1.0, 2.0), (8.0, 0.25), (1.0, 1.0), (0.25, float("inf")), (float("nan"), 8.0), (1.0,), 3.0):
        refused("t_range", t_range=r)
    refused("steps", steps="goals")
    refused("steps", steps=None)
    refused("way-points", waypoints=[])
    for bad in (0.0, -1.0, float("nan")):
        refused("positive and finite", temperature=bad)
    assert cal.STEPS == ("waypoints", "goal", "all")
    assert cal._selected_planes("waypoints", [14, 29], 30) == [14, 29] and cal._selected_planes("goal", [14, 29], 30) == [29]
    assert cal._selected_planes("all", [11], 12) == list(range(12))
    assert cal._goal_maps is pkg("utils.evaluate")._goal_maps                       # evaluate's own helper, not a copy


def test_trainer_wrapper_refuses_before_preparing_any_data():
    from test_predict_host import _trainer
    t = _trainer()
    before = dict(t.params)
    for kw, match in ((dict(rounds=0), "rounds"), (dict(n_temps=1), "n_temps"), (dict(n_temps=32), "n_temps"), (dict(t_range=(2.0, 1.0)), "t_range"),
                      (dict(steps="every"), "steps")):
        with pytest.raises(ValueError, match=match):
            t.calibrate_temperature(None, None, **kw)                               # (no data frame, no images: never looked at)
    with pytest.raises(ValueError, match="way-points"):
        _trainer(waypoints=[]).calibrate_temperature(None, None)
    with pytest.raises(ValueError, match="positive and finite"):
        _trainer(temperature=0.0).calibrate_temperature(None, None)
    assert t.params == before


def test_signatures():
    cal, lk, ops, trn, ev, P = (pkg(m) for m in ("utils.calibrate", "utils.likelihood", "ops", "models.trainer", "utils.evaluate", "utils.predict"))
    sig = inspect.signature(cal.calibrate_temperature).parameters
    assert list(sig) == ["model", "val_loader", "val_images", "device", "input_template", "waypoints", "obs_len", "batch_size", "resize_factor",
                         "temperature", "t_range", "n_temps", "rounds", "steps", "network", "swap_semantic"]
    d = {k: v.default for k, v in sig.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(t_range=(0.25, 8.0), n_temps=16, rounds=2, steps="waypoints", network=None, swap_semantic=False)
    tp = inspect.signature(trn.YNetTrainer.calibrate_temperature).parameters
    assert list(tp) == ["self", "df_val", "image_path", "t_range", "n_temps", "rounds", "steps"]
    assert {k: v.default for k, v in tp.items() if v.default is not inspect.Parameter.empty} == dict(t_range=(0.25, 8.0), n_temps=16, rounds=2,
                                                                                                    steps="waypoints")
    assert list(inspect.signature(ops.map_likelihood_sweep).parameters) == ["x", "gt_xy", "temperatures", "want"]
    assert inspect.signature(ops.map_likelihood_sweep).parameters["want"].default == ("nll", "hpd")
    assert list(inspect.signature(lk.temperature_grid).parameters) == ["lo", "hi", "n", "include"]
    assert list(inspect.signature(lk.next_bracket).parameters) == ["temps", "curve"] == list(inspect.signature(lk.best_temperature).parameters)
    # the existing interfaces are as they were
    assert list(inspect.signature(ops.map_likelihood).parameters) == ["x", "gt_xy", "temperature", "want"]
    assert list(inspect.signature(ev.evaluate).parameters)[-1] == "return_likelihood" and P._PREDICT_SIGNATURE == inspect.signature(P.predict)

"""Temperature scaling on the MI355X: ynet_map_likelihood_sweep against the fp64 restatement of tests/_likelihood_cases.py (called once
per temperature) over the table of tests/_temperature_cases.py, against the one-temperature kernel it extends, the edge rules per
temperature, the layouts, and calibrate_temperature on the planted sets and on the reference's fixtures.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), E32 = the error of the same restatement run in fp32 over the
sweep's temperatures (recorded per shape in tests/_temperature_cases.py; measured on the spot for the inputs that are not in it).

Measured on the MI355X (largest |device - fp64| over the table): see DESIGN.md section 4.12."""
import contextlib
import io
import math
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

import _likelihood_cases as C
import _temperature_cases as T
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, what):
    """every finite reference entry within the bound, every other entry of the same class (NaN / +inf / -inf); prints the margin"""
    for k, g in got.items():
        g, r = g.detach().cpu().double(), ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        fin = torch.isfinite(r)
        assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, k, "NaN pattern")
        assert torch.equal(g[~fin & ~torch.isnan(r)], r[~fin & ~torch.isnan(r)]), (what, k, "infinities")
        if fin.any():
            err, bnd = (g - r).abs()[fin], C.bound(r, e[k])[fin]
            print(f"{what} {k}: max error {float(err.max()):.3e} (bound there {float(bnd[err.argmax()]):.3e})")
            assert bool((err <= bnd).all()), (what, k, float(err.max()), float(bnd[err.argmax()]))


# ---- 1. the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_sweep_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    (H, W), _, _ = C.SHAPES[si]
    e = T.E32[(H, W)]
    for kind in range(len(C.KINDS)):
        x, gt = T.case(si, kind)
        dx, dgt = x.to(dev), gt.to(dev)
        for n in T.n_temps_for(H, W):
            temps = T.grid(n)
            what = f"{H}x{W} kind {kind} n_T {n}"
            both = ops.map_likelihood_sweep(dx, dgt, temps)
            assert set(both) == set(T.SWEEP_OUTPUTS) and all(v.shape == (n, C.B, C.C) and v.dtype == torch.float32 and v.is_cuda for v in both.values())
            check(both, T.ref_sweep(si, kind, temps), e, what)
            if n >= 2:                                              # one temperature given twice: the same bits, whatever chunk each copy sits in
                i, j = T.repeated(n)
                assert all(torch.equal(v[i], v[j]) for v in both.values()), what
            for k in T.SWEEP_OUTPUTS:                               # each output alone, the other NULL: the same bits
                alone = ops.map_likelihood_sweep(dx, dgt, temps, want=(k,))
                assert set(alone) == {k} and torch.equal(alone[k], both[k]), (what, k)
            again = ops.map_likelihood_sweep(dx, dgt, temps)        # a second run: the same bits
            assert all(torch.equal(again[k], both[k]) for k in T.SWEEP_OUTPUTS), what
        assert torch.equal(dx.cpu(), x)                             # the input is read, never written
    ops.check_likelihood_status()


# ---- 2. against the one-temperature kernel ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_sweep_agrees_with_map_likelihood_at_every_temperature(dev, si):
    ops = pkg("ops")
    (H, W), _, _ = C.SHAPES[si]
    e, temps = T.E32[(H, W)], T.grid(3 if (H, W) == (512, 512) else 17)
    worst = {k: 0.0 for k in T.SWEEP_OUTPUTS}
    for kind in range(len(C.KINDS)):
        x, gt = T.case(si, kind)
        dx, dgt = x.to(dev), gt.to(dev)
        sweep, ref = ops.map_likelihood_sweep(dx, dgt, temps), T.ref_sweep(si, kind, temps)
        for i, t in enumerate(temps):
            one = ops.map_likelihood(dx, dgt, float(t), want=T.SWEEP_OUTPUTS)
            for k in T.SWEEP_OUTPUTS:
                d = (sweep[k][i].double() - one[k].double()).abs().cpu()
                worst[k] = max(worst[k], float(d.max()))
                assert bool((d <= 2.0 * C.bound(ref[k][i], e[k])).all()), (H, W, kind, float(t), k, float(d.max()))      # the two calls' bounds, summed
    print(f"{H}x{W}: largest |sweep - map_likelihood| {worst}")
    ops.check_likelihood_status()


# ---- 3. known answers ------------------------------------------------------------------------------------------------------------------------
def test_known_answers_at_every_temperature(dev):
    ops = pkg("ops")
    temps = T.grid(9)
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        e = T.E32[(H, W)]
        x, gt, _, _ = C.constant_plane(H, W)
        got = ops.map_likelihood_sweep(x.to(dev), gt.to(dev), temps)
        check(got, T.constant_answers(H, W, temps), e, f"constant {H}x{W}")
        assert bool((got["hpd"] == 1.0).all())                      # every pixel is a member: exactly 1 at every temperature
        if H * W < 2:
            continue
        x, gt, _, _ = C.spike_planes(H, W)
        got = ops.map_likelihood_sweep(x.to(dev), gt.to(dev), temps)
        check(got, T.spike_answers(H, W, temps), e, f"spike {H}x{W}")
        assert bool((got["hpd"][:, 0, 1] == 1.0).all())
    ops.check_likelihood_status()


# ---- 4. the edge rules and the status flag, per temperature ----------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.EDGE_SHAPES)
def test_edge_planes_and_status_flag(dev, H, W):
    ops = pkg("ops")
    ops.check_likelihood_status()
    x, gt = T.edge_planes(H, W)
    temps, e = T.EDGE_TEMPS, T.E32[(H, W)]
    name = {n: i for i, n in enumerate(C.EDGE_PLANES)}
    no_mass = len(C.EDGE_PLANES)
    ref = T.sweep_ref(x, gt, temps)
    for k in T.SWEEP_OUTPUTS:                                       # the rule fp64 cannot show: sigmoids below fp32's range are 0, Z_k = 0, NaN
        assert math.isfinite(float(ref[k][0, 0, no_mass]))
        ref[k][0, 0, no_mass] = float("nan")
    got = ops.map_likelihood_sweep(x.to(dev), gt.to(dev), temps)
    with pytest.raises(RuntimeError, match="outside the map"):
        ops.check_likelihood_status()
    ops.check_likelihood_status()                                   # raised once, then cleared
    check(got, ref, e, f"edge planes {H}x{W}")                      # the planes beside the offending ones are unaffected
    h = {k: v.cpu() for k, v in got.items()}
    for i in range(len(temps)):                                     # section 4.10's pattern, for every k separately
        for k in T.SWEEP_OUTPUTS:
            assert math.isnan(float(h[k][i, 0, name["nan"]])) and math.isnan(float(h[k][i, 0, name["all_minus_inf"]])), (k, i)
            assert math.isfinite(float(h[k][i, 0, name["plus_and_minus_inf"]])) and math.isfinite(float(h[k][i, 0, name["minus_inf_elsewhere"]])), (k, i)
            assert math.isfinite(float(h[k][i, 0, name["gt_minus_0.4"]])), (k, i)
            assert math.isnan(float(h[k][i, 0, no_mass])) == (i == 0), (k, i)      # no mass at T = 0.25 alone
        assert float(h["nll"][i, 0, name["gt_on_minus_inf"]]) == float("inf") and float(h["hpd"][i, 0, name["gt_on_minus_inf"]]) == 1.0
        for p, outside in enumerate(C.edge_outside(H, W)):
            if outside:
                assert math.isnan(float(h["nll"][i, 0, p])) and math.isnan(float(h["hpd"][i, 0, p])), (i, p)
    # without the offending planes the same launch raises nothing
    keep = [p for p, o in enumerate(C.edge_outside(H, W) + [False]) if not o]
    clean = ops.map_likelihood_sweep(x[:, keep].to(dev), gt[:, keep].to(dev), temps)
    ops.check_likelihood_status()
    for k in T.SWEEP_OUTPUTS:
        assert torch.equal(clean[k].cpu()[:, 0].nan_to_num(nan=-7.0), h[k][:, 0, keep].nan_to_num(nan=-7.0)), k


# ---- 5. other layouts ------------------------------------------------------------------------------------------------------------------------
def test_other_layouts(dev):
    ops = pkg("ops")
    temps = T.grid(9)
    x, gt, _ = C.many_planes()                                      # 70000 workgroups along blockIdx.x
    got = ops.map_likelihood_sweep(x.to(dev), gt.to(dev), temps)
    check(got, T.sweep_ref(x, gt, temps), T.sweep_e32(x, gt, np.unique(temps)), "70000 planes of 2x2")
    for H, W in [(17, 23), (8, 8)]:                                 # a channel slice, read in place: batch stride 5 planes, 2 planes scored
        x5, gt, _ = C.sliced(H, W)
        d5 = x5.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        got = ops.map_likelihood_sweep(view, gt.to(dev), temps)
        xs = x5[:, 1:3].contiguous()
        check(got, T.sweep_ref(xs, gt, temps), T.sweep_e32(xs, gt, np.unique(temps)), f"channel slice {H}x{W}")
        dense = ops.map_likelihood_sweep(xs.to(dev), gt.to(dev), temps)
        if (H * W) % 4 == 0:                                         # same alignment, same path: the same bits
            assert all(torch.equal(dense[k], got[k]) for k in T.SWEEP_OUTPUTS)
        assert torch.equal(d5.cpu(), x5)
    ops.check_likelihood_status()
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_likelihood_sweep(x5, gt.to(dev), temps)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_likelihood_sweep(d5[:, 1:3], gt, temps)
    with pytest.raises(ValueError, match="gt_xy"):
        ops.map_likelihood_sweep(d5, gt.to(dev), temps)
    with pytest.raises(TypeError, match="host"):
        ops.map_likelihood_sweep(d5[:, 1:3], gt.to(dev), torch.tensor([1.0, 2.0], device=dev))


# ---- 6. the search on the planted set ------------------------------------------------------------------------------------------------------
def grid_search(curve_of, lk, rounds, include):
    """utils.calibrate's search with the mean NLL of a grid supplied by `curve_of(temps)` -> [(temps, curve) per round], best temperature"""
    bracket, out = (0.25, 8.0), []
    for _ in range(rounds):
        temps = lk.temperature_grid(bracket[0], bracket[1], 16, include=include)
        curve = curve_of(temps)
        out.append((temps, curve))
        bracket = lk.next_bracket(temps, curve)
    return out, lk.best_temperature(*out[-1])[0]


def test_search_on_the_planted_set_finds_the_fp64_optimum(dev):
    ops, lk = pkg("ops"), pkg("utils.likelihood")
    (H, W), planes = T.PLANTED[1]
    assert (H, W) == (17, 23)
    x, gt = T.planted(H, W, planes)
    dx, dgt = x.to(dev), gt.to(dev)

    def on_device(temps):
        return ops.map_likelihood_sweep(dx, dgt, temps, want=("nll",))["nll"].double().mean(dim=(1, 2)).cpu().numpy()

    def in_fp64(temps):
        return T.planted_curve(H, W, planes, tuple(float(t) for t in temps))

    dev_rounds, t_dev = grid_search(on_device, lk, 2, None)
    ref_rounds, t_ref = grid_search(in_fp64, lk, 2, None)
    assert np.array_equal(dev_rounds[0][0], T.cal_grid()) and lk.best_temperature(*dev_rounds[0])[1] == T.PLANTED_BEST      # round 1: grid point 10
    assert np.array_equal(dev_rounds[1][0], ref_rounds[1][0])                          # so both searches refine the same bracket
    g2 = dev_rounds[1][0]
    i_dev, i_ref = int(np.flatnonzero(g2 == np.float32(t_dev))[0]), int(np.flatnonzero(g2 == np.float32(t_ref))[0])
    assert abs(i_dev - i_ref) <= 1                                                     # within one round-2 grid step
    # the check that allows no left-out case: the fp64 NLL at the device's choice is the grid's fp64 minimum up to twice the bound
    e = T.sweep_e32(x, gt, g2)["nll"]
    ref2 = ref_rounds[1][1]
    bound = 2.0 * e + 2.0 ** -21 * max(1.0, float(np.abs(ref2).max()))
    print(f"planted 17x23: device {t_dev}, fp64 {t_ref}; fp64 NLL excess at the device's choice {ref2[i_dev] - ref2.min():.3e}, bound {bound:.3e}; "
          f"largest curve error {np.abs(dev_rounds[1][1] - ref2).max():.3e}")
    assert np.abs(dev_rounds[1][1] - ref2).max() <= bound and np.abs(dev_rounds[0][1] - ref_rounds[0][1]).max() <= bound
    assert ref2[i_dev] - ref2.min() <= 2.0 * bound
    ops.check_likelihood_status()


# ---- 7., 8. calibrate_temperature on the reference's fixtures, and the trainer's wrapper ------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


def restate(gm, gt, planes, temps):
    """the fp64 mean NLL of the returned goal map at every temperature over the planes that are finite at all of them
    -> (curve [n_T], the mean of the per-plane bounds [n_T], the number of planes left out, which planes are kept [B, c])"""
    xs, gs = gm[:, planes].contiguous(), gt[:, planes].contiguous()
    ref = T.sweep_ref(xs, gs, temps)["nll"]                                            # [n_T, B, c]
    fin = torch.isfinite(ref).all(dim=0)
    e = T.sweep_e32(xs, gs, temps)["nll"]
    bnd = C.bound(ref, e)[:, fin].mean(dim=1).numpy()
    return ref[:, fin].mean(dim=1).numpy(), bnd, int((~fin).sum()), fin


@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws", "trained_tiny_long"])
def test_calibrate_temperature_on_the_fixtures(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, cal, lk, ops = pkg("utils.evaluate"), pkg("utils.calibrate"), pkg("utils.likelihood"), pkg("ops")
    in_t = O.dist_template(cfg.template_size).to(dev)
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, images = m["B"], g.t("traj"), {"scene0": g.t("scene")[0]}
    wp = list(cfg.waypoints)

    def run():
        torch.manual_seed(11)
        return ev.evaluate(model, loader_for(traj), images, dev, "sdd", None, in_t, wp, "test", n_goal, n_traj, cfg.obs_len, B,
                           cfg.resize_factor, cfg.temperature, return_preds=True, return_samples=True, network=cfg.network)

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    ev.evaluate(model, loader_for(traj), images, dev, "sdd", None, in_t, wp, "test", n_goal, n_traj, cfg.obs_len, B, cfg.resize_factor,
                cfg.temperature, network=cfg.network)                                 # a plain sweep: it may enter the cache
    ade0, fde0, df0, td0 = run()
    gm, gt = torch.from_numpy(td0["goal_map"]), traj[:, cfg.obs_len:].float()
    assert gm.shape == (B, cfg.pred_len, m["H"], m["W"])

    for steps, train_flag in (("waypoints", True), ("all", False), ("goal", False)):
        model.train(train_flag)
        flags = [mod.training for mod in model.modules()]
        before = cache_state()
        rng = (torch.get_rng_state(), torch.cuda.get_rng_state(dev), np.random.get_state())
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")                                            # (a fixture track that leaves the map: one warning)
            out = cal.calibrate_temperature(model, loader_for(traj), images, dev, in_t, wp, cfg.obs_len, B, cfg.resize_factor, cfg.temperature,
                                            network=cfg.network, steps=steps)
        # nothing else moved: the mode, the captured sweeps, the generators, the status flag
        assert [mod.training for mod in model.modules()] == flags and model.training is train_flag
        assert cache_state() == before
        assert torch.equal(torch.get_rng_state(), rng[0]) and torch.equal(torch.cuda.get_rng_state(dev), rng[1])
        now = np.random.get_state()
        assert now[0] == rng[2][0] and np.array_equal(now[1], rng[2][1]) and now[2:] == rng[2][2:]
        ops.check_likelihood_status()
        planes = cal._selected_planes(steps, wp, cfg.pred_len)
        assert set(out) == {"temperature", "nll", "nll_before", "ece", "ece_before", "curve", "temperature_steps", "excluded", "n_planes",
                            "at_boundary"} and len(out["curve"]) == 2 and len(out["temperature_steps"]) == len(planes)
        # every round's curve against the fp64 restatement on the goal map evaluate() returned for the same batch
        bracket = (0.25, 8.0)
        for r, (temps, curve) in enumerate(out["curve"]):
            assert np.array_equal(temps, lk.temperature_grid(bracket[0], bracket[1], 16, include=cfg.temperature)), r
            want, bnd, left_out, fin = restate(gm, gt, planes, temps)
            print(f"{case} {steps} round {r}: largest curve error {np.abs(curve - want).max():.3e} (bound {bnd.min():.3e}), left out {left_out}")
            assert bool((np.abs(curve - want) <= bnd).all()), (case, steps, r, np.abs(curve - want).max())
            bracket = lk.next_bracket(temps, curve)
        assert out["excluded"] == left_out and out["n_planes"] == B * len(planes) - left_out
        k_best, k_in = int(np.flatnonzero(temps == np.float32(out["temperature"]))[0]), int(np.flatnonzero(temps == np.float32(cfg.temperature))[0])
        assert isinstance(out["temperature"], float) and out["nll"] == curve[k_best] and out["nll_before"] == curve[k_in]
        assert abs(out["nll_before"] - want[k_in]) <= bnd[k_in] and out["nll"] <= out["nll_before"]
        assert want[k_best] - want.min() <= 2.0 * bnd.max()                            # (a flat curve passes too: no margin is asked for)
        assert out["at_boundary"] == (out["temperature"] in (0.25, 8.0))
        for c, t_c in enumerate(out["temperature_steps"]):                             # reported only; each is a grid point
            assert np.float32(t_c) in temps or (math.isnan(t_c) and not bool(fin[:, c].any()))
        for k in ("ece", "ece_before"):
            assert 0.0 <= out[k] <= 1.0 or (math.isnan(out[k]) and not bool(fin[:, planes.index(wp[-1])].any()))

    # a following evaluate() is the one before, bit for bit
    ade1, fde1, df1, td1 = run()
    assert ade0 == ade1 and fde0 == fde1 and df0.equals(df1) and set(td0) == set(td1)
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k


def test_trainer_wrapper_returns_the_functions_dict(dev):
    from test_gpu_style_bank import trainer_params
    g = Golden("tiny_long_cws")
    cfg, m = g.cfg(), g.meta
    trn, cal = pkg("models.trainer"), pkg("utils.calibrate")
    traj, scene = g.t("traj"), g.t("scene")[0]
    B = traj.shape[0]
    rows = []
    for i in range(B):
        xy = traj[i].numpy() / cfg.resize_factor
        rows.append(pd.DataFrame({"metaId": i, "sceneId": "scene0", "x": xy[:, 0], "y": xy[:, 1]}))
    df = pd.concat(rows, ignore_index=True)
    text = io.StringIO()
    with contextlib.redirect_stdout(text), warnings.catch_warnings():
        warnings.simplefilter("ignore")
        t = trn.YNetTrainer(trainer_params(cfg, batch_size=B, pred_len=cfg.pred_len), device=dev)
        t.model.load_state_dict(g.state_dict(), strict=True)
        params = dict(t.params)
        got = t.calibrate_temperature(df, {"scene0": scene}, n_temps=8, steps="all")
        images, loader, _ = t.prepare_data(df, {"scene0": scene}, "sdd", "test", cfg.obs_len, cfg.pred_len, cfg.resize_factor, False)
        want = cal.calibrate_temperature(t.model, loader, images, dev, t.templates(), list(cfg.waypoints), cfg.obs_len, B, cfg.resize_factor,
                                         cfg.temperature, n_temps=8, steps="all", network=cfg.network)
    assert t.params == params and t.params["temperature"] == cfg.temperature          # the caller decides
    assert set(got) == set(want)
    for k in want:
        if k == "temperature_steps":
            assert np.array_equal(np.asarray(got[k]), np.asarray(want[k]), equal_nan=True)
        elif k == "curve":
            assert len(got[k]) == len(want[k]) and all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(got[k], want[k]))
        else:
            assert got[k] == want[k] or (isinstance(want[k], float) and math.isnan(want[k]) and math.isnan(got[k])), k
    line = text.getvalue()
    assert f"Calibrated temperature: {got['temperature']}" in line and f"Val NLL: {got['nll_before']} -> {got['nll']}" in line
    assert f"Val goal ECE: {got['ece_before']} -> {got['ece']}" in line
    pkg("ops").check_likelihood_status()

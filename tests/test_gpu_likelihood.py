"""Likelihood scores of the goal map on the MI355X: ynet_map_likelihood against the fp64 restatement of tests/_likelihood_cases.py over
its whole table, the edge rules and the status flag, evaluate(return_likelihood=True) and predict_with_entropy() on the
reference's fixtures, and the captured-sweep cache left alone.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), E32 = the error of the same restatement run in fp32 (recorded
per shape in the table; measured on the spot for the inputs that are not in it).

Measured on the MI355X (largest |device - fp64| over the table): see DESIGN.md section 4.10."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import _likelihood_cases as C
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, what):
    """every finite reference entry within the bound, every other entry of the same class (NaN / +inf / -inf); prints the margin"""
    worst = 0.0
    for k, g in got.items():
        g, r = g.detach().cpu().double(), ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        fin = torch.isfinite(r)
        assert torch.equal(torch.isnan(g), torch.isnan(r)), (what, k, "NaN pattern")
        assert torch.equal(g[~fin & ~torch.isnan(r)], r[~fin & ~torch.isnan(r)]), (what, k, "infinities")
        if fin.any():
            err, bnd = (g - r).abs()[fin], C.bound(r, e[k])[fin]
            worst = max(worst, float((err / bnd).max()))
            print(f"{what} {k}: max error {float(err.max()):.3e} (bound there {float(bnd[err.argmax()]):.3e})")
            assert bool((err <= bnd).all()), (what, k, float(err.max()), float(bnd[err.argmax()]))
    return worst


# ---- (a) the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    (H, W), _, e = C.SHAPES[si]
    for kind in range(len(C.KINDS)):
        x, gt, T, ref = C.case(si, kind)
        dx, dgt = x.to(dev), gt.to(dev)
        what = f"{H}x{W} kind {kind}"
        allthree = ops.map_likelihood(dx, dgt, T)
        assert set(allthree) == set(C.OUTPUTS) and all(v.shape == (C.B, C.C) and v.dtype == torch.float32 for v in allthree.values())
        check(allthree, ref, e, what)
        for k in C.OUTPUTS:                                     # each output alone, the other two NULL: the same bits
            alone = ops.map_likelihood(dx, dgt, T, want=(k,))
            assert set(alone) == {k} and torch.equal(alone[k], allthree[k]), (what, k)
        ent = ops.map_likelihood(dx, None, T, want=("entropy",))      # no ground truth at all
        assert torch.equal(ent["entropy"], allthree["entropy"]), what
    ops.check_likelihood_status()
    assert torch.equal(dx.cpu(), x)                             # the input is read, never written


def test_known_answers(dev):
    ops = pkg("ops")
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        e = C.shape_e32(H, W)
        x, gt, T, want = C.constant_plane(H, W)
        got = ops.map_likelihood(x.to(dev), gt.to(dev), T)
        check(got, {k: torch.tensor([[want[k]]], dtype=torch.float64) for k in C.OUTPUTS}, e, f"constant {H}x{W}")
        assert float(got["hpd"]) == 1.0                         # every pixel is a member: exactly 1
        if H * W < 2:
            continue
        x, gt, T, want = C.spike_planes(H, W)
        got = ops.map_likelihood(x.to(dev), gt.to(dev), T)
        check(got, {k: torch.tensor([want[k]], dtype=torch.float64) for k in C.OUTPUTS}, e, f"spike {H}x{W}")
        assert float(got["hpd"][0, 1]) == 1.0


# ---- (b) the edge rules and the status flag ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.EDGE_SHAPES)
def test_edge_planes_and_status_flag(dev, H, W):
    ops = pkg("ops")
    ops.check_likelihood_status()
    x, gt, T = C.edge_planes(H, W)
    ref, e = C.like_ref(x, gt, T), C.shape_e32(H, W)
    name = {n: i for i, n in enumerate(C.EDGE_PLANES)}
    got = ops.map_likelihood(x.to(dev), gt.to(dev), T)
    with pytest.raises(RuntimeError, match="outside the map"):
        ops.check_likelihood_status()
    ops.check_likelihood_status()                               # raised once, then cleared
    check(got, ref, e, f"edge planes {H}x{W}")                  # the planes beside the offending ones are unaffected
    h = {k: v.cpu() for k, v in got.items()}
    for k in C.OUTPUTS:
        assert math.isnan(float(h[k][0, name["nan"]])) and math.isnan(float(h[k][0, name["all_minus_inf"]])), k
        assert math.isfinite(float(h[k][0, name["plus_and_minus_inf"]])) and math.isfinite(float(h[k][0, name["minus_inf_elsewhere"]])), k
    assert float(h["nll"][0, name["gt_on_minus_inf"]]) == float("inf") and float(h["hpd"][0, name["gt_on_minus_inf"]]) == 1.0
    for i, outside in enumerate(C.edge_outside(H, W)):
        if outside:
            assert math.isnan(float(h["nll"][0, i])) and math.isnan(float(h["hpd"][0, i])) and math.isfinite(float(h["entropy"][0, i])), i
    # without the offending planes the same launch raises nothing
    keep = [i for i, o in enumerate(C.edge_outside(H, W)) if not o]
    clean = ops.map_likelihood(x[:, keep].to(dev), gt[:, keep].to(dev), T)
    ops.check_likelihood_status()
    for k in C.OUTPUTS:
        assert torch.equal(clean[k].cpu()[0].nan_to_num(nan=-7.0), h[k][0, keep].nan_to_num(nan=-7.0)), k


def test_other_layouts(dev):
    ops = pkg("ops")
    x, gt, T = C.many_planes()                                  # 70000 workgroups along blockIdx.x
    got = ops.map_likelihood(x.to(dev), gt.to(dev), T)
    check(got, C.like_ref(x, gt, T), C.e32(x, gt, T), "70000 planes of 2x2")
    for H, W in [(17, 23), (8, 8)]:                             # a channel slice, read in place: batch stride 5 planes, 2 planes scored
        x5, gt, T = C.sliced(H, W)
        d5 = x5.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        got = ops.map_likelihood(view, gt.to(dev), T)
        xs = x5[:, 1:3].contiguous()
        check(got, C.like_ref(xs, gt, T), C.e32(xs, gt, T), f"channel slice {H}x{W}")
        dense = ops.map_likelihood(xs.to(dev), gt.to(dev), T)
        if (H * W) % 4 == 0:                                     # same alignment, same path: the same bits
            assert all(torch.equal(dense[k], got[k]) for k in C.OUTPUTS)
    ops.check_likelihood_status()
    with pytest.raises(ValueError, match="gt_xy"):
        ops.map_likelihood(d5, gt.to(dev), T)
    with pytest.raises(ValueError, match="temperature"):
        ops.map_likelihood(d5, None, 0.0, want=("entropy",))
    with pytest.raises(ValueError, match="ground truth"):
        ops.map_likelihood(d5, None, 1.0)


# ---- (c), (d), (e): the drivers on the reference's fixtures ------------------------------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws"])
def test_evaluate_and_predict_on_the_fixtures(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P = pkg("utils.evaluate"), pkg("utils.predict")
    in_t = O.dist_template(cfg.template_size).to(dev)
    S = g.t("eval/waypoint_samples")                                # [K, B, n_wp, 2], the reference's own samples
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj = m["B"], g.t("traj")

    def run(**kw):
        torch.manual_seed(11)
        return ev.evaluate(model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal,
                           n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=True, return_samples=True,
                           network=cfg.network, forced_samples={0: S}, **kw)

    # (e) with dp=None the flag leaves the captured-sweep cache as it finds it
    ev.evaluate(model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
                cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network)          # a plain sweep: it may enter the cache

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    before = cache_state()
    ade1, fde1, df1, td1 = run(return_likelihood=True)
    assert cache_state() == before
    ade0, fde0, df0, td0 = run()
    assert cache_state() == before

    # (c) the flag changes nothing else, bit for bit
    assert ade0 == ade1 and fde0 == fde1
    assert set(td1) - set(td0) == {"nll_steps", "entropy_steps", "hpd_steps"} and list(df0.columns) == list(df1.columns)[:len(df0.columns)]
    assert list(df1.columns)[len(df0.columns):] == ["nll", "nll_goal", "entropy_goal", "hpd_goal"]
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k
    pkg("ops").check_likelihood_status()                            # evaluate() consumed the flag itself
    assert df0["ade"].equals(df1["ade"]) and df0["fde"].equals(df1["fde"])
    # the returned steps = the fp64 restatement on the RETURNED goal map and the fixture's ground truth (resized pixels)
    gm, gt = torch.from_numpy(td1["goal_map"]), traj[:, cfg.obs_len:].float()
    assert gm.shape == (B, cfg.pred_len, m["H"], m["W"]) and gt.shape == (B, cfg.pred_len, 2)
    ref, e = C.like_ref(gm, gt, cfg.temperature), C.e32(gm, gt, cfg.temperature)
    steps = {k: torch.from_numpy(td1[k + "_steps"]) for k in C.OUTPUTS}
    assert all(v.shape == (B, cfg.pred_len) and v.dtype == torch.float32 for v in steps.values())
    check(steps, ref, e, case)                                      # (a fixture track that leaves the map: NaN nll / hpd there, as the reference)
    inside = torch.isfinite(ref["nll"])
    assert bool(inside.any()) and bool(torch.isfinite(steps["entropy"]).all())
    assert bool(((steps["hpd"][inside] > 0) & (steps["hpd"][inside] <= 1)).all()) and bool((steps["entropy"] >= -1e-6).all())
    assert bool((steps["entropy"] <= math.log(m["H"] * m["W"]) + 1e-5).all())
    # the columns are the stated reductions of those arrays
    assert np.array_equal(df1["nll"].to_numpy(), td1["nll_steps"].mean(axis=1), equal_nan=True)
    assert np.array_equal(df1["nll_goal"].to_numpy(), td1["nll_steps"][:, -1], equal_nan=True)
    assert np.array_equal(df1["entropy_goal"].to_numpy(), td1["entropy_steps"][:, -1])
    assert np.array_equal(df1["hpd_goal"].to_numpy(), td1["hpd_steps"][:, -1], equal_nan=True)
    # without return_preds the columns come alone
    _, _, df2, td2 = ev.evaluate(model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test",
                                 n_goal, n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network,
                                 forced_samples={0: S}, return_likelihood=True)
    assert td2 is None and df2["nll"].equals(df1["nll"]) and df2["hpd_goal"].equals(df1["hpd_goal"])
    assert cache_state() == before

    # (d) predict_with_entropy(): evaluate's entropies bit for bit at the same batch size, every other key predict()'s bit for bit
    args = (model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor,
            cfg.temperature)
    pa = P.predict_with_entropy(*args, network=cfg.network, batch_size=B, forced_samples={0: S})
    pb = P.predict(*args, network=cfg.network, batch_size=B, forced_samples={0: S})
    assert set(pa) - set(pb) == {"entropy"} and pa["entropy"].is_cuda and pa["entropy"].shape == (B, cfg.pred_len)
    assert np.array_equal(pa["entropy"].cpu().numpy(), td1["entropy_steps"])
    for k in pb:
        assert torch.equal(pa[k], pb[k]), k

    # a report left pending by the caller's own map_likelihood call is raised by evaluate(return_likelihood=True), not swallowed
    ops = pkg("ops")
    ops.map_likelihood(torch.zeros(1, 1, 2, 2, device=dev), torch.full((1, 1, 2), 9.0, device=dev), 1.0)
    with pytest.raises(RuntimeError, match="outside the map"):
        run(return_likelihood=True)
    ops.check_likelihood_status()

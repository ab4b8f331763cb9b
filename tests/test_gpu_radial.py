"""Radial goal-map scores on the MI355X: ynet_map_radial against the fp64 restatement of tests/_radial_cases.py over its whole table, the
bit-for-bit cases, the ring edges, the plane-level rules and the status flag, and evaluate(return_radial=...) on the reference's fixture.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), for ring and tail + n * 2^-40 (the kernel's fixed-point
truncation); E32 = the error of the same restatement run in fp32 (recorded per shape in the table; measured on the spot for the inputs
that are not in it).

Measured on the MI355X (largest |device - fp64| / bound over the table): see DESIGN.md section 4.16."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import _likelihood_cases as LC
import _radial_cases as C
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, H, W, what):
    """every finite reference entry within the bound, NaN where the reference is NaN; prints the margin -> the worst error / bound"""
    worst = 0.0
    for k, g in got.items():
        g, r = g.detach().cpu().double(), ref[k]
        assert g.shape == r.shape, (what, k, g.shape, r.shape)
        fin = torch.isfinite(r)
        assert torch.equal(torch.isnan(g), ~fin), (what, k, "NaN pattern")
        if fin.any():
            err, bnd = (g - r).abs()[fin], C.bound(r, e[k], k, H, W)[fin]
            worst = max(worst, float((err / bnd).max()))
            print(f"{what} {k}: max error {float(err.max()):.3e} (bound there {float(bnd[err.argmax()]):.3e})")
            assert bool((err <= bnd).all()), (what, k, float(err.max()), float(bnd[err.argmax()]))
    return worst


def check_sums(got, what):
    """sum ring + tail = 1 within 2^-22; mean^2 <= mean_sq (Jensen), up to the roundings of the two stored fp32 values (2^-22 relative)"""
    ring, tail = got["ring"].cpu().double(), got["tail"].cpu().double()
    fin = torch.isfinite(tail)
    assert float((ring.sum(dim=-1) + tail - 1)[fin].abs().max()) <= 2.0 ** -22, what
    assert bool((ring[fin] >= 0).all()) and bool((tail[fin] >= 0).all())
    mean, mean_sq = got["mean"].cpu().double()[fin], got["mean_sq"].cpu().double()[fin]
    assert bool((mean * mean <= mean_sq * (1 + 2.0 ** -22)).all()), what


# ---- (a) the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    ops.check_radial_status()
    (H, W), _, e = C.SHAPES[si]
    worst = 0.0
    for kind in range(len(C.KINDS)):
        x, gt, T, refs = C.case(si, kind)
        dx, dgt = x.to(dev), gt.to(dev)
        for R, ref in refs.items():
            what = f"{H}x{W} kind {kind} n_rings {R}"
            got = ops.map_radial(dx, dgt, R, T)
            assert set(got) == set(C.OUTPUTS) and got["ring"].shape == (C.B, C.C, R)
            assert all(got[k].shape == (C.B, C.C) for k in ("tail", "mean", "mean_sq")) and all(v.dtype == torch.float32 for v in got.values())
            worst = max(worst, check(got, ref, e, H, W, what))
            check_sums(got, what)
        default = ops.map_radial(dx, dgt, None, T)                  # n_rings=None is the default count
        Rd = C.default_rings(H, W)
        assert default["ring"].shape[-1] == Rd
        full = ops.map_radial(dx, dgt, Rd, T)
        assert all(torch.equal(default[k], full[k]) for k in C.OUTPUTS), what
        for k in C.OUTPUTS:                                         # each output alone, the other three NULL: the same bits
            alone = ops.map_radial(dx, dgt, Rd, T, want=(k,))
            assert set(alone) == {k} and torch.equal(alone[k], full[k]), (what, k)
        # the ground truth outside the map raised nothing
    assert ops.check_radial_status() is False
    assert torch.equal(dx.cpu(), x)                                 # the input is read, never written
    print(f"{H}x{W}: worst error / bound {worst:.3f}")


# ---- (b) bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", [(5, 4), (17, 23), (96, 160), (256, 256)])
def test_exact_inputs_bit_for_bit(dev, H, W):
    """logits in {0, 40}: fp32 weights 0.5 and 1, exact sums -- ring, tail and mean_sq are the restatement's, rounded to fp32"""
    ops = pkg("ops")
    for R in (3, C.default_rings(H, W)):
        x, gt, T = C.exact_planes(H, W)
        ref = C.radial_ref(x, gt, T, R)
        got = ops.map_radial(x.to(dev), gt.to(dev), R, T)
        for k in ("ring", "tail", "mean_sq"):
            assert torch.equal(got[k].cpu(), ref[k].float()), (H, W, R, k)
        check({"mean": got["mean"]}, ref, C.e32(x, gt, T, R), H, W, f"exact {H}x{W} n_rings {R}")
        # a channel view, read in place: batch stride 5 planes, 2 planes scored ((17, 23): they start off a 16-byte boundary)
        x5, gt5, T = C.exact_planes(H, W, channels=5)
        d5 = x5.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        xs, gts = x5[:, 1:3].contiguous(), gt5[:, 1:3].contiguous()
        ref = C.radial_ref(xs, gts, T, R)
        got = ops.map_radial(view, gts.to(dev), R, T)
        for k in ("ring", "tail", "mean_sq"):
            assert torch.equal(got[k].cpu(), ref[k].float()), (H, W, R, k, "view")
    assert ops.check_radial_status() is False


def test_ring_edges(dev):
    """one pixel of weight at d2 = 20, 25, 34, 36, 45, 49, 50 from g lands in ring 4, 5, 5, 6, 6, 7, 7 (see _radial_cases.RING_EDGES for
    why 20, 34 and 45 stand in for 24, 35 and 48)"""
    ops = pkg("ops")
    x, gt, T = C.ring_edge_planes()
    got = {k: v.cpu() for k, v in ops.map_radial(x.to(dev), gt.to(dev), 10, T).items()}
    for i, (_, d2, ring) in enumerate(C.RING_EDGES):
        want = torch.zeros(10)
        want[ring] = 1.0
        assert torch.equal(got["ring"][0, i], want), (d2, got["ring"][0, i])
        assert float(got["tail"][0, i]) == 0.0 and float(got["mean_sq"][0, i]) == float(d2)
        assert abs(float(got["mean"][0, i]) - math.sqrt(d2)) <= 2.0 ** -23 * math.sqrt(d2)
    assert ops.check_radial_status() is False


def test_ring_zero_is_the_likelihood_of_the_ground_truth_pixel(dev):
    """ring[0] holds the pixel g alone: it equals exp(-nll) of ops.map_likelihood on the same logits, within the two kernels' summed bounds"""
    ops = pkg("ops")
    for si in (2, 3, 5, 6):
        (H, W), _, e = C.SHAPES[si]
        for kind in range(len(C.KINDS)):
            x, gt, T, refs = C.case(si, kind)
            dx, dgt = x.to(dev), gt.to(dev)
            ring0 = ops.map_radial(dx, dgt, 1, T, want=("ring",))["ring"][..., 0].cpu().double()
            nll = ops.map_likelihood(dx, dgt, T, want=("nll",))["nll"].cpu().double()
            inside = torch.isfinite(nll)                              # (the ground truth outside the map has a ring 0, and no nll)
            assert ops.check_likelihood_status(raise_error=False) == bool((~inside).any())
            nll_ref = LC.like_ref(x, gt, T)["nll"]
            b_nll = LC.bound(nll_ref, LC.e32(x, gt, T)["nll"])
            p = refs[1]["ring"][..., 0]
            bnd = C.bound(p, e["ring"], "ring", H, W) + p * torch.expm1(b_nll)
            err = (ring0 - torch.exp(-nll)).abs()
            assert bool(inside.any()) and bool((err[inside] <= bnd[inside]).all()), (H, W, kind, float(err[inside].max()))
            assert bool((ring0[~inside] == 0).all())                 # no pixel of the map is the ground truth
    assert ops.check_radial_status() is False


def test_two_runs_give_the_same_bits(dev):
    ops = pkg("ops")
    x, gt, T, _ = C.case(6, 4)
    dx, dgt = x.to(dev), gt.to(dev)
    a, b = ops.map_radial(dx, dgt, None, T), ops.map_radial(dx, dgt, None, T)
    for k in C.OUTPUTS:
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k


# ---- (c) the plane-level rules and the status flag --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.RULE_SHAPES)
def test_plane_rules_and_status_flag(dev, H, W):
    ops = pkg("ops")
    ops.check_radial_status()
    x, gt, T, raises = C.rule_planes(H, W)
    ref, e = C.radial_ref(x, gt, T, 3), C.e32(x, gt, T, 3)
    got = ops.map_radial(x.to(dev), gt.to(dev), 3, T)
    with pytest.raises(RuntimeError, match="map_radial: a ground-truth position"):
        ops.check_radial_status()
    assert ops.check_radial_status() is False                       # raised once, then cleared
    check(got, ref, e, H, W, f"rule planes {H}x{W}")                # NaN exactly where the rules say, the planes beside them unaffected
    name = {n: i for i, n in enumerate(C.RULE_PLANES)}
    h = {k: v.cpu() for k, v in got.items()}
    for k in C.OUTPUTS:
        assert bool(torch.isnan(h[k][0, name["nan_logit"]]).all()) and bool(torch.isfinite(h[k][0, name["plain"]]).all()), k
        assert bool(torch.isfinite(h[k][0, name["gt_outside_valid"]]).all()) and bool(torch.isfinite(h[k][0, name["gt_at_the_margin"]]).all()), k
    # without the planes that must raise, the same launch raises nothing -- the NaN logit and the ground truth outside the map included
    keep = [i for i, r in enumerate(raises) if not r]
    clean = ops.map_radial(x[:, keep].to(dev), gt[:, keep].to(dev), 3, T)
    assert ops.check_radial_status() is False
    for k in C.OUTPUTS:
        assert torch.equal(clean[k].cpu()[0].nan_to_num(nan=-7.0), h[k][0, keep].nan_to_num(nan=-7.0)), k
    with pytest.raises(ValueError, match="gt_xy"):
        ops.map_radial(x.to(dev), gt[:, :2].to(dev))
    with pytest.raises(ValueError, match="temperature"):
        ops.map_radial(x.to(dev), gt.to(dev), temperature=0.0)
    for bad in (0, 1025):
        with pytest.raises(ValueError, match="n_rings"):
            ops.map_radial(x.to(dev), gt.to(dev), bad)


# ---- (d) evaluate(return_radial=...) on the reference's fixture ------------------------------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


def test_evaluate_returns_the_reduced_profile(dev):
    g = Golden("tiny_short_mosa1")
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, ops, R_ = pkg("utils.evaluate"), pkg("ops"), pkg("utils.radial")
    in_t = O.dist_template(cfg.template_size).to(dev)
    S = g.t("eval/waypoint_samples")                                # [K, B, n_wp, 2], the reference's own samples
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, H, W = m["B"], g.t("traj"), m["H"], m["W"]

    def run(**kw):
        torch.manual_seed(11)
        return ev.evaluate(model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal,
                           n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=True, return_samples=True,
                           network=cfg.network, forced_samples={0: S}, **kw)

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    before = cache_state()
    out0 = run()
    opt = {"radii": (0, 1, 3, 40), "k": (1, 4)}
    out1 = run(return_radial=opt)
    assert cache_state() == before and ops.check_radial_status() is False
    # with the flag off: the tuple of the parent commit
    assert len(out0) == 4
    ade0, fde0, df0, td0 = out0
    assert list(df0.columns) == ["metaId", "sceneId", "ade", "fde"] and len(df0) == B
    assert set(td0) == {"groundtruth", "prediction", "waypoint_sample", "goal_map", "goal_sigmoid_map", "metaId", "sceneId"}
    # with it on: nothing else moves, bit for bit
    ade1, fde1, df1, td1 = out1
    assert ade0 == ade1 and fde0 == fde1 and df0.equals(df1[list(df0.columns)])
    new = ["radial_mean_goal", "radial_rms_goal", "hit0_goal", "hit1_goal", "hit3_goal", "hit40_goal", "best_of_1_lower_goal", "best_of_1_upper_goal",
           "best_of_4_lower_goal", "best_of_4_upper_goal"]
    assert list(df1.columns) == list(df0.columns) + new
    steps = {"radial_mean_steps": (), "radial_rms_steps": (), "radial_hit_steps": (4,), "best_of_k_lower_steps": (2,), "best_of_k_upper_steps": (2,)}
    assert set(td1) - set(td0) == set(steps)
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k
    for k, tail in steps.items():
        assert td1[k].shape == (B, cfg.pred_len) + tail, k
    # the returned quantities = ops.map_radial + utils/radial on the RETURNED goal map and the fixture's ground truth (resized pixels)
    gm, gt = torch.from_numpy(td1["goal_map"]).to(dev), traj[:, cfg.obs_len:].float().to(dev)
    n_rings = max(ops.radial_rings(H, W), 40)
    prof = ops.map_radial(gm, gt, n_rings, cfg.temperature)
    far = R_.farthest_corner(gt, H, W)
    lower, upper = R_.expected_best_of_k(prof["ring"], prof["tail"], opt["k"], far)
    rf = cfg.resize_factor
    want = {"radial_mean_steps": prof["mean"].double() / rf, "radial_rms_steps": prof["mean_sq"].double().sqrt() / rf,
            "radial_hit_steps": R_.hit_rate(prof["ring"], opt["radii"]), "best_of_k_lower_steps": lower / rf, "best_of_k_upper_steps": upper / rf}
    for k, v in want.items():
        assert np.array_equal(td1[k], v.cpu().numpy(), equal_nan=True), k
    assert bool(np.isfinite(td1["radial_mean_steps"]).all())      # a track that leaves the map is still scored
    # and the profile behind them is the restatement's
    x_host = torch.from_numpy(td1["goal_map"])
    ref = C.radial_ref(x_host, gt.cpu(), cfg.temperature, n_rings)
    check(prof, ref, C.e32(x_host, gt.cpu(), cfg.temperature, n_rings), H, W, "fixture")
    # the columns are the last step
    assert np.array_equal(df1["radial_mean_goal"].to_numpy(), td1["radial_mean_steps"][:, -1])
    assert np.array_equal(df1["radial_rms_goal"].to_numpy(), td1["radial_rms_steps"][:, -1])
    assert np.array_equal(df1["hit3_goal"].to_numpy(), td1["radial_hit_steps"][:, -1, 2])
    assert np.array_equal(df1["best_of_4_upper_goal"].to_numpy(), td1["best_of_k_upper_steps"][:, -1, 1])
    assert (df1["hit0_goal"] == 0).all() and (df1["best_of_1_lower_goal"] <= df1["radial_mean_goal"] + 1e-6).all()
    assert (df1["radial_mean_goal"] <= df1["best_of_1_upper_goal"] + 1e-6).all() and (df1["best_of_4_upper_goal"] <= df1["best_of_1_upper_goal"]).all()
    # without return_preds the columns come alone; True is the documented default
    _, _, df2, td2 = ev.evaluate(model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test",
                                 n_goal, n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network,
                                 forced_samples={0: S}, return_radial=True)
    assert td2 is None and df2["radial_mean_goal"].equals(df1["radial_mean_goal"])
    assert [c for c in df2.columns if c.startswith(("hit", "best_of"))] == ["hit4_goal", "hit8_goal", "hit16_goal", "best_of_1_lower_goal", "best_of_1_upper_goal",
                                                                            "best_of_5_lower_goal", "best_of_5_upper_goal", "best_of_20_lower_goal",
                                                                            "best_of_20_upper_goal"]
    # a ground truth the kernel cannot score: a warning, NaN scores, ADE / FDE as before
    bad = traj.clone()
    bad[0, -1, 0] = 30000.0
    with pytest.warns(UserWarning, match="return_radial"):
        _, _, df3, _ = ev.evaluate(model, loader_for(bad), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test",
                                   n_goal, n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network,
                                   forced_samples={0: S}, return_radial=True)
    assert math.isnan(df3["radial_mean_goal"][0]) and math.isnan(df3["hit4_goal"][0]) and bool(np.isfinite(df3["radial_mean_goal"][1:]).all())
    assert ops.check_radial_status() is False                       # evaluate() consumed the flag itself

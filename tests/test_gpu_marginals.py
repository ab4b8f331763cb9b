"""Goal-map marginals on the MI355X: ynet_map_marginals against the fp64 restatement of tests/_marginals_cases.py over its whole table,
the bit-for-bit cases, the closed forms, the plane-level rules and the status flag, the vector and the element-wise path against each other, and
evaluate(return_marginals=...) / predict_with_intervals() on the reference's fixture.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|) + the kernel's fixed-point truncation (n * 2^-39 for col, row and
pit, 2 * side * n * 2^-39 for crps); E32 = the error of the same restatement run in fp32 (recorded per shape in the table; measured on
the spot for the inputs that are not in it).

Measured on the MI355X (largest |device - fp64| / bound over the table): see DESIGN.md section 4.17."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import _marginals_cases as C
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
    """col and row each sum to 1 within 2^-22; pit lower <= upper, both in [0, 1]"""
    for k in ("col", "row"):
        v = got[k].cpu().double()
        fin = torch.isfinite(v).all(dim=-1)
        assert float((v.sum(dim=-1) - 1)[fin].abs().max()) <= 2.0 ** -22, (what, k)
        assert bool((v[fin] >= 0).all())
    pit = got["pit"].cpu()
    fin = torch.isfinite(pit).all(dim=-1)
    assert bool((pit[..., 0] <= pit[..., 1])[fin].all()) and bool((pit[fin] >= 0).all()) and bool((pit[fin] <= 1).all()), what


# ---- (a) the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    ops.check_marginals_status()
    (H, W), _, e = C.SHAPES[si]
    worst = 0.0
    for kind in range(len(C.KINDS)):
        x, gt, T, ref = C.case(si, kind)
        dx, dgt = x.to(dev), gt.to(dev)
        what = f"{H}x{W} kind {kind}"
        full = ops.map_marginals(dx, dgt, T)
        assert set(full) == set(C.OUTPUTS) and all(v.dtype == torch.float32 and v.is_cuda for v in full.values())
        assert full["col"].shape == (C.B, C.C, W) and full["row"].shape == (C.B, C.C, H)
        assert full["crps"].shape == (C.B, C.C, 2) and full["pit"].shape == (C.B, C.C, 2, 2)
        worst = max(worst, check(full, ref, e, H, W, what))
        check_sums(full, what)
        for k in C.OUTPUTS:                                         # each output alone, the other three NULL: the same bits
            alone = ops.map_marginals(dx, dgt, T, want=(k,))
            assert set(alone) == {k} and torch.equal(alone[k], full[k]), (what, k)
        free = ops.map_marginals(dx, None, T, want=("col", "row"))  # without a ground truth: the same bits
        assert set(free) == {"col", "row"} and torch.equal(free["col"], full["col"]) and torch.equal(free["row"], full["row"]), what
        assert torch.equal(dx.cpu(), x)                             # the input is read, never written
    assert ops.check_marginals_status() is False                    # the ground truth outside the map raised nothing
    print(f"{H}x{W}: worst error / bound {worst:.3f}")


# ---- (b) bit for bit ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.EXACT_SHAPES)
def test_exact_inputs_bit_for_bit(dev, H, W):
    """logits in {0, 40}: fp32 weights 0.5 and 1, exact sums -- col, row and pit are the restatement's, rounded to fp32"""
    ops = pkg("ops")
    x, gt, T = C.exact_planes(H, W)
    ref = C.marginals_ref(x, gt, T)
    got = ops.map_marginals(x.to(dev), gt.to(dev), T)
    for k in ("col", "row", "pit"):
        assert torch.equal(got[k].cpu(), ref[k].float()), (H, W, k)
    check({"crps": got["crps"]}, ref, C.e32(x, gt, T), H, W, f"exact {H}x{W}")
    # a channel view, read in place: batch stride 5 planes, 2 planes scored ((17, 23): they start off a 16-byte boundary)
    x5, gt5, T = C.exact_planes(H, W, channels=5)
    d5 = x5.to(dev)
    view = d5[:, 1:3]
    assert not view.is_contiguous()
    xs, gts = x5[:, 1:3].contiguous(), gt5[:, 1:3].contiguous()
    ref = C.marginals_ref(xs, gts, T)
    got = ops.map_marginals(view, gts.to(dev), T)
    for k in ("col", "row", "pit"):
        assert torch.equal(got[k].cpu(), ref[k].float()), (H, W, k, "view")
    assert torch.equal(d5.cpu(), x5)
    assert ops.check_marginals_status() is False


# ---- (c) closed forms --------------------------------------------------------------------------------------------------------------------
def test_one_hot_and_two_mass_planes(dev):
    ops = pkg("ops")
    H, W = C.CLOSED_MAP
    x, gt, T, (a, r) = C.one_hot_planes()
    got = {k: v.cpu() for k, v in ops.map_marginals(x.to(dev), gt.to(dev), T).items()}
    g = torch.round(gt)
    assert torch.equal(got["crps"][0, :, 0], (g[0, :, 0] - a).abs()) and torch.equal(got["crps"][0, :, 1], (g[0, :, 1] - r).abs())      # |a - g|, exactly
    assert got["crps"][0, 3].tolist() == [a + 5.0, 0.0] and got["crps"][0, 4].tolist() == [0.0, H + 3.0 - r]
    assert got["pit"][0].tolist() == [[[0.0, 1.0], [0.0, 1.0]], [[1.0, 1.0], [1.0, 1.0]], [[0.0, 0.0], [0.0, 0.0]], [[0.0, 0.0], [0.0, 1.0]],
                                      [[0.0, 1.0], [1.0, 1.0]]]
    for i in range(x.shape[1]):
        assert got["col"][0, i].tolist() == [1.0 if j == a else 0.0 for j in range(W)] and got["row"][0, i].tolist() == [1.0 if j == r else 0.0 for j in range(H)]
    x, gt, T, (a, b, r) = C.two_mass_planes()
    got = {k: v.cpu() for k, v in ops.map_marginals(x.to(dev), gt.to(dev), T).items()}
    for i, gx in enumerate((a, 6, b)):
        assert float(got["crps"][0, i, 0]) == (abs(a - gx) + abs(b - gx)) / 2 - (b - a) / 4 and float(got["crps"][0, i, 1]) == 0.0
    assert got["pit"][0, :, 0].tolist() == [[0.0, 0.5], [0.5, 0.5], [0.5, 1.0]]
    assert ops.check_marginals_status() is False


# ---- (d) the plane-level rules and the status flag --------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.RULE_SHAPES)
def test_plane_rules_and_status_flag(dev, H, W):
    ops = pkg("ops")
    ops.check_marginals_status()
    x, gt, T, raises = C.rule_planes(H, W)
    ref, e = C.marginals_ref(x, gt, T), C.e32(x, gt, T)
    got = ops.map_marginals(x.to(dev), gt.to(dev), T)
    with pytest.raises(RuntimeError, match="map_marginals: a ground-truth position"):
        ops.check_marginals_status()
    assert ops.check_marginals_status() is False                    # raised once, then cleared
    check(got, ref, e, H, W, f"rule planes {H}x{W}")                # NaN exactly where the rules say, the planes beside them unaffected
    name = {n: i for i, n in enumerate(C.RULE_PLANES)}
    h = {k: v.cpu() for k, v in got.items()}
    for k in C.OUTPUTS:
        for n in ("nan_logit", "all_minus_inf"):
            assert bool(torch.isnan(h[k][0, name[n]]).all()), (k, n)
        for n in ("plain", "gt_outside_valid", "gt_at_the_margin"):
            assert bool(torch.isfinite(h[k][0, name[n]]).all()), (k, n)
    for n in ("gt_nan", "gt_inf", "gt_20000_away"):
        assert bool(torch.isnan(h["crps"][0, name[n]]).all()) and bool(torch.isnan(h["pit"][0, name[n]]).all()), n
        assert bool(torch.isfinite(h["col"][0, name[n]]).all()) and bool(torch.isfinite(h["row"][0, name[n]]).all()), n
    # exactly at the margin: 16384 pixels left of the map adds 16384 to the CRPS of the border pixel, the other end likewise
    m = name["gt_at_the_margin"]
    border = ops.map_marginals(x[:, m:m + 1].to(dev), torch.tensor([[[0.0, H - 1.0]]], device=dev), T, want=("crps",))["crps"].cpu().double()
    away = h["crps"][0, m].double() - border[0, 0]
    assert float((away - C.GT_MARGIN).abs().max()) <= 2.0 ** -23 * 2 * C.GT_MARGIN, away
    assert h["pit"][0, m].tolist() == [[0.0, 0.0], [1.0, 1.0]]
    # without the planes that must raise, the same launch raises nothing -- the NaN logit and the ground truth outside the map included
    keep = [i for i, r in enumerate(raises) if not r]
    clean = ops.map_marginals(x[:, keep].to(dev), gt[:, keep].to(dev), T)
    assert ops.check_marginals_status() is False
    for k in C.OUTPUTS:
        assert torch.equal(clean[k].cpu()[0].nan_to_num(nan=-7.0), h[k][0, keep].nan_to_num(nan=-7.0)), k
    # the marginals alone need no ground truth and raise nothing, whatever it holds
    free = ops.map_marginals(x.to(dev), None, T, want=("col", "row"))
    assert ops.check_marginals_status() is False and torch.equal(free["col"].cpu().nan_to_num(nan=-7.0), h["col"].nan_to_num(nan=-7.0))
    # the wrapper's refusals that need a device tensor
    for want in (("crps",), ("col", "pit"), C.OUTPUTS):
        with pytest.raises(ValueError, match="crps and pit need the ground truth"):
            ops.map_marginals(x.to(dev), None, want=want)
    with pytest.raises(ValueError, match="gt_xy"):
        ops.map_marginals(x.to(dev), gt[:, :2].to(dev))
    with pytest.raises(ValueError, match="temperature"):
        ops.map_marginals(x.to(dev), gt.to(dev), temperature=0.0)
    with pytest.raises(RuntimeError, match="side above 2048"):
        ops.map_marginals(torch.zeros(1, 1, 1, 2049, device=dev), None, want=("col",))


# ---- (e), (f) the same bits run after run and path after path ----------------------------------------------------------------------------
def test_two_runs_give_the_same_bits(dev):
    ops = pkg("ops")
    x, gt, T, _ = C.case(11, 4)                                     # 256 x 256, trained-looking
    dx, dgt = x.to(dev), gt.to(dev)
    a, b = ops.map_marginals(dx, dgt, T), ops.map_marginals(dx, dgt, T)
    for k in C.OUTPUTS:
        assert bool(torch.isfinite(a[k]).all()) and torch.equal(a[k], b[k]), k


@pytest.mark.parametrize("H,W", [(5, 4), (3, 64), (6, 16), (9, 256), (2, 1024), (256, 256)])
def test_vector_path_and_element_path_give_the_same_bits(dev, H, W):
    """the same planes once on a 16-byte boundary (16-byte vectors) and once as a view that starts 4 bytes off one (element by element):
    integer sums are order-free, so col, row and pit are the same bits; crps sums the same fp64 terms in the same order"""
    ops = pkg("ops")
    si = [hw for hw, _, _ in C.SHAPES].index((H, W))
    for kind in (1, 4):
        x, gt, T, _ = C.case(si, kind)
        aligned = x.to(dev)
        buf = torch.empty(x.numel() + 1, device=dev)
        shifted = buf[1:].view(x.shape)
        shifted.copy_(aligned)
        assert aligned.data_ptr() % 16 == 0 and shifted.data_ptr() % 16 == 4 and (H * W) % 4 == 0
        a, b = ops.map_marginals(aligned, gt.to(dev), T), ops.map_marginals(shifted, gt.to(dev), T)
        for k in C.OUTPUTS:
            assert torch.equal(a[k], b[k]), (H, W, kind, k)


# ---- (g) evaluate(return_marginals=...) on the reference's fixture ---------------------------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


def fixture(dev):
    g = Golden("tiny_short_mosa1")
    cfg, m = g.cfg(), g.meta
    return g, cfg, m, build_model(cfg, g.state_dict(), dev), O.dist_template(cfg.template_size).to(dev)


def test_evaluate_returns_the_reduced_marginals(dev):
    g, cfg, m, model, in_t = fixture(dev)
    ev, ops, M = pkg("utils.evaluate"), pkg("ops"), pkg("utils.marginals")
    S = g.t("eval/waypoint_samples")                                # [K, B, n_wp, 2], the reference's own samples
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, H, W = m["B"], g.t("traj"), m["H"], m["W"]
    levels = (0.5, 0.9)

    def run(tr=traj, preds=True, **kw):
        torch.manual_seed(11)
        return ev.evaluate(model, loader_for(tr), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal,
                           n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=preds, return_samples=preds,
                           network=cfg.network, forced_samples={0: S}, **kw)

    ade0, fde0, df0, td0 = run()
    ade1, fde1, df1, td1 = run(return_marginals=levels)
    assert ops.check_marginals_status() is False
    # with the flag off: the tuple of the parent commit; with it on nothing else moves, bit for bit
    assert list(df0.columns) == ["metaId", "sceneId", "ade", "fde"] and len(df0) == B
    assert ade0 == ade1 and fde0 == fde1 and df0.equals(df1[list(df0.columns)])
    new = ["crps_x_goal", "crps_y_goal", "crps_goal", "pit_x_goal", "pit_y_goal", "width50_x_goal", "inside50_x_goal", "width50_y_goal",
           "inside50_y_goal", "width90_x_goal", "inside90_x_goal", "width90_y_goal", "inside90_y_goal"]
    assert list(df1.columns) == list(df0.columns) + new
    steps = {"crps_steps": (2,), "pit_steps": (2, 2), "interval_steps": (2, 2, 2)}
    assert set(td1) - set(td0) == set(steps)
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k
    for k, tail in steps.items():
        assert td1[k].shape == (B, cfg.pred_len) + tail, k
    # the returned quantities against the fp64 restatement of the RETURNED goal map and the fixture's ground truth (resized pixels)
    x_host, gt = torch.from_numpy(td1["goal_map"]), traj[:, cfg.obs_len:].float()
    ref, e = C.marginals_ref(x_host, gt, cfg.temperature), C.e32(x_host, gt, cfg.temperature)
    rf = cfg.resize_factor
    got = {"crps": torch.from_numpy(td1["crps_steps"]) * rf, "pit": torch.from_numpy(td1["pit_steps"])}
    assert bool(torch.isfinite(ref["crps"]).all())                  # a track that leaves the map is still scored
    # (crps_steps is the launch's fp32 value divided by resize_factor in fp64: multiplying back costs one more rounding of 2^-53)
    check(got, {k: ref[k] for k in got}, e, H, W, "fixture")
    prof = ops.map_marginals(x_host.to(dev), gt.to(dev), cfg.temperature)
    assert np.array_equal(td1["crps_steps"], (prof["crps"].double() / rf).cpu().numpy()) and np.array_equal(td1["pit_steps"], prof["pit"].cpu().numpy())
    check({k: prof[k] for k in ("col", "row")}, ref, e, H, W, "fixture profiles")
    # the intervals: utils/marginals.py on the launch's profiles, and against the restatement's fp64 profiles wherever no CDF value of
    # those lies within the bound of a quantile (there the fp32 profile may round to the neighbouring pixel)
    iv = torch.stack([M.central_intervals(prof["col"], levels), M.central_intervals(prof["row"], levels)], dim=2).cpu()
    assert np.array_equal(td1["interval_steps"], iv.numpy()) and bool((iv[..., 0] <= iv[..., 1]).all()) and bool((iv >= 0).all())
    qs = torch.tensor([(1 - q) / 2 for q in levels] + [(1 + q) / 2 for q in levels], dtype=torch.float64)
    clear = 0
    for a, key in enumerate(("col", "row")):
        cdf = M.profile_cdf(ref[key])
        side = cdf.shape[-1]
        tol = 2.0 * side * float(C.bound(torch.ones(()), e[key], key, H, W))
        safe = ((cdf[..., None, :] - qs[:, None]).abs() > tol).all(dim=-1)      # [B, pred_len, 2 L]
        want = M.central_intervals(ref[key], levels)                            # [B, pred_len, L, 2]
        safe = torch.stack([safe[..., :len(levels)], safe[..., len(levels):]], dim=-1)
        assert bool((iv[:, :, a][safe] == want[safe]).all()), key
        clear += int(safe.sum())
    assert clear > 0
    # inside: the rounded ground truth against the interval
    gr = torch.round(gt.double())
    want_in = ((gr[..., None] >= iv[..., 0].double()) & (gr[..., None] <= iv[..., 1].double())).double()      # [B, pred_len, 2, L]
    # the columns are the last step, in the units of FDE
    crps = td1["crps_steps"][:, -1]
    assert np.array_equal(df1["crps_x_goal"].to_numpy(), crps[:, 0]) and np.array_equal(df1["crps_y_goal"].to_numpy(), crps[:, 1])
    assert np.array_equal(df1["crps_goal"].to_numpy(), crps[:, 0] + crps[:, 1])
    pit = td1["pit_steps"][:, -1].astype(np.float64)
    assert np.array_equal(df1["pit_x_goal"].to_numpy(), 0.5 * (pit[:, 0, 0] + pit[:, 0, 1])) and np.array_equal(df1["pit_y_goal"].to_numpy(), 0.5 * (pit[:, 1, 0] + pit[:, 1, 1]))
    for l, pct in enumerate((50, 90)):
        for a, axis in enumerate("xy"):
            assert np.array_equal(df1[f"width{pct}_{axis}_goal"].to_numpy(), (iv[:, -1, a, l, 1] - iv[:, -1, a, l, 0]).double().numpy() / rf)
            assert np.array_equal(df1[f"inside{pct}_{axis}_goal"].to_numpy(), want_in[:, -1, a, l].numpy())
    # without return_preds the columns come alone; True is the documented default
    _, _, df2, td2 = run(preds=False, return_marginals=True)
    assert td2 is None and all(df2[c].equals(df1[c]) for c in df1.columns)
    # a ground truth the kernel cannot score: a warning, NaN scores, ADE / FDE as before
    bad = traj.clone()
    bad[0, -1, 0] = 30000.0
    with pytest.warns(UserWarning, match="return_marginals"):
        _, _, df3, _ = run(tr=bad, preds=False, return_marginals=True)
    assert math.isnan(df3["crps_goal"][0]) and math.isnan(df3["pit_x_goal"][0]) and math.isnan(df3["inside50_y_goal"][0])
    assert bool(np.isfinite(df3["width50_x_goal"]).all()) and bool(np.isfinite(df3["crps_goal"][1:]).all())      # the interval needs no ground truth
    assert ops.check_marginals_status() is False                    # evaluate() consumed the flag itself


# ---- (h) predict_with_intervals() ---------------------------------------------------------------------------------------------------------
def test_predict_with_intervals(dev):
    g, cfg, m, model, in_t = fixture(dev)
    P, ops, M = pkg("utils.predict"), pkg("ops"), pkg("utils.marginals")
    S = g.t("eval/waypoint_samples")
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, scene = m["B"], g.t("traj"), g.t("scene")[0]
    levels = (0.25, 0.5, 0.9)
    args = (model, scene, traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor, cfg.temperature)
    pa = P.predict_with_intervals(*args, levels=levels, network=cfg.network, batch_size=B, forced_samples={0: S}, return_maps=True)
    pb = P.predict(*args, network=cfg.network, batch_size=B, forced_samples={0: S}, return_maps=True)
    assert set(pa) - set(pb) == {"median_xy", "interval_xy", "marginal_mean_xy"}
    for k in pb:                                                    # predict()'s own keys, bit for bit
        assert torch.equal(pa[k], pb[k]), k
    assert pa["median_xy"].shape == (B, cfg.pred_len, 2) and pa["interval_xy"].shape == (B, cfg.pred_len, 2, 3, 2)
    assert pa["marginal_mean_xy"].shape == (B, cfg.pred_len, 2) and all(pa[k].is_cuda and pa[k].dtype == torch.float32 for k in set(pa) - set(pb))
    # = utils/marginals.py on ops.map_marginals of the returned maps
    prof = ops.map_marginals(pa["goal_map"], None, cfg.temperature, want=("col", "row"))
    axes = (prof["col"], prof["row"])
    assert torch.equal(pa["median_xy"], torch.stack([M.quantiles(p, (0.5,))[..., 0] for p in axes], dim=-1).float())
    assert torch.equal(pa["interval_xy"], torch.stack([M.central_intervals(p, levels) for p in axes], dim=2).float())
    assert torch.equal(pa["marginal_mean_xy"], torch.stack([M.profile_mean(p) for p in axes], dim=-1).float())
    lo, hi, med = pa["interval_xy"][..., 0], pa["interval_xy"][..., 1], pa["median_xy"][..., None]
    assert bool((lo <= med).all()) and bool((med <= hi).all()) and bool((lo >= 0).all())
    assert bool((hi[..., 0] <= torch.tensor([m["W"] - 1.0, m["H"] - 1.0], device=dev)).all())
    assert bool((lo[..., 1:] <= lo[..., :-1]).all()) and bool((hi[..., 1:] >= hi[..., :-1]).all())      # the intervals are nested
    if B > 1:      # chunked = unchunked
        h = (B + 1) // 2
        pc = P.predict_with_intervals(*args, levels=levels, network=cfg.network, batch_size=h, forced_samples={0: S[:, :h], h: S[:, h:]})
        for k in ("median_xy", "interval_xy", "marginal_mean_xy"):
            assert torch.equal(pc[k], pa[k]), k

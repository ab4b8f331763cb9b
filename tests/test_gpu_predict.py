"""predict() on the MI355X: ynet_score_rank_samples against an fp64 restatement, the driver against evaluate() and the reference's
fixtures, reproducibility, a C2-sized call that leaves a following training step untouched, and a goal map beyond 2^31 elements."""
import numpy as np
import pandas as pd
import pytest
import torch

import _predict_cases as C
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


def unrank(ranked, order):
    """[B, K, ...] rows in ranked order -> rows in sample order (row order[b, r] <- ranked row r)"""
    out = torch.empty_like(ranked)
    idx = order.long().view(order.shape + (1,) * (ranked.dim() - 2)).expand_as(ranked)
    return out.scatter_(1, idx, ranked)


# ---- 1. the kernel ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", C.BS)
@pytest.mark.parametrize("n_wp", C.NWPS)
@pytest.mark.parametrize("K", C.KS)
def test_score_rank_kernel_matches_fp64(dev, K, n_wp, B):
    ops = pkg("ops")
    prob, wps, trajs = C.make_case(K, n_wp, B)
    want = C.score_fp64(prob, wps)                                  # [B, K], sample order
    rf = 0.25
    d_prob, d_wps, d_trajs = (torch.from_numpy(a).to(dev) for a in (prob, wps, trajs))
    ranked, goals, score, order = ops.score_rank_samples(d_prob, d_wps, d_trajs, rf)
    assert ranked.shape == (B, K, C.PRED, 2) and goals.shape == (B, K, n_wp, 2) and score.shape == (B, K)
    assert order.shape == (B, K) and order.dtype == torch.int32
    order_h = order.cpu().numpy().astype(np.int64)
    frac = C.check_order(order_h, want, n_wp)
    score_h = score.cpu().numpy().astype(np.float64)
    want_sorted = np.take_along_axis(want, order_h, axis=1)
    rel = np.abs(score_h - want_sorted) / np.abs(want_sorted)
    print(f"K {K} n_wp {n_wp} B {B}: pairs inside the gap {frac:.5f}, max relative score error {rel.max():.3e}")
    assert frac < 0.01
    assert rel.max() <= 1e-5
    assert (score_h[:, :-1] >= score_h[:, 1:]).all()                # handed back sorted
    idx = order.long().t()                                          # [K, B]
    cols = torch.arange(B, device=dev)[None].expand(K, B)
    assert torch.equal(ranked, (d_trajs[idx, cols] / rf).permute(1, 0, 2, 3))           # bit-equal to torch's own division
    assert torch.equal(goals, d_wps[idx, cols].permute(1, 0, 2, 3))


def test_score_rank_other_resize_factors_and_odd_lengths(dev):
    """pred_len odd (rows of 8-byte pairs only), K * pred_len not a multiple of 64, resize factors that are no powers of two."""
    ops = pkg("ops")
    for K, n_wp, B, pred_len, rf in ((33, 2, 5, 1, 0.1185), (3, 1, 2, 29, 0.5021), (64, 3, 9, 7, 1.0)):
        prob, wps, trajs = C.make_case(K, n_wp, B, pred_len=pred_len)
        d_prob, d_wps, d_trajs = (torch.from_numpy(a).to(dev) for a in (prob, wps, trajs))
        ranked, goals, score, order = ops.score_rank_samples(d_prob, d_wps, d_trajs, rf)
        want = C.score_fp64(prob, wps)
        C.check_order(order.cpu().numpy().astype(np.int64), want, n_wp)
        idx = order.long().t()
        cols = torch.arange(B, device=dev)[None].expand(K, B)
        assert torch.equal(ranked, (d_trajs[idx, cols] / rf).permute(1, 0, 2, 3)), (K, pred_len, rf)
        assert torch.equal(goals, d_wps[idx, cols].permute(1, 0, 2, 3))


def test_score_rank_refusals(dev):
    ops = pkg("ops")
    prob, wps, trajs = (torch.from_numpy(a).to(dev) for a in C.make_case(20, 1, 3))
    with pytest.raises(RuntimeError, match="1 .. 64"):
        ops.score_rank_samples(prob, wps.repeat(4, 1, 1, 1), trajs.repeat(4, 1, 1, 1), 0.25)
    with pytest.raises(RuntimeError, match="1 .. 64"):
        ops.score_rank_samples(prob, wps[:0], trajs[:0], 0.25)
    with pytest.raises(ValueError, match="not contiguous"):
        ops.score_rank_samples(prob, wps.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3), trajs, 0.25)
    with pytest.raises(ValueError, match="not contiguous"):
        ops.score_rank_samples(prob[:, :, :, ::2], wps, trajs, 0.25)
    for bad in ((C.W, 0.0), (0.0, C.H), (-1.0, 3.0), (float("nan"), 3.0)):      # just outside the map (x = W, y = H), negative, NaN
        w2 = wps.clone()
        w2[5, 1, 0] = torch.tensor(bad, device=dev)
        with pytest.raises(RuntimeError, match="outside"):
            ops.score_rank_samples(prob, w2, trajs, 0.25)
    ops.score_rank_samples(prob, wps, trajs, 0.25)                               # the flag was cleared: a good call passes again
    # fractional samples (TTST / CWS way-points) are scored at the nearest pixel, halves to even like the patch windows
    w3 = wps.clone()
    w3[..., 0] = (wps[..., 0] + 0.4).clamp(max=C.W - 1)
    a, b = ops.score_rank_samples(prob, w3, trajs, 0.25), ops.score_rank_samples(prob, wps, trajs, 0.25)
    assert torch.equal(a[2], b[2]) and torch.equal(a[3], b[3])


# ---- 2. the driver against evaluate() and the reference's fixtures --------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws"])
def test_predict_is_consistent_with_evaluate_and_the_reference(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P = pkg("utils.evaluate"), pkg("utils.predict")
    in_t = O.dist_template(cfg.template_size).to(dev)
    S = g.t("eval/waypoint_samples")                                # [K, B, n_wp, 2], the reference's own samples
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    K, B = S.shape[0], m["B"]
    traj = g.t("traj")
    _, _, _, td = ev.evaluate(
        model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
        cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=True, network=cfg.network, forced_samples={0: S})
    res = P.predict(model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len,
                    cfg.resize_factor, cfg.temperature, network=cfg.network, batch_size=B, forced_samples={0: S})
    assert set(res) == {"trajectories", "waypoints", "scores", "order"} and all(v.is_cuda for v in res.values())
    assert res["trajectories"].shape == (B, K, cfg.pred_len, 2) and res["waypoints"].shape == (B, K, len(cfg.waypoints), 2)
    best = torch.from_numpy(td["prediction"]).to(dev)               # [B, pred, 2]: evaluate's best-of-K, original pixels
    hit = (res["trajectories"] == best[:, None]).flatten(2).all(dim=2).any(dim=1)
    assert bool(hit.all()), "evaluate's best-of-K prediction is not among predict's K trajectories, bit for bit"
    in_order = unrank(res["trajectories"], res["order"]).permute(1, 0, 2, 3).cpu().numpy() * cfg.resize_factor
    np.testing.assert_allclose(in_order, g.z["eval/trajs"], rtol=1e-5, atol=1e-4)       # the reference's K trajectories, resized pixels
    assert torch.equal(unrank(res["waypoints"], res["order"]).permute(1, 0, 2, 3).cpu(), S.float())
    sc = res["scores"].cpu()
    assert bool(torch.isfinite(sc).all()) and bool((sc[:, :-1] >= sc[:, 1:]).all())
    # the tensor form of forced_samples and one chunk per agent give the same bits
    res1 = P.predict(model, g.t("scene")[0], traj[:, :cfg.obs_len].numpy(), in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len,
                     cfg.resize_factor, cfg.temperature, network=cfg.network, batch_size=1, forced_samples=S)
    # (up to the rounding of another batch size: compared in sample order, 1e-4 px of the resized map)
    assert torch.equal(unrank(res1["waypoints"], res1["order"]), unrank(res["waypoints"], res["order"]))
    np.testing.assert_allclose(unrank(res1["trajectories"], res1["order"]).cpu().numpy() * cfg.resize_factor,
                               unrank(res["trajectories"], res["order"]).cpu().numpy() * cfg.resize_factor, rtol=1e-5, atol=1e-4)
    with pytest.raises(ValueError, match="never cut silently"):
        P.predict(model, g.t("scene")[0], traj, in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor, cfg.temperature)


# ---- 3. draws: the same as evaluate()'s, and reproducible ----------------------------------------------------------------------
@pytest.mark.parametrize("case,use_ttst,use_cws", [("tiny_short_mosa1", False, False), ("tiny_long_train", False, False),
                                                   ("tiny_long_ttst_cws_ntraj2", True, True)])
def test_predict_takes_evaluates_draws_and_is_reproducible(dev, case, use_ttst, use_cws):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P = pkg("utils.evaluate"), pkg("utils.predict")
    in_t = O.dist_template(cfg.template_size).to(dev)
    n_goal, n_traj = (m["n_goal"], m["n_traj"]) if use_ttst else (20, 1)
    cws = (m.get("cws_params") or None) if use_cws else None
    rel = m.get("rel_thresh") or 0.002
    traj, B = g.t("traj"), m["B"]

    def seed():
        np.random.seed(123)
        torch.manual_seed(77)

    seed()
    _, _, _, td = ev.evaluate(
        model, loader_for(traj), {"scene0": g.t("scene")[0]}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
        cfg.obs_len, B, cfg.resize_factor, cfg.temperature, use_ttst, use_cws, rel, cws, return_preds=True, return_samples=True,
        network=cfg.network)
    args = (model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor,
            cfg.temperature)
    kw = dict(use_TTST=use_ttst, use_CWS=use_cws, rel_thresh=rel, CWS_params=cws, network=cfg.network, batch_size=B, return_maps=True)
    seed()
    a = P.predict(*args, **kw)
    seed()
    b = P.predict(*args, **kw)
    want = torch.from_numpy(td["waypoint_sample"]).permute(0, 2, 1, 3)              # [B, K, n_wp, 2] in sample order
    assert torch.equal(unrank(a["waypoints"], a["order"]).cpu(), want)
    assert set(a) == {"trajectories", "waypoints", "scores", "order", "goal_map", "goal_sigmoid_map"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert np.array_equal(a["goal_map"].cpu().numpy(), td["goal_map"]) and np.array_equal(a["goal_sigmoid_map"].cpu().numpy(), td["goal_sigmoid_map"])
    best = torch.from_numpy(td["prediction"]).to(dev)
    assert bool((a["trajectories"] == best[:, None]).flatten(2).all(dim=2).any(dim=1).all())


# ---- 4. a C2-sized call, and what it leaves behind ------------------------------------------------------------------------------
def test_c2_sized_predict_leaves_the_training_step_untouched(dev):
    g = Golden("trained_short_full")                                # the C2 architecture at 256^2
    cfg, m = g.cfg(), g.meta
    te, trn, P = pkg("utils.train_epoch"), pkg("models.trainer"), pkg("utils.predict")
    S = cfg.template_size
    in_t, gt_t = O.dist_template(S).to(dev), O.gaussian_template(S, cfg.kernlen, cfg.nsig).to(dev)
    traj = g.t("traj")
    assert (m["H"], m["W"]) == (256, 256)

    def step(with_predict):
        model = build_model(cfg, g.state_dict(), dev)
        model.train()
        res = None
        if with_predict:
            torch.manual_seed(5)
            observed = traj[:, :cfg.obs_len].repeat(32 // traj.shape[0], 1, 1)       # B 32
            res = P.predict(model, g.t("scene")[0], observed, in_t, list(cfg.waypoints), 20, 1, cfg.obs_len, cfg.resize_factor,
                            cfg.temperature, network=cfg.network, batch_size=32)
            assert model.training
        torch.manual_seed(6)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        out = te.train_epoch(model, loader_for(traj), {"scene0": g.t("scene")[0]}, opt, trn.HipBCEWithLogitsLoss(), cfg.loss_scale, dev,
                             "sdd", None, gt_t, in_t, list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, m["B"], 10000,
                             cfg.resize_factor, cfg.network, False)
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}, res

    out0, p0, _ = step(False)
    out1, p1, res = step(True)
    assert res["trajectories"].shape == (32, 20, cfg.pred_len, 2)
    assert bool(torch.isfinite(res["scores"]).all()) and bool(torch.isfinite(res["trajectories"]).all())
    assert bool((res["order"].long().sort(dim=1)[0] == torch.arange(20, device=dev)[None]).all())
    assert out0 == out1, (out0, out1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n


# ---- 5. offsets beyond 2^31 elements ----------------------------------------------------------------------------------------------
def test_goal_map_beyond_2_31_elements(dev):
    ops = pkg("ops")
    B, n_wp, H, W, K, pred_len = 33, 1, 8192, 8192, 20, 12
    assert B * n_wp * H * W > 2 ** 31
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 12 * 2 ** 30, "the 8.9 GB goal map of this test does not fit beside what the device already holds"
    prob = torch.empty((B, n_wp, H, W), device=dev, dtype=torch.float32)
    gen = torch.Generator(device=dev).manual_seed(9)
    for b in range(B):
        prob[b].uniform_(1e-3, 0.999, generator=gen)
    rng = np.random.default_rng(4)
    wps = np.stack([rng.integers(0, W, size=(K, B, n_wp)), rng.integers(0, H, size=(K, B, n_wp))], axis=-1).astype(np.float32)
    wps[0, B - 1, 0] = (W - 1, H - 1)                               # the very last element of the array
    wps[K - 1, B - 1, 0] = (W - 1, H - 1)
    trajs = rng.standard_normal(size=(K, B, pred_len, 2)).astype(np.float32)
    d_wps, d_trajs = torch.from_numpy(wps).to(dev), torch.from_numpy(trajs).to(dev)
    ranked, goals, score, order = ops.score_rank_samples(prob, d_wps, d_trajs, 0.25)
    for b in (0, B - 2, B - 1):
        x, y = torch.from_numpy(wps[:, b, 0, 0]).long().to(dev), torch.from_numpy(wps[:, b, 0, 1]).long().to(dev)
        p = prob[b, 0][y, x].cpu().numpy().astype(np.float64)
        want = np.log(p + 1e-12)[None]                              # [1, K]
        o = order[b].cpu().numpy().astype(np.int64)[None]
        C.check_order(o, want, n_wp)
        got = score[b].cpu().numpy().astype(np.float64)[None]
        want_sorted = np.take_along_axis(want, o, axis=1)
        assert (np.abs(got - want_sorted) <= 1e-5 * np.abs(want_sorted)).all(), b
        assert torch.equal(ranked[b], d_trajs[torch.from_numpy(o[0]).to(dev), b] / 0.25)
    del prob
    torch.cuda.empty_cache()

"""Deterministic goal modes on the MI355X: ynet_map_modes against the CPU greedy loop of tests/_modes_cases.py over its whole table
and its planted planes, other layouts (70000 planes, a channel slice, a view beyond 2^31 elements), and predict_modes on the
reference's fixtures.

xy, logit and count are compared EXACTLY (the picks are decided on raw fp32 values: no case is ambiguous); the masses within
|device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), E32 = the error of the same sums taken in fp32 on the CPU (recorded per shape in
the table; measured on the spot for the inputs that are not in it).

Measured on the MI355X (largest mass error over the table): see DESIGN.md section 4.11."""
import numpy as np
import pytest
import torch

import _modes_cases as C
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, what, mass=True):
    """picks bit for bit; every mass within the bound -> the largest mass error over its bound"""
    assert set(got) == ({"xy", "logit", "count", "mass"} if mass else {"xy", "logit", "count"}), (what, set(got))
    assert got["count"].dtype == torch.int32 and got["xy"].dtype == torch.float32
    assert torch.equal(got["count"].cpu(), ref["count"]), (what, "count", got["count"].cpu(), ref["count"])
    assert torch.equal(got["xy"].cpu(), ref["xy"]), (what, "xy")
    assert torch.equal(C.bits(got["logit"]), C.bits(ref["logit"])), (what, "logit")
    if not mass:
        return 0.0
    g, r = got["mass"].cpu().double(), ref["mass"][0]
    assert g.shape == r.shape and bool(torch.isfinite(g).all()), (what, "mass")
    err, bnd = (g - r).abs(), C.bound(r, e)
    assert bool((err <= bnd).all()), (what, "mass", float(err.max()), float(bnd.view(-1)[err.argmax()]))
    return float((err / bnd).max())


# ---- 1. the kernel against the table ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_the_greedy_loop_over_the_table(dev, si):
    ops = pkg("ops")
    (H, W), _, e = C.SHAPES[si]
    worst = 0.0
    for s, kind, r in C.table():
        if s != si:
            continue
        x, T, ref = C.case(si, kind, r)
        dx = x.to(dev)
        for M in C.table_modes(si):
            what = f"{H}x{W} kind {kind} r {r} M {M}"
            got = ops.map_modes(dx, M, r, T)
            assert got["xy"].shape == (C.LC.B, C.LC.C, M, 2) and got["mass"].shape == (C.LC.B, C.LC.C, M)
            worst = max(worst, check(got, C.cut(ref, M), e, what))
            bare = ops.map_modes(dx, M, r, want_mass=False)           # without the masses: the same picks, bit for bit
            check(bare, C.cut(ref, M), e, what + " no mass", mass=False)
            again = ops.map_modes(dx, M, r, T)                        # two runs: the same bits, masses included
            assert all(torch.equal(C.bits(got[k]) if got[k].dtype == torch.float32 else got[k],
                                   C.bits(again[k]) if again[k].dtype == torch.float32 else again[k]) for k in got), what
        assert torch.equal(dx.cpu(), x)                               # the input is read, never written
    ops.check_modes_status()
    print(f"{H}x{W}: largest mass error over its bound {worst:.3f}")


def test_planted_planes(dev):
    ops = pkg("ops")
    ops.check_modes_status()
    for name, x, M, r, T, want in C.planted():
        ref = C.modes_ref(x, M, r, T, (torch.float64, torch.float32))
        got = ops.map_modes(x.to(dev), M, r, T)
        check(got, ref, C.e32_of(ref), name)
        C.check_planted(name, {k: v.cpu() for k, v in got.items()}, want)
        check(ops.map_modes(x.to(dev), M, r, want_mass=False), ref, 0.0, name, mass=False)
        if want.get("nan"):                                           # both launches met the NaN plane
            with pytest.raises(RuntimeError, match="NaN"):
                ops.check_modes_status()
            # without the NaN plane the neighbours give the same bits
            keep = [i for i, c in enumerate(want["count"]) if c >= 0]
            clean = ops.map_modes(x[:, keep].to(dev), M, r, T)
            for k in got:
                assert torch.equal(C.bits(clean[k].float()), C.bits(got[k][:, keep].float())), (name, k)
        ops.check_modes_status()                                      # raised once, then cleared; the other planes raise nothing


# ---- 2. other layouts ----------------------------------------------------------------------------------------------------------------------
def test_other_layouts(dev):
    ops = pkg("ops")
    x, M, r, T = C.many_planes()                                      # 70000 workgroups along blockIdx.x
    ref = C.many_planes_ref(x, M, r, T, (torch.float64, torch.float32))
    check(ops.map_modes(x.to(dev), M, r, T), ref, C.e32_of(ref), "70000 planes of 2x2")
    for H, W in [(17, 23), (8, 8)]:                                   # a channel slice, read in place: batch stride 5 planes, 2 planes ranked
        x5, M, r, T = C.sliced(H, W)
        d5 = x5.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        xs = x5[:, 1:3].contiguous()
        ref = C.modes_ref(xs, M, r, T, (torch.float64, torch.float32))
        got = ops.map_modes(view, M, r, T)
        check(got, ref, C.e32_of(ref), f"channel slice {H}x{W}")
        dense = ops.map_modes(xs.to(dev), M, r, T)
        assert all(torch.equal(dense[k], got[k]) for k in got)        # a plane's sums do not depend on where it lies
    ops.check_modes_status()
    with pytest.raises(ValueError, match="n_modes"):
        ops.map_modes(d5, 65, 3)
    with pytest.raises(ValueError, match="radius"):
        ops.map_modes(d5, 20, -1)
    with pytest.raises(ValueError, match="temperature"):
        ops.map_modes(d5, 20, 3, 0.0)
    ops.map_modes(d5, 20, 3, 0.0, want_mass=False)                    # the temperature is read only with the masses
    with pytest.raises(RuntimeError, match="cap"):
        ops.map_modes(torch.zeros(1, 1, 512, 513, device=dev), 2, 1)


def test_view_whose_last_plane_starts_beyond_2_31_elements(dev):
    ops = pkg("ops")
    H, W, M, r = 17, 23, 20, 3
    stride = 2 ** 31 + 8                                              # elements between the two images of the view
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 10 * 2 ** 30, "the 8.6 GB buffer of this test does not fit beside what the device already holds"
    buf = torch.empty(stride + 2 * H * W, device=dev, dtype=torch.float32)      # never initialised: only the viewed planes are written
    view = buf.as_strided((2, 2, H, W), (stride, H * W, W, 1))
    x, T, ref = C.case(3, 1, r)
    xs = x[:, :2].contiguous()
    view.copy_(xs.to(dev))
    assert view.data_ptr() == buf.data_ptr() and view[1, 1].data_ptr() - buf.data_ptr() == 4 * (stride + H * W)
    got = ops.map_modes(view, M, r, T)
    want = {k: (v[:, :2] if k != "mass" else [m[:, :2] for m in v]) for k, v in C.cut(ref, M).items()}
    check(got, want, C.shape_e32(H, W), "view beyond 2^31 elements")
    ops.check_modes_status()
    del buf, view
    torch.cuda.empty_cache()


# ---- 3. predict_modes on the reference's fixtures ------------------------------------------------------------------------------------------
def unrank(ranked, order):
    """[B, K, ...] rows in ranked order -> rows in sample order (row order[b, r] <- ranked row r)"""
    out = torch.empty_like(ranked)
    idx = order.long().view(order.shape + (1,) * (ranked.dim() - 2)).expand_as(ranked)
    return out.scatter_(1, idx, ranked)


@pytest.mark.parametrize("case,cws", [("tiny_short_mosa1", False), ("tiny_long_cws", True), ("tiny_long_cws", False)])
def test_predict_modes_on_the_fixtures(dev, case, cws):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P, ops = pkg("utils.evaluate"), pkg("utils.predict"), pkg("ops")
    in_t = O.dist_template(cfg.template_size).to(dev)
    traj, B = g.t("traj"), m["B"]
    wps, n_wp = list(cfg.waypoints), len(cfg.waypoints)
    cws_params = (m.get("cws_params") or None) if cws else None
    assert not cws or cws_params is not None
    M, r = 6, 2
    assert (M - 1) * C.disk_area(r) < m["H"] * m["W"]
    args = (model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, wps)
    tail = (cfg.obs_len, cfg.resize_factor, cfg.temperature)
    kw = dict(CWS_params=cws_params, network=cfg.network)

    # what must be left alone: the training mode, the filter caches, evaluate()'s sweep cache, the generators
    ev.evaluate(model, [(traj.clone(), [__import__("pandas").DataFrame({"metaId": np.arange(B)})], "scene0")], {"scene0": g.t("scene")[0]}, dev,
                "sdd", None, in_t, wps, "test", 20, 1, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network)

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    def filters():      # what the packed / transformed filter caches are keyed by: every parameter's identity, address and version
        return ev._weights_token(model)

    model.train()
    torch.manual_seed(11)
    before = P.predict(*args, 4, 1, *tail, network=cfg.network)        # a predict() call under a fixed seed, for later
    cache0, filt0 = cache_state(), filters()
    torch.manual_seed(3)
    np.random.seed(4)
    t_state, n_state = torch.get_rng_state(), np.random.get_state()
    a = P.predict_modes(*args, M, r, *tail, return_maps=True, **kw)
    assert torch.equal(torch.get_rng_state(), t_state)                # no generator was read
    assert all(np.array_equal(p, q) for p, q in zip(np.random.get_state(), n_state))
    assert model.training and cache_state() == cache0 and filters() == filt0
    torch.manual_seed(99)
    np.random.seed(98)
    b = P.predict_modes(*args, M, r, *tail, return_maps=True, **kw)   # another seed: the same bits
    assert set(a) == {"trajectories", "waypoints", "scores", "order", "goal_map", "goal_sigmoid_map", "mode_mass", "mode_logit"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    assert a["trajectories"].shape == (B, M, cfg.pred_len, 2) and a["waypoints"].shape == (B, M, n_wp, 2)
    assert a["mode_mass"].shape == (B, M) and a["mode_logit"].shape == (B, M) and a["order"].dtype == torch.int32

    # the goals = the reference loop on the RETURNED goal map, exactly; masses within the bound; both handed back in ranked order
    gm = a["goal_map"].cpu()
    ref = C.modes_ref(gm[:, wps[-1]:wps[-1] + 1], M, r, cfg.temperature, (torch.float64, torch.float32))
    way = unrank(a["waypoints"], a["order"])                          # [B, M, n_wp, 2] in mode order
    assert torch.equal(way[:, :, -1].cpu(), ref["xy"][:, 0])
    assert torch.equal(C.bits(unrank(a["mode_logit"], a["order"])), C.bits(ref["logit"][:, 0]))
    mass = unrank(a["mode_mass"], a["order"]).cpu().double()
    assert bool(((mass - ref["mass"][0][:, 0]).abs() <= C.bound(ref["mass"][0][:, 0], C.e32_of(ref))).all())
    if n_wp == 1:
        assert torch.equal(a["order"].cpu(), torch.arange(M, dtype=torch.int32)[None].expand(B, M))
    elif not cws:                                                     # the top pixel of each intermediate plane, shared by the modes
        for j, w in enumerate(wps[:-1]):
            top = C.modes_ref(gm[:, w:w + 1], 1, 0, 1.0)["xy"][:, 0, 0]             # [B, 2]
            assert torch.equal(way[:, :, j].cpu(), top[:, None].expand(B, M, 2))

    # every other result = predict() forced onto those way-points, bit for bit
    forced = way.permute(1, 0, 2, 3).contiguous()                     # [M, B, n_wp, 2]
    f = P.predict(*args, M, 1, *tail, network=cfg.network, forced_samples=forced)
    for k in ("trajectories", "waypoints", "scores", "order"):
        assert torch.equal(a[k], f[k]), k

    # chunking changes nothing
    c = P.predict_modes(*args, M, r, *tail, batch_size=max(1, B // 2), return_maps=True, **kw)
    for k in ("waypoints", "order", "mode_mass", "mode_logit"):
        assert torch.equal(a[k], c[k]), k
    c1 = P.predict_modes(*args, M, r, *tail, batch_size=B, **kw)
    for k in c1:
        assert torch.equal(a[k], c1[k]), k

    # predict() after it gives the bits it gave before it
    torch.manual_seed(11)
    after = P.predict(*args, 4, 1, *tail, network=cfg.network)
    for k in before:
        assert torch.equal(before[k], after[k]), k

    # modes that cannot fit are refused once H and W are known; too few finite logits raise at the sync point, naming the agent
    with pytest.raises(ValueError, match="may not fit"):
        P.predict_modes(*args, 64, 8, *tail, **kw)
    ops.check_modes_status()


def test_predict_modes_leaves_the_training_step_untouched_and_names_a_short_agent(dev):
    g = Golden("tiny_short_mosa1")
    cfg, m = g.cfg(), g.meta
    te, trn, P, ops = pkg("utils.train_epoch"), pkg("models.trainer"), pkg("utils.predict"), pkg("ops")
    S = cfg.template_size
    in_t, gt_t = O.dist_template(S).to(dev), O.gaussian_template(S, cfg.kernlen, cfg.nsig).to(dev)
    traj = g.t("traj")
    import pandas as pd

    def step(with_modes):
        model = build_model(cfg, g.state_dict(), dev)
        model.train()
        if with_modes:
            res = P.predict_modes(model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), 6, 2, cfg.obs_len, cfg.resize_factor,
                                  cfg.temperature, network=cfg.network)
            assert model.training and bool(torch.isfinite(res["trajectories"]).all())
        torch.manual_seed(6)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        loader = [(traj.clone(), [pd.DataFrame({"metaId": np.arange(traj.shape[0])})], "scene0")]
        out = te.train_epoch(model, loader, {"scene0": g.t("scene")[0]}, opt, trn.HipBCEWithLogitsLoss(), cfg.loss_scale, dev, "sdd", None,
                             gt_t, in_t, list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, m["B"], 10000, cfg.resize_factor, cfg.network, False)
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}

    out0, p0 = step(False)
    out1, p1 = step(True)
    assert out0 == out1, (out0, out1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n

    # an agent whose goal map holds too few logits above -inf: an ordinary input with a defined result -- the chunk raises and names it
    model = build_model(cfg, g.state_dict(), dev)
    pred_goal = model.pred_goal

    def holed(features):
        out = pred_goal(features).clone()
        out[1, :, 1:] = float("-inf")                                 # agent 1 keeps one row of candidates: radius 2 leaves room for few modes
        out[1, :, 0, 5:] = float("-inf")
        return out

    model.pred_goal = holed
    with pytest.raises(RuntimeError, match="predict_modes: agent 1:"):
        P.predict_modes(model, g.t("scene")[0], traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), 6, 2, cfg.obs_len, cfg.resize_factor,
                        cfg.temperature, network=cfg.network)
    ops.check_modes_status()
    ops.check_patch_status()                                          # nothing left pending for the next caller

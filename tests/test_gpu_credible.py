"""Credible regions on the MI355X: ynet_map_credible against the fp64 restatement of tests/_credible_cases.py over its whole table and its
planted planes, determinism, the edge rules, other layouts (70000 planes, a channel slice, a view beyond 2^31 elements), the sibling
kernel's hpd as a cross-check, and evaluate(return_sharpness=...) / predict_with_regions() on the reference's fixtures.

Acceptance of EVERY launch (`_credible_cases.accept`): the threshold is a logit of its plane, area == #{x >= threshold}, the fp64 share
of {x >= threshold} is >= q - delta, the fp64 share of {x > threshold} is < q + delta, and |mass - fp64 share| <= delta, with
delta = 2 * E32 + 2^-21 * max(1, |fp64|) + n * 2^-39 (E32 recorded per shape in the table; measured on the spot for the inputs that are
not in it).  (area, threshold) equal the restatement's EXACTLY on the integer grid and the planted planes; on the continuous kinds they
may differ only where the acceptance still holds, and in at most 5 % of the cases.

Measured on the MI355X: see DESIGN.md section 4.14."""
import math

import numpy as np
import pandas as pd
import pytest
import torch

import _credible_cases as C
import _likelihood_cases as LC
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def host(got):
    assert set(got) == {"area", "threshold", "mass"}, set(got)
    assert got["area"].dtype == torch.int32 and got["threshold"].dtype == torch.float32 and got["mass"].dtype == torch.float32
    assert all(v.is_cuda for v in got.values())
    return {k: v.cpu() for k, v in got.items()}


def same_regions(got, ref):
    """(area, threshold) equal to the restatement's -> [B, C, L] bool"""
    return (got["area"].long() == ref["area"]) & (got["threshold"] == ref["threshold"])


def spot_e32(x, thr, T):
    """E32 of an input that is not in the table: the fp32 shares at `thr` against the fp64 ones"""
    return float((C.share(x, thr, T, torch.float32).double() - C.share(x, thr, T)).abs().max())


def run_case(ops, dx, si, kind, ti, L):
    """one launch of the table -> (host results, agreement with the restatement [B, C, L])"""
    (H, W), _ = C.SHAPES[si]
    x, T, ref, _, _ = C.case(si, kind, ti)
    levels, idx = C.LEVEL_SETS[L], C.level_index(L)
    got = host(ops.map_credible(dx, levels, T))
    assert got["area"].shape == (C.B, C.C, L)
    ge, d = C.accept(x, T, levels, got, C.shape_e32(H, W))
    q = torch.from_numpy(C.levels32(levels))
    print(f"{H}x{W} {C.KINDS[kind]} T {T} L {L}: largest (q - share) / delta {float(((q - ge) / d).max()):.3f}, "
          f"|mass - share| / delta {float(((got['mass'].double() - ge).abs() / d).max()):.3f}")
    # nested: area and mass do not fall as q rises
    assert bool((got["area"][..., 1:] >= got["area"][..., :-1]).all()) and bool((got["mass"][..., 1:] >= got["mass"][..., :-1]).all())
    return got, same_regions(got, {k: v[..., idx] for k, v in ref.items()})


# ---- 1. the kernel against fp64 over the whole table ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", range(len(C.KINDS)), ids=[k.replace(" ", "_") for k in C.KINDS])
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _ in C.SHAPES])
def test_kernel_against_fp64_over_the_table(dev, si, kind):
    ops = pkg("ops")
    dx = C.case(si, kind, 0)[0].to(dev)
    for ti in range(len(C.TEMPS)):
        for L in C.LEVEL_SETS:
            _, same = run_case(ops, dx, si, kind, ti, L)
            if kind == C.GRID:      # plateaus: no boundary lies near a level
                assert bool(same.all()), (C.SHAPES[si][0], C.TEMPS[ti], L)
    ops.check_credible_status()
    assert torch.equal(dx.cpu(), C.case(si, kind, 0)[0])      # the input is read, never written


def test_continuous_cases_off_the_restatement_are_few(dev):
    """Where the device's region differs from the restatement's, the acceptance (run_case) still held; such cases stay below 5 %."""
    ops = pkg("ops")
    off = total = 0
    for si in range(2, len(C.SHAPES)):
        for kind in C.CONTINUOUS:
            dx = C.case(si, kind, 0)[0].to(dev)
            for ti in range(len(C.TEMPS)):
                _, same = run_case(ops, dx, si, kind, ti, 8)
                per_level = same.all(dim=0).all(dim=0)
                off += int((~per_level).sum())
                total += per_level.numel()
    print(f"{off} of {total} continuous (shape, kind, T, level) cases differ from the restatement")
    assert total == 6 * 3 * 2 * 8 and off <= 0.05 * total


def test_two_runs_give_the_same_bits(dev):
    ops = pkg("ops")
    for si in range(len(C.SHAPES)):
        for kind in range(len(C.KINDS)):
            dx = C.case(si, kind, 0)[0].to(dev)
            for T in C.TEMPS:
                a, b = ops.map_credible(dx, C.LEVELS8, T), ops.map_credible(dx, C.LEVELS8, T)
                for k in a:
                    assert torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)), (C.SHAPES[si][0], kind, T, k)


# ---- 2. planted planes --------------------------------------------------------------------------------------------------------------------
def test_planted_planes(dev):
    ops = pkg("ops")
    for name, x, levels, T, areas in C.planted():
        got = host(ops.map_credible(x.to(dev), levels, T))
        ref = C.restate(x, levels, T)
        C.accept(x, T, levels, got, spot_e32(x, ref["threshold"], T))
        assert bool(same_regions(got, ref).all()), (name, got["area"].tolist(), ref["area"].tolist(), got["threshold"].tolist())
        if areas is not None:
            assert np.array_equal(got["area"][0].numpy(), areas), (name, got["area"][0].tolist())
    ops.check_credible_status()


def test_saturated_512_plane(dev):
    """every fp32 sigmoid is 1: the integer sum is at its largest, and the shares are pixel counts: area = ceil(q * n)"""
    ops = pkg("ops")
    x, _ = C.saturated()
    levels = (0.1, 0.3, 0.7, 0.9, 0.99, 0.999, 0.999999)
    n = x.shape[2] * x.shape[3]
    got = host(ops.map_credible(x.to(dev), levels, 1.0))
    C.accept(x, 1.0, levels, got, spot_e32(x, got["threshold"], 1.0))
    want = [math.ceil(float(q) * n) for q in C.levels32(levels)]
    assert got["area"][0, 0].tolist() == want
    assert np.array_equal(got["mass"][0, 0].numpy(), (np.array(want, dtype=np.float64) / n).astype(np.float32))


def test_nan_plane_among_clean_ones_and_the_status_flag(dev):
    ops = pkg("ops")
    ops.check_credible_status()
    x = C.nan_among_clean()
    levels = (0.5, 0.9)
    got = host(ops.map_credible(x.to(dev), levels, 1.3))
    ref = C.restate(x, levels, 1.3)
    assert got["area"][1, 0].tolist() == [-1, -1] and bool(torch.isnan(got["threshold"][1, 0]).all()) and bool(torch.isnan(got["mass"][1, 0]).all())
    for b, c in ((0, 2), (1, 2)):      # all -inf / every sigmoid 0 in fp32: Z == 0, no region, no flag
        assert got["area"][b, c].tolist() == [0, 0] and bool(torch.isnan(got["threshold"][b, c]).all()) and bool(torch.isnan(got["mass"][b, c]).all())
    clean = [(0, 0), (0, 1), (1, 1)]
    for b, c in clean:
        assert torch.equal(got["area"][b, c].long(), ref["area"][b, c]) and torch.equal(got["threshold"][b, c], ref["threshold"][b, c])
    with pytest.raises(RuntimeError, match="NaN"):
        ops.check_credible_status()
    ops.check_credible_status()      # cleared
    x2 = x.clone()
    x2[1, 0] = 0.0
    again = host(ops.map_credible(x2.to(dev), levels, 1.3))
    assert ops.check_credible_status(raise_error=False) is False      # Z == 0 alone raises nothing
    for b, c in clean:
        for k in got:
            assert torch.equal(again[k][b, c], got[k][b, c])
    assert again["area"][1, 0].tolist() == [x.shape[2] * x.shape[3]] * 2      # a constant plane: the whole map at every level


# ---- 3. addressing ----------------------------------------------------------------------------------------------------------------------
def test_many_planes_and_a_channel_slice(dev):
    ops = pkg("ops")
    x = C.many_planes()      # 70000 workgroups along blockIdx.x
    levels = (0.5, 0.9)
    got = host(ops.map_credible(x.to(dev), levels, 1.0))
    C.accept(x, 1.0, levels, got, C.shape_e32(1, 3))
    for sl in (slice(0, 300), slice(-300, None)):
        ref = C.restate(x[sl], levels, 1.0)
        assert bool(same_regions({k: v[sl] for k, v in got.items()}, ref).all())
    x5 = C.sliced()          # channels 1:3 read in place: odd-sized planes, most of them off a 16-byte boundary
    d5 = x5.to(dev)
    view = d5[:, 1:3]
    assert not view.is_contiguous() and any(view[b, c].data_ptr() % 16 for b in range(2) for c in range(2))
    xs = x5[:, 1:3].contiguous()
    a, b = host(ops.map_credible(view, C.LEVELS8, 1.8)), host(ops.map_credible(xs.to(dev), C.LEVELS8, 1.8))
    ref = C.restate(xs, C.LEVELS8, 1.8)
    C.accept(xs, 1.8, C.LEVELS8, a, spot_e32(xs, ref["threshold"], 1.8))
    assert bool(same_regions(a, ref).all())
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # a plane of 64 x 64 moved off its 16-byte boundary gives the aligned call's bits (integer sums know no order)
    si = [hw for hw, _ in C.SHAPES].index((64, 64))
    x64 = C.case(si, 0, 1)[0]
    buf = torch.empty(x64.numel() + 4, device=dev)
    off = buf[1:1 + x64.numel()].view(x64.shape)
    off.copy_(x64.to(dev))
    assert off.data_ptr() % 16 == 4
    a, b = ops.map_credible(off, C.LEVELS8, 1.8), ops.map_credible(x64.to(dev), C.LEVELS8, 1.8)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # refusals that need device tensors
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_credible(x5, levels)
    with pytest.raises(ValueError, match="levels"):
        ops.map_credible(d5, (0.9, 0.5))
    with pytest.raises(ValueError, match="temperature"):
        ops.map_credible(d5, levels, 0.0)
    ops.check_credible_status()


def test_view_whose_last_plane_starts_beyond_2_31_elements(dev):
    ops = pkg("ops")
    H, W = 17, 23
    stride = 2 ** 31 + 8                                              # elements between the two images of the view
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 10 * 2 ** 30, "the 8.6 GB buffer of this test does not fit beside what the device already holds"
    buf = torch.empty(stride + 2 * H * W, device=dev, dtype=torch.float32)      # never initialised: only the viewed planes are written
    view = buf.as_strided((2, 2, H, W), (stride, H * W, W, 1))
    si = [hw for hw, _ in C.SHAPES].index((H, W))
    x, T, ref, _, _ = C.case(si, C.GRID, 1)
    xs = x[:, :2].contiguous()
    view.copy_(xs.to(dev))
    assert view.data_ptr() == buf.data_ptr() and view[1, 1].data_ptr() - buf.data_ptr() == 4 * (stride + H * W)
    got = host(ops.map_credible(view, C.LEVELS8, T))
    C.accept(xs, T, C.LEVELS8, got, C.shape_e32(H, W))
    assert bool(same_regions(got, {k: v[:, :2] for k, v in ref.items()}).all())
    ops.check_credible_status()
    del buf, view
    torch.cuda.empty_cache()


# ---- 4. the sibling kernel ------------------------------------------------------------------------------------------------------------------
def test_hpd_of_map_likelihood_falls_on_the_right_side_of_every_region(dev):
    """x_g >= threshold => hpd_g <= mass, x_g < threshold => hpd_g > mass, with both kernels' bounds as slack"""
    ops = pkg("ops")
    gen = torch.Generator().manual_seed(C.SEED)
    for si, kind, ti in ((2, 0, 0), (3, 3, 1), (4, 4, 0), (5, 1, 1), (6, 2, 0), (7, 0, 1)):
        (H, W), _ = C.SHAPES[si]
        x, T, _, _, _ = C.case(si, kind, ti)
        dx = x.to(dev)
        got = host(ops.map_credible(dx, C.LEVELS8, T))
        n = H * W
        e_hpd = max(e["hpd"] for _, _, e in LC.SHAPES)
        for trial in range(6):
            if trial < 4:      # the corners, then random pixels
                gx = torch.full((C.B, C.C), float((W - 1) * (trial & 1)))
                gy = torch.full((C.B, C.C), float((H - 1) * (trial >> 1)))
            else:
                gx = torch.randint(0, W, (C.B, C.C), generator=gen).float()
                gy = torch.randint(0, H, (C.B, C.C), generator=gen).float()
            gt = torch.stack([gx, gy], dim=-1)
            hpd = ops.map_likelihood(dx, gt.to(dev), T, want=("hpd",))["hpd"].cpu().double()[..., None]
            xg = torch.gather(x.view(C.B, C.C, -1), 2, (gy * W + gx).long()[..., None])      # [B, C, 1]
            mass = got["mass"].double()
            slack = C.bound(mass, C.shape_e32(H, W), n) + LC.bound(mass, e_hpd)
            inside = xg >= got["threshold"]
            assert bool(torch.where(inside, hpd <= mass + slack, hpd > mass - slack).all()), (H, W, kind, trial)
            assert bool(inside.any()) or trial < 4
    ops.check_likelihood_status()
    ops.check_credible_status()


# ---- 5. the drivers on the reference's fixtures ------------------------------------------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws"])
def test_evaluate_and_predict_on_the_fixtures(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P, ops = pkg("utils.evaluate"), pkg("utils.predict"), pkg("ops")
    in_t = O.dist_template(cfg.template_size).to(dev)
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, scene = m["B"], g.t("traj"), g.t("scene")[0]
    H, W = m["H"], m["W"]
    levels = (0.5, 0.9)

    def run(**kw):
        torch.manual_seed(11)
        state = torch.cuda.get_rng_state(dev)
        out = ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
                          cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=True, return_samples=True, network=cfg.network, **kw)
        return out, (torch.get_rng_state(), state, torch.cuda.get_rng_state(dev))

    # with dp=None the flag leaves the captured-sweep cache as it finds it
    ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
                cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network)          # a plain sweep: it may enter the cache

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    before = cache_state()
    (ade1, fde1, df1, td1), rng1 = run(return_sharpness=levels)
    assert cache_state() == before
    (ade0, fde0, df0, td0), rng0 = run()
    # the flag changes nothing else, bit for bit, and leaves the generators where the plain call leaves them
    assert ade0 == ade1 and fde0 == fde1 and list(df0.columns) == list(df1.columns)[:len(df0.columns)]
    assert all(df0[c].equals(df1[c]) for c in df0.columns)
    assert all(torch.equal(a, b) for a, b in zip(rng0, rng1))
    assert list(df1.columns)[len(df0.columns):] == ["area50_goal", "inside50_goal", "area90_goal", "inside90_goal"]
    assert set(td1) - set(td0) == {"area_steps", "threshold_steps", "inside_steps"}
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k
    # the returned steps against the fp64 restatement of the RETURNED goal map
    gm = torch.from_numpy(td1["goal_map"])
    assert gm.shape == (B, cfg.pred_len, H, W)
    got = {"area": torch.from_numpy(td1["area_steps"]), "threshold": torch.from_numpy(td1["threshold_steps"])}
    assert got["area"].shape == (B, cfg.pred_len, 2) and got["area"].dtype == torch.int32 and got["threshold"].dtype == torch.float32
    ref = C.restate(gm, levels, cfg.temperature)
    e = spot_e32(gm, ref["threshold"], cfg.temperature)
    direct = host(ops.map_credible(gm.to(dev), levels, cfg.temperature))
    assert torch.equal(direct["area"], got["area"]) and torch.equal(direct["threshold"], got["threshold"])
    C.accept(gm, cfg.temperature, levels, direct, e)
    same = same_regions(got, ref)
    print(f"{case}: {int((~same).sum())} of {same.numel()} regions differ from the restatement")
    assert int((~same).sum()) <= 0.05 * same.numel()
    # inside: the launch's own threshold against the logit at the rounded ground truth (NaN outside the map)
    gt = torch.round(traj[:, cfg.obs_len:].double())      # [B, pred_len, 2]
    ok = (gt[..., 0] >= 0) & (gt[..., 0] < W) & (gt[..., 1] >= 0) & (gt[..., 1] < H)
    ix = (gt[..., 1].clamp(0, H - 1) * W + gt[..., 0].clamp(0, W - 1)).long()
    xg = torch.gather(gm.view(B, cfg.pred_len, -1), 2, ix[..., None])
    want = torch.where(ok[..., None], (xg >= got["threshold"]).double(), torch.full((), math.nan, dtype=torch.float64))
    inside = torch.from_numpy(td1["inside_steps"]).double()
    assert inside.shape == (B, cfg.pred_len, 2) and bool(ok.any())
    assert torch.equal(torch.isnan(inside), torch.isnan(want)) and bool((inside[ok] == want[ok]).all())
    for l, pct in enumerate((50, 90)):
        assert np.array_equal(df1[f"area{pct}_goal"].to_numpy(), td1["area_steps"][:, -1, l])
        assert np.array_equal(df1[f"inside{pct}_goal"].to_numpy(), td1["inside_steps"][:, -1, l], equal_nan=True)
    # without return_preds the columns come alone; True means (0.5, 0.9)
    torch.manual_seed(11)
    _, _, df2, td2 = ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal,
                                 n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network, return_sharpness=True)
    assert td2 is None and all(df2[c].equals(df1[c]) for c in df1.columns) and cache_state() == before

    # predict_with_regions(): evaluate's regions bit for bit at the same batch size, every other key predict()'s bit for bit
    S = g.t("eval/waypoint_samples")
    args = (model, scene, traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor, cfg.temperature)
    pa = P.predict_with_regions(*args, levels=levels, network=cfg.network, batch_size=B, forced_samples={0: S})
    pb = P.predict(*args, network=cfg.network, batch_size=B, forced_samples={0: S})
    assert set(pa) - set(pb) == {"region_area", "region_threshold", "region_mass"} and pa["region_area"].is_cuda
    assert np.array_equal(pa["region_area"].cpu().numpy(), td1["area_steps"])
    assert np.array_equal(pa["region_threshold"].cpu().numpy(), td1["threshold_steps"])
    assert torch.equal(pa["region_mass"].cpu(), direct["mass"])
    for k in pb:
        assert torch.equal(pa[k], pb[k]), k
    if B > 1:      # chunked = unchunked
        h = (B + 1) // 2
        pc = P.predict_with_regions(*args, levels=levels, network=cfg.network, batch_size=h, forced_samples={0: S[:, :h], h: S[:, h:]})
        for k in ("region_area", "region_threshold", "region_mass"):
            assert torch.equal(pc[k], pa[k]), k
    ops.check_credible_status()


def test_regions_leave_the_training_step_untouched(dev):
    g = Golden("tiny_short_mosa1")
    cfg, m = g.cfg(), g.meta
    te, trn, P, ev = pkg("utils.train_epoch"), pkg("models.trainer"), pkg("utils.predict"), pkg("utils.evaluate")
    S = cfg.template_size
    in_t, gt_t = O.dist_template(S).to(dev), O.gaussian_template(S, cfg.kernlen, cfg.nsig).to(dev)
    traj, scene = g.t("traj"), g.t("scene")[0]
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1

    def step(with_regions):
        model = build_model(cfg, g.state_dict(), dev)
        model.train()
        if with_regions:
            res = P.predict_with_regions(model, scene, traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len,
                                         cfg.resize_factor, cfg.temperature, network=cfg.network, levels=C.LEVELS8)
            assert model.training and bool((res["region_area"] >= 1).all()) and res["region_area"].shape[-1] == 8
            ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "val", n_goal, n_traj,
                        cfg.obs_len, m["B"], cfg.resize_factor, cfg.temperature, network=cfg.network, return_sharpness=True)
            model.train()
        torch.manual_seed(6)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        out = te.train_epoch(model, loader_for(traj), {"scene0": scene}, opt, trn.HipBCEWithLogitsLoss(), cfg.loss_scale, dev, "sdd", None,
                             gt_t, in_t, list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, m["B"], 10000, cfg.resize_factor, cfg.network, False)
        return out, {n: p.detach().clone() for n, p in model.named_parameters()}

    out0, p0 = step(False)
    out1, p1 = step(True)
    assert out0 == out1, (out0, out1)
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n

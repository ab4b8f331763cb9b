"""Scene compliance on the MI355X: ynet_map_class_mass against the fp64 restatement of tests/_compliance_cases.py over its whole table,
the exactness and edge rules, the layouts, the sibling kernel as a cross-check, and evaluate(return_compliance=True) /
predict_with_compliance() on the reference's fixtures.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), E32 = the error of the same restatement run in fp32 (recorded
per shape in the table; measured on the spot for the inputs that are not in it).

Measured on the MI355X (largest |device - fp64| over the table): see DESIGN.md section 4.13."""
import numpy as np
import pandas as pd
import pytest
import torch

import _compliance_cases as C
import _likelihood_cases as LC
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, what):
    """every finite reference entry within the bound, NaN where the reference has NaN; -> the largest error / bound"""
    g = got.detach().cpu().double()
    assert got.dtype == torch.float32 and g.shape == ref.shape, (what, got.dtype, g.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(g), torch.isnan(ref)) and bool(torch.isnan(ref[~fin]).all()), (what, "NaN pattern")
    if not fin.any():
        return 0.0
    err, bnd = (g - ref).abs()[fin], C.bound(ref, e)[fin]
    print(f"{what}: max error {float(err.max()):.3e} (bound there {float(bnd[err.argmax()]):.3e})")
    assert bool((err <= bnd).all()), (what, float(err.max()), float(bnd[err.argmax()]))
    return float((err / bnd).max())


# ---- (a) the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    (H, W), _, e = C.SHAPES[si]
    worst, dx, dlab = 0.0, {}, {}
    for kind, pat in C.cases(si):
        x, lab, K, T, ref = C.case(si, kind, pat)
        if kind not in dx:
            dx[kind] = x.to(dev)
        if pat not in dlab:
            dlab[pat] = lab.to(dev)
        what = f"{H}x{W} kind {kind} pattern {pat}"
        got = ops.map_class_mass(dx[kind], dlab[pat], K, T)
        assert got.shape == (C.B, C.C, K) and got.is_cuda
        worst = max(worst, check(got, ref, e, what))
        g = got.cpu()
        rows, slack = g.double().sum(-1), K * C.bound(torch.ones(()), e)
        if bool((lab < K).all()):                              # every label below K: the classes share the whole distribution
            assert bool(((rows - 1.0).abs() <= slack).all()), (what, rows)
        else:                                                  # pixels of no class count in the normaliser only
            assert pat in (5, 7) and bool((rows <= 1.0 + slack).all()) and (H * W < 90 or bool((rows < 1.0 - slack).all())), (what, rows)
        if pat == 3:                                           # all one class: the class sum IS the normaliser, bit for bit
            assert bool((g[..., 2] == 1.0).all()) and bool((g[..., :2] == 0.0).all()), (what, g)
        if pat == 4:                                           # a class that occurs nowhere sums zeros alone
            assert bool((g[..., C.ABSENT] == 0.0).all()), what
    print(f"{H}x{W}: largest error / bound {worst:.3f}")
    for kind, d in dx.items():
        assert torch.equal(d.cpu(), C.case(si, kind, 0)[0])    # the input is read, never written


def test_known_answers(dev):
    ops = pkg("ops")
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        e = C.shape_e32(H, W)
        x, lab, K, T, area = C.constant_plane(H, W)
        check(ops.map_class_mass(x.to(dev), lab.to(dev), K, T), area.view(1, 1, K), e, f"constant {H}x{W}")
        if H * W < 2:
            continue
        x, lab, K, T, want = C.spike_planes(H, W)
        check(ops.map_class_mass(x.to(dev), lab.to(dev), K, T), want.view(1, 2, K), e, f"spike {H}x{W}")


# ---- (b) the edge rules --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.EDGE_SHAPES)
def test_edge_planes(dev, H, W):
    ops = pkg("ops")
    x, lab, K, T = C.edge_planes(H, W)
    ref, e = C.mass_ref(x, lab, K, T), C.shape_e32(H, W)
    name = {n: i for i, n in enumerate(C.EDGE_PLANES)}
    got = ops.map_class_mass(x.to(dev), lab.to(dev), K, T)
    check(got, ref, e, f"edge planes {H}x{W}")                  # +inf beside -inf and a row of -inf: the restatement's finite numbers
    h = got.cpu()
    assert bool(torch.isnan(h[0, name["nan"]]).all()) and bool(torch.isnan(h[0, name["all_minus_inf"]]).all())
    for n in ("minus_inf_elsewhere", "minus_inf_pixels", "plus_and_minus_inf"):
        assert bool(torch.isfinite(h[0, name[n]]).all()), n
    # the planes beside the poisoned ones are unaffected: the same launch without them gives the same bits
    keep = [name[n] for n in ("minus_inf_elsewhere", "minus_inf_pixels", "plus_and_minus_inf")]
    clean = ops.map_class_mass(x[:, keep].to(dev), lab.to(dev), K, T).cpu()
    assert torch.equal(clean[0], h[0, keep])                    # (wherever the planes now start: both paths add in the same order)


# ---- (c) layouts ---------------------------------------------------------------------------------------------------------------------------
def test_channel_slice_batched_labels_and_many_planes(dev):
    ops = pkg("ops")
    for H, W in [(17, 23), (8, 8)]:                             # a channel slice, read in place: batch stride 5 planes, 2 planes scored
        x5, lab, K, T = C.sliced(H, W)
        d5, dl = x5.to(dev), lab.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        got = ops.map_class_mass(view, dl, K, T)
        xs = x5[:, 1:3].contiguous()
        check(got, C.mass_ref(xs, lab, K, T), C.e32(xs, lab, K, T), f"channel slice {H}x{W}")
        assert torch.equal(ops.map_class_mass(xs.to(dev), dl, K, T), got)      # (both paths add the same terms in the same order)
        # [B, H, W] labels: copies of the shared plane give the shared form's bits; rows that differ are told apart
        rows = dl[None].repeat(2, 1, 1)
        assert torch.equal(ops.map_class_mass(view, rows, K, T), got)
        assert torch.equal(ops.map_class_mass(view, dl[None].expand(2, -1, -1), K, T), got)
        other = C.labels(H, W, 6)[0] % 6
        two = torch.stack([lab, other])
        check(ops.map_class_mass(view, two.to(dev), K, T), C.mass_ref(xs, two, K, T), C.e32(xs, two, K, T), f"per-row labels {H}x{W}")
    x, lab, K, T = C.many_planes()                              # 70000 workgroups along blockIdx.x
    check(ops.map_class_mass(x.to(dev), lab.to(dev), K, T), C.mass_ref(x, lab, K, T), C.e32(x, lab, K, T), "70000 planes of 2x2")
    # refusals that need device tensors
    with pytest.raises(ValueError, match="labels"):
        ops.map_class_mass(d5, dl[:-1], K, T)
    with pytest.raises(ValueError, match="labels"):
        ops.map_class_mass(d5, dl[None].repeat(3, 1, 1), K, T)
    with pytest.raises(ValueError, match="contiguous"):
        ops.map_class_mass(d5, dl.t().contiguous().t(), K, T)
    with pytest.raises(TypeError, match="uint8"):
        ops.map_class_mass(d5, dl.int(), K, T)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_class_mass(d5, lab, K, T)
    for bad in (0, 9):
        with pytest.raises(ValueError, match="n_classes"):
            ops.map_class_mass(d5, dl, bad, T)
    with pytest.raises(ValueError, match="temperature"):
        ops.map_class_mass(d5, dl, K, 0.0)


@pytest.mark.parametrize("H,W", [(5, 4), (96, 160)])
def test_labels_at_any_byte_offset(dev, H, W):
    """a label plane off a 4-byte boundary under an aligned map: element-wise loads, the aligned call's bits"""
    ops = pkg("ops")
    si = [hw for hw, _, _ in C.SHAPES].index((H, W))
    for kind, pat in ((1, 0), (4, 1)):
        x, lab, K, T, ref = C.case(si, kind, pat)
        dx, n = x.to(dev), H * W
        aligned = ops.map_class_mass(dx, lab.to(dev), K, T)
        check(aligned, ref, C.shape_e32(H, W), f"{H}x{W} aligned")
        buf = torch.full((n + 8,), 255, dtype=torch.uint8, device=dev)
        assert buf.data_ptr() % 4 == 0
        for off in (1, 2, 3):
            buf.fill_(255)
            view = buf[off:off + n].view(H, W)
            view.copy_(lab.to(dev))
            assert view.data_ptr() % 4 == off
            assert torch.equal(ops.map_class_mass(dx, view, K, T), aligned), (H, W, kind, pat, off)


# ---- (d) the sibling kernel, as an extra ----------------------------------------------------------------------------------------------------
def test_two_class_labels_reproduce_the_hpd_of_map_likelihood(dev):
    """labels = (x >= x_g): class 1 is the highest-density region through g, whose mass ynet_map_likelihood reports as hpd"""
    ops = pkg("ops")
    for si, kind in ((2, 0), (3, 2), (5, 4)):
        (H, W), _, eh = LC.SHAPES[si]
        x, gt, T, _ = LC.case(si, kind)
        x, gt = x[:, :1].contiguous(), gt[:, :1].contiguous()          # (labels are per row: one plane per row)
        g = torch.round(gt.double()).long()
        xg = torch.stack([x[b, 0, g[b, 0, 1], g[b, 0, 0]] for b in range(x.shape[0])])
        lab = (x[:, 0] >= xg.view(-1, 1, 1)).to(torch.uint8)
        mass = ops.map_class_mass(x.to(dev), lab.to(dev), 2, T).cpu().double()
        hpd = ops.map_likelihood(x.to(dev), gt.to(dev), T, want=("hpd",))["hpd"].cpu().double()
        ops.check_likelihood_status()
        ref = C.mass_ref(x, lab, 2, T)[..., 1]
        both = C.bound(ref, C.shape_e32(H, W)) + LC.bound(ref, eh["hpd"])
        print(f"{H}x{W}: |class-1 mass - hpd| {float((mass[..., 1] - hpd).abs().max()):.3e} (bounds added {float(both.min()):.3e})")
        assert bool(((mass[..., 1] - hpd).abs() <= both).all())


# ---- (e) the drivers on the reference's fixtures ------------------------------------------------------------------------------------------
def loader_for(traj):
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    return [(traj.clone(), [meta], "scene0")]


@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws"])
def test_evaluate_and_predict_on_the_fixtures(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, P, cls = pkg("utils.evaluate"), pkg("utils.predict"), pkg("utils.compliance")
    in_t = O.dist_template(cfg.template_size).to(dev)
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, scene = m["B"], g.t("traj"), g.t("scene")[0]
    K = scene.shape[0]
    assert 1 <= K <= 8

    def run(**kw):
        torch.manual_seed(11)
        return ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj,
                           cfg.obs_len, B, cfg.resize_factor, cfg.temperature, return_preds=True, return_samples=True, network=cfg.network, **kw)

    ade1, fde1, df1, td1 = run(return_compliance=True)
    ade0, fde0, df0, td0 = run()
    # the flag changes nothing else, bit for bit: the same draws under the same seed
    assert ade0 == ade1 and fde0 == fde1 and df0["ade"].equals(df1["ade"]) and df0["fde"].equals(df1["fde"])
    assert set(td1) - set(td0) == {"class_mass_steps"} and list(df0.columns) == list(df1.columns)[:len(df0.columns)]
    assert list(df1.columns)[len(df0.columns):] == ([f"goal_mass_{k}" for k in range(K)] + ["gt_goal_class"]
                                                    + [f"sample_goal_rate_{k}" for k in range(K)])
    for k in td0:
        assert np.array_equal(np.asarray(td0[k]), np.asarray(td1[k])), k
    # the returned steps = the fp64 restatement on the RETURNED goal map under the scene's own labels
    lab = scene.argmax(dim=0).to(torch.uint8)
    assert torch.equal(cls.scene_labels(scene), lab)
    gm = torch.from_numpy(td1["goal_map"])
    assert gm.shape == (B, cfg.pred_len, m["H"], m["W"]) and lab.shape == (m["H"], m["W"])
    steps = torch.from_numpy(td1["class_mass_steps"])
    assert steps.shape == (B, cfg.pred_len, K) and steps.dtype == torch.float32
    check(steps, C.mass_ref(gm, lab, K, cfg.temperature), C.e32(gm, lab, K, cfg.temperature), case)
    for k in range(K):
        assert np.array_equal(df1[f"goal_mass_{k}"].to_numpy(), td1["class_mass_steps"][:, -1, k])
    # the sampled goals and the ground-truth goal, recomputed on the host from what evaluate() returned
    ws = torch.from_numpy(td1["waypoint_sample"])                   # [B, n_wp, K_samples, 2]
    goals = torch.round(ws[:, -1].double()).long()                  # [B, K_samples, 2] (x, y): drawn pixels, inside the map
    on = lab[goals[..., 1], goals[..., 0]].long()
    for k in range(K):
        assert np.array_equal(df1[f"sample_goal_rate_{k}"].to_numpy(), ((on == k).sum(dim=1).double() / on.shape[1]).numpy()), k
    gt = torch.round(traj[:, -1].double())
    inside = (gt[:, 0] >= 0) & (gt[:, 0] < m["W"]) & (gt[:, 1] >= 0) & (gt[:, 1] < m["H"])
    want = torch.full((B,), -1, dtype=torch.int64)
    want[inside] = lab[gt[inside, 1].long(), gt[inside, 0].long()].long()
    assert df1["gt_goal_class"].to_numpy().tolist() == want.tolist() and bool(inside.any())
    # without return_preds the columns come alone
    torch.manual_seed(11)
    _, _, df2, td2 = ev.evaluate(model, loader_for(traj), {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal,
                                 n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network, return_compliance=True)
    assert td2 is None and all(df2[c].equals(df1[c]) for c in df1.columns)
    with pytest.raises(ValueError, match="planes"):                 # refused before the sweep starts
        ev.evaluate(model, loader_for(traj), {"scene0": scene, "other": torch.zeros(9, 4, 4)}, dev, "sdd", None, in_t, list(cfg.waypoints),
                    "test", n_goal, n_traj, cfg.obs_len, B, cfg.resize_factor, cfg.temperature, network=cfg.network, return_compliance=True)

    # predict_with_compliance(): evaluate's masses bit for bit at the same batch size, every other key predict()'s bit for bit
    S = g.t("eval/waypoint_samples")
    args = (model, scene, traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor, cfg.temperature)
    pa = P.predict_with_compliance(*args, network=cfg.network, batch_size=B, forced_samples={0: S})
    pb = P.predict(*args, network=cfg.network, batch_size=B, forced_samples={0: S})
    assert set(pa) - set(pb) == {"goal_class_mass"} and pa["goal_class_mass"].is_cuda
    assert np.array_equal(pa["goal_class_mass"].cpu().numpy(), td1["class_mass_steps"])
    for k in pb:
        assert torch.equal(pa[k], pb[k]), k
    pc = P.predict_with_compliance(*args, network=cfg.network, batch_size=B, forced_samples={0: S}, return_entropy=True)
    assert set(pc) - set(pa) == {"entropy"} and torch.equal(pc["goal_class_mass"], pa["goal_class_mass"])

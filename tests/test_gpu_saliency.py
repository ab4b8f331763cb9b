"""forward_test / saliency on the MI355X: input gradients (ynet_input_grad) against an fp64 referee, the batch sum of the scene
gradient, forward_test(decision='map'), the range-scaled noise (ynet_add_range_noise), no side effects on the training step, and
tensors beyond 2 and 4 GiB.  models/trainer.py:354-516."""
import contextlib
import io

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def _params(cfg, B):
    return dict(obs_len=cfg.obs_len, pred_len=cfg.pred_len, segmentation_model_fp=None, use_features_only=False,
                n_semantic_classes=cfg.n_classes, encoder_channels=list(cfg.enc), decoder_channels=list(cfg.dec),
                waypoints=list(cfg.waypoints), train_net=cfg.train_net, position=list(cfg.position), network=cfg.network,
                n_fusion=cfg.n_fusion, resize_factor=cfg.resize_factor, dataset_name="sdd", batch_size=B, kernlen=cfg.kernlen,
                nsig=cfg.nsig, loss_scale=cfg.loss_scale, use_raw_data=False, decision="loss")


def _trainer(cfg, sd, dev, B):
    trn = pkg("models.trainer")
    with contextlib.redirect_stdout(io.StringIO()):
        t = trn.YNetTrainer(_params(cfg, B), device=dev)
    t.model.load_state_dict(sd, strict=True)
    trn.apply_freeze_policy(t.model, cfg.train_net, list(cfg.position), cfg.network)
    t.model.to(dev)
    return t


def _df(traj, cfg, scene_ids=("scene0",)):
    B, T, _ = traj.shape
    rows = []
    for sid in scene_ids:
        rows.append(pd.DataFrame({"sceneId": sid, "metaId": np.repeat(np.arange(B), T),
                                  "x": (traj[..., 0] / cfg.resize_factor).reshape(-1).numpy(),
                                  "y": (traj[..., 1] / cfg.resize_factor).reshape(-1).numpy()}))
    return pd.concat(rows, ignore_index=True)


def _loader_traj(t, df, images, cfg):
    with contextlib.redirect_stdout(io.StringIO()):
        _, loader, _ = t.prepare_data(df, images, "sdd", "test", cfg.obs_len, cfg.pred_len, cfg.resize_factor, False)
    traj, _, _ = next(iter(loader))
    return torch.as_tensor(traj).float()


def _oracle(sd, cfg, scene, traj, dev, target="both", observed=None):
    """d(goal_loss + traj_loss) / d scene, / d observed_map as models/trainer.py:459-516 defines the losses (the trajectory decoder
    reads the PREDICTED goal map's waypoints), fp64 on the device."""
    H, W = scene.shape[-2:]
    S = cfg.template_size
    obs, gt, _ = O.build_maps(cfg, traj.cpu(), H, W, O.dist_template(S), O.gaussian_template(S, cfg.kernlen, cfg.nsig))
    if observed is not None:
        obs = observed
    p = {k: (v.to(dev).double() if v.is_floating_point() else v.to(dev)) for k, v in sd.items()}
    sc = scene.to(dev).double().detach().requires_grad_()
    ob = obs.to(dev).double().detach().requires_grad_()
    gt = gt.to(dev).double()
    B = ob.shape[0]
    feats = O.encoder(p, cfg, sc.expand(B, -1, -1, -1), ob, training=True)
    goal = O.decoder(p, cfg, "goal_decoder", feats)
    gl = O.bce_logits_mean(goal, gt) * cfg.loss_scale
    traj_map = O.decoder(p, cfg, "traj_decoder", O.traj_inputs(feats, goal[:, list(cfg.waypoints)]))
    tl = O.bce_logits_mean(traj_map, gt) * cfg.loss_scale
    loss = gl + tl if target == "both" else (gl if target == "goal" else tl)
    gs, go = torch.autograd.grad(loss, [sc, ob])
    return gs[0], go, goal.detach(), traj_map.detach(), obs


def _close(name, got, want, rel=1e-4, isolated=0):
    """max|got - want| <= rel * max|want|.  isolated > 0: up to that fraction of the elements (at least 4) may exceed the bound -- at the
    full-size shapes a max-pool whose 2 x 2 window holds two near-equal values, or a ReLU input within rounding of 0, sends the
    gradient down the other branch in fp32 than in fp64 (a discontinuity of the gradient itself, measured at single pixels with
    the Winograd and the implicit-GEMM convolutions alike); the mean deviation must then stay below rel * mean|want|."""
    got, want = got.double().cpu(), want.double().cpu()
    assert got.shape == want.shape, (name, tuple(got.shape), tuple(want.shape))
    d = (got - want).abs()
    err, ref = float(d.max()), float(want.abs().max())
    n_bad = int((d > rel * ref).sum())
    print(f"{name}: max|d| {err:.3e}  bound {rel * ref:.3e}  (margin x{rel * ref / max(err, 1e-30):.1f}); {n_bad} of {d.numel()} "
          f"elements beyond it; mean|d| {float(d.mean()):.3e} vs mean|ref| {float(want.abs().mean()):.3e}")
    assert ref > 0
    if not isolated:
        assert err <= rel * ref, (name, err, ref)
    else:
        assert n_bad <= max(4, int(isolated * d.numel())), (name, n_bad)
        assert float(d.mean()) <= rel * float(want.abs().mean()), name


CASES = {
    "golden_tiny_short_mosa1": None,
    "tiny_original": (O.sdd_short(train_net="mosa_1", position=["0", "1", "2", "3", "4"]), 3, 64, 64),
    "fusion": (O.sdd_short(train_net="mosa_1", position=["scene", "motion", "fusion"], network="fusion", n_fusion=2), 3, 64, 64),
    "c2": (O.sdd_short(train_net="mosa_1", position=["0", "1", "2", "3", "4"]), 32, 256, 256),
    "c4": (O.sdd_long(train_net="mosa_1", position=["scene", "motion", "fusion"], network="fusion", n_fusion=2), 16, 512, 512),
}


def _case(name):
    if CASES[name] is None:
        g = Golden("tiny_short_mosa1")
        return g.cfg(), g.state_dict(), g.t("scene"), g.t("traj")
    cfg, B, H, W = CASES[name]
    sd = O.make_state_dict(cfg, seed=0, lora_b_std=0.05)
    return cfg, sd, O.synthetic_scene(cfg, H, W, 0), O.synthetic_trajectories(cfg, B, H, W, 0)


@pytest.mark.parametrize("name", list(CASES))
def test_input_gradients_match_fp64_oracle(dev, name):
    cfg, sd, scene, traj = _case(name)
    t = _trainer(cfg, sd, dev, traj.shape[0])
    images = {"scene0": scene[0]}
    df = _df(traj, cfg)
    traj_l = _loader_traj(t, df, images, cfg)
    before = {n: (p.grad.clone() if p.grad is not None else None) for n, p in t.model.named_parameters()}
    g = t.saliency(df, images, target="both", set_input=("scene", "traj"))
    ref_s, ref_o, _, _, _ = _oracle(sd, cfg, scene, traj_l, dev)
    iso = 1e-2 if name in ("c2", "c4") else 0
    _close(f"{name} scene", g["scene"], ref_s, isolated=iso)
    _close(f"{name} traj", g["traj"], ref_o, isolated=iso)
    for n, p in t.model.named_parameters():
        assert (p.grad is None) == (before[n] is None), n
    if name == "tiny_original":
        for target in ("goal", "traj"):
            g1 = t.saliency(df, images, target=target, set_input=("traj",))
            _, ref_o1, _, _, _ = _oracle(sd, cfg, scene, traj_l, dev, target=target)
            _close(f"{name} traj ({target})", g1["traj"], ref_o1)


def test_scene_gradient_is_the_batch_sum_and_reproducible(dev):
    ops = pkg("ops")
    torch.manual_seed(0)
    B, H, W, cout = 32, 256, 256, 32
    w = torch.randn(cout, 14, 3, 3, device=dev) * 0.1
    wp = ops.pack_weight(w, 1)
    dy = torch.randn(B, cout, H, W, device=dev)
    y = torch.relu(torch.randn(B, cout, H, W, device=dev))
    ds, dm = ops.input_grad(dy, wp, 6, 8, relu_of=y)
    ds2, dm2 = ops.input_grad(dy, wp, 6, 8, relu_of=y)
    assert torch.equal(ds, ds2) and torch.equal(dm, dm2)
    ref = F.conv_transpose2d((dy * (y > 0)).double(), w.double(), padding=1)
    _close("per-image motion vs fp64", dm, ref[:, 6:])
    _close("batch-summed scene vs fp64", ds, ref[:, :6].sum(0, keepdim=True))
    singles = torch.zeros_like(ds)
    for b in range(B):
        s1, m1 = ops.input_grad(dy[b:b + 1], wp, 6, 8, relu_of=y[b:b + 1])
        singles += s1
        assert torch.equal(m1, dm[b:b + 1])
    assert float((singles - ds).abs().max()) <= 1e-5 * float(ds.abs().max())
    # Y-Net-Mod's separate first layers: one destination each
    s_only, none = ops.input_grad(dy[:, :cout], ops.pack_weight(w[:, :6].contiguous(), 1), 6, 0)
    assert none is None
    _close("scene-only layer", s_only, F.conv_transpose2d(dy.double(), w[:, :6].double(), padding=1).sum(0, keepdim=True))


def test_forward_test_map_and_errors(dev):
    cfg, sd, scene, traj = _case("tiny_original")
    t = _trainer(cfg, sd, dev, traj.shape[0])
    t.params["decision"] = "map"
    images = {"scene0": scene[0]}
    df = _df(traj, cfg)
    ops = pkg("ops")
    with torch.no_grad():
        goal, traj_map, raw = t.forward_test(df, images, [], None)
        traj_l = _loader_traj(t, df, images, cfg)
        B, (H, W) = traj_l.shape[0], scene.shape[-2:]
        tmpl = t.templates()
        observed = ops.gather_patches(tmpl, traj_l[:, :cfg.obs_len].reshape(-1, 2), H, W).view(-1, cfg.obs_len, H, W)
        sem = scene.to(dev).expand(B, -1, -1, -1)
        feats = t.model.pred_features(sem, observed)
        g2 = t.model.pred_goal(feats)
        pyr = ops.avgpool_pyramid(g2[:, list(cfg.waypoints)].contiguous(), len(feats))
        tr2 = t.model.pred_traj([ops.lazy_cat([f, p]) for f, p in zip(feats, pyr)])
    assert torch.equal(goal, g2) and torch.equal(traj_map, tr2)
    assert raw.shape == (1,) + tuple(scene.shape[1:])
    _, _, ref_goal, ref_traj, _ = _oracle(sd, cfg, scene, traj_l, dev)
    _close("map goal vs oracle", goal, ref_goal)
    _close("map traj vs oracle", traj_map, ref_traj)
    with pytest.raises(ValueError, match=r"Received more than 1 scene \(2\)"):
        t.forward_test(_df(traj, cfg, ("scene0", "scene1")), {"scene0": scene[0], "scene1": scene[0]}, [], None)
    with pytest.raises(ValueError, match="No data is provided"):
        t.forward_test(_df(traj[:0], cfg), images, [], None)
    t.params["decision"] = "both"
    with pytest.raises(ValueError, match="No support for decision=both"):
        t.forward_test(df, images, [], None)


def test_range_noise(dev):
    ops = pkg("ops")
    torch.manual_seed(1)
    x = torch.rand(1, 14, 256, 256, device=dev) * 3.0 - 1.0
    frac = 0.05
    a = ops.add_range_noise(x, frac, 1234)
    b = ops.add_range_noise(x, frac, 1234)
    assert torch.equal(a, b) and not torch.equal(a, ops.add_range_noise(x, frac, 1235))
    n = (a - x).double()
    std = frac * float(x.max() - x.min())
    assert abs(float(n.std()) / std - 1.0) <= 0.02, (float(n.std()), std)
    assert abs(float(n.mean())) <= 3 * std / n.numel() ** 0.5
    # the documented generator: Philox4x32-10 + Box-Muller, reproduced on the host for the first elements
    i = np.arange(4096, dtype=np.uint64)
    seed = 1234

    def u(row):
        x0, x1 = O._philox4x32_10(i & np.uint64(0xFFFFFFFF), i >> np.uint64(32), np.full_like(i, row), np.full_like(i, 2),
                                  seed & 0xFFFFFFFF, seed >> 32)
        return ((x0 >> np.uint64(5)).astype(np.float64) * 67108864.0 + (x1 >> np.uint64(6)).astype(np.float64) + 0.5) / 9007199254740992.0
    z = np.sqrt(-2.0 * np.log(u(0))) * np.cos(2 * np.pi * u(1))
    want = z.astype(np.float32) * np.float32(std)
    np.testing.assert_allclose(n.reshape(-1)[:4096].cpu().numpy(), want, rtol=1e-5, atol=1e-6 * std)


def test_noisy_forward_test_is_reproducible_and_matches_oracle(dev):
    cfg, sd, scene, traj = _case("tiny_original")
    t = _trainer(cfg, sd, dev, traj.shape[0])
    images = {"scene0": scene[0]}
    df = _df(traj, cfg)
    outs = []
    for _ in range(2):
        torch.manual_seed(7)
        gl, tl, raw, noisy = t.forward_test(df, images, ["scene", "traj"], 0.1)
        (gl + tl).backward()
        outs.append((noisy.detach().clone(), t.forward_inputs["traj"].detach().clone(), noisy.grad.clone(), t.forward_inputs["traj"].grad.clone()))
        t.model.zero_grad(set_to_none=True)
    for u, v in zip(*outs):
        assert torch.equal(u, v)
    noisy, noisy_obs, g_s, g_o = outs[0]
    assert not torch.equal(noisy, raw.detach())
    traj_l = _loader_traj(t, df, images, cfg)
    ref_s, ref_o, _, _, _ = _oracle(sd, cfg, noisy.cpu(), traj_l, dev, observed=noisy_obs.cpu())
    _close("noisy scene", g_s[0], ref_s)
    _close("noisy traj", g_o, ref_o)
    # decision='map' with noise: the reference's five outputs
    t.params["decision"] = "map"
    torch.manual_seed(7)
    out = t.forward_test(df, images, ["scene", "traj"], 0.1)
    assert len(out) == 5 and torch.equal(out[3].detach(), noisy)
    assert out[4].shape == (traj.shape[0], cfg.n_classes + cfg.obs_len) + tuple(scene.shape[-2:])


def _step(cfg, sd, dev, scene, traj, n_steps=3):
    te = pkg("utils.train_epoch")
    trn = pkg("models.trainer")
    model = build_model(cfg, sd, dev)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    S = cfg.template_size
    in_t = pkg("utils.image_utils").analytic_dist_template(S, dev)
    gt_t = pkg("utils.image_utils").analytic_gaussian_template(S, cfg.kernlen, cfg.nsig, False, dev)
    B = traj.shape[0]
    loader = [(traj.clone(), [pd.DataFrame({"metaId": np.arange(B)})], "s")] * n_steps
    ade, fde, loss = te.train_epoch(model, loader, {"s": scene[0].to(dev)}, opt, trn.HipBCEWithLogitsLoss(), cfg.loss_scale, dev, "sdd", None,
                                    gt_t, in_t, list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, B, 10000, cfg.resize_factor, "original", False)
    grads = {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}
    return loss, grads


def test_saliency_leaves_the_training_step_unchanged(dev):
    ops = pkg("ops")
    cfg, sd, scene, traj = _case("c2")
    counters = lambda: (dict(ops.premask_stats), dict(ops.wino_stats), dict(ops.pool_code_stats))
    c0 = counters()
    loss_a, grads_a = _step(cfg, sd, dev, scene, traj)
    c1 = counters()
    t = _trainer(cfg, sd, dev, traj.shape[0])
    t.saliency(_df(traj, cfg), {"scene0": scene[0]})
    for reg in (*ops._STEP_REGISTRIES, ops._skip_registry):
        assert not reg, reg
    assert not any(e.ref() is not None for e in ops._pooled_outputs.values()) and not ops._blob_targets
    c2 = counters()
    loss_b, grads_b = _step(cfg, sd, dev, scene, traj)
    c3 = counters()
    assert loss_a == loss_b
    assert grads_a.keys() == grads_b.keys() and all(torch.equal(grads_a[n], grads_b[n]) for n in grads_a)
    for d0, d1, d2, d3 in zip(c0, c1, c2, c3):
        assert {k: d1.get(k, 0) - d0.get(k, 0) for k in d1} == {k: d3.get(k, 0) - d2.get(k, 0) for k in d3}


def test_input_grad_beyond_2_and_4_gib(dev):
    ops = pkg("ops")
    B, H, W, cout = 33, 2048, 2048, 32
    assert B * 8 * H * W * 4 > 4 * 2 ** 30          # d_motion crosses 2 and 4 GiB; dy (cout 32) reaches 17.7 GB
    torch.manual_seed(3)
    w = torch.randn(cout, 14, 3, 3, device=dev) * 0.1
    wp = ops.pack_weight(w, 1)
    dy = torch.empty(B, cout, H, W, device=dev)
    for b in range(B):
        dy[b].normal_()
    ds, dm = ops.input_grad(dy, wp, 6, 8)
    for b in (0, 16, B - 1):
        s1, m1 = ops.input_grad(dy[b:b + 1].clone(), wp, 6, 8)
        assert torch.equal(m1, dm[b:b + 1]), b
    ref = F.conv_transpose2d(dy[B - 1:].double(), w.double(), padding=1)
    _close("last image beyond 4 GiB", dm[B - 1:], ref[:, 6:])
    assert torch.isfinite(ds).all()

"""The style bank on the MI355X: the two kernels against fp64 / NumPy restatements, one style against predict(), mixed styles against
the CPU oracle, what a bank call leaves behind (parameter versions, a training sequence, a step graph captured BEFORE it), bit
repeatability and chunking.  Every test runs under a time limit of its own."""
import contextlib
import io
import signal

import numpy as np
import pandas as pd
import pytest
import torch

import _predict_cases as C
import _style_cases as S
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu
TEST_SECONDS = 420


@pytest.fixture(autouse=True)
def _time_limit():
    def stop(*_):
        raise TimeoutError(f"the test ran longer than {TEST_SECONDS} s")
    old = signal.signal(signal.SIGALRM, stop)
    signal.alarm(TEST_SECONDS)
    yield
    signal.alarm(0)
    signal.signal(signal.SIGALRM, old)


def perturbed(sd, seed, scale=0.05):
    """A style: the lora_A / lora_B of ``sd`` moved by N(0, scale^2) draws of a fixed seed."""
    gen = torch.Generator().manual_seed(seed)
    return {k: v + scale * torch.randn(v.shape, generator=gen) for k, v in sd.items() if "lora_" in k}


def unrank(ranked, order):
    out = torch.empty_like(ranked)
    idx = order.long().view(order.shape + (1,) * (ranked.dim() - 2)).expand_as(ranked)
    return out.scatter_(1, idx, ranked)


# ---- 1. the kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", C.BS)
@pytest.mark.parametrize("n_wp", C.NWPS)
@pytest.mark.parametrize("K", C.KS)
def test_score_rank_rows_matches_fp64(dev, K, n_wp, B):
    ops = pkg("ops")
    prob, wps, trajs = C.make_case(K, n_wp, B)
    rf = 0.25
    inv = np.float32(1.0 / rf)
    d_prob, d_wps, d_trajs = (torch.from_numpy(a).to(dev) for a in (prob, wps, trajs))
    for kind in S.PERMS:
        rows = S.out_rows(kind, B)
        want_score, want_order, _, _ = S.rank_rows_fp64(prob, wps, trajs, rows, rf)      # [B, K] at the output rows, sample order
        ranked, goals, score, order = ops.score_rank_samples_rows(d_prob, d_wps, d_trajs, rf, rows)
        assert ranked.shape == (B, K, C.PRED, 2) and goals.shape == (B, K, n_wp, 2) and score.shape == (B, K)
        assert order.shape == (B, K) and order.dtype == torch.int32
        order_h = order.cpu().numpy().astype(np.int64)
        frac = C.check_order(order_h, want_score, n_wp)            # (a run of one fp64 neighbour: the very sample of the fp64 rule)
        score_h = score.cpu().numpy().astype(np.float64)
        want_sorted = np.take_along_axis(want_score, order_h, axis=1)
        rel = np.abs(score_h - want_sorted) / np.abs(want_sorted)
        print(f"K {K} n_wp {n_wp} B {B} {kind}: pairs inside the gap {frac:.5f}, max relative score error {rel.max():.3e}")
        assert frac < 0.01
        assert rel.max() <= 1e-5
        assert (score_h[:, :-1] >= score_h[:, 1:]).all()
        # the copies, bit for bit: output row rows[b] holds agent b's samples in the order the device reported
        agent = np.argsort(rows)                                    # output row -> agent
        cols = agent[:, None]
        assert np.array_equal(ranked.cpu().numpy(), trajs.transpose(1, 0, 2, 3)[cols, order_h] * inv)
        assert np.array_equal(goals.cpu().numpy(), wps.transpose(1, 0, 2, 3)[cols, order_h])


@pytest.mark.parametrize("B", C.BS)
@pytest.mark.parametrize("n_wp", C.NWPS)
@pytest.mark.parametrize("K", C.KS)
def test_score_rank_rows_with_the_identity_is_score_rank_bit_for_bit(dev, K, n_wp, B):
    """The two entries run one body: with out_row = 0 .. B - 1 all four results are equal bit for bit, `order` and its ties included."""
    ops = pkg("ops")
    prob, wps, trajs = (torch.from_numpy(a).to(dev) for a in C.make_case(K, n_wp, B))
    plain = ops.score_rank_samples(prob, wps, trajs, 0.25)
    rows = ops.score_rank_samples_rows(prob, wps, trajs, 0.25, out_row=torch.arange(B, device=dev, dtype=torch.int32))
    for name, a, b in zip(("ranked", "ranked_goals", "score", "order"), plain, rows):
        assert a.dtype == b.dtype and a.shape == b.shape, name
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)), name      # (bits: a NaN would not hide a difference, -0 is not +0)


def test_score_rank_rows_refusals(dev):
    ops = pkg("ops")
    prob, wps, trajs = (torch.from_numpy(a).to(dev) for a in C.make_case(20, 1, 3))
    with pytest.raises(ValueError, match="permutation"):
        ops.score_rank_samples_rows(prob, wps, trajs, 0.25, [0, 1, 1])
    with pytest.raises(RuntimeError, match="1 .. 64"):
        ops.score_rank_samples_rows(prob, wps.repeat(4, 1, 1, 1), trajs.repeat(4, 1, 1, 1), 0.25, [0, 1, 2])
    with pytest.raises(ValueError, match="not contiguous"):
        ops.score_rank_samples_rows(prob[:, :, :, ::2], wps, trajs, 0.25, [0, 1, 2])
    w2 = wps.clone()
    w2[5, 1, 0] = torch.tensor((float(C.W), 0.0), device=dev)
    with pytest.raises(RuntimeError, match="outside the"):
        ops.score_rank_samples_rows(prob, w2, trajs, 0.25, [2, 0, 1])
    # a device-side row out of range is never used as an address: that agent writes nothing, the call raises
    with pytest.raises(RuntimeError, match="out_row names a row outside"):
        ops.score_rank_samples_rows(prob, wps, trajs, 0.25, torch.tensor([0, 7, 2], device=dev, dtype=torch.int32))
    ops.score_rank_samples_rows(prob, wps, trajs, 0.25, [2, 0, 1])                     # the flag was cleared


@pytest.mark.parametrize("L", S.GATHER_LS)
def test_gather_rows_is_bit_exact(dev, L):
    ops = pkg("ops")
    src, idx = S.gather_case(L, 37, 50)
    d_src = torch.from_numpy(src).to(dev)
    assert np.array_equal(ops.gather_rows(d_src, idx).cpu().numpy(), src[idx])
    assert np.array_equal(ops.gather_rows(d_src, torch.from_numpy(idx.astype(np.int32)).to(dev)).cpu().numpy(), src[idx])
    # a source that starts 4 bytes off an 8-byte boundary (rows of even L then move float by float), and rows with inner dimensions
    buf = torch.zeros(37 * L + 1, device=dev)
    odd = buf[1:].view(37, L)
    odd.copy_(d_src)
    assert odd.data_ptr() % 8 == 4
    assert np.array_equal(ops.gather_rows(odd, idx).cpu().numpy(), src[idx])
    if L % 2 == 0:
        assert np.array_equal(ops.gather_rows(d_src.view(37, L // 2, 2), idx).cpu().numpy(), src[idx].reshape(-1, L // 2, 2))
    with pytest.raises(ValueError, match="outside"):
        ops.gather_rows(d_src, [0, 37])
    ops.gather_rows(d_src, torch.tensor([0, 37], device=dev, dtype=torch.int32))      # device-side: reported at the next check
    with pytest.raises(RuntimeError, match="outside the source"):
        ops.check_gather_status()
    ops.check_gather_status()


def test_gather_rows_beyond_2_31_floats(dev):
    ops = pkg("ops")
    L, rows = 4096, 2 ** 19 + 8
    assert rows * L > 2 ** 31
    free, _ = torch.cuda.mem_get_info(dev)
    assert free > 12 * 2 ** 30, "the 8.6 GB source of this test does not fit beside what the device already holds"
    src = torch.empty((rows, L), device=dev, dtype=torch.float32)
    gen = torch.Generator(device=dev).manual_seed(11)
    for r0 in range(0, rows, 2 ** 16):
        src[r0:r0 + 2 ** 16].normal_(generator=gen)
    idx = np.array([rows - 1, 0, 2 ** 19, rows - 1, 2 ** 19 - 1, 12345], dtype=np.int64)      # the very last row, rows around 2^31 floats
    got = ops.gather_rows(src, idx)
    assert torch.equal(got, src[torch.from_numpy(idx).to(dev)])
    del src, got
    torch.cuda.empty_cache()


# ---- the drivers ----------------------------------------------------------------------------------------------------------------
def trainer_params(cfg, **over):
    p = dict(obs_len=cfg.obs_len, pred_len=cfg.pred_len, segmentation_model_fp=None, use_features_only=False, n_semantic_classes=cfg.n_classes,
             encoder_channels=list(cfg.enc), decoder_channels=list(cfg.dec), waypoints=list(cfg.waypoints), train_net=cfg.train_net,
             position=list(cfg.position), network=cfg.network, n_fusion=cfg.n_fusion, resize_factor=cfg.resize_factor, dataset_name="sdd",
             batch_size=None, n_goal=20, n_traj=1, temperature=cfg.temperature, rel_threshold=0.002, use_TTST=False, use_CWS=False,
             CWS_params=None, use_raw_data=False)
    p.update(over)
    return p


def predict_args(cfg, in_t, n_goal=20):
    return (in_t, list(cfg.waypoints), n_goal, 1, cfg.obs_len, cfg.resize_factor, cfg.temperature)


# ---- 2. one style is predict() ---------------------------------------------------------------------------------------------------
def test_one_style_is_predict_bit_for_bit(dev, tmp_path):
    g = Golden("tiny_short_mosa1")
    cfg = g.cfg()
    trn, P = pkg("models.trainer"), pkg("utils.predict")
    sd = g.state_dict()
    base_file = tmp_path / "base.pt"
    torch.save(sd, base_file)
    files = {}
    for name, seed in (("biker", 1), ("car", 2), ("cart", 3)):
        files[name] = str(tmp_path / f"{name}.pt")
        torch.save(perturbed(sd, seed), files[name])
    in_t = O.dist_template(cfg.template_size).to(dev)
    scene, observed = g.t("scene")[0], g.t("traj")[:, :cfg.obs_len]
    N = observed.shape[0]
    with contextlib.redirect_stdout(io.StringIO()):
        single, one, three = (trn.YNetTrainer(trainer_params(cfg), device=dev) for _ in range(3))
        single.load_separated_params(str(base_file), files["car"])
        single.model.to(dev)
        bank1 = one.load_styles(str(base_file), {"car": files["car"]})
        bank3 = three.load_styles(str(base_file), files)
    assert one.styles is bank1 and bank3.names == ("base", "biker", "car", "cart")
    for kw in (dict(), dict(return_maps=True, batch_size=2)):
        torch.manual_seed(31)
        want = P.predict(single.model, scene, observed, *predict_args(cfg, in_t), network=cfg.network, **kw)
        for bank in (bank1, bank3):
            torch.manual_seed(31)
            got = P.predict_styles(bank, scene, observed, ["car"] * N, *predict_args(cfg, in_t), network=cfg.network, **kw)
            assert set(got) == set(want) | {"style_index"}
            for k in want:
                assert torch.equal(got[k], want[k]), (k, len(bank))
            assert got["style_index"].tolist() == [bank.index("car")] * N
    # the trainer's wrapper: a DataFrame with a style column, every agent on one style -> YNetTrainer.predict on the single-style model
    rows = []
    for i in range(N):
        xy = observed[i].numpy() / cfg.resize_factor
        rows.append(pd.DataFrame({"metaId": i, "sceneId": "scene0", "x": xy[:, 0], "y": xy[:, 1], "style": "car"}))
    df = pd.concat(rows, ignore_index=True)
    with contextlib.redirect_stdout(io.StringIO()):
        torch.manual_seed(32)
        res_w, frame_w = single.predict(df.drop(columns="style"), {"scene0": scene})
        torch.manual_seed(32)
        res_g, frame_g = three.predict_styles(df, {"scene0": scene})
    for k in res_w["scene0"]:
        assert torch.equal(res_g["scene0"][k], res_w["scene0"][k]), k
    assert frame_g.equals(frame_w)
    with pytest.raises(ValueError, match="unknown style 'truck'"):
        three.predict_styles(df.assign(style="truck"), {"scene0": scene})


# ---- 3. mixed styles against the CPU oracle ----------------------------------------------------------------------------------------
def mixed_case(which):
    """(cfg, base state dict, scene [1, C, H, W], trajectories, style per agent, K): the tiny LoRA fixture, and C2's architecture
    with B = 32 at 256^2.  C2 runs K = 4 forced samples: the K decoder passes are K runs of one launch sequence over all rows (the
    bank does not enter them), and the fp32 oracle costs ~6 GFLOP per agent and pass on the CPU."""
    if which == "tiny":
        g = Golden("tiny_short_mosa1")
        cfg, sd, scene = g.cfg(), g.state_dict(), g.t("scene")
        n, K = 9, 20
        names = ["a", "b", "a", "c", "b", "a", "b", "a", "b"]       # interleaved; c has ONE agent; the base style has none
    else:
        cfg = O.sdd_short(train_net="mosa_1", position=["0", "1", "2", "3", "4"])
        sd = O.make_state_dict(cfg, seed=3, lora_b_std=0.05)
        scene = O.synthetic_scene(cfg, 256, 256, 5)
        n, K = 32, 4
        names = (["a", "b", "b"] * 11)[:32]                          # interleaved: 11 / 20 / 1 agents, the base style has none
        names[8] = "c"
    H, W = scene.shape[-2:]
    traj = O.synthetic_trajectories(cfg, n, H, W, 7)
    return cfg, sd, scene, traj, names, K


@pytest.mark.parametrize("which", ["tiny", "c2"])
def test_mixed_styles_match_the_oracle(dev, which):
    cfg, sd, scene, traj, names, K = mixed_case(which)
    SB, P = pkg("models.style_bank"), pkg("utils.predict")
    H, W = scene.shape[-2:]
    n, n_wp = traj.shape[0], len(cfg.waypoints)
    styles = {name: perturbed(sd, seed) for name, seed in (("a", 11), ("b", 12), ("c", 13))}
    assert names.count("c") == 1 and SB.BASE_STYLE not in names and len(set(names)) == 3
    rng = np.random.default_rng(21)
    forced = torch.from_numpy(np.stack([rng.integers(W // 4, 3 * W // 4, size=(K, n, n_wp)),
                                        rng.integers(H // 4, 3 * H // 4, size=(K, n, n_wp))], axis=-1).astype(np.float32))
    model = build_model(cfg, sd, dev)
    bank = SB.StyleBank(model, styles)
    in_t = O.dist_template(cfg.template_size)
    res = P.predict_styles(bank, scene[0], traj[:, :cfg.obs_len], names, in_t.to(dev), list(cfg.waypoints), K, 1, cfg.obs_len,
                           cfg.resize_factor, cfg.temperature, network=cfg.network, forced_samples=forced, return_maps=True)
    assert res["style_index"].tolist() == [bank.index(s) for s in names]
    got_traj = unrank(res["trajectories"], res["order"]).cpu().numpy() * cfg.resize_factor       # [n, K, pred, 2], sample order
    got_wps = unrank(res["waypoints"], res["order"]).cpu()
    assert torch.equal(got_wps, forced.permute(1, 0, 2, 3)), "the forced samples did not come back at their agents (caller's order)"
    for name in ("a", "b", "c"):
        who = [i for i, s in enumerate(names) if s == name]
        want = O.eval_batch({**sd, **styles[name]}, cfg, scene, traj[who], in_t, n_goal=K, n_traj=1, waypoint_samples=forced[:, who])
        err = np.abs(got_traj[who] - want["trajs"].permute(1, 0, 2, 3).numpy()).max()
        gm = res["goal_map"][who].cpu().numpy()
        gerr = np.abs(gm - want["goal_map"].numpy()).max()
        print(f"{which} style {name} ({len(who)} agents): max coordinate error {err:.3e} px, max goal-map error {gerr:.3e}")
        assert err <= 1e-4
        np.testing.assert_allclose(gm, want["goal_map"].numpy(), rtol=1e-4, atol=2e-5)
        # scores, compared after sorting (a tie-induced swap does not fail).  Bound: d/dx log sigmoid(x / T) <= 1 / T, so a logit inside
        # rtol 1e-4 / atol 2e-5 moves a way-point's term by at most (1e-4 |x| + 2e-5) / T; plus the ranking kernel's own 1e-5 |score|.
        # Sorting is 1-Lipschitz in the maximum norm: every sorted score is within the agent's largest per-sample bound.
        logit = want["goal_map"][:, list(cfg.waypoints)].double().numpy()
        sig = want["wp_sigmoid"].double().numpy()
        x, y = forced[:, who, :, 0].long().numpy(), forced[:, who, :, 1].long().numpy()
        b_ = np.arange(len(who))[None, :, None]
        w_ = np.arange(n_wp)[None, None, :]
        score64 = np.log(sig[b_, w_, y, x] + 1e-12).sum(axis=2).T                      # [agents, K]
        bound = ((1e-4 * np.abs(logit[b_, w_, y, x]) + 2e-5) / cfg.temperature).sum(axis=2).T + 1e-5 * np.abs(score64)
        serr = np.abs(res["scores"][who].cpu().numpy() - np.sort(score64, axis=1)[:, ::-1])
        print(f"{which} style {name}: max score error {serr.max():.3e} (bound {bound.max(axis=1).min():.3e} .. {bound.max():.3e})")
        assert (serr <= bound.max(axis=1, keepdims=True)).all()
    # the styles do differ: one style's oracle does not describe another style's agents
    a0, b0 = names.index("a"), names.index("b")
    other = O.eval_batch({**sd, **styles["b"]}, cfg, scene, traj[[a0]], in_t, n_goal=K, n_traj=1, waypoint_samples=forced[:, [a0]])
    assert np.abs(res["goal_map"][a0].cpu().numpy() - other["goal_map"][0].numpy()).max() > 1e-3, (a0, b0)


# ---- 4. the base model is untouched ------------------------------------------------------------------------------------------------
def test_bank_call_leaves_the_model_and_its_captured_step_untouched(dev):
    """eager, capture, replay (three equal batches), then two more replays of the graph captured before: with a bank built and a
    C2-sized predict_styles call in between, everything is bit-equal to the run without them -- whether or not step graphs are on."""
    cfg = O.sdd_short(train_net="mosa_1", position=["0", "1", "2", "3", "4"])
    sd = O.make_state_dict(cfg, seed=3, lora_b_std=0.05)
    scene = O.synthetic_scene(cfg, 256, 256, 5)
    traj = O.synthetic_trajectories(cfg, 8, 256, 256, 7)
    te, trn, P, SB, ev = (pkg(m) for m in ("utils.train_epoch", "models.trainer", "utils.predict", "models.style_bank", "utils.evaluate"))
    S_ = cfg.template_size
    in_t, gt_t = O.dist_template(S_).to(dev), O.gaussian_template(S_, cfg.kernlen, cfg.nsig).to(dev)
    meta = pd.DataFrame({"metaId": np.arange(traj.shape[0])})
    styles = {name: perturbed(sd, seed) for name, seed in (("a", 11), ("b", 12), ("c", 13))}

    def run(with_bank):
        model = build_model(cfg, sd, dev)
        model.train()
        torch.manual_seed(6)
        opt = torch.optim.Adam(model.parameters(), lr=1e-3)
        crit = trn.HipBCEWithLogitsLoss()

        def epoch(steps):
            return te.train_epoch(model, [(traj.clone(), [meta], "s")] * steps, {"s": scene[0]}, opt, crit, cfg.loss_scale, dev, "sdd", None,
                                  gt_t, in_t, list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, traj.shape[0], 10000, cfg.resize_factor,
                                  cfg.network, False)
        outs = [epoch(3)]
        res = None
        if with_bank:
            versions = {n: (id(p), p.data_ptr(), p._version) for n, p in model.named_parameters()}
            token = ev._weights_token(model)
            bank = SB.StyleBank(model, styles)
            observed = traj[:, :cfg.obs_len].repeat(4, 1, 1)
            names = (["a", "b", "a", "c", "b", "base"] * 6)[:32]
            torch.manual_seed(5)
            res = P.predict_styles(bank, scene[0], observed, names, in_t, list(cfg.waypoints), 20, 1, cfg.obs_len, cfg.resize_factor,
                                   cfg.temperature, network=cfg.network)
            assert model.training
            assert versions == {n: (id(p), p.data_ptr(), p._version) for n, p in model.named_parameters()}
            assert token == ev._weights_token(model)
        outs.append(epoch(2))
        return outs, {n: p.detach().clone() for n, p in model.named_parameters()}, \
            {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, res

    out0, p0, g0, _ = run(False)
    out1, p1, g1, res = run(True)
    assert res["trajectories"].shape == (32, 20, cfg.pred_len, 2) and bool(torch.isfinite(res["scores"]).all())
    assert out0 == out1, (out0, out1)
    assert set(g0) == set(g1) and len(g0) > 0
    for n in p0:
        assert torch.equal(p0[n], p1[n]), n
    for n in g0:
        assert torch.equal(g0[n], g1[n]), n


# ---- 5. / 6. bits repeat; chunking ---------------------------------------------------------------------------------------------------
def test_bits_repeat_and_chunks_agree(dev):
    cfg, sd, scene, traj, names, K = mixed_case("tiny")
    SB, P = pkg("models.style_bank"), pkg("utils.predict")
    model = build_model(cfg, sd, dev)
    bank = SB.StyleBank(model, {name: perturbed(sd, seed) for name, seed in (("a", 11), ("b", 12), ("c", 13))})
    in_t = O.dist_template(cfg.template_size).to(dev)
    args = (bank, scene[0], traj[:, :cfg.obs_len], names, in_t, list(cfg.waypoints), K, 1, cfg.obs_len, cfg.resize_factor, cfg.temperature)
    torch.manual_seed(41)
    a = P.predict_styles(*args, network=cfg.network, return_maps=True)
    torch.manual_seed(41)
    b = P.predict_styles(*args, network=cfg.network, return_maps=True)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    # chunks smaller than a segment (style a has 4 agents, b has 4) and larger than N; forced samples, so every chunking takes the same ones
    n, n_wp = traj.shape[0], len(cfg.waypoints)
    H, W = scene.shape[-2:]
    rng = np.random.default_rng(22)
    forced = torch.from_numpy(np.stack([rng.integers(W // 4, 3 * W // 4, size=(K, n, n_wp)),
                                        rng.integers(H // 4, 3 * H // 4, size=(K, n, n_wp))], axis=-1).astype(np.float32))
    whole = P.predict_styles(*args, network=cfg.network, forced_samples=forced)
    for bs in (2, 3, n + 5):
        part = P.predict_styles(*args, network=cfg.network, forced_samples=forced, batch_size=bs)
        assert torch.equal(unrank(part["waypoints"], part["order"]), unrank(whole["waypoints"], whole["order"]))
        err = (unrank(part["trajectories"], part["order"]) - unrank(whole["trajectories"], whole["order"])).abs().max().item() * cfg.resize_factor
        print(f"batch_size {bs}: max coordinate difference to one chunk {err:.3e} px")
        assert err <= 1e-4
        assert torch.equal(part["style_index"], whole["style_index"])

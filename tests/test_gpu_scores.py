"""The four goal-map scores of evaluate() together on the MI355X (utils/scores.py): on the reference's smallest fixture, one scene run as
two batches, the call with all four flags reports bit for bit what each flag reports alone, in the documented column and key order, and
moves nothing else -- ADE / FDE, the predictions, the goal maps, the captured-sweep cache, the status flags."""
import numpy as np
import pandas as pd
import pytest
import torch

from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu

FLAGS = {"return_likelihood": True, "return_compliance": True, "return_sharpness": (0.5, 0.9), "return_radial": {"radii": (4, 8), "k": (1, 5)}}


def test_all_four_flags_at_once_equal_each_alone(dev):
    g = Golden("tiny_short_mosa1")
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    ev, ops = pkg("utils.evaluate"), pkg("ops")
    in_t = O.dist_template(cfg.template_size).to(dev)
    S = g.t("eval/waypoint_samples")                                # [K, B, n_wp, 2], the reference's own samples
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    B, traj, scene = m["B"], g.t("traj"), g.t("scene")[0]
    bs = (B + 1) // 2                                               # two batches: the per-batch lists are really concatenated
    forced = {b: S[:, b:b + bs] for b in range(0, B, bs)}           # keyed by each batch's first row
    assert len(forced) == 2
    loader = [(traj.clone(), [pd.DataFrame({"metaId": np.arange(B)})], "scene0")]

    def run(**kw):
        torch.manual_seed(11)
        return ev.evaluate(model, loader, {"scene0": scene}, dev, "sdd", None, in_t, list(cfg.waypoints), "test", n_goal, n_traj, cfg.obs_len,
                           bs, cfg.resize_factor, cfg.temperature, network=cfg.network, **kw)

    def cache_state():
        c = ev._sweep_graphs.get(model)
        return None if c is None else (c["token"], [(k, id(v), v.seen, v.ready, v.failed) for k, v in c["entries"].items()])

    run()                                                           # a plain sweep: it may enter the cache
    before = cache_state()
    kw = dict(return_preds=True, return_samples=True, forced_samples=forced)
    base = run(**kw)
    combined = run(**kw, **FLAGS)
    alone = {flag: run(**kw, **{flag: value}) for flag, value in FLAGS.items()}
    assert cache_state() == before
    assert ops.check_likelihood_status() is False and ops.check_credible_status() is False and ops.check_radial_status() is False
    ops.check_patch_status()

    # the documented orders
    n_cls = scene.shape[0]
    base_cols, base_keys = ["metaId", "sceneId", "ade", "fde"], ["groundtruth", "prediction", "waypoint_sample", "goal_map", "goal_sigmoid_map"]
    cols = {"return_likelihood": ["nll", "nll_goal", "entropy_goal", "hpd_goal"],
            "return_compliance": [f"goal_mass_{k}" for k in range(n_cls)] + ["gt_goal_class"] + [f"sample_goal_rate_{k}" for k in range(n_cls)],
            "return_sharpness": ["area50_goal", "inside50_goal", "area90_goal", "inside90_goal"],
            "return_radial": ["radial_mean_goal", "radial_rms_goal", "hit4_goal", "hit8_goal", "best_of_1_lower_goal", "best_of_1_upper_goal",
                              "best_of_5_lower_goal", "best_of_5_upper_goal"]}
    keys = {"return_radial": ["radial_mean_steps", "radial_rms_steps", "radial_hit_steps", "best_of_k_lower_steps", "best_of_k_upper_steps"],
            "return_sharpness": ["area_steps", "threshold_steps", "inside_steps"],
            "return_compliance": ["class_mass_steps"],
            "return_likelihood": ["nll_steps", "entropy_steps", "hpd_steps"]}
    _, _, df_all, td_all = combined
    assert list(base[2].columns) == base_cols and list(base[3]) == base_keys + ["metaId", "sceneId"]
    assert list(df_all.columns) == base_cols + sum((cols[f] for f in ("return_likelihood", "return_compliance", "return_sharpness", "return_radial")), [])
    assert list(td_all) == base_keys + sum((keys[f] for f in ("return_radial", "return_sharpness", "return_compliance", "return_likelihood")), []) \
        + ["metaId", "sceneId"]
    assert len(df_all) == B and all(td_all[k].shape[0] == B for k in sum(keys.values(), []))

    def same(a, b, what):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=a.dtype.kind == "f"), what

    # every score of the combined call is the single-flag call's, bit for bit
    for flag, (_, _, df1, td1) in alone.items():
        assert list(df1.columns) == base_cols + cols[flag] and list(td1) == base_keys + keys[flag] + ["metaId", "sceneId"], flag
        for c in cols[flag]:
            same(df_all[c].to_numpy(), df1[c].to_numpy(), (flag, c))
        for k in keys[flag]:
            same(td_all[k], td1[k], (flag, k))
    # and no flag moves anything else
    for what, (ade, fde, df, td) in [("all", combined)] + list(alone.items()):
        assert ade == base[0] and fde == base[1], what
        for c in base_cols:
            same(df[c].to_numpy(), base[2][c].to_numpy(), (what, c))
        for k in base_keys + ["metaId"]:
            same(td[k], base[3][k], (what, k))
        assert td["sceneId"] == base[3]["sceneId"], what

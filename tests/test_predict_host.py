"""predict(): the ground-truth-free K-sample forecast (utils/predict.py, YNetTrainer.predict, ynet_score_rank_samples) -- everything
that is decided before the device is touched: signatures, argument validation, the exported symbol."""
import contextlib
import ctypes
import inspect
import io

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import pkg

OBS, PRED = 8, 12


def _trainer(**over):
    trn = pkg("models.trainer")
    params = dict(obs_len=OBS, pred_len=PRED, segmentation_model_fp=None, use_features_only=False, n_semantic_classes=6,
                  encoder_channels=[8, 8, 16, 16, 16], decoder_channels=[16, 16, 16, 8, 8], waypoints=[11], train_net="mosa_1",
                  position=["0"], network="original", n_fusion=None, resize_factor=0.25, dataset_name="sdd", batch_size=4, n_goal=20,
                  n_traj=1, temperature=1.0, rel_threshold=0.01, use_TTST=False, use_CWS=False, CWS_params=None, use_raw_data=False)
    params.update(over)
    with contextlib.redirect_stdout(io.StringIO()):
        return trn.YNetTrainer(params, device=torch.device("cpu"))


def _df(rows_per_agent):
    parts = []
    for i, n in enumerate(rows_per_agent):
        parts.append(pd.DataFrame({"metaId": i, "sceneId": "scene0", "x": np.linspace(40, 80, n) + i, "y": np.linspace(60, 90, n)}))
    return pd.concat(parts, ignore_index=True)


def test_symbol_is_declared_bound_and_exported():
    L = pkg("_lib")
    name = "ynet_score_rank_samples"
    assert name in L.header_symbols()
    assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == 16
    assert hasattr(ctypes.CDLL(L.LIB_PATH), name)
    with open(L.HEADER_PATH) as f:
        text = f.read()
    decl = text.index("int " + name)
    comment = text[text.rindex("/*", 0, decl):decl]
    assert "utils/evaluate.py:229-266" in comment and "utils/image_utils.py:110-135" in comment      # every entry cites what it serves


def test_entry_refuses_bad_arguments_before_any_launch():
    L = pkg("_lib")
    lib = L.load()
    vp = ctypes.c_void_p
    p = vp(64)

    def call(K=20, B=2, n_wp=1, pred_len=PRED, H=32, W=48, inv=4.0, prob=p, wps=p):
        return lib.ynet_score_rank_samples(prob, wps, p, B, K, n_wp, pred_len, H, W, inv, p, p, p, p, p, None)

    assert call(K=65) != 0 and b"1 .. 64" in lib.ynet_last_error()
    assert call(K=0) != 0 and b"1 .. 64" in lib.ynet_last_error()
    assert call(K=-3) != 0
    assert call(prob=None) != 0 and b"null" in lib.ynet_last_error()
    assert call(B=0) != 0 and b"bad shape" in lib.ynet_last_error()
    assert call(H=0) != 0
    assert call(inv=0.0) != 0 and b"resize_factor" in lib.ynet_last_error()
    assert call(inv=float("inf")) != 0
    assert call(wps=vp(68)) != 0 and b"aligned" in lib.ynet_last_error()


def test_op_refuses_host_tensors():
    ops = pkg("ops")
    assert list(inspect.signature(ops.score_rank_samples).parameters) == ["prob", "waypoint_samples", "trajs", "resize_factor"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_rank_samples(torch.rand(2, 1, 8, 8), torch.zeros(4, 2, 1, 2), torch.zeros(4, 2, PRED, 2), 0.25)
    with pytest.raises(TypeError):
        ops.score_rank_samples(np.zeros((2, 1, 8, 8), np.float32), torch.zeros(4, 2, 1, 2), torch.zeros(4, 2, PRED, 2), 0.25)


def test_predict_signature():
    P = pkg("utils.predict")
    names = list(inspect.signature(P.predict).parameters)
    assert names == ["model", "scene_image", "observed", "input_template", "waypoints", "n_goal", "n_traj", "obs_len", "resize_factor",
                     "temperature", "use_TTST", "use_CWS", "rel_thresh", "CWS_params", "network", "swap_semantic", "batch_size",
                     "max_effective_batch", "forced_samples", "return_maps"]
    d = {k: v.default for k, v in inspect.signature(P.predict).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(use_TTST=False, use_CWS=False, rel_thresh=0.002, CWS_params=None, network=None, swap_semantic=False, batch_size=None,
                     max_effective_batch=256, forced_samples=None, return_maps=False)
    # the shared pieces of the sweep are evaluate()'s own, not copies
    ev, iu = pkg("utils.evaluate"), pkg("utils.image_utils")
    assert P._decoder_passes is ev._decoder_passes and P._goal_maps is ev._goal_maps and P._draw_waypoints is ev._draw_waypoints
    assert ev.sampling is iu.sampling and ev.gather_patches is iu.gather_patches
    for name in ("ttst_goals", "cws_waypoints", "sampling", "gather_patches", "_plain_sweep", "_best_of_k"):      # (reached through those)
        assert getattr(P, name, getattr(ev, name)) is getattr(ev, name)
    assert list(inspect.signature(pkg("models.trainer").YNetTrainer.predict).parameters) == ["self", "df_obs", "image_path_or_images",
                                                                                              "return_maps"]


def test_predict_validates_before_touching_the_device():
    P = pkg("utils.predict")
    scene = torch.zeros(6, 64, 64)
    base = dict(model=None, scene_image=scene, input_template=None, waypoints=[11], n_goal=20, n_traj=1, obs_len=OBS, resize_factor=0.25,
                temperature=1.0)
    with pytest.raises(ValueError, match="never cut silently"):          # more than obs_len steps
        P.predict(observed=np.zeros((3, OBS + PRED, 2), np.float32), **base)
    with pytest.raises(ValueError, match="obs_len is 8"):                # fewer
        P.predict(observed=np.zeros((3, OBS - 1, 2), np.float32), **base)
    with pytest.raises(ValueError, match="up to 64"):                    # K > 64
        P.predict(observed=np.zeros((3, OBS, 2), np.float32), **{**base, "n_goal": 13, "n_traj": 5})
    with pytest.raises(ValueError, match="at least one sample"):         # K < 1
        P.predict(observed=np.zeros((3, OBS, 2), np.float32), **{**base, "n_goal": 0})
    with pytest.raises(ValueError, match=r"\[N, obs_len, 2\]"):
        P.predict(observed=np.zeros((3, OBS), np.float32), **base)
    with pytest.raises(ValueError, match="no agents"):
        P.predict(observed=np.zeros((0, OBS, 2), np.float32), **base)
    with pytest.raises(ValueError, match="CWS_params"):
        P.predict(observed=np.zeros((3, OBS, 2), np.float32), **{**base, "waypoints": [5, 11], "use_CWS": True})
    with pytest.raises(ValueError, match="forced_samples"):
        P.predict(observed=np.zeros((3, OBS, 2), np.float32), forced_samples=torch.zeros(20, 2, 1, 2), **base)


def test_trainer_predict_validates_rows_and_refuses_eth():
    images = {"scene0": torch.zeros(6, 64, 64)}
    t = _trainer()
    with pytest.raises(ValueError, match="exactly obs_len = 8 rows.*metaId 1 has 20"):       # a full track slipped in
        t.predict(_df([OBS, OBS + PRED, OBS]), images)
    with pytest.raises(ValueError, match="metaId 0 has 7"):
        t.predict(_df([OBS - 1, OBS]), images)
    with pytest.raises(ValueError, match="never cut silently"):                               # the dict form, too long
        t.predict({"scene0": np.zeros((2, OBS + 1, 2))}, images)
    with pytest.raises(ValueError, match="up to 64"):
        _trainer(n_goal=33, n_traj=2).predict(_df([OBS, OBS]), images)
    with pytest.raises(NotImplementedError, match="world coordinates"):
        _trainer(dataset_name="eth").predict(_df([OBS, OBS]), images)
    with pytest.raises(ImportError, match="dict"):                                            # image decoding stays out of scope
        t.predict(_df([OBS, OBS]), "some/directory")


def test_kernel_test_inputs_meet_the_ambiguity_cap_in_fp64():
    """The GPU test lets either order pass where neighbouring fp64 scores are closer than n_wp * 2^-20 * |score| and caps such pairs at 1 %:
    the seed of tests/_predict_cases.py meets that cap by the fp64 restatement alone, and plants exact ties in every case with K >= 2."""
    import _predict_cases as C
    for K in C.KS:
        for n_wp in C.NWPS:
            for B in C.BS:
                prob, wps, _ = C.make_case(K, n_wp, B)
                assert prob.min() > 0 and prob.max() < 1 and (wps == np.round(wps)).all()
                score = C.score_fp64(prob, wps)
                assert score.shape == (B, K) and np.isfinite(score).all()
                order = C.rank_fp64(score)
                frac = C.check_order(order, score, n_wp)
                assert frac < 0.01, (K, n_wp, B, frac)
                if K >= 2:
                    gap, _ = C.adjacent_pairs(score, order, n_wp)
                    assert (gap == 0).any(axis=1).all()
                    with pytest.raises(AssertionError, match="index order"):          # the checker does catch a swapped tie
                        swapped = order.copy()
                        r = int(np.argmax(gap[0] == 0))
                        swapped[0, [r, r + 1]] = swapped[0, [r + 1, r]]
                        C.check_order(swapped, score, n_wp)

"""The style bank (models/style_bank.py, utils/predict.py: predict_styles, ynet_score_rank_samples_rows, ynet_gather_rows) -- everything
that is decided before the device is touched: the exported symbols, every refusal, the sort / offset bookkeeping, and the fp64
restatements the GPU tests compare against, checked on their own case tables."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _predict_cases as C
import _style_cases as S
from conftest import Golden, build_model, pkg

OBS = 8


def _model():
    g = Golden("tiny_short_mosa1")
    return build_model(g.cfg(), g.state_dict()), g


def _style(g, seed, scale=0.05):
    gen = torch.Generator().manual_seed(seed)
    return {k: v + scale * torch.randn(v.shape, generator=gen) for k, v in g.state_dict().items() if "lora_" in k}


def test_symbols_are_declared_bound_and_exported():
    L = pkg("_lib")
    lib = ctypes.CDLL(L.LIB_PATH)
    with open(L.HEADER_PATH) as f:
        text = f.read()
    for name, nargs in (("ynet_score_rank_samples_rows", 17), ("ynet_gather_rows", 8)):
        assert name in L.header_symbols()
        assert name in L.SIGNATURES and len(L.SIGNATURES[name][1]) == nargs
        assert hasattr(lib, name)
        decl = text.index("int " + name)
        comment = text[text.rindex("/*", 0, decl):decl]
        assert "predict_styles" in comment                          # every entry says which call site it serves
    ops = pkg("ops")
    assert list(inspect.signature(ops.score_rank_samples_rows).parameters) == ["prob", "waypoint_samples", "trajs", "resize_factor", "out_row"]
    assert list(inspect.signature(ops.gather_rows).parameters) == ["src", "idx"]


def test_entries_refuse_bad_arguments_before_any_launch():
    L = pkg("_lib")
    lib = L.load()
    p = ctypes.c_void_p(64)

    def rank(K=20, B=2, rows=p, wps=p, inv=4.0):
        return lib.ynet_score_rank_samples_rows(p, wps, p, rows, B, K, 1, 12, 32, 48, inv, p, p, p, p, p, None)

    assert rank(K=65) != 0 and b"1 .. 64" in lib.ynet_last_error()
    assert rank(K=0) != 0 and b"1 .. 64" in lib.ynet_last_error()
    assert rank(rows=None) != 0 and b"null" in lib.ynet_last_error()
    assert rank(B=0) != 0 and b"bad shape" in lib.ynet_last_error()
    assert rank(inv=0.0) != 0 and b"resize_factor" in lib.ynet_last_error()
    assert rank(wps=ctypes.c_void_p(68)) != 0 and b"aligned" in lib.ynet_last_error()

    def gather(src=p, rows=4, n=3, L_=2, st=p):
        return lib.ynet_gather_rows(src, rows, p, p, n, L_, st, None)

    assert gather(src=None) != 0 and b"null" in lib.ynet_last_error()
    assert gather(st=None) != 0
    assert gather(rows=0) != 0 and b"bad shape" in lib.ynet_last_error()
    assert gather(n=0) != 0 and gather(L_=0) != 0
    assert gather(src=ctypes.c_void_p(66)) != 0 and b"aligned" in lib.ynet_last_error()


def test_ops_refuse_on_the_host():
    ops = pkg("ops")
    for bad in ([0, 1, 1], [0, 1, 3], [0, 1], [-1, 0, 1], [0, 1, 2, 3]):
        with pytest.raises(ValueError, match="permutation"):
            ops.check_row_permutation(bad, 3)
    with pytest.raises(ValueError, match="integers"):
        ops.check_row_permutation(np.array([0.0, 1.0, 2.0]), 3)
    ops.check_row_permutation(torch.tensor([2, 0, 1]), 3)
    ops.check_row_permutation(np.array([0]), 1)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.score_rank_samples_rows(torch.rand(2, 1, 8, 8), torch.zeros(4, 2, 1, 2), torch.zeros(4, 2, 12, 2), 0.25, [0, 1])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.gather_rows(torch.zeros(4, 2), [0, 1])


def test_bank_refusals_name_the_key():
    SB = pkg("models.style_bank")
    model, g = _model()
    good = _style(g, 1)
    key = "encoder.stages.1.1.lora_A"
    with pytest.raises(ValueError, match="empty"):
        SB.StyleBank(model, {})
    with pytest.raises(ValueError, match="'biker' is given twice"):
        SB.StyleBank(model, [("biker", good), ("car", good), ("biker", good)])
    with pytest.raises(ValueError, match="reserved"):
        SB.StyleBank(model, {SB.BASE_STYLE: good})
    with pytest.raises(ValueError, match=r"encoder\.stages\.9\.1\.lora_A is not a parameter"):
        SB.StyleBank(model, {"a": {**good, "encoder.stages.9.1.lora_A": good[key]}})
    with pytest.raises(ValueError, match=r"encoder\.stages\.1\.1\.lora_A has shape.*another rank needs its own model"):
        SB.StyleBank(model, {"a": {**good, key: torch.zeros(good[key].shape[0] * 2, good[key].shape[1])}})
    sd = g.state_dict()
    with pytest.raises(ValueError, match=r"goal_decoder\.center\.0\.weight belongs to no adapted or bias-trainable"):
        SB.StyleBank(model, {"a": {**good, "goal_decoder.center.0.weight": sd["goal_decoder.center.0.weight"]}})
    with pytest.raises(ValueError, match=r"traj_decoder\.predictor\.bias belongs to no"):
        SB.StyleBank(model, {"a": {**good, "traj_decoder.predictor.bias": sd["traj_decoder.predictor.bias"]}})
    # a whole-filter checkpoint (train_net all / train / encoder) is named as such, whatever else it holds
    whole = {k: v for k, v in sd.items() if k.startswith("encoder.")}
    with pytest.raises(ValueError, match="replaces whole filters.*adapter-style checkpoints"):
        SB.StyleBank(model, {"a": whole})
    with pytest.raises(ValueError, match="replaces whole filters.*adapter-style checkpoints"):
        SB.StyleBank(model, {"a": dict(sd)})
    with pytest.raises(ValueError, match="holds no tensor"):
        SB.StyleBank(model, {"a": {}})
    gs = Golden("tiny_short_serial_blocks")
    serial = build_model(gs.cfg(), gs.state_dict())
    k2 = next(k for k in gs.state_dict() if "serial_layer" in k and k.endswith("weight"))
    with pytest.raises(NotImplementedError, match="serial / parallel / semantic"):
        SB.StyleBank(serial, {"a": {k2: gs.state_dict()[k2]}})
    gf = Golden("tiny_long_fusion_mosa3_scene")
    with pytest.raises(NotImplementedError, match="fusion network"):
        SB.StyleBank(build_model(gf.cfg(), gf.state_dict()), {"a": {k: v for k, v in gf.state_dict().items() if "lora_" in k}})


def test_bank_order_ownership_and_files(tmp_path):
    SB = pkg("models.style_bank")
    model, g = _model()
    before = {n: (id(p), p.data_ptr(), p._version) for n, p in model.named_parameters()}
    caches = {n: (id(m._packed), dict(m._packed)) for n, m in model.named_modules() if hasattr(m, "_packed")}
    path = tmp_path / "car.pt"
    torch.save(_style(g, 2), path)
    bias_only = {"encoder.stages.2.1.bias": g.state_dict()["encoder.stages.2.1.bias"] + 1.0}
    bank = SB.StyleBank(model, [("biker", _style(g, 1)), ("car", str(path)), ("shift", bias_only)])
    assert len(bank) == 4 and bank.names == (SB.BASE_STYLE, "biker", "car", "shift")
    assert [bank.index(n) for n in bank.names] == [0, 1, 2, 3] and bank.index(2) == 2
    assert bank.indices(["car", SB.BASE_STYLE, 1, np.int64(3)]) == [2, 0, 1, 3]
    for bad in ("truck", 4, -1, 1.5):
        with pytest.raises(ValueError, match="unknown style"):
            bank.index(bad)
    # nothing of the model was written, and the shadows share the frozen filter but own adapters and caches
    assert before == {n: (id(p), p.data_ptr(), p._version) for n, p in model.named_parameters()}
    assert caches == {n: (id(m._packed), dict(m._packed)) for n, m in model.named_modules() if hasattr(m, "_packed")}
    base = model.get_submodule("encoder.stages.2.1")
    for s, layers in enumerate(bank._shadows):
        twin = layers["encoder.stages.2.1"]
        assert type(twin) is type(base) and twin.weight is base.weight and twin._packed is not base._packed
        assert (twin.lora_A is base.lora_A) == (s in (0, 3)) and (twin.bias is base.bias) == (s != 3)
        assert not any(twin._packed is other["encoder.stages.2.1"]._packed for other in bank._shadows[:s])
    assert torch.equal(bank._shadows[2]["encoder.stages.0.0"].lora_B, _style(g, 2)["encoder.stages.0.0.lora_B"])
    # the copies of the encoder hold the model's own modules wherever no style differs
    assert bank._mixed.stages[1][0] is model.encoder.stages[1][0] and bank._mixed.stages[5] is model.encoder.stages[5]
    assert model.encoder.stages[1][1] is base.__class__ or type(model.encoder.stages[1][1]).__name__ == "LoRAConv2d"      # (the model's tree is intact)
    assert not any(isinstance(m, SB._SegmentedConv) for m in model.modules())
    with pytest.raises(ValueError, match="ascending row bounds"):
        bank.pred_features(torch.zeros(3, 6, 8, 8), torch.zeros(3, OBS, 8, 8), [0, 1, 3])


def test_sort_and_offsets():
    SB = pkg("models.style_bank")
    perm, off = SB.sort_by_style([2, 0, 2, 0, 3, 2], 4)              # style 1 is an empty segment in the middle
    assert perm.tolist() == [1, 3, 0, 2, 5, 4] and off == [0, 2, 2, 5, 6]
    perm, off = SB.sort_by_style([1, 1, 1], 3)                       # all on one style: the identity
    assert perm.tolist() == [0, 1, 2] and off == [0, 0, 3, 3]
    perm, off = SB.sort_by_style([2], 3)                             # N = 1
    assert perm.tolist() == [0] and off == [0, 0, 0, 1]
    perm, off = SB.sort_by_style([0, 1, 0, 2, 1], 3)                 # interleaved: stable inside a style
    assert perm.tolist() == [0, 2, 1, 4, 3] and off == [0, 2, 4, 5]
    for bad in ([3], [-1, 0]):
        with pytest.raises(ValueError, match="outside"):
            SB.sort_by_style(bad, 3)
    with pytest.raises(ValueError, match="one style index per agent"):
        SB.sort_by_style([], 3)


def test_predict_styles_signature_and_validation():
    P, SB = pkg("utils.predict"), pkg("models.style_bank")
    names = list(inspect.signature(P.predict_styles).parameters)
    want = list(inspect.signature(P.predict).parameters)
    assert names == ["bank", "scene_image", "observed", "style"] + want[3:]          # predict()'s remaining arguments
    d = lambda f: {k: v.default for k, v in inspect.signature(f).parameters.items() if v.default is not inspect.Parameter.empty}      # noqa: E731
    assert d(P.predict_styles) == d(P.predict)
    assert list(inspect.signature(pkg("models.trainer").YNetTrainer.predict_styles).parameters) == [
        "self", "df_obs", "image_path_or_images", "style_column", "return_maps"]
    assert list(inspect.signature(pkg("models.trainer").YNetTrainer.load_styles).parameters) == ["self", "pretrained_path", "styles"]
    model, g = _model()
    bank = SB.StyleBank(model, {"a": _style(g, 1), "b": _style(g, 2)})
    base = dict(bank=bank, scene_image=torch.zeros(6, 64, 64), input_template=None, waypoints=[11], n_goal=20, n_traj=1, obs_len=OBS,
                resize_factor=0.25, temperature=1.0)
    obs = np.zeros((3, OBS, 2), np.float32)
    with pytest.raises(ValueError, match="unknown style 'truck'"):
        P.predict_styles(observed=obs, style=["a", "truck", "b"], **base)
    with pytest.raises(ValueError, match="unknown style"):
        P.predict_styles(observed=obs, style=[0, 3, 1], **base)
    with pytest.raises(ValueError, match="2 styles for 3 agents"):
        P.predict_styles(observed=obs, style=["a", "b"], **base)
    with pytest.raises(ValueError, match=r"forced_samples \(20, 2, 1, 2\), expected \(20, 3, 1, 2\)"):
        P.predict_styles(observed=obs, style=["a", "b", "a"], forced_samples=torch.zeros(20, 2, 1, 2), **base)
    with pytest.raises(ValueError, match="never cut silently"):
        P.predict_styles(observed=np.zeros((3, OBS + 12, 2), np.float32), style=["a", "b", "a"], **base)
    with pytest.raises(ValueError, match="up to 64"):
        P.predict_styles(observed=obs, style=["a", "b", "a"], **{**base, "n_goal": 13, "n_traj": 5})
    assert model.training == build_model(g.cfg(), g.state_dict()).training


def test_rows_restatement_on_its_own_case_table():
    """rank_rows_fp64 is the existing fp64 ranking rule with its rows scattered: with the identity it IS that rule; any permutation moves
    whole rows and nothing inside them; planted ties stay in index order at the output rows."""
    for K in C.KS:
        for n_wp in C.NWPS:
            for B in C.BS:
                prob, wps, trajs = C.make_case(K, n_wp, B)
                score0, order0 = C.score_fp64(prob, wps), C.rank_fp64(C.score_fp64(prob, wps))
                for kind in S.PERMS:
                    rows = S.out_rows(kind, B)
                    assert np.array_equal(np.sort(rows), np.arange(B))
                    score, order, ranked, goals = S.rank_rows_fp64(prob, wps, trajs, rows, 0.25)
                    if kind == "identity":
                        assert np.array_equal(order, order0) and np.array_equal(score, score0)
                    assert np.array_equal(order[rows], order0) and np.array_equal(score[rows], score0)
                    b = B - 1
                    assert np.array_equal(ranked[rows[b], 0], trajs[order0[b, 0], b] * np.float32(4.0))
                    assert np.array_equal(goals[rows[b], K - 1], wps[order0[b, K - 1], b])
                    if K >= 2:      # sample K - 1 repeats sample 0: an exact tie, the lower index first, at every output row
                        pos = np.argsort(order, axis=1)
                        assert (score[:, K - 1] == score[:, 0]).all() and (pos[:, K - 1] > pos[:, 0]).all()


def test_rows_inputs_meet_the_ambiguity_cap_in_fp64():
    """The GPU test lets either order pass where neighbouring fp64 scores are closer than n_wp * 2^-20 * |score|, and caps the share of
    such pairs at the 1 % tests/test_predict_host.py allows: met here by the fp64 restatement alone, at the OUTPUT rows, for every
    permutation the GPU test uses."""
    for K in C.KS:
        for n_wp in C.NWPS:
            for B in C.BS:
                prob, wps, trajs = C.make_case(K, n_wp, B)
                for kind in S.PERMS:
                    score, order, _, _ = S.rank_rows_fp64(prob, wps, trajs, S.out_rows(kind, B), 0.25)
                    frac = C.check_order(order, score, n_wp)
                    assert frac < 0.01, (K, n_wp, B, kind, frac)
                    if K >= 2:
                        gap, _ = C.adjacent_pairs(score, order, n_wp)
                        assert (gap == 0).any(axis=1).all()


def test_gather_restatement_cases():
    for L in S.GATHER_LS:
        src, idx = S.gather_case(L, 37, 50)
        assert src.shape == (37, L) and idx.shape == (50,) and idx.min() >= 0 and idx.max() < 37
        assert idx[-1] == idx[0] and idx[25] == idx[0]                               # repeated indices are planted
        assert len(np.unique(src)) == src.size                                       # a wrong row or column cannot pass by coincidence

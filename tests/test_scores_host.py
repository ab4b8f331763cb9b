"""The scorer objects of evaluate() (utils/scores.py) -- everything that needs no GPU, on CPU tensors: the zero-row scores of a data-parallel
rank without rows, the gather / collect / concatenate mechanics over two simulated ranks, the columns and keys on planted arrays, the
refusals of compliance, and the once-per-call warnings with the status calls replaced (nothing touches the device)."""
import warnings

import numpy as np
import pandas as pd
import pytest
import torch

from conftest import pkg

STEPS, K_CLS = 3, 3
LEVELS = (0.25, 0.5, 0.999)
RADIAL = {"radii": (2, 7), "k": (1, 5, 20)}
KINDS = ["likelihood", "compliance", "sharpness", "radial"]


def scene_planes():
    """[K_CLS, 4, 6] one-hot planes: class = column // 2"""
    cls = (torch.arange(6) // 2)[None, :].expand(4, 6)
    return torch.stack([(cls == k).float() for k in range(K_CLS)])


def make(kind):
    S = pkg("utils.scores")
    s = {"likelihood": lambda: S.LikelihoodScore(True), "compliance": lambda: S.ComplianceScore(True),
         "sharpness": lambda: S.SharpnessScore(LEVELS), "radial": lambda: S.RadialScore(RADIAL)}[kind]()
    assert s.on
    s.scene("scene0", scene_planes(), "cpu")
    return s


def spec(kind):
    """key -> (shape after the rows, dtype): what the issue pins for the n_local == 0 branch, per key"""
    f32, f64 = torch.float32, torch.float64
    return {"likelihood": {"nll": ((STEPS,), f32), "entropy": ((STEPS,), f32), "hpd": ((STEPS,), f32)},
            "compliance": {"mass": ((STEPS, K_CLS), f32), "gt_class": ((), torch.int64), "rate": ((K_CLS,), f64)},
            "sharpness": {"area": ((STEPS, len(LEVELS)), torch.int32), "threshold": ((STEPS, len(LEVELS)), f32),
                          "inside": ((STEPS, len(LEVELS)), f32)},
            "radial": {"mean": ((STEPS,), f64), "rms": ((STEPS,), f64), "hit": ((STEPS, 2), f64), "best_of_k_lower": ((STEPS, 3), f64),
                       "best_of_k_upper": ((STEPS, 3), f64)}}[kind]


def planted(kind, n, seed):
    """n rows of distinct values per key, in score()'s dtypes; a NaN in the first row of every floating key"""
    g = torch.Generator().manual_seed(seed)
    out = {}
    for k, (tail, dt) in spec(kind).items():
        v = torch.rand((n,) + tail, generator=g, dtype=torch.float64) * 50
        if dt.is_floating_point:
            v = v.to(dt)
            v.view(n, -1)[0, 0] = float("nan")
        else:
            v = v.round().to(dt)
        out[k] = v
    return out


class FakeDP:
    """Two ranks, the second without rows: ``per_rank[r]`` is rank r's scores dict of the batch, this object stands on ``rank``.
    gather_rows concatenates the planted per-rank tensors (the keys come in the dict's order) after checking what an all_gather needs:
    the same dtype and trailing shape on every rank."""

    def __init__(self, per_rank, rank):
        self.per_rank, self.rank, self.calls = per_rank, rank, 0

    def shard_sizes(self, n):
        return [n, 0]

    def gather_rows(self, t, sizes):
        key = list(self.per_rank[self.rank])[self.calls]
        self.calls += 1
        assert t is self.per_rank[self.rank][key]
        parts = [p[key] for p in self.per_rank]
        assert [len(p) for p in parts] == sizes, key
        assert all(p.dtype == t.dtype and p.shape[1:] == t.shape[1:] for p in parts), (key, [(p.dtype, p.shape) for p in parts])
        return torch.cat(parts)


@pytest.fixture
def quiet_status(monkeypatch):
    """the three status calls, replaced: -> the list of (name, raise_error) calls made"""
    ops, calls = pkg("ops"), []
    for name in ("likelihood", "credible", "radial"):
        def check(raise_error=True, name=name):
            calls.append((name, raise_error))
            return False
        monkeypatch.setattr(ops, f"check_{name}_status", check)
    return calls


@pytest.mark.parametrize("kind", KINDS)
def test_empty_states_every_shape_and_dtype(kind):
    s = make(kind)
    e = s.empty(STEPS, "cpu", "scene0")
    assert list(e) == list(spec(kind)) == list(s.keys)
    for k, (tail, dt) in spec(kind).items():
        assert e[k].shape == (0,) + tail and e[k].dtype == dt, (k, e[k].shape, e[k].dtype)


@pytest.mark.parametrize("kind", KINDS)
def test_two_ranks_two_batches_give_the_planted_rows(kind, quiet_status):
    batches = [planted(kind, 3, seed=1), planted(kind, 2, seed=2)]
    for rank in (0, 1):                                             # the rank with the rows, the rank without
        s = make(kind)
        for rows in batches:
            per_rank = [rows, s.empty(STEPS, "cpu", "scene0")]
            dp = FakeDP(per_rank, rank)
            got = s.gather(per_rank[rank], dp, dp.shard_sizes(len(rows[s.keys[0]])))
            assert dp.calls == len(s.keys) and list(got) == list(s.keys)
            s.collect(got)
        a = s.arrays()
        assert list(a) == list(s.keys) and s.arrays() is a
        for k, (tail, dt) in spec(kind).items():
            want = torch.cat([b[k] for b in batches]).numpy()
            assert a[k].dtype == want.dtype and a[k].shape == (5,) + tail and np.array_equal(a[k], want, equal_nan=dt.is_floating_point), k
    # one status report read per collected batch, raising only for the credible regions
    per_batch = {"likelihood": ("likelihood", False), "sharpness": ("credible", True), "radial": ("radial", False)}
    assert quiet_status == ([per_batch[kind]] * 4 if kind in per_batch else [])


def test_columns_and_steps_on_planted_arrays(quiet_status):
    scorers = [make(kind) for kind in KINDS]
    rows = {kind: planted(kind, 4, seed=7) for kind in KINDS}
    for s, kind in zip(scorers, KINDS):
        s.collect(rows[kind])
    df = pd.DataFrame({"metaId": np.arange(4), "sceneId": ["scene0"] * 4, "ade": np.zeros(4), "fde": np.zeros(4)})
    for s in scorers:
        s.columns(df)
    assert list(df.columns) == (["metaId", "sceneId", "ade", "fde", "nll", "nll_goal", "entropy_goal", "hpd_goal"]
                                + [f"goal_mass_{k}" for k in range(K_CLS)] + ["gt_goal_class"] + [f"sample_goal_rate_{k}" for k in range(K_CLS)]
                                + ["area25_goal", "inside25_goal", "area50_goal", "inside50_goal", "area99.9_goal", "inside99.9_goal"]
                                + ["radial_mean_goal", "radial_rms_goal", "hit2_goal", "hit7_goal"]
                                + [f"best_of_{k}_{side}_goal" for k in (1, 5, 20) for side in ("lower", "upper")])
    like, comp, sharp, rad = ({k: v.numpy() for k, v in rows[kind].items()} for kind in KINDS)

    def same(column, want):
        assert df[column].dtype == want.dtype and np.array_equal(df[column].to_numpy(), want, equal_nan=True), column

    assert np.isnan(like["nll"][0, 0]) and np.isnan(df["nll"][0]) and np.isfinite(df["nll"][1:]).all()      # a NaN step keeps its row NaN
    same("nll", like["nll"].mean(axis=1))
    same("nll_goal", like["nll"][:, -1])
    same("entropy_goal", like["entropy"][:, -1])
    same("hpd_goal", like["hpd"][:, -1])
    for k in range(K_CLS):
        same(f"goal_mass_{k}", comp["mass"][:, -1, k])
        same(f"sample_goal_rate_{k}", comp["rate"][:, k])
    same("gt_goal_class", comp["gt_class"])
    level_name = pkg("utils.sharpness").level_name
    for l, q in enumerate(LEVELS):
        same(f"area{level_name(q)}_goal", sharp["area"][:, -1, l])
        same(f"inside{level_name(q)}_goal", sharp["inside"][:, -1, l])
    same("radial_mean_goal", rad["mean"][:, -1])
    same("radial_rms_goal", rad["rms"][:, -1])
    for j, r in enumerate(RADIAL["radii"]):
        same(f"hit{r}_goal", rad["hit"][:, -1, j])
    for j, k in enumerate(RADIAL["k"]):
        same(f"best_of_{k}_lower_goal", rad["best_of_k_lower"][:, -1, j])
        same(f"best_of_{k}_upper_goal", rad["best_of_k_upper"][:, -1, j])

    td = {"groundtruth": 0, "prediction": 0}
    for s in reversed(scorers):
        s.steps(td)
    want = {"radial_mean_steps": rad["mean"], "radial_rms_steps": rad["rms"], "radial_hit_steps": rad["hit"],
            "best_of_k_lower_steps": rad["best_of_k_lower"], "best_of_k_upper_steps": rad["best_of_k_upper"],
            "area_steps": sharp["area"], "threshold_steps": sharp["threshold"], "inside_steps": sharp["inside"],
            "class_mass_steps": comp["mass"], "nll_steps": like["nll"], "entropy_steps": like["entropy"], "hpd_steps": like["hpd"]}
    assert list(td) == ["groundtruth", "prediction"] + list(want)
    for k, v in want.items():
        assert td[k].dtype == v.dtype and np.array_equal(td[k], v, equal_nan=v.dtype.kind == "f"), k


def test_compliance_labels_rates_and_refusals():
    S = pkg("utils.scores")
    s = make("compliance")
    labels, n_cls = s.label_maps["scene0"]
    assert n_cls == K_CLS and labels.dtype == torch.uint8 and labels.tolist() == [[0, 0, 1, 1, 2, 2]] * 4
    s.scene("scene0", torch.zeros(1, 4, 6), "cpu")                  # once per scene: the second sighting changes nothing
    assert s.label_maps["scene0"][0] is labels
    # the goals as drawn [K = 4, n = 2, n_wp = 2, 2] (x, y): the last way-point counts; agent 0 draws classes 0, 0, 2 and one outside
    goals = torch.tensor([[[0.0, 0.0], [2.0, 1.0]], [[1.0, 3.0], [3.0, 0.0]], [[5.0, 2.0], [2.0, 2.0]], [[6.0, 0.0], [4.0, 3.0]]])
    samples = torch.stack([torch.full_like(goals, 99.0), goals], dim=2)
    scores = {}
    s.after_draw(scores, samples, "scene0")
    assert scores["rate"].dtype == torch.float64 and scores["rate"].tolist() == [[0.5, 0.0, 0.25], [0.0, 0.75, 0.25]]
    # more than 8 planes in ANY scene: refused before the sweep starts
    s.start({"scene0": scene_planes()})
    with pytest.raises(ValueError, match="scene other has 9 planes"):
        s.start({"scene0": scene_planes(), "other": torch.zeros(9, 4, 4)})
    # scenes that differ in their number of planes: one table cannot hold them
    for width in (3, 4):
        s.collect({"mass": torch.zeros(2, STEPS, width), "gt_class": torch.zeros(2, dtype=torch.int64),
                   "rate": torch.zeros(2, width, dtype=torch.float64)})
    with pytest.raises(ValueError, match=r"scenes differ in their number of planes \(\[3, 4\]\)"):
        s.columns(pd.DataFrame({"ade": np.zeros(4)}))
    assert isinstance(S.ComplianceScore(False), S.Score) and not S.ComplianceScore(False).on


@pytest.mark.parametrize("kind,name,text", [("likelihood", "likelihood", "return_likelihood=True"), ("radial", "radial", "return_radial")])
def test_warns_once_per_call(kind, name, text, monkeypatch):
    monkeypatch.setattr(pkg("ops"), f"check_{name}_status", lambda raise_error=True: not raise_error)      # every batch reports
    s = make(kind)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        for seed in (1, 2):
            s.collect(planted(kind, 2, seed))
    assert len(seen) == 1 and text in str(seen[0].message) and "ADE / FDE are unaffected" in str(seen[0].message)
    assert seen[0].filename == __file__                             # attributed to the caller of collect(): evaluate()'s own line
    assert len(s.arrays()[s.keys[0]]) == 4                          # both batches were kept
    with pytest.warns(UserWarning, match=text):                     # per call = per scorer object: the next call warns again
        make(kind).collect(planted(kind, 2, 3))


def test_status_reports_raise_where_they_did(monkeypatch):
    ops = pkg("ops")

    def pending(raise_error=True):
        if raise_error:
            raise RuntimeError("pending report")
        return True
    for kind, name in (("likelihood", "likelihood"), ("sharpness", "credible"), ("radial", "radial")):
        with monkeypatch.context() as m:
            m.setattr(ops, f"check_{name}_status", pending)
            with pytest.raises(RuntimeError, match="pending report"):      # left by an earlier call: raised in front of the sweep
                make(kind).start({})
            if kind == "sharpness":                                         # a NaN logit in a goal map raises at its batch
                with pytest.raises(RuntimeError, match="pending report"):
                    make(kind).collect(planted(kind, 2, 1))
    make("compliance").start({})                                            # has no status of its own


def test_flags_and_orders():
    S = pkg("utils.scores")
    assert [S.LikelihoodScore(False).on, S.ComplianceScore(False).on, S.SharpnessScore(False).on, S.RadialScore(False).on] == [False] * 4
    assert S.SharpnessScore(True).levels == (0.5, 0.9) and S.SharpnessScore(None).on is False
    r = S.RadialScore(True)
    assert (r.radii, r.ks) == ((4, 8, 16), (1, 5, 20)) and S.RadialScore({"k": (3,)}).ks == (3,)
    for bad in ((0.9, 0.5), (0.0,), 0.5, "0.5"):
        with pytest.raises((ValueError, TypeError)):
            S.SharpnessScore(bad)
    with pytest.raises(ValueError, match="return_radial"):
        S.RadialScore({"k": (0,)})
    # the per-batch status checks: credible raises first, then radial's warning, then likelihood's
    scorers = [make(kind) for kind in KINDS]
    assert [type(s).__name__ for s in sorted(scorers, key=lambda s: s.collect_rank)] == ["ComplianceScore", "SharpnessScore", "RadialScore",
                                                                                         "LikelihoodScore"]

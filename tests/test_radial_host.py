"""Radial goal-map scores (ynet_map_radial, ops.map_radial, utils/radial.py, evaluate(return_radial=...)) -- everything that needs no
GPU: the case table of tests/_radial_cases.py is self-consistent, the profile arithmetic of utils/radial.py on the restatement's fp64
profiles (with one seeded Monte-Carlo check of the best-of-K bracket), the C entry point's refusals, and the signatures."""
import ctypes
import inspect
import math

import pytest
import torch

import _radial_cases as C
from conftest import pkg


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error(si):
    (H, W), _, recorded = C.SHAPES[si]
    measured = {k: 0.0 for k in C.OUTPUTS}
    for kind in range(len(C.KINDS)):
        x, gt, T, refs = C.case(si, kind)
        for R, ref in refs.items():
            assert all(bool(torch.isfinite(ref[k]).all()) for k in C.OUTPUTS), (H, W, kind, R)
            for k, v in C.e32(x, gt, T, R).items():
                measured[k] = max(measured[k], v)
    print(f"{H}x{W}: E32 measured {measured}, recorded {recorded}")
    # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and the
    # vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two below.
    for k in C.OUTPUTS:
        assert measured[k] <= 1.25 * recorded[k] and recorded[k] <= 2.0 * measured[k] + 1e-12, (k, measured[k], recorded[k])


def test_the_table_holds_what_it_says():
    assert [hw for hw, _, _ in C.SHAPES] == [(1, 1), (1, 3), (5, 4), (17, 23), (90, 12), (96, 160), (256, 256), (512, 512)]
    assert C.default_rings(256, 256) == 364 and C.default_rings(3, 4) == 6 and C.default_rings(1, 1) == 3 and C.default_rings(2048, 2048) == 1024
    assert C.ring_counts(512, 512) == [1, 3, 726, 1024] and C.ring_counts(17, 23) == [1, 3, 30]
    for (H, W), _, _ in C.SHAPES:
        pos = C.positions(H, W)
        hit = set()
        for kind in range(len(C.KINDS)):
            g = torch.round(C.ground_truth(H, W, kind).double())
            for p in range(C.B * C.C):
                want = pos[(p + 3 * kind) % len(pos)][1]
                assert (int(g[p // C.C, p % C.C, 0]), int(g[p // C.C, p % C.C, 1])) == want
                hit.add(want)
        assert hit == {px for _, px in pos}, (H, W)
        assert (-3, H + 2) in hit and {(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (W // 2, H // 2)} <= hit
    assert ((2.5, 2.5), (2, 2)) in C.positions(96, 160) and ((3.5, 3.5), (4, 4)) in C.positions(96, 160)
    # n_rings = 3 leaves a tail, the default none for a ground truth inside the map
    x, gt, T, refs = C.case(3, 0)
    assert bool((refs[3]["tail"] > 0).all())
    assert bool((refs[30]["tail"] == 0).all())                  # (kind 0: the planes take the first six positions, all inside the map)


def test_integer_rings_and_the_restatements_rules():
    d2 = torch.arange(0, 70000, dtype=torch.int64)
    k = C.isqrt_tensor(d2)
    assert bool((k * k <= d2).all()) and bool(((k + 1) * (k + 1) > d2).all())
    big = torch.tensor([2 ** 31 - 1, 46340 ** 2, 46340 ** 2 - 1, 46341 ** 2 - 1], dtype=torch.int64)
    assert C.isqrt_tensor(big).tolist() == [46340, 46340, 46339, 46340]
    # the ring edges: one pixel of weight at a known offset
    x, gt, T = C.ring_edge_planes()
    r = C.radial_ref(x, gt, T, 10)
    for i, (_, d2_, ring) in enumerate(C.RING_EDGES):
        assert float(r["ring"][0, i, ring]) == 1.0 and float(r["ring"][0, i].sum()) == 1.0 and float(r["tail"][0, i]) == 0.0
        assert float(r["mean_sq"][0, i]) == d2_ and abs(float(r["mean"][0, i]) - math.sqrt(d2_)) < 1e-14
    assert [ring for _, _, ring in C.RING_EDGES] == [4, 5, 5, 6, 6, 7, 7]
    # the plane-level rules
    for H, W in C.RULE_SHAPES:
        x, gt, T, raises = C.rule_planes(H, W)
        r = C.radial_ref(x, gt, T, 3)
        name = {n: i for i, n in enumerate(C.RULE_PLANES)}
        for k in C.OUTPUTS:
            for n in ("nan_logit", "all_minus_inf", "gt_nan", "gt_inf", "gt_20000_away"):
                assert bool(torch.isnan(r[k][0, name[n]]).all()), (k, n)
            for n in ("plain", "gt_outside_valid", "gt_at_the_margin"):
                assert bool(torch.isfinite(r[k][0, name[n]]).all()), (k, n)
        assert raises == [n in ("gt_nan", "gt_inf", "gt_20000_away") for n in C.RULE_PLANES]
        assert float(r["tail"][0, name["gt_at_the_margin"]]) == 1.0 and float(r["mean_sq"][0, name["gt_at_the_margin"]]) < 2.0 ** 31
    # exact inputs: the fp32 restatement is the fp64 one
    x, gt, T = C.exact_planes(17, 23)
    assert set(x.unique().tolist()) == {0.0, 40.0}
    a, b = C.radial_ref(x, gt, T, 30), C.radial_ref(x, gt, T, 30, torch.float32)
    for k in ("ring", "tail", "mean_sq"):
        assert torch.equal(a[k].float(), b[k]), k


# ---- 2. utils/radial.py on the restatement's fp64 profiles -----------------------------------------------------------------------------
def test_profile_arithmetic_on_fp64_profiles():
    R_ = pkg("utils.radial")
    ks = (1, 2, 5, 20)
    for si in (3, 4, 5):
        (H, W), _, _ = C.SHAPES[si]
        for kind in range(len(C.KINDS)):
            x, gt, T, refs = C.case(si, kind)
            far = R_.farthest_corner(gt, H, W)
            for R, ref in refs.items():
                F = R_.radial_cdf(ref["ring"])
                assert F.shape == (C.B, C.C, R + 1) and F.dtype == torch.float64 and bool((F[..., 0] == 0).all())
                assert bool((F[..., 1:] >= F[..., :-1]).all())                                   # monotone
                assert float((F[..., -1] + ref["tail"] - 1).abs().max()) <= 1e-12               # F(R) + tail = 1
                radii = [0, 1, min(2, R), R]
                hit = R_.hit_rate(ref["ring"], radii)
                assert torch.equal(hit, F[..., radii])
                lower, upper = R_.expected_best_of_k(ref["ring"], ref["tail"], ks, far)
                assert lower.shape == upper.shape == (C.B, C.C, len(ks))
                mean = ref["mean"]
                assert bool((lower[..., 0] <= mean + 1e-9).all()) and bool((mean <= upper[..., 0] + 1e-9).all()), (H, W, kind, R)
                assert bool((lower <= upper).all())
                assert bool((lower[..., 1:] <= lower[..., :-1] + 1e-12).all()) and bool((upper[..., 1:] <= upper[..., :-1] + 1e-12).all())
                empty = ref["tail"] == 0
                if bool(empty.any()):                                                            # exactly one pixel wide
                    assert float(((upper - lower)[empty] - 1).abs().max()) <= 1e-12
                    l2, u2 = R_.expected_best_of_k(ref["ring"][empty], ref["tail"][empty], ks)      # no tail: `far` is not needed
                    assert torch.equal(l2, lower[empty]) and torch.equal(u2, upper[empty])
                if bool((~empty).any()):
                    with pytest.raises(ValueError, match="far"):
                        R_.expected_best_of_k(ref["ring"], ref["tail"], ks)
    # the farthest corner
    fc = R_.farthest_corner(torch.tensor([[0.0, 0.0], [22.0, 16.0], [11.4, 8.0], [-3.4, 19.0]]), 17, 23)
    assert fc.tolist() == [math.ceil(math.hypot(22, 16)), math.ceil(math.hypot(22, 16)), math.ceil(math.hypot(11, 8)), math.ceil(math.hypot(25, 19))]
    # a NaN plane stays NaN, beside a finite one
    ring = torch.tensor([[0.25, 0.75], [float("nan")] * 2], dtype=torch.float64)
    tail = torch.tensor([0.0, float("nan")], dtype=torch.float64)
    lo, up = R_.expected_best_of_k(ring, tail, (1, 3))
    assert lo[0].tolist() == [0.75, 0.75 ** 3] and up[0].tolist() == [1.75, 1 + 0.75 ** 3] and bool(torch.isnan(lo[1]).all() and torch.isnan(up[1]).all())
    lo1, up1 = R_.expected_best_of_k(ring[:, :1], torch.tensor([0.75, float("nan")], dtype=torch.float64), (2,), far=3)
    assert lo1[0].tolist() == [0.75 ** 2] and up1[0].tolist() == [1 + 2 * 0.75 ** 2] and bool(torch.isnan(lo1[1]).all() and torch.isnan(up1[1]).all())
    for bad in ([0.5], [-1], [3]):
        with pytest.raises(ValueError, match="radius"):
            R_.hit_rate(ring, bad)
    for bad in ([], [0], [1.5]):
        with pytest.raises(ValueError, match="ks"):
            R_.expected_best_of_k(ring, tail, bad)
    with pytest.raises(ValueError, match="belong together"):
        R_.expected_best_of_k(ring, tail[:1], (1,))


def test_best_of_five_bracket_against_a_seeded_draw():
    """E[min of 5 i.i.d. distances] by 20000 torch.multinomial draws with replacement must lie in the bracket, widened by five
    standard errors of that mean (the restatement's profile alone: no code of the package's kernels)."""
    R_ = pkg("utils.radial")
    H, W, K, N = 17, 23, 5, 20000
    x, gt, T, refs = C.case(3, 1)
    g = torch.Generator().manual_seed(C.LC.SEED)
    for b, c in ((0, 0), (1, 1), (1, 2)):
        p = torch.sigmoid(x[b, c].double() / T).reshape(-1)
        p = p / p.sum()
        d2, _ = C.squared_distances(gt, H, W)
        dist = torch.sqrt(d2[b, c].double()).reshape(-1)
        draws = torch.multinomial(p.expand(N, -1), K, replacement=True, generator=g)
        best = dist[draws].min(dim=1)[0]
        m, se = float(best.mean()), float(best.std()) / math.sqrt(N)
        for R in (3, 30):
            ref = refs[R]
            lower, upper = R_.expected_best_of_k(ref["ring"][b, c], ref["tail"][b, c], (K,), R_.farthest_corner(gt[b, c], H, W))
            print(f"plane ({b}, {c}) n_rings {R}: sampled {m:.4f} +- {se:.4f}, bracket {float(lower):.4f} .. {float(upper):.4f}")
            assert float(lower) - 5 * se <= m <= float(upper) + 5 * se, (b, c, R)
        one = dist[draws[:, 0]]
        assert abs(float(one.mean()) - float(refs[30]["mean"][b, c])) <= 5 * float(one.std()) / math.sqrt(N)


def test_radial_options():
    R_ = pkg("utils.radial")
    assert R_.radial_options(False) is None and R_.radial_options(None) is None
    assert R_.radial_options(True) == {"radii": (4, 8, 16), "k": (1, 5, 20)}
    assert R_.radial_options({"radii": [2, 0], "k": (3,)}) == {"radii": (2, 0), "k": (3,)}
    assert R_.radial_options({"k": [7]}) == {"radii": (4, 8, 16), "k": (7,)} and R_.radial_options({}) == R_.radial_options(True)
    for bad in ((4, 8), "yes", 1, {"radius": (4,)}, {"radii": ()}, {"radii": (2.5,)}, {"radii": (-1,)}, {"radii": (1025,)}, {"radii": 4},
                {"k": (0,)}, {"k": (1.5,)}, {"k": []}, {"k": (True,)}):
        with pytest.raises(ValueError, match="return_radial"):
            R_.radial_options(bad)
    with pytest.raises(ValueError, match=r"test\(return_radial"):
        R_.radial_options({"k": (0,)}, "test(return_radial=...)")


# ---- 3. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_radial_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_radial" in L.header_symbols() and len(L.SIGNATURES["ynet_map_radial"][1]) == 15
    with open(L.HEADER_PATH) as f:
        assert "#define YNET_MAP_RADIAL_MAX_RINGS 1024" in f.read()
    p = ctypes.c_void_p(4096)      # (never dereferenced: every call below is refused before anything is launched)

    def refused(x=p, bs=48, gt=p, B=2, Cn=3, H=4, W=4, T=1.0, R=5, ring=p, tail=p, mean=p, mean_sq=p, status=p):
        assert lib.ynet_map_radial(x, bs, gt, B, Cn, H, W, T, R, ring, tail, mean, mean_sq, status, None) != 0
        return lib.ynet_last_error().decode()

    assert refused(x=None) == "map_radial: null map"
    assert refused(gt=None) == "map_radial: null ground truth (gt_xy)"
    assert refused(ring=None, tail=None, mean=None, mean_sq=None) == "map_radial: no output asked for"
    assert refused(status=None) == "map_radial: null status flag"
    assert refused(R=0) == "map_radial: n_rings = 0, expected 1 .. 1024" and refused(R=1025) == "map_radial: n_rings = 1025, expected 1 .. 1024"
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert refused(T=T) == "map_radial: the temperature and its reciprocal must be positive and finite", T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert "map_radial: bad shape" in refused(**kw), kw
    assert refused(H=16385, W=1, bs=3 * 16385) == "map_radial: a plane of 16385x1 has a side above 16384"
    assert refused(H=1, W=16385, bs=3 * 16385) == "map_radial: a plane of 1x16385 has a side above 16384"
    assert refused(H=2048, W=2049, bs=3 * 2048 * 2049) == "map_radial: a plane of 2048x2049 has more than the 4194304 pixels the integer sums hold"
    assert refused(bs=47) == "map_radial: batch stride 47 below the 3 planes of 4x4 of an image"
    assert refused(B=1 << 31, Cn=1, bs=16) == "map_radial: too many planes"
    assert refused(T=0.0, H=0, bs=47) == "map_radial: the temperature and its reciprocal must be positive and finite"


def test_wrapper_refuses_host_tensors_and_bad_requests():
    ops = pkg("ops")
    x, gt = torch.zeros(2, 3, 4, 4), torch.zeros(2, 3, 2)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_radial(x, gt)
    with pytest.raises(TypeError):
        ops.map_radial(x.numpy(), gt)
    for want in ((), ("ring", "ring"), ("variance",)):
        with pytest.raises(ValueError, match="want"):
            ops.map_radial(x, gt, want=want)
    assert ops.check_radial_status() is False                   # nothing launched, nothing to report
    assert ops.RADIAL_OUTPUTS == C.OUTPUTS and ops.RADIAL_MAX_RINGS == C.MAX_RINGS
    for H, W in [(1, 1), (3, 4), (17, 23), (256, 256), (512, 512), (2048, 2048)]:
        assert ops.radial_rings(H, W) == C.default_rings(H, W) == min(1024, math.ceil(math.hypot(H, W)) + 1)
    assert list(inspect.signature(ops.map_radial).parameters) == ["x", "gt_xy", "n_rings", "temperature", "want"]


def test_drivers_take_the_flag_and_default_to_off():
    ev, trn = pkg("utils.evaluate"), pkg("models.trainer")
    assert inspect.signature(ev.evaluate).parameters["return_radial"].default is False
    assert inspect.signature(trn.YNetTrainer.test).parameters["return_radial"].default is False
    with pytest.raises(ValueError, match="return_radial"):      # a bad flag raises before anything runs
        ev.evaluate(None, [], {}, "cpu", "sdd", None, None, [0], "test", 1, 1, 1, 1, return_radial={"k": (0,)})
    # the report of YNetTrainer.test on planted columns
    import pandas as pd
    df = pd.DataFrame({"radial_mean_goal": [30.0, 32.0, float("nan")], "hit4_goal": [0.1, 0.3, float("nan")], "best_of_5_lower_goal": [4.0, 6.0, float("nan")],
                       "best_of_5_upper_goal": [8.0, 10.0, float("nan")]})
    text = trn.radial_report_of(df, {"radii": (4,), "k": (5,)}, fde=6.5)
    assert "n = 2" in text and "one draw: 31.0000" in text and "best-of-5 goal error: 5.0000 .. 9.0000" in text and "6.5000" in text
    assert "r = 4: 0.2000" in text

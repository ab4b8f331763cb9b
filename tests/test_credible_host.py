"""Credible regions, without a GPU: the case table and fp64 restatement of tests/_credible_cases.py against closed forms and their own
identities, the recorded E32, a numpy model of the kernel's fixed-point arithmetic, every refusal of ynet_map_credible through ctypes, the
refusals and signatures of the wrappers, and utils/sharpness.py on planted inputs."""
import ctypes
import inspect
import math

import numpy as np
import pytest
import torch

import _credible_cases as C
from conftest import pkg

SMALL = [si for si, ((H, W), _) in enumerate(C.SHAPES) if H * W <= 64 * 64]


# ---- 1. the restatement -----------------------------------------------------------------------------------------------------------------
def test_planted_planes_against_closed_forms():
    names = set()
    for name, x, levels, T, areas in C.planted():
        ref = C.restate(x, levels, T)
        names.add(name)
        assert ref["area"].shape == (1, x.shape[1], len(levels)), name
        if areas is not None:
            assert np.array_equal(ref["area"][0].numpy(), areas), (name, ref["area"][0].tolist())
        assert bool(C.is_logit_of(x, ref["threshold"]).all()) and torch.equal(ref["area"], C.count_ge(x, ref["threshold"])), name
        assert not bool(torch.isinf(ref["threshold"]).any()) or name == "+-inf pixels", name      # -inf is never a member
    assert len(names) == 13
    # the two-valued planes in closed form: k upper pixels of sigmoid 1/2 over sigmoid 1/4 hold 2k / (n + k)
    x = [p for p in C.planted() if p[0] == "two values around q"][0][1]
    ref = C.restate(x, (0.5,), 1.0)
    n = x.shape[2] * x.shape[3]
    assert math.isclose(float(ref["mass"][0, 0, 0]), 1.0) and math.isclose(float(ref["mass"][0, 1, 0]), 2 * 109 / (n + 109), rel_tol=1e-6)
    # a constant plane: the whole map at every level, mass 1; one pixel: itself
    ref = C.restate(torch.full((1, 1, 3, 5), 2.0), C.LEVELS8, 1.8)
    assert ref["area"].unique().tolist() == [15] and ref["mass"].unique().tolist() == [1.0] and ref["threshold"].unique().tolist() == [2.0]
    # the edge rules
    ref = C.restate(C.nan_among_clean(), (0.5, 0.9), 1.3)
    assert ref["area"][1, 0].tolist() == [-1, -1] and bool(torch.isnan(ref["threshold"][1, 0]).all()) and bool(torch.isnan(ref["mass"][1, 0]).all())
    assert ref["area"][0, 2].tolist() == [0, 0] and bool(torch.isnan(ref["mass"][0, 2]).all())
    assert bool((ref["area"][0, :2] > 0).all())
    # the saturated plane: counts decide
    x, _ = C.saturated()
    lv = (0.1, 0.3, 0.7, 0.999999)
    assert C.restate(x, lv, 1.0)["area"][0, 0].tolist() == [math.ceil(float(q) * x[0, 0].numel()) for q in C.levels32(lv)]


@pytest.mark.parametrize("si", SMALL, ids=[f"{C.SHAPES[si][0][0]}x{C.SHAPES[si][0][1]}" for si in SMALL])
def test_restatement_identities(si):
    (H, W), _ = C.SHAPES[si]
    gen = torch.Generator().manual_seed(si)
    for kind in range(len(C.KINDS)):
        for ti in range(len(C.TEMPS)):
            x, T, ref, ge, gt = C.case(si, kind, ti)
            q = torch.from_numpy(C.levels32(C.LEVELS8))
            assert bool((ref["area"][..., 1:] >= ref["area"][..., :-1]).all()) and bool((ref["mass"][..., 1:] >= ref["mass"][..., :-1]).all())
            assert torch.equal(ref["area"], C.count_ge(x, ref["threshold"])) and bool(C.is_logit_of(x, ref["threshold"]).all())
            assert bool((ref["area"] >= 1).all()) and bool((ref["area"] <= H * W).all())
            tiny = 1e-12
            assert bool(((ref["mass"] - ge).abs() <= tiny).all()) and bool((ge >= q - tiny).all()) and bool((gt < q + tiny).all())
            # the hpd identities: x_g >= tau => hpd_g <= mass, x_g < tau => hpd_g > mass
            g = torch.randint(0, H * W, (C.B, C.C, 1), generator=gen)
            xg = torch.gather(x.view(C.B, C.C, -1), 2, g)
            hpd = C.share(x, xg, T)      # [B, C, 1]
            inside = xg >= ref["threshold"]
            assert bool(torch.where(inside, hpd <= ref["mass"] + tiny, hpd > ref["mass"] - tiny).all()), (H, W, kind, ti)


@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _ in C.SHAPES])
def test_recorded_e32_is_what_the_cpu_measures(si):
    (H, W), _ = C.SHAPES[si]
    measured = max(C.case_e32(si, kind, ti) for kind in range(len(C.KINDS)) for ti in range(len(C.TEMPS)))
    rec = C.shape_e32(H, W)
    print(f"{H}x{W}: E32 measured {measured:.3e}, recorded {rec:.3e}")
    # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and the
    # vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two below.
    assert measured <= 1.25 * rec and rec <= 2.0 * measured + 1e-12, (measured, rec)
    assert C.truncation(512 * 512) == 2.0 ** -21 and C.MAX_PIXELS * 2 ** (C.FRAC_BITS + 1) == 2 ** 63


def model_plane(x, levels, T):
    """The kernel's arithmetic in numpy: fp32 sigmoid, the power-of-two scaling by the largest w, truncation at 40 bits, integer sums,
    the comparison with q * Z in fp64 -> (area [L], threshold [L])"""
    x = x.reshape(-1).numpy() + np.float32(0.0)
    w = torch.sigmoid(torch.from_numpy(x) / np.float32(T)).numpy()
    e = math.floor(math.log2(float(w.max())))
    m = np.floor(np.ldexp(w.astype(np.float64), C.FRAC_BITS - e)).astype(np.int64)
    assert 2 ** 40 <= int(m.max()) < 2 ** 41
    vals, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)
    mass = np.zeros(vals.size, dtype=np.int64)
    np.add.at(mass, inv.reshape(-1), m)
    cum, count = np.cumsum(mass[::-1]), np.cumsum(cnt[::-1])
    Z = float(cum[-1])
    pick = [int(np.nonzero(cum.astype(np.float64) >= q * Z)[0][0]) for q in C.levels32(levels)]
    return count[pick], vals[::-1][pick]


def test_fixed_point_model_agrees_with_fp64():
    """the specified arithmetic, modelled on the CPU, picks the restatement's regions (or ones that still meet the acceptance)"""
    off = total = 0
    for si in SMALL[2:]:
        (H, W), _ = C.SHAPES[si]
        for kind in range(len(C.KINDS)):
            for ti in range(len(C.TEMPS)):
                x, T, ref, _, _ = C.case(si, kind, ti)
                got = {"area": torch.empty_like(ref["area"]), "threshold": torch.empty_like(ref["threshold"])}
                for b in range(C.B):
                    for c in range(C.C):
                        a, t = model_plane(x[b, c], C.LEVELS8, T)
                        got["area"][b, c], got["threshold"][b, c] = torch.from_numpy(a.copy()), torch.from_numpy(t.copy())
                got["mass"] = C.share(x, got["threshold"], T).float()
                C.accept(x, T, C.LEVELS8, got, C.shape_e32(H, W))
                same = ((got["area"] == ref["area"]) & (got["threshold"] == ref["threshold"])).all(dim=0).all(dim=0)
                assert bool(same.all()) or kind != C.GRID
                off += int((~same).sum())
                total += same.numel()
    print(f"{off} of {total} (shape, kind, T, level) cases of the model differ from fp64")
    assert off <= 0.05 * total


# ---- 2. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_credible_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_credible" in L.header_symbols() and len(L.SIGNATURES["ynet_map_credible"][1]) == 14
    with open(L.HEADER_PATH) as f:
        text = f.read()
    assert "#define YNET_MAP_CREDIBLE_MAX_LEVELS 8" in text and "#define YNET_MAP_CREDIBLE_FRAC_BITS 40" in text
    cap = int(text.split("#define YNET_MAP_CREDIBLE_MAX_PIXELS")[1].split()[0])
    assert cap == C.MAX_PIXELS >= 262144
    p = ctypes.c_void_p(4096)

    def call(x=p, bs=48, B=2, Cn=3, H=4, W=4, levels=(0.5, 0.9), n=None, T=1.0, area=p, thr=p, mass=p, status=p):
        q = None if levels is None else (ctypes.c_float * max(len(levels), 1))(*levels)
        return lib.ynet_map_credible(x, bs, B, Cn, H, W, q, len(levels) if n is None else n, T, area, thr, mass, status, None)

    for kw, word in (({"x": None}, b"null map"), ({"levels": None, "n": 2}, b"null levels"), ({"area": None}, b"null output"),
                     ({"thr": None}, b"null output"), ({"mass": None}, b"null output"), ({"status": None}, b"null status")):
        assert call(**kw) != 0 and word in lib.ynet_last_error(), kw
    for n in (0, -1, 9, 256):
        assert call(n=n) != 0 and b"n_levels" in lib.ynet_last_error(), n
    for lv in ((0.0,), (1.0,), (-0.1, 0.5), (0.5, 1.5), (float("nan"),), (0.5, float("nan")), (float("inf"),)):
        assert call(levels=lv) != 0 and b"open interval" in lib.ynet_last_error(), lv
    for lv in ((0.9, 0.5), (0.5, 0.5), (0.1, 0.5, 0.4), (0.5, 0.5 + 1e-9)):      # (the last pair is one fp32 number)
        assert call(levels=lv) != 0 and b"ascend" in lib.ynet_last_error(), lv
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert call(T=T) != 0 and b"temperature" in lib.ynet_last_error(), T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}, {"Cn": -1, "B": -1}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=1 << 23, B=1, Cn=1, H=2048, W=2049) != 0 and b"pixels" in lib.ynet_last_error()
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    assert call(bs=4, B=1 << 20, Cn=4, H=1, W=1) != 0 and b"too many planes" in lib.ynet_last_error()
    assert call(bs=4, B=1 << 40, Cn=4, H=1, W=1) != 0 and b"too many planes" in lib.ynet_last_error()


def test_wrapper_refusals_and_signatures():
    ops = pkg("ops")
    x = torch.zeros(2, 3, 4, 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_credible(x, (0.5, 0.9))
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ops.map_credible(x[:, -1:], (0.5,), temperature=1.8)
    with pytest.raises(TypeError):
        ops.map_credible(x.numpy(), (0.5,))
    for bad, msg in (((), "levels"), (tuple(0.1 * i for i in range(1, 10)), "levels"), ((0.0, 0.5), "open interval"), ((0.5, 1.0), "open interval"),
                     ((0.9, 0.5), "ascend"), ((0.5, 0.5), "ascend"), ((float("nan"),), "open interval")):
        with pytest.raises(ValueError, match=msg):
            ops.map_credible(x, bad)
    assert ops.credible_levels([0.5, 0.9]).dtype == np.float32 and ops.credible_levels(torch.tensor([0.25])).tolist() == [0.25]
    assert list(inspect.signature(ops.map_credible).parameters) == ["x", "levels", "temperature"]
    assert inspect.signature(ops.map_credible).parameters["temperature"].default == 1.0
    assert ops.MAP_MAX_LEVELS == 8 == C.MAX_LEVELS and ops.MAP_CREDIBLE_MAX_PIXELS == C.MAX_PIXELS
    assert ops.check_credible_status() is False and ops.check_credible_status(raise_error=False) is False      # nothing launched
    ev, P, trn = pkg("utils.evaluate"), pkg("utils.predict"), pkg("models.trainer")
    names = list(inspect.signature(ev.evaluate).parameters)
    assert names[-2:] == ["return_sharpness", "return_likelihood"] and inspect.signature(ev.evaluate).parameters["return_sharpness"].default is False
    tp = inspect.signature(trn.YNetTrainer.test).parameters
    assert list(tp)[-1] == "return_sharpness" and tp["return_sharpness"].default is False
    for bad in ((0.9, 0.5), (0.0,), 0.5, "0.5", ((0.5, 0.9),)):      # refused before the model is touched
        with pytest.raises((ValueError, TypeError)):
            ev.evaluate(None, [], {}, "cpu", "sdd", None, None, [0], "test", 1, 1, 1, 1, return_sharpness=bad)
    # the forecast form takes predict()'s arguments, defaults included, through predict()'s own body
    assert P._PREDICT_SIGNATURE == inspect.signature(P.predict)
    assert list(inspect.signature(P._forecast).parameters)[-1] == "regions" and inspect.signature(P._forecast).parameters["regions"].default is None
    assert inspect.signature(P.predict_with_regions).parameters["levels"].default == (0.5, 0.9)
    assert inspect.signature(P.predict_with_regions).parameters["levels"].kind is inspect.Parameter.KEYWORD_ONLY
    for k in ("region_area", "region_threshold", "region_mass"):
        assert k in P.predict_with_regions.__doc__
    with pytest.raises(TypeError):
        P.predict_with_regions(None, regions=(0.5,))
    with pytest.raises(ValueError, match="ascend"):
        P.predict_with_regions(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0, levels=(0.9, 0.5))
    with pytest.raises(ValueError, match="observed must be"):      # the same validation, through the same body
        P.predict_with_regions(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0)
    assert "regions" in P.predict_styles.__doc__ and "predict_with_regions" in P.predict.__doc__


# ---- 3. utils/sharpness.py --------------------------------------------------------------------------------------------------------------
def test_levels_names_mask_and_inside():
    S = pkg("utils.sharpness")
    assert S.sharpness_levels(False) is None and S.sharpness_levels(None) is None and S.sharpness_levels(True) == (0.5, 0.9)
    assert S.sharpness_levels([0.1, 0.999]) == (0.1, 0.999)
    assert [S.level_name(q) for q in (0.5, 0.9, 0.99, 0.999, 0.999999, 0.25)] == ["50", "90", "99", "99.9", "99.9999", "25"]
    nan = float("nan")
    g = torch.arange(12.0).view(1, 1, 3, 4)
    m = S.region_mask(g, torch.tensor([[5.0]]))
    assert m.dtype == torch.bool and m.shape == g.shape and int(m.sum()) == 7 and not bool(m[0, 0, 1, 0]) and bool(m[0, 0, 1, 1])
    assert int(S.region_mask(g, torch.tensor([[nan]])).sum()) == 0                        # no region: an empty mask
    assert S.region_mask(g[:, :, None], torch.tensor([[[5.0, 0.0, nan]]])).sum(dim=(-1, -2)).tolist() == [[[7, 12, 0]]]
    thr = torch.tensor([[[5.0, 9.5, nan]]])
    # (x, y) = (column, row), rounded half-even: (1.4, 1.5) -> pixel (row 2, column 1) = 9; (0.5, 0.5) -> (0, 0) = 0
    cases = [((1.4, 1.5), [1.0, 0.0, nan]), ((0.5, 0.5), [0.0, 0.0, nan]), ((3.49, 2.49), [1.0, 1.0, nan]), ((4.0, 1.0), [nan] * 3),
             ((3.51, 0.0), [nan] * 3), ((0.0, -0.51), [nan] * 3), ((nan, 1.0), [nan] * 3), ((-0.5, 2.5), [1.0, 0.0, nan])]
    for xy, want in cases:
        got = S.inside_regions(g, torch.tensor([[xy]]), thr)
        assert got.dtype == torch.float32 and got.shape == (1, 1, 3)
        assert np.array_equal(got[0, 0].numpy(), np.array(want, dtype=np.float32), equal_nan=True), (xy, got)
    # against the restatement: inside <=> the pixel is counted in the area
    x, T, ref, _, _ = C.case(3, 0, 0)
    H, W = x.shape[2:]
    for gy, gx in ((0, 0), (H - 1, W - 1), (5, 7)):
        gt = torch.tensor([float(gx), float(gy)]).expand(C.B, C.C, 2)
        assert torch.equal(S.inside_regions(x, gt, ref["threshold"]) == 1.0, x[:, :, gy, gx, None] >= ref["threshold"])


def test_sharpness_table_on_planted_inputs():
    S = pkg("utils.sharpness")
    nan = float("nan")
    inside = [[1, 1], [0, 1], [nan, nan], [1, 0]]
    area = [[10, 40], [20, 60], [-1, -1], [30, 110]]
    t = S.sharpness_table((0.5, 0.9), inside, area, 200, 0.25)
    assert [r["level"] for r in t] == [0.5, 0.9] and [r["n"] for r in t] == [3, 3]
    assert math.isclose(t[0]["coverage"], 2 / 3) and math.isclose(t[1]["coverage"], 2 / 3)
    assert (t[0]["area_mean"], t[0]["area_median"]) == (20.0, 20.0) and (t[1]["area_mean"], t[1]["area_median"]) == (70.0, 60.0)
    assert math.isclose(t[1]["share_mean"], 0.35) and math.isclose(t[1]["share_median"], 0.3)
    assert t[1]["area_orig_mean"] == 70.0 * 16 and t[1]["area_orig_median"] == 60.0 * 16
    per_row = S.sharpness_table((0.5, 0.9), inside, area, [100, 200, 100, 300], 0.25)      # scenes of different size
    assert math.isclose(per_row[0]["share_mean"], (0.1 + 0.1 + 0.1) / 3) and per_row[0]["area_mean"] == 20.0
    none = S.sharpness_table((0.5,), [[nan]], [[-1]], 100, 1.0)[0]
    assert none["n"] == 0 and all(math.isnan(none[k]) for k in ("coverage", "area_mean", "share_median", "area_orig_mean"))
    with pytest.raises(ValueError):
        S.sharpness_table((0.5, 0.9), [[1, 1]], [[1, 1], [2, 2]], 100, 0.25)
    with pytest.raises(ValueError):
        S.sharpness_table((0.5,), [[1]], [[1]], 0, 0.25)
    text = S.sharpness_report((0.5, 0.9), inside, area, 200, 0.25)
    assert text.count("\n") == 2 and "50 %" in text and "90 %" in text

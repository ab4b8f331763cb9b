"""Scene compliance (ynet_map_class_mass, ops.map_class_mass, utils/compliance.py, evaluate(return_compliance=True)) -- everything that
needs no GPU: the case table of tests/_compliance_cases.py is self-consistent, the helpers of utils/compliance.py, the C entry point's
refusals, and the signatures."""
import ctypes
import inspect
import math

import pytest
import torch

import _compliance_cases as C
from conftest import pkg


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error(si):
    (H, W), _, recorded = C.SHAPES[si]
    measured = 0.0
    for kind, pat in C.cases(si):
        assert bool(torch.isfinite(C.case(si, kind, pat)[4]).all()), (H, W, kind, pat)
        measured = max(measured, C.case_e32(si, kind, pat))
    print(f"{H}x{W}: E32 measured {measured:.3e}, recorded {recorded:.3e}")
    # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and the
    # vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two below.
    assert measured <= 1.25 * recorded and recorded <= 2.0 * measured + 1e-12, (measured, recorded)


def test_the_table_holds_the_shapes_kinds_and_patterns_it_says():
    import _likelihood_cases as L
    assert [hw for hw, _, _ in C.SHAPES] == [(1, 1), (1, 3), (5, 4), (17, 23), (90, 12), (96, 160), (256, 256), (512, 512)]
    assert C.KINDS is L.KINDS and len(C.PATTERNS) == 8
    for (H, W), _, _ in C.SHAPES:
        for pat, (_, K) in enumerate(C.PATTERNS):
            lab, k = C.labels(H, W, pat)
            assert k == K and lab.dtype == torch.uint8 and lab.shape == (H, W)
        assert C.applies(H, W, 2) == ((H, W) in [(96, 160), (256, 256), (512, 512)])
    H, W = 96, 160
    assert all(sorted(C.labels(H, W, 1)[0][r, c:c + 4].tolist()) == sorted({(c + j) % 6 for j in range(4)}) for r in (0, 95) for c in (0, 4, 156))
    blocks = C.labels(H, W, 2)[0]
    assert bool((blocks[:32, :32] == blocks[0, 0]).all()) and blocks[0, 0] != blocks[0, 32] and blocks[0, 0] != blocks[32, 0]
    assert bool((C.labels(H, W, 3)[0] == 2).all())
    absent = C.labels(H, W, 4)[0]
    assert not bool((absent == C.ABSENT).any()) and set(absent.unique().tolist()) == {0, 1, 2, 4, 5}
    assert set(C.labels(H, W, 5)[0].unique().tolist()) == {0, 1} and set(C.labels(H, W, 6)[0].unique().tolist()) == set(range(8))
    assert set(C.labels(H, W, 7)[0].unique().tolist()) == {0, 1, 2, 3, 4, 5, 7, 255}
    # what the patterns are there for, in the reference itself
    for si in (2, 5):
        full = C.case(si, 0, 3)[4]
        assert bool((full[..., 2] == 1.0).all()) and bool((full[..., :2] == 0.0).all())
        assert bool((C.case(si, 1, 4)[4][..., C.ABSENT] == 0.0).all())
        assert bool((C.case(si, 0, 0)[4].sum(-1) - 1.0).abs().max() < 1e-12)
        short = C.case(si, 0, 7)[4].sum(-1)
        assert bool((short < 0.999).all()) and bool((short > 0.0).all())


def test_fp64_restatement_reproduces_the_closed_forms():
    for H, W in [(1, 1), (1, 3), (5, 4), (17, 23), (96, 160)]:
        x, lab, K, T, area = C.constant_plane(H, W)
        got = C.mass_ref(x, lab, K, T)
        assert got.shape == (1, 1, K) and float((got[0, 0] - area).abs().max()) <= 1e-12
        cls = pkg("utils.compliance")
        assert torch.equal(cls.class_area(lab, K), area)             # the report's "area" column is that closed form
        if H * W < 2:
            continue
        x, lab, K, T, want = C.spike_planes(H, W)
        got = C.mass_ref(x, lab, K, T)
        assert float((got[0] - want).abs().max()) <= 1e-12, (H, W)


def test_edge_planes_follow_the_rules_in_fp64():
    for H, W in C.EDGE_SHAPES:
        x, lab, K, T = C.edge_planes(H, W)
        r = C.mass_ref(x, lab, K, T)
        name = {n: i for i, n in enumerate(C.EDGE_PLANES)}
        assert bool(torch.isnan(r[0, name["nan"]]).all()) and bool(torch.isnan(r[0, name["all_minus_inf"]]).all())
        for n in ("minus_inf_elsewhere", "minus_inf_pixels", "plus_and_minus_inf"):
            assert bool(torch.isfinite(r[0, name[n]]).all()) and abs(float(r[0, name[n]].sum()) - 1.0) < 1e-12, n
        assert C.shape_e32(H, W) > 0


# ---- 2. utils/compliance.py ------------------------------------------------------------------------------------------------------------
def test_scene_labels():
    cls = pkg("utils.compliance")
    lab = C.labels(17, 23, 0)[0]
    planes = torch.nn.functional.one_hot(lab.long(), 6).permute(2, 0, 1).float()
    got = cls.scene_labels(planes)
    assert got.dtype == torch.uint8 and got.is_contiguous() and torch.equal(got, lab)              # exact on one-hot planes
    assert torch.equal(cls.scene_labels(planes.numpy()), lab)
    soft = torch.tensor([[[0.2, 0.5]], [[0.7, 0.5]], [[0.1, 0.0]]])                                  # the hard decision; a tie goes to the lowest class
    assert cls.scene_labels(soft).tolist() == [[1, 0]]
    assert "hard decision" in " ".join(cls.scene_labels.__doc__.lower().split())
    assert cls.scene_labels(torch.zeros(8, 2, 2)).shape == (2, 2)
    with pytest.raises(ValueError, match="9 planes"):
        cls.scene_labels(torch.zeros(9, 2, 2))
    for bad in (torch.zeros(4, 4), torch.zeros(1, 6, 4, 4)):
        with pytest.raises(ValueError, match="K, H, W"):
            cls.scene_labels(bad)


def test_point_classes_rounds_half_even_and_marks_the_outside():
    cls = pkg("utils.compliance")
    H, W = 6, 7
    lab = (torch.arange(H).view(H, 1) * 10 + torch.arange(W).view(1, W)).to(torch.uint8)           # label = 10 * row + column
    nan = float("nan")
    xy = torch.tensor([[2.5, 2.5], [3.5, 3.5], [0.0, 0.0], [6.0, 5.0], [6.49, 5.49], [-0.5, 0.5], [-0.4, 1.0],
                       [6.51, 0.0], [0.0, 5.51], [-0.51, 0.0], [nan, 1.0], [1.0, nan], [7.0, 0.0], [0.0, -1.0]])
    want = [22, 44, 0, 56, 56, 0, 10, -1, -1, -1, -1, -1, -1, -1]
    got = cls.point_classes(xy, lab)
    assert got.dtype == torch.int64 and got.tolist() == want
    assert cls.point_classes(xy.double().view(2, 7, 2), lab).tolist() == [want[:7], want[7:]]       # any leading shape, any float dtype
    assert cls.point_classes(xy.numpy(), lab).tolist() == want
    with pytest.raises(ValueError, match=r"\[\.\.\., 2\]"):
        cls.point_classes(torch.zeros(4, 3), lab)
    with pytest.raises(ValueError, match="label map"):
        cls.point_classes(xy, lab[None])


def test_class_rates_and_class_area():
    cls = pkg("utils.compliance")
    c = torch.tensor([[0, 1, 1, -1], [2, 2, 2, 2], [-1, -1, -1, -1]])
    r = cls.class_rates(c, 3)
    assert r.dtype == torch.float64 and r.tolist() == [[0.25, 0.5, 0.0], [0.0, 0.0, 1.0], [0.0, 0.0, 0.0]]      # -1 is in no class
    assert cls.class_rates(c.t(), 3, dim=0).tolist() == r.t().tolist()
    assert cls.class_rates(c, 2).tolist() == [[0.25, 0.5], [0.0, 0.0], [0.0, 0.0]]                 # a class beyond K counts in none
    assert cls.class_rates(c.view(3, 2, 2), 3, dim=1).shape == (3, 3, 2)
    for bad, kw, msg in ((c.float(), {}, "integer"), (c, {"n_classes": 0}, "n_classes"), (c[:, :0], {}, "no points")):
        with pytest.raises(ValueError, match=msg):
            cls.class_rates(bad, **({"n_classes": 3} | kw))
    lab = torch.tensor([[0, 0, 1], [5, 2, 255]], dtype=torch.uint8)
    assert cls.class_area(lab, 3).tolist() == [2 / 6, 1 / 6, 1 / 6]                                   # labels >= K: the denominator only
    assert cls.class_area(lab, 8).tolist() == [2 / 6, 1 / 6, 1 / 6, 0, 0, 1 / 6, 0, 0]
    with pytest.raises(ValueError, match="label map"):
        cls.class_area(lab[None], 3)


# ---- 3. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_class_mass_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_class_mass" in L.header_symbols() and len(L.SIGNATURES["ynet_map_class_mass"][1]) == 12
    with open(L.HEADER_PATH) as f:
        assert "#define YNET_MAP_MAX_CLASSES 8" in f.read()
    vp = ctypes.c_void_p
    p = vp(4096)

    def call(x=p, bs=48, lab=p, lbs=0, B=2, Cn=3, H=4, W=4, K=6, T=1.0, mass=p):
        return lib.ynet_map_class_mass(x, bs, lab, lbs, B, Cn, H, W, K, T, mass, None)

    for kw, word in (({"x": None}, b"null map"), ({"lab": None}, b"null labels"), ({"mass": None}, b"null output")):
        assert call(**kw) != 0 and word in lib.ynet_last_error(), kw
    for K in (0, -1, 9, 256):
        assert call(K=K) != 0 and b"n_classes" in lib.ynet_last_error(), K
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert call(T=T) != 0 and b"temperature" in lib.ynet_last_error(), T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=1 << 31, B=1, Cn=1, H=32768, W=65536) != 0 and b"32-bit" in lib.ynet_last_error()
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    for lbs in (15, 1, -16):
        assert call(lbs=lbs) != 0 and b"label batch stride" in lib.ynet_last_error(), lbs
    assert call(bs=4, B=1 << 29, Cn=4, H=1, W=1) != 0 and b"too many planes" in lib.ynet_last_error()


def test_wrapper_refuses_host_tensors_and_signatures():
    ops = pkg("ops")
    x, lab = torch.zeros(2, 3, 4, 4), torch.zeros(4, 4, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_class_mass(x, lab, 6)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_class_mass(x[:, -1:], lab, 6, temperature=1.8)
    with pytest.raises(TypeError):
        ops.map_class_mass(x.numpy(), lab, 6)
    assert list(inspect.signature(ops.map_class_mass).parameters) == ["x", "labels", "n_classes", "temperature"]
    assert inspect.signature(ops.map_class_mass).parameters["temperature"].default == 1.0 and ops.MAP_MAX_CLASSES == 8
    ev, P, trn = pkg("utils.evaluate"), pkg("utils.predict"), pkg("models.trainer")
    assert inspect.signature(ev.evaluate).parameters["return_compliance"].default is False
    assert inspect.signature(trn.YNetTrainer.test).parameters["return_compliance"].default is False
    # the forecast form takes predict()'s arguments, defaults included, through predict()'s own body; the other forms say they have none
    assert "goal_class_mass" in P.predict_with_compliance.__doc__ and "goal_class_mass" in P.predict.__doc__
    with pytest.raises(TypeError):
        P.predict_with_compliance(None, return_compliance=True)
    with pytest.raises(ValueError, match="observed must be"):
        P.predict_with_compliance(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0)
    assert "compliance" in P.predict_styles.__doc__ and "compliance" in P.predict_modes.__doc__
    assert math.isclose(sum(pkg("utils.compliance").class_area(C.labels(5, 4, 0)[0], 6).tolist()), 1.0)

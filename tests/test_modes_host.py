"""Deterministic goal modes (ynet_map_modes, ops.map_modes, utils.predict.predict_modes, YNetTrainer.predict_modes) -- everything that
needs no GPU: the case table of tests/_modes_cases.py against its closed forms and its own invariants, the recorded E32, the C entry
point's refusals (made before the device is touched), the signatures, and every refusal of predict_modes."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import _modes_cases as C
from conftest import pkg

OBS = 8


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
def test_planted_planes_give_their_closed_forms():
    for name, x, M, r, T, want in C.planted():
        ref = C.modes_ref(x, M, r, T)
        C.check_planted(name, ref, want)
        filled = torch.arange(M)[None, None] < ref["count"][:, :, None]
        assert bool((ref["xy"][~filled] == C.FILL_XY).all()) and bool((ref["logit"][~filled] == C.FILL_LOGIT).all()), name
        assert bool((ref["mass"][0][~filled] == 0).all()), name
    # +0.0 beside -0.0: the logit comes back with the sign it was stored with
    name, x, M, r, T, _ = [p for p in C.planted() if p[0] == "+0.0 beside -0.0"][0]
    ref = C.modes_ref(x, M, r, T)
    assert C.bits(ref["logit"])[0, 0].tolist() == [-2 ** 31, 0] and C.bits(ref["logit"])[0, 1].tolist() == [0, -2 ** 31]
    # the constant plane in full: row-major order under suppression, restated with a list of taken pixels
    for r in (0, 3):
        _, x, M, _, T, _ = [p for p in C.planted() if p[0] == f"constant r{r}"][0]
        H, W = x.shape[2:]
        taken, want = [], []
        for lin in range(H * W):
            row, col = divmod(lin, W)
            if all((row - a) ** 2 + (col - b) ** 2 > r * r for a, b in taken):
                taken.append((row, col))
                want.append([float(col), float(row)])
        assert C.modes_ref(x, M, r, T)["xy"][0, 0].tolist() == want[:M]


def test_greedy_prefix_and_the_vectorised_restatement():
    x, T, ref = C.case(3, 1, 3)
    for M in (1, 2, 20):
        direct, cutref = C.modes_ref(x, M, 3, T, (torch.float64, torch.float32)), C.cut(ref, M)
        for k in ("xy", "logit", "count"):
            assert torch.equal(direct[k], cutref[k]), (M, k)
        assert all(torch.equal(a, b) for a, b in zip(direct["mass"], cutref["mass"])), M
    x, M, r, T = C.many_planes()
    fast, slow = C.many_planes_ref(x, M, r, T), C.modes_ref(x[:40], M, r, T)
    for k in ("xy", "logit", "count"):
        assert torch.equal(fast[k][:40], slow[k]), k
    assert float((fast["mass"][0][:40] - slow["mass"][0]).abs().max()) <= 1e-15


def test_masses_are_disjoint_and_cover_and_finite_planes_fill_up():
    for si, kind, r in C.table():
        (H, W), _, _ = C.SHAPES[si]
        x, T, ref = C.case(si, kind, r)
        assert bool(torch.isfinite(x).all())
        for M in C.table_modes(si):
            rf = C.cut(ref, M)
            m64, cnt = rf["mass"][0], rf["count"]
            assert bool((m64 >= 0).all()) and bool((m64.sum(dim=2) <= 1 + 1e-12).all())
            if (M - 1) * C.disk_area(min(r, H + W)) < H * W:             # the first M - 1 disks cannot cover the map
                assert bool((cnt == M).all()), (H, W, kind, r, M)
            covered = cnt < M                                             # finite logits stop early only on a covered map
            assert bool(((m64.sum(dim=2) - 1).abs()[covered] <= 1e-12).all()), (H, W, kind, r, M)
            if r == C.over_radius(H, W):
                assert bool((cnt == 1).all()) and bool(((m64[:, :, 0] - 1).abs() <= 1e-12).all())
            # every mode's pixel is unsuppressed by the earlier ones, and its logit is what the map holds there
            xy, lg = rf["xy"].long(), rf["logit"]
            for b in range(x.shape[0]):
                for c in range(x.shape[1]):
                    n = int(cnt[b, c])
                    pts = xy[b, c, :n]
                    assert torch.equal(x[b, c][pts[:, 1], pts[:, 0]], lg[b, c, :n])
                    d2 = ((pts[:, None] - pts[None]) ** 2).sum(dim=2) + torch.eye(n, dtype=torch.long) * (r * r + 1)
                    assert bool((d2 > r * r).all()), (H, W, kind, r, M, b, c)
                    assert bool((lg[b, c, :n - 1] >= lg[b, c, 1:n]).all())      # suppression only removes: the maxima never rise


@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error(si):
    (H, W), _, recorded = C.SHAPES[si]
    measured = max(C.e32_of(C.case(s, kind, r)[2]) for s, kind, r in C.table() if s == si)
    print(f"{H}x{W}: E32 measured {measured:.3e}, recorded {recorded:.3e}")
    # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and the
    # vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two below.
    assert measured <= 1.25 * recorded and recorded <= 2.0 * measured + 1e-12, (measured, recorded)


def test_disk_area():
    P = pkg("utils.predict")
    assert [P.disk_area(r) for r in (0, 1, 2, 3, 8)] == [1, 5, 13, 29, 197]
    assert all(P.disk_area(r) == C.disk_area(r) for r in range(0, 40))


# ---- 2. the C entry point and its wrappers ----------------------------------------------------------------------------------------------
def test_map_modes_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert "ynet_map_modes" in L.header_symbols() and len(L.SIGNATURES["ynet_map_modes"][1]) == 15
    with open(L.HEADER_PATH) as f:
        assert "#define YNET_MAP_MODES_MAX_PIXELS 262144" in f.read()
    vp = ctypes.c_void_p
    p = vp(4096)

    def call(x=p, bs=48, B=2, Cn=3, H=4, W=4, M=20, r=3, T=1.0, xy=p, logit=p, mass=p, count=p, status=p):
        return lib.ynet_map_modes(x, bs, B, Cn, H, W, M, r, T, xy, logit, mass, count, status, None)

    for kw in ({"x": None}, {"xy": None}, {"logit": None}, {"count": None}, {"status": None}):
        assert call(**kw) != 0 and b"null" in lib.ynet_last_error(), kw
    for M in (0, 65, -1):
        assert call(M=M) != 0 and b"1 .. 64" in lib.ynet_last_error(), M
    assert call(r=-1) != 0 and b"radius" in lib.ynet_last_error()
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"B": -3}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert call(T=T) != 0 and b"temperature" in lib.ynet_last_error(), T
    assert call(bs=1 << 20, B=1, Cn=1, H=512, W=513) != 0 and b"cap" in lib.ynet_last_error()        # one column beyond 512 x 512
    assert call(bs=1 << 20, B=1, Cn=1, H=1, W=262145) != 0 and b"cap" in lib.ynet_last_error()
    assert call(bs=1 << 40, B=1, Cn=1, H=1 << 20, W=1 << 20) != 0 and b"cap" in lib.ynet_last_error()  # H * W beyond an int
    assert call(bs=16, B=1 << 22, Cn=1) != 0 and b"planes" in lib.ynet_last_error()


def test_wrapper_refuses_host_tensors_and_bad_requests():
    ops = pkg("ops")
    assert list(inspect.signature(ops.map_modes).parameters) == ["x", "n_modes", "radius", "temperature", "want_mass"]
    d = {k: v.default for k, v in inspect.signature(ops.map_modes).parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(temperature=1.0, want_mass=True) and ops.MAX_MODES == 64
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_modes(torch.zeros(2, 3, 4, 4), 20, 3)
    with pytest.raises(TypeError):
        ops.map_modes(np.zeros((2, 3, 4, 4), np.float32), 20, 3)
    ops.check_modes_status()                                    # nothing launched, nothing to report


def test_signatures():
    P, trn = pkg("utils.predict"), pkg("models.trainer")
    sig = inspect.signature(P.predict_modes)
    assert list(sig.parameters) == ["model", "scene_image", "observed", "input_template", "waypoints", "n_modes", "radius", "obs_len",
                                    "resize_factor", "temperature", "CWS_params", "network", "swap_semantic", "batch_size",
                                    "max_effective_batch", "return_maps"]
    d = {k: v.default for k, v in sig.parameters.items() if v.default is not inspect.Parameter.empty}
    assert d == dict(CWS_params=None, network=None, swap_semantic=False, batch_size=None, max_effective_batch=256, return_maps=False)
    assert list(inspect.signature(trn.YNetTrainer.predict_modes).parameters) == ["self", "df_obs", "image_path_or_images", "n_modes", "radius",
                                                                                 "return_maps"]
    doc = P.predict_modes.__doc__
    assert "Out of scope" in doc and all(w in doc for w in ("predict_styles", "evaluate()", "sub-pixel", "hipGraph"))
    assert P._PREDICT_SIGNATURE == inspect.signature(P.predict)             # predict()'s pinned parameter list did not move


def test_predict_modes_refuses_before_touching_the_device():
    P = pkg("utils.predict")
    scene = torch.zeros(6, 64, 64)
    obs = np.zeros((3, OBS, 2), np.float32)
    base = dict(model=None, scene_image=scene, input_template=None, waypoints=[11], n_modes=20, radius=3, obs_len=OBS, resize_factor=0.25,
                temperature=1.0)

    def run(observed=obs, **over):
        return P.predict_modes(observed=observed, **{**base, **over})

    for M in (0, 65, -2):
        with pytest.raises(ValueError, match="n_modes"):
            run(n_modes=M)
    with pytest.raises(ValueError, match="radius"):
        run(radius=-1)
    # _validated's refusals, under this function's name
    with pytest.raises(ValueError, match="predict_modes: .*never cut silently"):
        run(np.zeros((3, OBS + 12, 2), np.float32))
    with pytest.raises(ValueError, match="predict_modes: .*obs_len is 8"):
        run(np.zeros((3, OBS - 1, 2), np.float32))
    with pytest.raises(ValueError, match=r"predict_modes: .*\[N, obs_len, 2\]"):
        run(np.zeros((3, OBS), np.float32))
    with pytest.raises(ValueError, match="predict_modes: no agents"):
        run(np.zeros((0, OBS, 2), np.float32))
    with pytest.raises(ValueError, match="predict_modes: no way-points"):
        run(waypoints=[])
    with pytest.raises(ValueError, match="predict_modes: resize_factor"):
        run(resize_factor=0.0)
    with pytest.raises(ValueError, match="predict_modes: batch_size"):
        run(batch_size=0)
    with pytest.raises(ValueError, match="predict_modes: scene_image"):
        run(scene_image=np.zeros((6, 64, 64)))
    # the modes must fit the map: (n_modes - 1) * A(radius) < H * W, checked once H and W are known
    P._check_modes_fit("predict_modes", 20, 8, 64, 64)                       # 19 * 197 = 3743 < 4096
    P._check_modes_fit("predict_modes", 1, 10 ** 6, 64, 64)                  # one mode always fits
    with pytest.raises(ValueError, match="predict_modes: 22 modes of radius 8 .*4137 >= 4096"):
        P._check_modes_fit("predict_modes", 22, 8, 64, 64)
    with pytest.raises(ValueError, match="may not fit"):
        P._check_modes_fit("predict_modes", 2, 10 ** 6, 64, 64)


def test_trainer_predict_modes_refuses_bad_requests():
    from test_predict_host import _df, _trainer
    images = {"scene0": torch.zeros(6, 64, 64)}
    t = _trainer()
    for M, r in ((0, 3), (65, 3), (20, -1)):
        with pytest.raises(ValueError, match="predict_modes"):
            t.predict_modes(_df([OBS, OBS]), images, M, r)
    with pytest.raises(ValueError, match="exactly obs_len = 8 rows"):
        t.predict_modes(_df([OBS, OBS + 12]), images, 20, 3)
    with pytest.raises(NotImplementedError, match="world coordinates"):
        _trainer(dataset_name="eth").predict_modes(_df([OBS, OBS]), images, 20, 3)
    with pytest.raises(ValueError, match="exactly obs_len = 8 rows"):        # (n_goal * n_traj > 64 is predict()'s limit, not this call's)
        _trainer(n_goal=33, n_traj=2).predict_modes(_df([OBS, OBS + 12]), images, 20, 3)

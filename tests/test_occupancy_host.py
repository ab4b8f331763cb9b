"""Scene occupancy (ynet_map_occupancy, ops.map_occupancy, utils/occupancy.py, predict_with_occupancy) -- everything that needs no GPU:
the case table of tests/_occupancy_cases.py is self-consistent, the restatement's identities, the helpers of utils/occupancy.py, the C
entry points' refusals, and the signatures."""
import ctypes
import inspect

import pytest
import torch

import _occupancy_cases as C
from conftest import pkg


# ---- 1. the case table ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_recorded_e32_is_the_fp32_restatements_error(si):
    (H, W), _, recorded = C.SHAPES[si]
    measured = {k: 0.0 for k in C.OUTPUTS}
    for cell, li, kind in C.cases(si):
        ref = C.case(si, cell, li, kind)[3]
        assert all(bool(torch.isfinite(ref[k]).all()) for k in C.OUTPUTS), (H, W, cell, li, kind)
        for k, v in C.case_e32(si, cell, li, kind).items():
            measured[k] = max(measured[k], v)
    for k in C.OUTPUTS:
        print(f"{H}x{W} {k}: E32 measured {measured[k]:.3e}, recorded {recorded[k]:.3e}")
        # recorded = what one CPU measured, rounded up to three digits.  The order of a stock-torch fp32 sum depends on the thread count and
        # the vector width, so another machine may measure a little more: a quarter of headroom above, never padded beyond a factor of two.
        assert measured[k] <= 1.25 * recorded[k] and recorded[k] <= 2.0 * measured[k] + 1e-12, (k, measured[k], recorded[k])


def test_the_table_holds_the_shapes_cells_and_layouts_it_says():
    import _likelihood_cases as L
    assert [hw for hw, _, _ in C.SHAPES] == [(1, 1), (1, 3), (5, 4), (17, 23), (90, 12), (96, 160), (256, 256)]
    assert C.KINDS is L.KINDS and C.CELLS == (1, 2, 4, 8) and C.C == 3
    for want in ([1], [2], [0, 3, 1], [5], [9], [4, 0, 4]):
        assert want in C.LAYOUTS
    sizes = {s for lay in C.LAYOUTS for s in lay}
    assert C.runs(9, 1) == [9] and C.runs(9, 2) == [5, 4] and C.runs(9, 4) == [3, 3, 3, 0] and C.runs(9, 8) == [2, 2, 2, 2, 1, 0, 0, 0]
    for cell, d in C.DEPTH.items():                                 # the walk's edges: a wave with d - 1, d and d + 1 agents at every cell edge
        assert {d - 1, d, d + 1} <= {r for n in sizes for r in C.runs(n, cell)}, (cell, d)
    for si in range(len(C.SHAPES)):
        cs = C.cases(si)
        assert {(cell, li) for cell, li, _ in cs} == {(cell, li) for cell in C.CELLS for li in range(len(C.LAYOUTS))}
    seen = {(cell, kind) for si in range(len(C.SHAPES)) for cell, _, kind in C.cases(si)}
    assert seen == {(cell, kind) for cell in C.CELLS for kind in range(len(C.KINDS))}
    seen = {(li, kind) for si in range(len(C.SHAPES)) for _, li, kind in C.cases(si)}
    assert seen == {(li, kind) for li in range(len(C.LAYOUTS)) for kind in range(len(C.KINDS))}
    x, sizes, T, ref = C.case(3, 4, 2, 1)
    assert x.shape == (4, 3, 17, 23) and x.dtype == torch.float32 and sizes == [0, 3, 1] and T == C.KINDS[1][1]
    assert ref["occupancy"].shape == ref["any"].shape == (3, 3, 5, 6) and ref["conflict"].shape == (3, 3) and ref["risk"].shape == (4, 3)
    assert C.case(1, 8, 0, 0)[3]["occupancy"].shape == (1, 3, 1, 1) and C.case(2, 8, 0, 0)[3]["occupancy"].shape == (1, 3, 1, 1)   # a cell larger than the map


def test_the_restatements_identities():
    for si in (2, 3, 5):
        for cell, li, kind in C.cases(si):
            x, sizes, T, r = C.case(si, cell, li, kind)
            n = torch.tensor(sizes, dtype=torch.float64)
            assert float((r["occupancy"].sum(dim=(2, 3)) - n[:, None]).abs().max()) < 1e-12           # a plane of D sums to the group's size
            first = 0
            for g, s in enumerate(sizes):
                assert float((r["risk"][first:first + s].sum(0) - 2.0 * r["conflict"][g]).abs().max()) < 1e-12
                if s == 0:                                                                               # an empty group: all zeros
                    assert bool((r["occupancy"][g] == 0).all()) and bool((r["any"][g] == 0).all()) and bool((r["conflict"][g] == 0).all())
                if s == 1:                                                                               # one agent: no pair; any = occupancy
                    assert bool((r["conflict"][g] == 0).all()) and bool((r["risk"][first] == 0).all())
                    assert float((r["any"][g] - r["occupancy"][g]).abs().max()) < 1e-15
                first += s
            assert bool((r["any"] <= r["occupancy"] + 1e-15).all()) and bool((r["any"] >= 0).all()) and bool((r["conflict"] >= -1e-15).all())


def test_fp64_restatement_reproduces_the_closed_forms():
    for H, W in [(5, 4), (17, 23), (96, 160)]:
        for cell in C.CELLS:
            for n in (1, 3):
                x, T, want = C.constant_planes(n, H, W, cell)
                got = C.occupancy_ref(x, [n], cell, T)
                for k in C.OUTPUTS:
                    assert got[k].shape == want[k].shape and float((got[k] - want[k]).abs().max()) <= 1e-12, (H, W, cell, n, k)
    x, T = C.disjoint_halves(16, 24)
    for cell in C.CELLS:
        r = C.occupancy_ref(x, [2], cell, T)
        assert bool((r["conflict"] == 0).all()) and bool((r["risk"] == 0).all()) and bool((r["occupancy"] > 0).any())


def test_edge_scene_follows_the_rules_in_fp64():
    for H, W in C.EDGE_SHAPES:
        bad, clean, sizes, T = C.edge_scene(H, W)
        for cell in C.CELLS:
            rb, rc = C.occupancy_ref(bad, sizes, cell, T), C.occupancy_ref(clean, sizes, cell, T)
            assert all(bool(torch.isfinite(rc[k]).all()) for k in C.OUTPUTS)
            for g in range(2):
                for c in range(C.C):
                    rows = slice(0, 3) if g == 0 else slice(3, 5)
                    if (g, c) in C.EDGE_BAD:                        # poisoned: all four outputs of (g, c), the risk of every agent of g at c
                        assert bool(torch.isnan(rb["occupancy"][g, c]).all()) and bool(torch.isnan(rb["any"][g, c]).all())
                        assert bool(torch.isnan(rb["conflict"][g, c])) and bool(torch.isnan(rb["risk"][rows, c]).all())
                    else:                                           # everything else as without the bad planes
                        for k in ("occupancy", "any", "conflict"):
                            assert torch.equal(rb[k][g, c], rc[k][g, c]), (k, g, c)
                        assert torch.equal(rb["risk"][rows, c], rc["risk"][rows, c])
        assert all(v > 0 for v in C.shape_e32(H, W).values())


# ---- 2. utils/occupancy.py ------------------------------------------------------------------------------------------------------------
def test_cell_grid_and_upsample_occupancy():
    occ = pkg("utils.occupancy")
    assert occ.cell_grid(256, 256, 4) == (64, 64) and occ.cell_grid(17, 23, 8) == (3, 3) and occ.cell_grid(5, 4, 8) == (1, 1)
    assert occ.cell_grid(17, 23, 1) == (17, 23) and occ.cell_grid(17, 23, 2) == (9, 12)
    for bad in (0, 3, 16):
        with pytest.raises(ValueError, match="cell"):
            occ.cell_grid(8, 8, bad)
    with pytest.raises(ValueError, match="no cells"):
        occ.cell_grid(0, 8, 2)
    for H, W in [(5, 4), (17, 23), (16, 24)]:
        for cell in C.CELLS:
            assert torch.equal(occ.cell_pixels(H, W, cell).double(), C.cell_pixels(H, W, cell))
            m = C.cell_shares(C.logits(2, H, W, 1), cell, 1.0)       # [2, 3, Hc, Wc]
            up = occ.upsample_occupancy(m, H, W, cell)
            assert up.shape == (2, 3, H, W) and float((up.sum(dim=(2, 3)) - 1.0).abs().max()) < 1e-12      # still a distribution per pixel
            assert float((C.pool(up, cell) - m).abs().max()) < 1e-15                    # pooled again: the cells' values
            y, x = H - 1, W - 1
            assert torch.equal(up[..., y, x], m[..., y // cell, x // cell] / float(C.cell_pixels(H, W, cell)[y // cell, x // cell]))
    with pytest.raises(ValueError, match="cells"):
        occ.upsample_occupancy(torch.zeros(3, 3), 17, 23, 4)


def test_conflict_report():
    occ = pkg("utils.occupancy")
    nan = float("nan")
    rows = occ.conflict_report(torch.tensor([0.5, 1.25]), torch.tensor([[0.25, nan], [0.75, 2.0], [0.0, 0.5]]), 0.25, 4)
    assert [r["step"] for r in rows] == [0, 1] and [r["pairs"] for r in rows] == [0.5, 1.25]
    assert rows[0]["agents"] == [1, 0, 2] and rows[0]["risk"] == [0.75, 0.25, 0.0]
    assert rows[1]["agents"] == [1, 2, 0] and rows[1]["risk"][:2] == [2.0, 0.5] and rows[1]["risk"][2] != rows[1]["risk"][2]      # NaN last
    assert all(r["cell_edge"] == 16.0 for r in rows)                                                 # 4 resized pixels at 0.25: 16 original
    assert occ.conflict_report(torch.zeros(1, 2), torch.zeros(3, 2), 1.0, 1)[1]["agents"] == [0, 1, 2]     # ties keep the row order
    with pytest.raises(ValueError, match="risk"):
        occ.conflict_report(torch.zeros(2), torch.zeros(3, 3), 0.25, 4)
    with pytest.raises(ValueError, match="cell"):
        occ.conflict_report(torch.zeros(2), torch.zeros(3, 2), 0.25, 3)
    with pytest.raises(ValueError, match="resize_factor"):
        occ.conflict_report(torch.zeros(2), torch.zeros(3, 2), 0.0, 4)


# ---- 3. the C entry points and their wrappers --------------------------------------------------------------------------------------------
def test_map_occupancy_is_exported_and_refuses_bad_arguments():
    L = pkg("_lib")
    lib = L.load()
    assert lib.ynet_abi_version() == 1
    assert {"ynet_map_occupancy", "ynet_map_occupancy_workspace_bytes"} <= set(L.header_symbols())
    assert len(L.SIGNATURES["ynet_map_occupancy"][1]) == 17 and len(L.SIGNATURES["ynet_map_occupancy_workspace_bytes"][1]) == 6
    with open(L.HEADER_PATH) as f:
        assert "#define YNET_MAP_OCCUPANCY_MAX_CELL 8" in f.read()
    vp = ctypes.c_void_p
    p = vp(4096)

    def call(x=p, bs=48, off=p, B=2, G=1, Cn=3, H=4, W=4, cell=2, T=1.0, occ=p, any_=p, conf=p, risk=p, ws=p, st=p):
        return lib.ynet_map_occupancy(x, bs, off, B, G, Cn, H, W, cell, T, occ, any_, conf, risk, ws, st, None)

    for kw, word in (({"x": None}, b"null map"), ({"off": None}, b"null offsets"), ({"occ": None}, b"null output"),
                     ({"ws": None}, b"null workspace"), ({"st": None}, b"null status"), ({"ws": vp(4100)}, b"8-byte")):
        assert call(**kw) != 0 and word in lib.ynet_last_error(), kw
    for cell in (0, -1, 3, 5, 16):
        assert call(cell=cell) != 0 and b"cell" in lib.ynet_last_error(), cell
    for T in (0.0, -1.0, float("inf"), float("nan"), 1e-39):
        assert call(T=T) != 0 and b"temperature" in lib.ynet_last_error(), T
    for kw in ({"B": 0}, {"Cn": 0}, {"H": 0}, {"W": 0}, {"G": 0}, {"B": -3}, {"G": -1}):
        assert call(**kw) != 0 and b"bad shape" in lib.ynet_last_error(), kw
    assert call(bs=1 << 31, B=1, Cn=1, H=32768, W=65536) != 0 and b"32-bit" in lib.ynet_last_error()
    assert call(bs=47) != 0 and b"batch stride" in lib.ynet_last_error()
    assert call(bs=4, B=1 << 29, Cn=4, H=1, W=1) != 0 and b"too many planes" in lib.ynet_last_error()
    assert call(bs=4, B=1, G=1 << 29, Cn=4, H=1, W=1) != 0 and b"too many tiles" in lib.ynet_last_error()


def test_workspace_bytes():
    lib = pkg("_lib").load()
    need = lib.ynet_map_occupancy_workspace_bytes
    # 8 bytes per plane (1 / Z), per (g, c, tile) (the conflict partial) and per (a, c, tile) (the risk partial); a tile is 64 patches of
    # max(4, cell) x cell pixels
    for (B, Cn, H, W, G, cell), tiles in {(128, 12, 256, 256, 1, 4): 64, (128, 12, 256, 256, 1, 1): 256, (128, 12, 256, 256, 3, 8): 16,
                                          (5, 3, 17, 23, 2, 2): 1, (5, 3, 17, 23, 2, 1): 2, (1, 1, 1, 1, 1, 8): 1, (9, 3, 96, 160, 1, 2): 30}.items():
        assert need(B, Cn, H, W, G, cell) == 8 * (B * Cn + G * Cn * tiles + B * Cn * tiles), (B, Cn, H, W, G, cell)
    for bad in ((0, 1, 4, 4, 1, 1), (1, 0, 4, 4, 1, 1), (1, 1, 0, 4, 1, 1), (1, 1, 4, 0, 1, 1), (1, 1, 4, 4, 0, 1), (1, 1, 4, 4, 1, 3),
                (1, 1, 32768, 65536, 1, 1), (1 << 29, 4, 1, 1, 1, 1)):
        assert need(*bad) == -1 and b"map_occupancy_workspace_bytes" in lib.ynet_last_error(), bad


def test_wrapper_refusals_and_signatures():
    ops = pkg("ops")
    x = torch.zeros(4, 3, 4, 4)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_occupancy(x)
    with pytest.raises(RuntimeError, match="HIP devices only"):
        ops.map_occupancy(x[:, -1:], [1, 3], cell=4, temperature=1.8)
    with pytest.raises(TypeError):
        ops.map_occupancy(x.numpy())
    for bad in (0, 3, 16, 2.5, None):
        with pytest.raises(ValueError, match="cell"):
            ops.map_occupancy(x, cell=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="temperature"):
            ops.map_occupancy(x, temperature=bad)
    for bad in (("occupancy", "mass"), ("risk", "risk")):
        with pytest.raises(ValueError, match="want"):
            ops.map_occupancy(x, want=bad)
    assert list(inspect.signature(ops.map_occupancy).parameters) == ["x", "group_sizes", "cell", "temperature", "want"]
    sig = inspect.signature(ops.map_occupancy).parameters
    assert sig["group_sizes"].default is None and sig["cell"].default == 1 and sig["temperature"].default == 1.0
    assert sig["want"].default == ("occupancy", "any", "conflict", "risk") and ops.OCCUPANCY_CELLS == (1, 2, 4, 8)
    assert inspect.signature(ops.check_occupancy_status).parameters["raise_error"].default is True
    # the group sizes are host data, checked on the host
    assert ops.occupancy_offsets(None, 5).tolist() == [0, 5] and ops.occupancy_offsets([0, 3, 1], 4).tolist() == [0, 0, 3, 4]
    assert ops.occupancy_offsets(torch.tensor([4, 0, 4]), 8).dtype.name == "int32"
    for bad, msg in (([2, 1], "sum to 3"), ([5, -1], "negative"), ([], "non-empty"), ([2.0, 2.0], "integers")):
        with pytest.raises(ValueError, match=msg):
            ops.occupancy_offsets(bad, 4)
    ops.check_occupancy_status()                                    # nothing ran: nothing to report
    P, trn = pkg("utils.predict"), pkg("models.trainer")
    assert inspect.signature(P.predict_with_occupancy).parameters["cell"].default == 4
    assert inspect.signature(P.predict_with_occupancy).parameters["cell"].kind is inspect.Parameter.KEYWORD_ONLY
    doc = " ".join(P.predict_with_occupancy.__doc__.split())
    assert all(w in doc for w in ("occupancy_any", "conflict", "risk", "ONE chunk", "ValueError", "would be lost"))
    assert "occupancy" in P.predict.__doc__ and "occupancy" in P.predict_styles.__doc__ and "occupancy" in P.predict_modes.__doc__
    with pytest.raises(ValueError, match="cell"):
        P.predict_with_occupancy(None, cell=3)
    with pytest.raises(TypeError):
        P.predict_with_occupancy(None, occupancy=4)
    with pytest.raises(ValueError, match="observed must be"):        # predict()'s own checks, through predict()'s own body
        P.predict_with_occupancy(None, None, [[1.0, 2.0]], None, [0], 1, 1, 1, 0.25, 1.0)
    assert list(inspect.signature(trn.YNetTrainer.predict_occupancy).parameters) == ["self", "df_obs", "image_path_or_images", "cell"]
    assert inspect.signature(trn.YNetTrainer.predict_occupancy).parameters["cell"].default == 4

"""Scene occupancy on the MI355X: ynet_map_occupancy against the fp64 restatement of tests/_occupancy_cases.py over its whole table, the
exactness rules bit for bit, the known answers, the edge rules, the layouts, and predict_with_occupancy() on the reference's fixtures.

Bound everywhere: |device - fp64| <= 2 * E32 + 2^-21 * max(1, |fp64|), E32 = the error of the same restatement run in fp32 (recorded
per shape and output in the table; measured on the spot for the inputs that are not in it).

Measured on the MI355X (largest |device - fp64| / bound over the table): see DESIGN.md section 4.15."""
import ctypes

import pytest
import torch

import _occupancy_cases as C
from conftest import Golden, build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def check(got, ref, e, what):
    """every finite reference entry within the bound, NaN where the reference has NaN; -> the largest error / bound"""
    g = got.detach().cpu().double()
    assert got.dtype == torch.float32 and g.shape == ref.shape, (what, got.dtype, g.shape, ref.shape)
    fin = torch.isfinite(ref)
    assert torch.equal(torch.isnan(g), torch.isnan(ref)) and bool(torch.isnan(ref[~fin]).all()), (what, "NaN pattern")
    if not fin.any():
        return 0.0
    err, bnd = (g - ref).abs()[fin], C.bound(ref, e)[fin]
    print(f"{what}: max error {float(err.max()):.3e} (bound there {float(bnd[err.argmax()]):.3e})")
    assert bool((err <= bnd).all()), (what, float(err.max()), float(bnd[err.argmax()]))
    return float((err / bnd).max())


def check_all(got, ref, e, what):
    assert set(got) == set(C.OUTPUTS) and all(v.is_cuda for v in got.values()), (what, set(got))
    return max(check(got[k], ref[k], e[k], f"{what} {k}") for k in C.OUTPUTS)


def same_bits(a, b, what, keys=C.OUTPUTS):
    for k in keys:
        assert torch.equal(a[k], b[k]), (what, k)


def clean_status(ops, what):
    assert ops.check_occupancy_status(raise_error=False) is False, what


# ---- 1. the kernel against fp64 over the whole table ------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", range(len(C.SHAPES)), ids=[f"{h}x{w}" for (h, w), _, _ in C.SHAPES])
def test_kernel_matches_fp64_over_the_table(dev, si):
    ops = pkg("ops")
    (H, W), _, e = C.SHAPES[si]
    worst, dx = 0.0, {}
    for cell, li, kind in C.cases(si):
        x, sizes, T, ref = C.case(si, cell, li, kind)
        if (li, kind) not in dx:
            dx[li, kind] = x.to(dev)
        what = f"{H}x{W} cell {cell} groups {sizes} kind {kind}"
        got = ops.map_occupancy(dx[li, kind], sizes, cell, T)
        worst = max(worst, check_all(got, ref, e, what))
        first = 0
        for g, s in enumerate(sizes):
            if s == 0:                                             # an empty group is all zeros
                assert all(bool((got[k][g] == 0.0).all()) for k in ("occupancy", "any", "conflict")), what
            if s == 1:                                             # one agent: no pair, bit for bit
                assert bool((got["conflict"][g] == 0.0).all()) and bool((got["risk"][first] == 0.0).all()), what
            first += s
    clean_status(ops, (H, W))
    print(f"{H}x{W}: largest error / bound {worst:.3f}")
    for (li, kind), d in dx.items():
        assert torch.equal(d.cpu(), C._input(si, li, kind))        # the input is read, never written


# ---- 2. exactness, bit for bit ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cell", C.CELLS)
def test_exactness(dev, cell):
    ops = pkg("ops")
    for H, W in [(16, 24), (16, 23), (96, 160)]:
        x, T = C.disjoint_halves(H, W)                             # two agents that share no cell: no conflict at all
        d = x.to(dev)
        got = ops.map_occupancy(d, [2], cell, T)
        assert bool((got["conflict"] == 0.0).all()) and bool((got["risk"] == 0.0).all()), (H, W)
        check_all(got, C.occupancy_ref(x, [2], cell, T), C.e32(x, [2], cell, T), f"disjoint halves {H}x{W} cell {cell}")
        same_bits(ops.map_occupancy(d, [2], cell, T), got, "two runs")
        # a null risk (and any other selection) leaves the other outputs' bits unchanged
        part = ops.map_occupancy(d, [2], cell, T, want=("occupancy", "any", "conflict"))
        assert set(part) == {"occupancy", "any", "conflict"}
        same_bits(part, got, "without risk", ("occupancy", "any", "conflict"))
        alone = ops.map_occupancy(d, [2], cell, T, want=())
        assert set(alone) == {"occupancy"} and torch.equal(alone["occupancy"], got["occupancy"])
        same_bits(ops.map_occupancy(d, [2], cell, T, want=("risk",)), got, "risk alone", ("occupancy", "risk"))
        # a group computed alone = the same group inside a three-group call
        x9 = C.logits(9, H, W, 1, 800)
        d9 = x9.to(dev)
        three = ops.map_occupancy(d9, [4, 2, 3], cell, T)
        check_all(three, C.occupancy_ref(x9, [4, 2, 3], cell, T), C.e32(x9, [4, 2, 3], cell, T), f"three groups {H}x{W} cell {cell}")
        for g, (lo, hi) in enumerate([(0, 4), (4, 6), (6, 9)]):
            one = ops.map_occupancy(d9[lo:hi], None, cell, T)
            for k in ("occupancy", "any", "conflict"):
                assert torch.equal(one[k][0], three[k][g]), (H, W, g, k)
            assert torch.equal(one["risk"], three["risk"][lo:hi]), (H, W, g)
    clean_status(ops, cell)


@pytest.mark.parametrize("cell", C.CELLS)
def test_channel_slice_and_planes_off_a_boundary(dev, cell):
    ops = pkg("ops")
    for H, W in [(17, 23), (8, 8)]:                                 # a channel slice, read in place: batch stride 5 planes, 2 planes read
        x5, T = C.sliced(H, W)
        d5 = x5.to(dev)
        view = d5[:, 1:3]
        assert not view.is_contiguous()
        got = ops.map_occupancy(view, None, cell, T)
        xs = x5[:, 1:3].contiguous()
        check_all(got, C.occupancy_ref(xs, [2], cell, T), C.e32(xs, [2], cell, T), f"channel slice {H}x{W} cell {cell}")
        same_bits(ops.map_occupancy(xs.to(dev), None, cell, T), got, f"slice against contiguous {H}x{W}")
    for si, li, kind in ((2, 3, 1), (5, 2, 4)):                      # W % 4 == 0, every plane 4, 8, 12 bytes off: element-wise loads, the same bits
        (H, W), _, _ = C.SHAPES[si]
        x = C._input(si, li, kind)
        sizes, T = C.LAYOUTS[li], C.KINDS[kind][1]
        aligned = ops.map_occupancy(x.to(dev), sizes, cell, T)
        buf = torch.empty(x.numel() + 4, device=dev)
        assert buf.data_ptr() % 16 == 0
        for off in (1, 2, 3):
            view = buf[off:off + x.numel()].view(x.shape)
            view.copy_(x)
            assert view.data_ptr() % 16 == 4 * off
            same_bits(ops.map_occupancy(view, sizes, cell, T), aligned, f"{H}x{W} off by {off}")
    clean_status(ops, cell)


# ---- 3. known answers ----------------------------------------------------------------------------------------------------------------------
def test_known_answers(dev):
    ops = pkg("ops")
    for H, W in [(5, 4), (17, 23), (96, 160)]:
        e = C.shape_e32(H, W)
        for cell in C.CELLS:
            for n in (1, 3, 9):
                x, T, want = C.constant_planes(n, H, W, cell)
                check_all(ops.map_occupancy(x.to(dev), None, cell, T), want, e, f"{n} constant planes {H}x{W} cell {cell}")
    clean_status(ops, "known answers")


# ---- 4. the edge rules ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("H,W", C.EDGE_SHAPES)
def test_edge_rules(dev, H, W):
    ops = pkg("ops")
    bad, clean, sizes, T = C.edge_scene(H, W)
    e = C.shape_e32(H, W)
    for cell in C.CELLS:
        got_clean = ops.map_occupancy(clean.to(dev), sizes, cell, T)
        check_all(got_clean, C.occupancy_ref(clean, sizes, cell, T), e, f"clean scene {H}x{W} cell {cell}")
        clean_status(ops, "clean scene")
        got = ops.map_occupancy(bad.to(dev), sizes, cell, T)
        check_all(got, C.occupancy_ref(bad, sizes, cell, T), e, f"edge scene {H}x{W} cell {cell}")      # (the NaN pattern is the reference's)
        with pytest.raises(RuntimeError, match="NaN"):
            ops.check_occupancy_status()
        clean_status(ops, "the flag is cleared")
        for g in range(2):
            rows = slice(0, 3) if g == 0 else slice(3, 5)
            for c in range(C.C):
                if (g, c) in C.EDGE_BAD:                            # exactly the poisoned (g, c): all four outputs
                    assert bool(torch.isnan(got["occupancy"][g, c]).all()) and bool(torch.isnan(got["any"][g, c]).all())
                    assert bool(torch.isnan(got["conflict"][g, c])) and bool(torch.isnan(got["risk"][rows, c]).all())
                else:                                               # the other steps and the other group keep their bits
                    for k in ("occupancy", "any", "conflict"):
                        assert torch.equal(got[k][g, c], got_clean[k][g, c]), (cell, g, c, k)
                    assert torch.equal(got["risk"][rows, c], got_clean["risk"][rows, c]), (cell, g, c)


SENTINEL = -7.0


def raw_call(x, offsets, cell, T):
    """ynet_map_occupancy through ctypes on device `offsets` as given (ops.map_occupancy checks its group sizes on the host) ->
    (outputs pre-filled with SENTINEL, status)"""
    L = pkg("_lib")
    lib = L.load()
    dev = x.device
    B, Cn, H, W = x.shape
    G = len(offsets) - 1
    Hc, Wc = -(-H // cell), -(-W // cell)
    out = {"occupancy": torch.full((G, Cn, Hc, Wc), SENTINEL, device=dev), "any": torch.full((G, Cn, Hc, Wc), SENTINEL, device=dev),
           "conflict": torch.full((G, Cn), SENTINEL, device=dev), "risk": torch.full((B, Cn), SENTINEL, device=dev)}
    off = torch.tensor(offsets, dtype=torch.int32, device=dev)
    st = torch.zeros(1, dtype=torch.int32, device=dev)
    need = lib.ynet_map_occupancy_workspace_bytes(B, Cn, H, W, G, cell)
    assert need > 0
    ws = torch.empty(need // 8, dtype=torch.float64, device=dev)
    L.check(lib.ynet_map_occupancy(x.data_ptr(), Cn * H * W, off.data_ptr(), B, G, Cn, H, W, cell, T, out["occupancy"].data_ptr(),
                                   out["any"].data_ptr(), out["conflict"].data_ptr(), out["risk"].data_ptr(), ws.data_ptr(), st.data_ptr(),
                                   ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), lib)
    torch.cuda.synchronize()
    return out, int(st.item())


@pytest.mark.parametrize("H,W", C.EDGE_SHAPES)
def test_offsets_beyond_the_rows(dev, H, W):
    """device offsets with a bound beyond B: status bit 2, a NaN group, the neighbours intact, nothing addressed through the bad bound"""
    ops = pkg("ops")
    _, clean, _, T = C.edge_scene(H, W)
    d = clean.to(dev)
    for cell in C.CELLS:
        good = ops.map_occupancy(d[:3], None, cell, T)
        legal, status = raw_call(d, [0, 3, 5], cell, T)
        assert status == 0
        same_bits(legal, ops.map_occupancy(d, [3, 2], cell, T), "the raw call is the wrapper's call")
        got, status = raw_call(d, [0, 3, 9], cell, T)              # group 1 = rows 3 .. 8 of a map of 5 rows
        assert status == 2
        for k in ("occupancy", "any", "conflict"):
            assert torch.equal(got[k][0], good[k][0]) and bool(torch.isnan(got[k][1]).all()), (cell, k)
        assert torch.equal(got["risk"][:3], good["risk"]) and bool(torch.isnan(got["risk"][3:]).all()), cell
        got, status = raw_call(d, [0, 6, 5], cell, T)              # both groups: 0 .. 5 is beyond B, 6 .. 4 is no range
        assert status == 2 and all(bool(torch.isnan(v).all()) for v in got.values()), cell
        got, status = raw_call(d, [-2, 2, 5], cell, T)             # a negative bound; group 1 = rows 2 .. 4 stays intact
        assert status == 2
        tail = ops.map_occupancy(d[2:], None, cell, T)
        for k in ("occupancy", "any", "conflict"):
            assert bool(torch.isnan(got[k][0]).all()) and torch.equal(got[k][1], tail[k][0]), (cell, k)
        assert torch.equal(got["risk"][2:], tail["risk"]) and bool(torch.isnan(got["risk"][:2]).all()), cell
    clean_status(ops, "raw calls use their own flag")


# ---- 5. layouts ----------------------------------------------------------------------------------------------------------------------------
def test_many_groups(dev):
    """70000 groups of one 2 x 2 plane each: more (g, c, tile) workgroups than blockIdx.y or .z could hold"""
    ops = pkg("ops")
    x, sizes, T = C.many_groups()
    d = x.to(dev)
    for cell in (1, 2):
        got = ops.map_occupancy(d, sizes, cell, T)
        check_all(got, C.occupancy_ref(x, sizes, cell, T), C.e32(x, sizes, cell, T), f"70000 groups of 2x2 cell {cell}")
        assert bool((got["conflict"] == 0.0).all()) and bool((got["risk"] == 0.0).all())
    pairs = ops.map_occupancy(d, [2] * 35000, 1, T)
    check_all(pairs, C.occupancy_ref(x, [2] * 35000, 1, T), C.e32(x, [2] * 35000, 1, T), "35000 groups of two 2x2 planes")
    clean_status(ops, "many groups")


def test_production_case(dev):
    ops = pkg("ops")
    x, sizes, cell, T = C.production()
    assert x.shape == (32, 2, 256, 256) and cell == 4
    got = ops.map_occupancy(x.to(dev), sizes, cell, T)
    ratio = check_all(got, C.occupancy_ref(x, sizes, cell, T), C.e32(x, sizes, cell, T), "32 agents of 256x256, cell 4")
    print(f"32 agents of 256x256: largest error / bound {ratio:.3f}")
    occ = got["occupancy"].double()
    assert float((occ.sum(dim=(2, 3)) - 32.0).abs().max()) < 32 * 2.0 ** -20           # a plane of D sums to the group's size
    assert float((got["risk"].double().sum(0) - 2.0 * got["conflict"].double()[0]).abs().max()) < 1e-5 * float(got["conflict"].max())
    clean_status(ops, "production")


# ---- 6. the driver on the reference's fixtures --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["tiny_short_mosa1", "tiny_long_cws"])
def test_predict_with_occupancy_on_the_fixtures(dev, case):
    g = Golden(case)
    cfg, m = g.cfg(), g.meta
    model = build_model(cfg, g.state_dict(), dev)
    P, occ = pkg("utils.predict"), pkg("utils.occupancy")
    in_t = O.dist_template(cfg.template_size).to(dev)
    n_goal, n_traj = m["n_goal"], m.get("n_traj") or 1
    N, traj, scene = m["B"], g.t("traj"), g.t("scene")[0]
    assert N >= 2
    args = (model, scene, traj[:, :cfg.obs_len], in_t, list(cfg.waypoints), n_goal, n_traj, cfg.obs_len, cfg.resize_factor, cfg.temperature)
    torch.manual_seed(11)
    pb = P.predict(*args, network=cfg.network, return_maps=True)
    after = torch.get_rng_state()
    for cell, bs in ((4, None), (1, N), (8, N + 3)):
        torch.manual_seed(11)
        pa = P.predict_with_occupancy(*args, network=cfg.network, return_maps=True, batch_size=bs, cell=cell)
        assert torch.equal(torch.get_rng_state(), after)            # no draw added
        assert set(pa) - set(pb) == {"occupancy", "occupancy_any", "conflict", "risk"}
        for k in pb:                                                # every other result is predict()'s, bit for bit: no draw moved
            assert torch.equal(pa[k], pb[k]), k
        gm = pb["goal_map"].cpu()
        H, W = gm.shape[2:]
        Hc, Wc = occ.cell_grid(H, W, cell)
        assert pa["occupancy"].shape == pa["occupancy_any"].shape == (cfg.pred_len, Hc, Wc)
        assert pa["conflict"].shape == (cfg.pred_len,) and pa["risk"].shape == (N, cfg.pred_len)
        ref, e = C.occupancy_ref(gm, [N], cell, cfg.temperature), C.e32(gm, [N], cell, cfg.temperature)
        what = f"{case} cell {cell}"
        check(pa["occupancy"], ref["occupancy"][0], e["occupancy"], what + " occupancy")
        check(pa["occupancy_any"], ref["any"][0], e["any"], what + " any")
        check(pa["conflict"], ref["conflict"][0], e["conflict"], what + " conflict")
        check(pa["risk"], ref["risk"], e["risk"], what + " risk")
        rows = occ.conflict_report(pa["conflict"], pa["risk"], cfg.resize_factor, cell)
        assert len(rows) == cfg.pred_len and sorted(rows[-1]["agents"]) == list(range(N)) and rows[0]["cell_edge"] == cell / cfg.resize_factor
    with pytest.raises(ValueError, match="one chunk"):              # a scene split over chunks would lose the pairs across them
        P.predict_with_occupancy(*args, network=cfg.network, batch_size=N - 1)
    with pytest.raises(ValueError, match="cell"):
        P.predict_with_occupancy(*args, network=cfg.network, cell=3)

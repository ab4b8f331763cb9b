"""tests/_conv_cases.py on the CPU: every row launches what it claims by the dispatcher's formulas (restated in plain Python there) and those formulas agree with the library's
own host code -- ynet_conv2d_plan over a grid of shapes, the *_supported queries, ynet_conv2d_relu_bits_words, ynet_conv2d_workspace_floats --; the gated rows sit at their
gates; every edge is claimed by a row that reaches it and no row is spare; the persistent walk visits every tile once for every grid a launch can have; and the references
are what the GPU test may hold the kernels to: family (b) exact in fp32 by a bound on the generated tensors, family (a) within the project's tolerances of stock fp32 torch
with at most 0.1 % of the gates ambiguous, three rows against a plain restatement of the convolution."""
import itertools
import os

import pytest
import torch

import _align_cases as A
import _conv_cases as C
from conftest import pkg


@pytest.fixture(scope="module")
def lib():
    return pkg("_lib").load()


def test_no_switch_of_the_dispatcher_is_set():
    """The gates are read from the environment once per process; the table is derived for the defaults."""
    assert [s for s in C.SWITCHES if s in os.environ] == []


@pytest.mark.parametrize("name", list(C.CASES))
def test_row_launches_what_it_claims(lib, name):
    c = C.case(name)
    o, B, H, W, K = c["opts"], c["B"], c["H"], c["W"], c["K"]
    p = C.launch_plan(name)
    vl, vs = C.aligned(c)
    assert C.claim_of(p, vl, vs) == c["claim"], (name, C.claim_of(p, vl, vs), p)
    assert c["entry"] in ("conv", "dgrad_relu", "bits", "pool", "add") and c["mode"] in (0, 1) and len(c["cs"]) <= 4 and len(c["couts"]) <= 4
    if "place" in o:
        assert o["place"][1] in A.PLACEMENTS
    # the entry's own query serves the shape
    if c["entry"] == "pool":
        assert lib.ynet_conv2d_pool_supported(B, H, W, c["cout"], K) == 1
    if c["entry"] == "add":
        assert lib.ynet_conv2d_add_supported(B, H, W, c["cout"], K) == 1
    if c["entry"] == "bits":
        assert lib.ynet_conv2d_relu_bits_words(B, H, W, c["cout"], K) == C.bits_words(B, H, W, c["cout"], K) > 0
    if c["entry"] == "dgrad_relu":      # "in the kernel" is what the library says it is
        assert lib.ynet_conv2d_dgrad_relu_supported(B, H, W, c["cout"], K) == int(p["kind"] == C.DMA)
    if "workspace" not in o and c["entry"] in ("conv", "dgrad_relu"):
        assert C.ws_of(c) == lib.ynet_conv2d_workspace_floats(B, H, W, c["ctot"])
    # the plan mirror, for the plain rows: rows, tile count, dma, fold, chunk depth
    if c["entry"] == "conv" and "mask" not in o and p["kind"] != C.STREAM:
        q = C.launch_plan(name, ignore_place=True)
        word = lib.ynet_conv2d_plan(B, H, W, c["cout"], K)
        assert word == C.plan_word(B, H, W, c["cout"], K)
        assert (word & 255, word >> 8 & 255, word >> 17 & 1, 1 << (word >> 19 & 3), word >> 21) == (q["rows"], q["tiles"], int(q["kind"] in (C.DMA, C.FOLDED)), q["fold"], q["cc"]), name
    # the limits
    assert B * c["ctot"] * H * W <= 2 ** 24 and 2 * B * H * W * c["cin"] * c["ctot"] * K * K <= 4e9, name
    # the walk of this launch, on every grid it can have
    if p["kind"] != C.STREAM:
        for per_cu in range(1, 9):
            grid = min(p["ntiles"], per_cu * 256)
            assert sorted(t for wg in C.walk(p["ntiles"], grid) for t in wg) == list(range(p["ntiles"])), (name, grid)


@pytest.mark.parametrize("name", C.GATED)
def test_gated_row_sits_at_its_gate(lib, name):
    c = C.case(name)
    here, below = C.gate_key(name, c["B"]), C.gate_key(name, c["B"] - 1)
    assert here is not None and here != below, (name, here, below)
    q = {"pool": lib.ynet_conv2d_pool_supported, "add": lib.ynet_conv2d_add_supported, "bits": lib.ynet_conv2d_relu_bits_words}.get(c["entry"])
    if q is not None:      # an epilogue row at its own two-row gate, or at the tile count's: one image fewer is refused, or tiles differently
        args = (c["H"], c["W"], c["cout"], c["K"])
        assert q(c["B"], *args) > 0 and (q(c["B"] - 1, *args) > 0) == (below is not None)
    if c["entry"] == "dgrad_relu":
        assert lib.ynet_conv2d_dgrad_relu_supported(c["B"], c["H"], c["W"], c["cout"], c["K"]) == 1
        assert lib.ynet_conv2d_dgrad_relu_supported(c["B"] - 1, c["H"], c["W"], c["cout"], c["K"]) == 0


def test_every_edge_is_reached_and_no_row_is_spare():
    claimed = {e for n in C.CASES for e in C.case(n)["edges"]}
    assert claimed == set(C.EDGES), claimed ^ set(C.EDGES)
    for n in C.CASES:
        assert C.case(n)["edges"], n
        for e in C.case(n)["edges"]:
            assert C.EDGES[e](n), (n, e)      # no row claims an edge its shape cannot reach
    # no row is spare: each is the only claimant of some edge, or differs from every other claimant of one in the launch it takes
    for n in C.CASES:
        alone = False
        for e in C.case(n)["edges"]:
            others = [m for m in C.CASES if m != n and e in C.case(m)["edges"]]
            alone |= all(C.case(m)["claim"] != C.case(n)["claim"] or C.case(m)["entry"] != C.case(n)["entry"] for m in others)
        assert alone, n
    assert set(C.GATED) <= set(C.CASES) and set(C.PLANTED) | set(C.MASKED_NAN) <= set(C.CASES)
    # every kind, every (kind, rows, tiles) the default gates can launch
    seen = {(C.case(n)["claim"][0], C.case(n)["claim"][1], C.case(n)["claim"][5]) for n in C.CASES}
    want = {(C.DMA, 4, 1), (C.DMA, 4, 2), (C.DMA, 2, 1), (C.DMA, 2, 2), (C.DMA, 2, 3), (C.DMA, 2, 4)} | {(C.FOLDED, 1, t) for t in (1, 2, 3, 4)} | {(C.STREAM, 0, 1), (C.STREAM, 0, 2)}
    want |= {(C.REG, 1, 1), (C.REG, 2, 1), (C.REG, 4, 1), (C.REG, 2, 2), (C.REG, 2, 3), (C.REG, 2, 4), (C.REG, 1, 2), (C.REG, 4, 2)}
    assert seen == want, seen ^ want
    # the epilogue forms on the LDS-DMA tiles: (entry, rows, tiles)
    epi = {(C.case(n)["entry"], C.case(n)["claim"][1], C.case(n)["claim"][5]) for n in C.CASES if C.case(n)["entry"] != "conv" and C.case(n)["claim"][0] == C.DMA}
    assert epi >= {("add", 2, 2), ("add", 2, 4), ("add", 4, 2), ("pool", 2, 1), ("pool", 4, 1), ("pool", 2, 2), ("pool", 2, 4), ("bits", 2, 1), ("bits", 2, 2), ("bits", 2, 4),
                   ("bits", 4, 2), ("dgrad_relu", 2, 1), ("dgrad_relu", 2, 2), ("dgrad_relu", 2, 4), ("dgrad_relu", 4, 1)}
    # planted rows: a two-row row, a folded row, a split-K row; the pooled copy with rows 2 and rows 4 on a ragged map
    kinds = {(C.case(n)["claim"][0], C.case(n)["claim"][2] > 1) for n in C.PLANTED}
    assert kinds >= {(C.DMA, False), (C.FOLDED, False), (C.FOLDED, True)}
    assert {C.case(n)["claim"][1] for n in C.PLANTED if C.case(n)["entry"] == "pool"} == {2, 4}
    for n, (b, ch, y, x) in C.PLANTED.items():
        c, p = C.case(n), C.launch_plan(n)
        assert b < C.images(c, 0) and ch < c["cs"][0] and y < c["H"] and x < c["W"] and (c["entry"] == "pool" or not c["relu"]), n
        if c["entry"] == "pool":      # the 3 x 3 neighbourhood lies inside the map, straddles four 2 x 2 blocks and the corner of four tiles, on a ragged map
            assert 0 < y < c["H"] - 1 and 0 < x < c["W"] - 1 and y % 2 == 0 and x % 2 == 0 and y % p["th"] == 0 and x % p["tw"] == 0, n
            assert c["H"] % p["th"] != 0 and c["W"] % p["tw"] != 0, n


def test_the_pooling_rule_is_stock_torchs():
    """C.pool_rule -- the block's maximum, NaN where any of the four is -- against F.max_pool2d on the CPU: finite data, ties, and NaNs that torch propagates too."""
    y = torch.randint(-3, 4, (2, 3, 6, 8), generator=A._gen(41)).double()
    assert torch.equal(C.pool_rule(y), torch.nn.functional.max_pool2d(y, 2, 2))
    y[0, 1, 2, 3] = y[1, 2, 5, 0] = float("nan")
    y[1, 0, 0, 0] = float("inf")
    got, want = C.pool_rule(y), torch.nn.functional.max_pool2d(y, 2, 2)
    assert int(torch.isnan(got).sum()) == 2 and bool(torch.isnan(got[0, 1, 1, 1])) and bool(torch.isnan(got[1, 2, 2, 0])) and float(got[1, 0, 0, 0]) == float("inf")
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0))


def test_the_formulas_are_the_librarys(lib):
    """ynet_conv2d_plan (what bench.py and tools/conv_bench.py name kernels by) and the queries against the formulas in _conv_cases, over the grid."""
    sizes = [1, 4, 8, 12, 16, 17, 32, 36, 64, 128]
    for B, H, W, cout, K in itertools.product([1, 2, 8, 64], sizes, sizes, [1, 16, 17, 32, 33, 48, 49, 64, 65, 130], [1, 3, 5]):
        at = (B, H, W, cout, K)
        assert lib.ynet_conv2d_plan(*at) == C.plan_word(*at), at
        assert lib.ynet_conv2d_pool_supported(*at) == int(C.pool_supported(*at)) and lib.ynet_conv2d_add_supported(*at) == int(C.add_supported(*at)), at
        assert lib.ynet_conv2d_relu_bits_words(*at) == C.bits_words(*at) and lib.ynet_conv2d_dgrad_relu_supported(*at) == int(C.rows_tiles_ok(*at)), at
    # the workspace: up to 65536 pixels, W % 4 == 0
    for B, H, W, cout in [(1, 256, 256, 8), (1, 256, 260, 8), (64, 32, 32, 64), (65, 32, 32, 64), (4, 16, 18, 16), (16384, 1, 4, 1), (16385, 1, 4, 1)]:
        want = 8 * B * cout * H * W if W % 4 == 0 and B * H * W <= 65536 else 0
        assert lib.ynet_conv2d_workspace_floats(B, H, W, cout) == C.workspace_floats(B, H, W, cout) == want
    # conv_ksplit's corners
    assert [C.conv_ksplit(i, n) for i, n in [(255, 4), (256, 4), (255, 3), (4, 9), (4, 16), (4, 64), (128, 12), (171, 7)]] == [2, 1, 1, 4, 8, 8, 4, 3]


def test_the_persistent_walk_visits_every_tile_once():
    """Every grid 8 k up to 2048 (the XCD walk) against tile counts at and above it, the plain walk below it; and advance_tile's carries against decode."""
    for grid in range(8, C.SLOTS_MAX + 1, 8):
        for ntiles in {grid, grid + 1, grid + 7, 2 * grid - 1, 8 * grid + 3, 2049, 2055, 2345}:
            if ntiles >= grid:
                wgs = C.walk(ntiles, grid)
                assert sorted(t for wg in wgs for t in wg) == list(range(ntiles)), (grid, ntiles)
                per_xcd = C.cdiv(ntiles, 8)
                assert all(t // per_xcd == blk % 8 for blk, wg in enumerate(wgs) for t in wg)      # an XCD keeps its own eighth
    for ntiles in (1, 3, 7, 9, 66, 255):
        assert sorted(t for wg in C.walk(ntiles, ntiles) for t in wg) == list(range(ntiles))
    w = C.walk(2049, 2048)      # a short last XCD: 257 tiles per XCD, the last holds 250; 6 workgroups of it stay idle
    assert [sum(len(wg) for wg in w[x::8]) for x in range(8)] == [257] * 7 + [250] and sum(not wg for wg in w) == 6 and max(len(wg) for wg in w) == 2
    # the mixed-radix step of a workgroup's walk lands on the tile decode names, for the rows whose workgroups take more than one tile
    for name in ("walk_2049", "walk_add_2055", "cg3_cout130", "t4", "ks_items_255", "fold4_w8"):
        c, p = C.case(name), C.launch_plan(name)
        radix = (p["ksplit"], p["cgroups"], C.cdiv(c["W"], p["tw"]), C.cdiv(c["H"], p["th"]))
        for grid in {min(p["ntiles"], 256 * k) for k in (1, 2, 3, 5, 8)} | {8}:
            wgs = C.walk(p["ntiles"], grid)
            stride = grid >> 3 if grid % 8 == 0 and p["ntiles"] >= grid else grid
            step = C.decode(stride, p, c["B"], c["H"], c["W"])
            for wg in wgs[::7]:
                at = C.decode(wg[0], p, c["B"], c["H"], c["W"]) if wg else None
                for t in wg[1:]:
                    at = C.advance(at, step, radix)
                    assert at == C.decode(t, p, c["B"], c["H"], c["W"]), (name, grid, t)


def test_pack_weight_restatement_is_the_layout_the_header_states():
    w = torch.arange(2 * 3 * 9, dtype=torch.float32).view(2, 3, 3, 3)
    p0, p1 = C.packed(w, 0), C.packed(w, 1)
    assert p0.shape == (32, 9, 64) and p1.shape == (32, 9, 64)
    assert float(p0[2, 5, 1]) == float(w[1, 2].flatten()[5]) and float(p1[1, 5, 2]) == float(w[1, 2].flatten()[3])
    assert float(p0[3:].abs().sum()) == 0 and float(p0[:, :, 2:].abs().sum()) == 0 and float(p1[2:].abs().sum()) == 0 and float(p1[:, :, 3:].abs().sum()) == 0


@pytest.mark.parametrize("name", ["fold2_w12", "k5_map_2x3", "k1_two_sources_shared"])
def test_reference_against_a_plain_restatement(name):
    """The fp64 reference of family (b) against loops over the taps: 3x3 with three ragged sources, 5x5 on a map smaller than the filter, 1x1 with a shared source."""
    c, inp, ref = C.case(name), C.inputs(name, "b"), C.ref64(name, "b")
    x = torch.cat([t[torch.arange(c["B"]) % t.shape[0]] for t in inp.xs], 1)
    got = C.restate(x, inp.w, inp.bias, c["K"])
    assert torch.equal(torch.relu(got) if c["relu"] else got, ref["y"])


@pytest.mark.parametrize("name", list(C.CASES))
def test_references(name):
    c = C.case(name)
    o, K = c["opts"], c["K"]
    # ---- family (b): exact.  Every tensor holds integers in its range, every partial sum of any summation order stays below 2^24
    b, rb = C.inputs(name, "b"), C.ref64(name, "b")
    for t, top in [(x, 3) for x in b.xs] + [(b.w, 2), (b.bias, 4), (b.addend, 4), (b.dy2, 4), (b.w2, 2), (b.mask, 3), (b.act, 3), (b.dmask, 3)]:
        assert t is None or (torch.equal(t, t.round()) and float(t.abs().max()) <= top)
    assert c["cin"] * K * K * 3 * 2 + 4 + 4 < 2 ** 24 and o.get("dy", 0) * 9 * 4 * 2 < 2 ** 24, name
    for t in (b.act, b.mask, b.dmask):
        assert t is None or (float(t.min()) >= 0 and 0.3 < float((t == 0).float().mean()) < 0.7)
    for k, t in rb.items():
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24 and torch.equal(t.float().double(), t), (name, k)
    if c["relu"] and rb["pre"].numel() > 4096:
        assert float((rb["pre"] == 0).float().mean()) > 1e-3, name      # zeros on the ReLU's edge are frequent
    if c["entry"] == "pool":
        # ... and so are ties between the two largest elements of a 2 x 2 block (behind a ReLU: between positive ones), in every pool row: the integer family is the sweep's
        # tie case, compared bit for bit; the planted test of the GPU file adds one block whose four elements are all the bias
        blk = rb["y"].view(c["B"], c["ctot"], c["H"] // 2, 2, c["W"] // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(-1, 4).topk(2, dim=-1).values
        assert float(((blk[:, 0] == blk[:, 1]) & ((blk[:, 0] > 0) | (not c["relu"]))).float().mean()) > 0.01, name
    # ---- family (a): a correct fp32 implementation (stock torch on the CPU) meets the tolerances the GPU test uses
    a, ra = C.inputs(name, "a"), C.ref64(name, "a")
    r32 = C.reference(name, a, torch.float32)
    tol = A.TOL_DX if c["mode"] == 1 else A.TOL_Y
    for k in ("y", "pooled"):
        if k in ra:
            assert A.mismatch(r32[k], ra[k], **tol)[0] == 0, (name, k)
    assert ra["y"].shape == (c["B"], c["ctot"], c["H"], c["W"]) and float(ra["y"].abs().max()) > 0.1
    el = C.ambiguous(name, ra)
    assert (el is not None) == (c["entry"] == "bits")
    if el is not None:      # the exclusion cap, on the reference alone; no gradient reaches an ambiguous gate, so the fp32 run's own gate decides nothing
        assert float(el.float().mean()) <= 1e-3, (name, float(el.float().mean()))
        assert A.mismatch(r32["gated"], ra["gated"], **A.TOL_DX)[0] == 0, name
        assert bool((ra["gated"][el] == 0).all()) and float((a.dy2 != 0).float().mean()) > 0.5
        eb = C.ambiguous(name, rb)      # (family (b) has no value near a gate that is not ON it)
        assert bool((rb["pre"][eb] == 0).all())

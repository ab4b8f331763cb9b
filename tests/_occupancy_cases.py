"""Seeded inputs and the fp64 restatement for the tests of ynet_map_occupancy / ops.map_occupancy (tests/test_occupancy_host.py checks this
table on the CPU, tests/test_gpu_occupancy.py runs the kernel against it).

The reference is stock torch on .double() inputs (`occupancy_ref`), never the code under test.  Per agent a (a row of x), step c and cell
of cell x cell pixels, with z = x / T, w = sigmoid(z), Z_a = sum w over the plane and m_a = the sum of w / Z_a over the cell's pixels
(the plane zero-padded to a multiple of cell, then a reshape-sum), and per group g of consecutive rows:
    occupancy = D = sum_a m_a      any = 1 - prod_a (1 - m_a)      conflict = 1/2 sum_cells (D^2 - sum_a m_a^2)
    risk_a = sum_cells m_a (D - m_a)
Run in fp32 the same code is the yardstick of the device test: E32 is its largest error against its own fp64 run, and the device bound
is 2 * E32 + 2^-21 * max(1, |ref|) (four fp32 ulps of the stored result; the factor 2 is the one tests/_compliance_cases.py gives the
device over the fp32 restatement).  The logit kinds (with their temperatures) are those of tests/_likelihood_cases.py."""
import functools

import numpy as np
import torch

import _likelihood_cases as L

SEED = 20250611
C = 3
KINDS = L.KINDS
CELLS = (1, 2, 4, 8)
OUTPUTS = ("occupancy", "any", "conflict", "risk")
DEPTH = {1: 8, 2: 4, 4: 2, 8: 1}      # d: the agents whose loads the walk keeps in flight, per cell edge (8 16-byte vectors per thread)
SPLIT = {1: 1, 2: 2, 4: 4, 8: 8}      # the waves that share a group's agents, per cell edge: wave w takes the w-th run of ceil(n / SPLIT)


def runs(n, cell):
    """the agents each wave of a workgroup walks, for a group of n"""
    per = -(-n // SPLIT[cell])
    return [max(0, min(n, (w + 1) * per) - min(n, w * per)) for w in range(SPLIT[cell])]


# Group layouts (sizes of consecutive groups), chosen around the edges of the agent walk: with d agents in flight per round, a run of
# k * d agents goes through rounds only, one of fewer than d through the one-by-one tail only, anything else through both.  Runs of d - 1,
# d and d + 1 agents occur at every cell edge (tests/test_occupancy_host.py checks that): at cell 1 the groups of 7, 8, 9; at cell 2 those
# of 5 (3 + 2), 8 (4 + 4), 9 (5 + 4); at cell 4 those of 4 (1 each), 8 (2 each), 9 (3 + 3 + 3); at cell 8 those of 1 .. 8 (1 or 0 each)
# and 9 (2 + 2 + 2 + 2 + 1).
LAYOUTS = [
    [1],                # one agent: no pair
    [2],
    [0, 3, 1],          # an empty group first
    [5],
    [9],
    [4, 0, 4],          # an empty group between two
    [7, 8],             # d - 1 and d at cell 1 (9 above is d + 1)
]


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


# ------------------------------------------------------------------------------------------------
# (H, W) -> the walk of the kernels the shape exists for.  Third field: E32 per output = the largest error of `occupancy_ref` run in fp32
# against its own fp64 run over the cases of the shape (`cases`), measured on the CPU (tests/test_occupancy_host.py re-measures it and
# holds the table to it) and rounded up to three digits.  At (1, 3) and (5, 4), cell 8 is a cell larger than the map.
# ------------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 1), "one pixel: every agent in the one cell", {"occupancy": 0.0, "any": 0.0, "conflict": 0.0, "risk": 0.0}),
    ((1, 3), "one row, element-wise", {"occupancy": 4.28e-07, "any": 1.43e-07, "conflict": 2.12e-06, "risk": 9.54e-07}),
    ((5, 4), "one patch row of vectors: idle threads, partial cells below", {"occupancy": 1.25e-06, "any": 1.41e-07, "conflict": 9.11e-06, "risk": 1.51e-06}),
    ((17, 23), "W % 4 != 0, 391 elements: planes sit off a 16-byte boundary; partial cells right and below", {"occupancy": 3.08e-07, "any": 2.50e-07, "conflict": 5.89e-07, "risk": 4.29e-07}),
    ((90, 12), "H % 4 != 0, H % 8 != 0: partial cells below; 270 vectors", {"occupancy": 1.49e-07, "any": 2.46e-07, "conflict": 2.21e-07, "risk": 1.11e-07}),
    ((96, 160), "several tiles per plane at every cell edge", {"occupancy": 1.56e-07, "any": 2.83e-07, "conflict": 9.14e-08, "risk": 5.20e-08}),
    ((256, 256), "the production size", {"occupancy": 8.15e-08, "any": 3.41e-07, "conflict": 2.34e-08, "risk": 1.11e-08}),
]


def logits(Bn, H, W, kind, *key):
    """[Bn, C, H, W] fp32 logits of KINDS[kind], as _likelihood_cases.logits forms them, for Bn agents"""
    g = _gen(100 + kind, Bn, H, W, *key)
    n = torch.randn(Bn, C, H, W, generator=g)
    if kind == 0:
        return n * 0.5
    if kind == 1:
        return n * 8.0
    if kind == 2:
        return n * 3.0 - 10.0
    if kind == 3:
        return n * 3.0 + 20.0
    cy = torch.rand(Bn, C, 1, 1, generator=g) * (H - 1)
    cx = torch.rand(Bn, C, 1, 1, generator=g) * (W - 1)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    s = max(1.0, 0.04 * max(H, W))
    return -12.0 + 14.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.05 * n


def cell_shares(x, cell, T, dtype=torch.float64):
    """m [B, C, Hc, Wc] at `dtype`: sigmoid, normalise, zero-pad to a multiple of `cell`, reshape-sum.  A NaN logit, or Z == 0, makes a
    plane NaN by itself (NaN / NaN, 0 / 0)."""
    w = torch.sigmoid(x.float().to(dtype) / T)
    return pool(w / w.sum(dim=(2, 3), keepdim=True), cell)


def pool(p, cell):
    """[B, C, H, W] per pixel -> [B, C, Hc, Wc] per cell: zero-pad to a multiple of `cell`, reshape-sum"""
    Bn, Cn, H, W = p.shape
    Hc, Wc = -(-H // cell), -(-W // cell)
    p = torch.nn.functional.pad(p, (0, Wc * cell - W, 0, Hc * cell - H))
    return p.reshape(Bn, Cn, Hc, cell, Wc, cell).sum(dim=(3, 5))


def occupancy_from(m, sizes):
    """The four formulas on the cell shares m [B, C, Hc, Wc] (any float dtype) of the groups `sizes` -> {"occupancy", "any" [G, C, Hc, Wc],
    "conflict" [G, C], "risk" [B, C]}.  The sums (and the product) over each group's rows are taken row by row in row order."""
    Bn = m.shape[0]
    sizes = [int(s) for s in sizes]
    assert sum(sizes) == Bn and all(s >= 0 for s in sizes)
    G = len(sizes)
    gi = torch.repeat_interleave(torch.arange(G), torch.tensor(sizes))      # the group of every row
    D = torch.zeros((G,) + tuple(m.shape[1:]), dtype=m.dtype).index_add_(0, gi, m)
    S2 = torch.zeros_like(D).index_add_(0, gi, m * m)
    Q = torch.ones_like(D)
    first = torch.cumsum(torch.tensor([0] + sizes[:-1]), 0)
    for j in range(max(sizes)):      # the j-th agent of every group that has one
        has = torch.tensor([s > j for s in sizes])
        Q[has] = Q[has] * (1.0 - m[first[has] + j])
    return {"occupancy": D, "any": 1.0 - Q, "conflict": 0.5 * (D * D - S2).sum(dim=(2, 3)), "risk": (m * (D[gi] - m)).sum(dim=(2, 3))}


def occupancy_ref(x, sizes, cell, T, dtype=torch.float64):
    """The four results in stock torch at `dtype`."""
    return occupancy_from(cell_shares(x, cell, T, dtype), sizes)


def _errors(r32, r64):
    out = {}
    for k in OUTPUTS:
        d = (r32[k].double() - r64[k]).abs()[torch.isfinite(r64[k])]
        out[k] = float(d.max()) if d.numel() else 0.0
    return out


def e32(x, sizes, cell, T):
    """{output: the largest error of the fp32 restatement against its own fp64 run (finite entries)}"""
    return _errors(occupancy_ref(x, sizes, cell, T, torch.float32), occupancy_ref(x, sizes, cell, T))


def cases(si):
    """The cases of SHAPES[si]: every cell edge with every layout; the logit kind rotates so that every kind meets every cell edge and
    every layout over the table -> [(cell, layout index, kind)]"""
    return [(cell, li, (ci + li + si) % len(KINDS)) for ci, cell in enumerate(CELLS) for li in range(len(LAYOUTS))]


@functools.lru_cache(maxsize=None)
def _input(si, li, kind):
    (H, W), _, _ = SHAPES[si]
    return logits(sum(LAYOUTS[li]), H, W, kind)


@functools.lru_cache(maxsize=None)
def case(si, cell, li, kind):
    """-> (x [B, C, H, W], sizes, T, fp64 reference) of SHAPES[si] at `cell`, LAYOUTS[li], KINDS[kind]; computed once, shared, never
    written to"""
    x, T = _input(si, li, kind), KINDS[kind][1]
    return x, LAYOUTS[li], T, occupancy_ref(x, LAYOUTS[li], cell, T)


def case_e32(si, cell, li, kind):
    """the fp32 restatement's errors on `case(si, cell, li, kind)`"""
    x, sizes, T, r64 = case(si, cell, li, kind)
    return _errors(occupancy_ref(x, sizes, cell, T, torch.float32), r64)


def bound(ref, e):
    """The device bound per entry: 2 * E32 + 2^-21 * max(1, |ref|)"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref.abs(), min=1.0)


def shape_e32(H, W):
    for (h, w), _, e in SHAPES:
        if (h, w) == (H, W):
            return e
    raise KeyError((H, W))


# ------------------------------------------------------------------------------------------------
# known answers
# ------------------------------------------------------------------------------------------------
def cell_pixels(H, W, cell):
    """[Hc, Wc] fp64: the pixels of the map inside every cell"""
    Hc, Wc = -(-H // cell), -(-W // cell)
    rows = torch.clamp(H - torch.arange(Hc) * cell, max=cell).double()
    cols = torch.clamp(W - torch.arange(Wc) * cell, max=cell).double()
    return rows.view(Hc, 1) * cols.view(1, Wc)


def constant_planes(n, H, W, cell, value=0.7):
    """n identical constant planes, one group, one step -> (x [n, 1, H, W], T, closed forms): every agent has m = (pixels in the cell) /
    HW, so occupancy = n m, any = 1 - (1 - m)^n, conflict = n (n - 1) / 2 * sum m^2, risk = (n - 1) * sum m^2"""
    m = cell_pixels(H, W, cell) / (H * W)
    s2 = float((m * m).sum())
    want = {"occupancy": (n * m)[None, None], "any": (1.0 - (1.0 - m) ** n)[None, None],
            "conflict": torch.full((1, 1), n * (n - 1) / 2 * s2, dtype=torch.float64),
            "risk": torch.full((n, 1), (n - 1) * s2, dtype=torch.float64)}
    return torch.full((n, 1, H, W), value), 1.3, want


def disjoint_halves(H, W, kind=1):
    """Two agents whose finite logits lie in disjoint halves of the map, -inf elsewhere (H a multiple of 16: the halves meet on a cell
    boundary at every cell edge) -> (x [2, C, H, W], T): no cell holds weight of both, so conflict and risk are 0 exactly"""
    assert H % 16 == 0
    x = logits(2, H, W, kind, 600)
    x[0, :, H // 2:] = -float("inf")
    x[1, :, :H // 2] = -float("inf")
    return x, KINDS[kind][1]


# ------------------------------------------------------------------------------------------------
# the edge rules
# ------------------------------------------------------------------------------------------------
EDGE_SHAPES = L.EDGE_SHAPES               # vector path / element-wise path
EDGE_SIZES = [3, 2]
EDGE_BAD = [(0, 0), (0, 2)]               # (group, step) poisoned: by a NaN logit, by a plane of -inf alone


def edge_scene(H, W):
    """Two groups (3 and 2 agents), C = 3 steps, on _likelihood_cases.edge_planes' planes -> (x_bad, x_clean [5, 3, H, W], sizes, T).
    In x_bad agent 1 of group 0 has the NaN plane at step 0 and agent 2 of group 0 the all -inf plane at step 2; x_clean has ordinary
    planes there.  Agent 0 carries the row of -inf, the two -inf pixels and +inf beside -inf (ordinary results)."""
    planes, _, T = L.edge_planes(H, W)
    planes = planes[0]
    name = {n: i for i, n in enumerate(L.EDGE_PLANES)}
    clean = torch.randn(5, C, H, W, generator=_gen(300, H, W)) * 2.0
    clean[0, 0] = planes[name["minus_inf_elsewhere"]]
    clean[0, 1] = planes[name["gt_on_minus_inf"]]
    clean[0, 2] = planes[name["plus_and_minus_inf"]]
    bad = clean.clone()
    bad[1, 0] = planes[name["nan"]]
    bad[2, 2] = planes[name["all_minus_inf"]]
    assert bool(torch.isnan(bad[1, 0]).any()) and bool((bad[2, 2] == -float("inf")).all())
    return bad, clean, EDGE_SIZES, T


# ------------------------------------------------------------------------------------------------
# other layouts
# ------------------------------------------------------------------------------------------------
def many_groups():
    """70000 groups of one 2 x 2 plane each (more than 65535 workgroups along blockIdx.x) -> (x [70000, 1, 2, 2], sizes, T)"""
    x, _, T = L.many_planes()
    return x.reshape(70000, 1, 2, 2), [1] * 70000, T


def sliced(H, W):
    """A 5-channel tensor whose channels 1:3 are read in place -> (x5 [2, 5, H, W], T)"""
    x5, _, T = L.sliced(H, W)
    return x5, T


def production():
    """One (256, 256) case with 32 agents, C = 2, cell 4: trained-looking maps -> (x [32, 2, 256, 256], sizes, cell, T)"""
    return logits(32, 256, 256, 4, 700)[:, :2].contiguous(), [32], 4, KINDS[4][1]

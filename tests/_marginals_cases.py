"""Seeded inputs and the fp64 restatement for the tests of ynet_map_marginals / ops.map_marginals / utils/marginals.py
(tests/test_marginals_host.py checks this table on the CPU, tests/test_gpu_marginals.py runs the kernel against it).

The reference is stock torch on .double() inputs (`marginals_ref`), never the code under test.  Per plane, with z = x / T,
w = sigmoid(z), Z = sum w and g the ground truth rounded half-even ((x, y) = (column, row); it need not lie inside the map):
    col = (sum over rows of w) / Z,  row = (sum over columns of w) / Z,
    F(t) = cumsum(the axis' sums)(t) / Z on the pixel grid, 0 below the map, 1 from its last bin on,
    crps = sum_{t < g} F(t)^2 + sum_{t >= g} (1 - F(t))^2 over all integers t (outside the map every term is 0 or 1: k pixels outside add k),
    pit = (F(g - 1), F(g)).
Run in fp32 the same code is the yardstick of the device test: E32 is its largest error against its own fp64 run, and the device bound
per entry is 2 * E32 + 2^-21 * max(1, |ref|), plus the truncation of the kernel's fixed-point sums: n * 2^-39 for col, row and pit, and
2 * side * n * 2^-39 for crps (n = H * W).  Re-derived: with 40 fraction bits the largest weight of a plane is at least 2^40 units and
every pixel drops less than one, so the integer total N and the true scaled total S obey 0 <= S - N < n <= n * 2^-40 * N, and a bin's
(or a run of bins') integer sum a and true sum A obey 0 <= A - a < n.  Then a / N <= A / N <= (A / S) (1 + n * 2^-40) and a / N >=
(A - n) / S >= A / S - n * 2^-40: a share and a CDF value move by less than n * 2^-40, half of what the header grants (its n * 2^-39 also
covers 1 / (1 - n * 2^-40)).  The bound below keeps the header's looser figure.  crps: at most `side` in-map terms F^2 or (1 - F)^2,
each moving by at most 2 dF (0 <= F <= 1), so by less than 2 * side * n * 2^-39."""
import functools

import torch

import _likelihood_cases as LC
import _radial_cases as RC

OUTPUTS = ("col", "row", "crps", "pit")
B, C = LC.B, LC.C
KINDS = LC.KINDS                 # the five logit kinds of the likelihood table, with their temperatures
GT_MARGIN = 16384                # YNET_MAP_MARGINALS_GT_MARGIN
MAX_SIDE = 2048                  # YNET_MAP_MARGINALS_MAX_SIDE

# ------------------------------------------------------------------------------------------------
# (H, W) -> the walk of the kernel the shape exists for.  Third field: E32 per output = the largest error of `marginals_ref` run in fp32
# against its own fp64 run over the logit kinds, measured on the CPU (tests/test_marginals_host.py re-measures it and holds the table to
# it) and rounded up to three digits.
# ------------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 1), "scalar path, one element", {"col": 0.0, "row": 0.0, "crps": 0.0, "pit": 0.0}),
    ((1, 3), "scalar path, one row", {"col": 9.33e-08, "row": 0.0, "crps": 2.12e-07, "pit": 4.08e-08}),
    ((5, 4), "vector path, W = 4: one row per lane, 5 of 256 lanes busy", {"col": 1.07e-07, "row": 6.89e-08, "crps": 4.03e-07, "pit": 1.03e-07}),
    ((3, 64), "W = 64: 4 rows per wave, 48 of 256 lanes busy", {"col": 4.50e-08, "row": 1.01e-07, "crps": 5.09e-06, "pit": 1.09e-07}),
    ((6, 16), "W = 16: 16 rows per wave", {"col": 1.09e-07, "row": 1.14e-07, "crps": 1.55e-06, "pit": 2.16e-07}),
    ((9, 256), "one row per wave, odd row count: the tail loop only", {"col": 1.27e-08, "row": 2.86e-08, "crps": 2.12e-05, "pit": 1.69e-07}),
    ((2, 1024), "one row per workgroup pass: every lane of a pass on one row bin", {"col": 4.03e-09, "row": 9.30e-08, "crps": 1.35e-04, "pit": 6.60e-08}),
    ((7, 12), "vector path, W does not divide 1024: a wave ends inside a row", {"col": 1.48e-07, "row": 1.72e-07, "crps": 7.54e-07, "pit": 2.18e-07}),
    ((17, 23), "W % 4 != 0, 391 elements: planes after the first start off a 16-byte boundary", {"col": 9.76e-08, "row": 2.64e-07, "crps": 3.75e-06, "pit": 2.91e-07}),
    ((2, 2048), "W > 1024 (the side cap): eight bins per thread in the scan", {"col": 2.21e-09, "row": 8.56e-08, "crps": 1.04e-04, "pit": 1.27e-07}),
    ((96, 160), "3840 vectors: the unrolled loop, then the tail", {"col": 2.83e-08, "row": 4.22e-08, "crps": 8.33e-06, "pit": 1.32e-07}),
    ((256, 256), "the production size: unrolled loop only", {"col": 2.57e-08, "row": 1.57e-08, "crps": 1.69e-05, "pit": 1.34e-07}),
    ((512, 512), "configuration C4: two waves per row", {"col": 9.64e-09, "row": 6.67e-09, "crps": 5.01e-05, "pit": 8.12e-08}),
]

logits = LC.logits
positions = RC.positions          # corners, centre, both half-way roundings, one valid position outside the map
ground_truth = RC.ground_truth


def rounded(gt, H, W):
    """-> (g [.., 2] int64 (x, y), valid [..]: finite and at most GT_MARGIN pixels outside the map; g = 0 where not)"""
    g = torch.round(gt.double())                            # half to even
    valid = torch.isfinite(g).all(dim=-1) & (g[..., 0] >= -GT_MARGIN) & (g[..., 0] <= W - 1 + GT_MARGIN) \
        & (g[..., 1] >= -GT_MARGIN) & (g[..., 1] <= H - 1 + GT_MARGIN)
    return torch.where(valid[..., None], g, torch.zeros_like(g)).long(), valid


def axis_scores(sums, Z, g, dtype):
    """One axis: sums [B, C, side] (the unnormalised marginal), Z [B, C], g [B, C] int64 -> (crps [B, C], pit [B, C, 2]) at `dtype`"""
    side = sums.shape[-1]
    one = Z / Z                                             # 1, or NaN for a plane with Z == 0 or a NaN
    F = sums.cumsum(dim=-1) / Z[..., None]
    F = torch.cat([F[..., :-1], one[..., None]], dim=-1)    # 1 from the last bin on, by definition
    t = torch.arange(side).view(1, 1, side)
    terms = torch.where(t < g[..., None], F * F, (1 - F) * (1 - F)).sum(dim=-1)
    outside = (g - side).clamp(min=0) + (-g).clamp(min=0)   # k pixels outside the map: k terms of 1
    crps = terms + outside.to(dtype)

    def cdf_at(k):                                          # F(k) for any integer k
        inside = F.gather(2, k.clamp(0, side - 1)[..., None])[..., 0]
        return torch.where(k < 0, 0 * one, torch.where(k >= side - 1, one, inside))
    return crps, torch.stack([cdf_at(g - 1), cdf_at(g)], dim=-1)


def marginals_ref(x, gt, T, dtype=torch.float64):
    """The four outputs in stock torch at `dtype` -> {"col" [B, C, W], "row" [B, C, H], "crps" [B, C, 2], "pit" [B, C, 2, 2]} at `dtype`;
    gt None: col and row alone.  A NaN logit, or Z == 0, makes a plane NaN by itself (NaN sums, 0 / 0); a ground truth that is not finite
    or more than GT_MARGIN pixels outside the map makes crps and pit NaN by the rule, and leaves col and row alone."""
    raw = x.float()
    Bn, Cn, H, W = raw.shape
    w = torch.sigmoid(raw.to(dtype) / T)
    Z = w.sum(dim=(2, 3))
    cs, rs = w.sum(dim=2), w.sum(dim=3)
    out = {"col": cs / Z[..., None], "row": rs / Z[..., None]}
    if gt is None:
        return out
    g, valid = rounded(gt, H, W)
    cx, px = axis_scores(cs, Z, g[..., 0], dtype)
    cy, py = axis_scores(rs, Z, g[..., 1], dtype)
    nan = torch.full((), float("nan"), dtype=dtype)
    out["crps"] = torch.where(valid[..., None], torch.stack([cx, cy], dim=-1), nan)
    out["pit"] = torch.where(valid[..., None, None], torch.stack([px, py], dim=-2), nan)
    return out


def e32(x, gt, T):
    """{output: the largest error of the fp32 restatement against its own fp64 run (finite entries)}"""
    r64, r32 = marginals_ref(x, gt, T), marginals_ref(x, gt, T, torch.float32)
    out = {}
    for k in r64:
        d = (r32[k].double() - r64[k]).abs()
        d = d[torch.isfinite(r64[k])]
        out[k] = float(d.max()) if d.numel() else 0.0
    return out


@functools.lru_cache(maxsize=None)
def case(si, kind):
    """-> (x [B, C, H, W], gt [B, C, 2], T, fp64 reference) of SHAPES[si], KINDS[kind]; computed once, shared, never written to"""
    (H, W), _, _ = SHAPES[si]
    x, gt, T = logits(H, W, kind), ground_truth(H, W, kind), KINDS[kind][1]
    return x, gt, T, marginals_ref(x, gt, T)


def truncation(key, H, W):
    """What the kernel's fixed-point sums may move an entry by (the module docstring): per output [..., axis] where the axes differ"""
    n = H * W
    if key == "crps":
        return torch.tensor([2.0 * W * n * 2.0 ** -39, 2.0 * H * n * 2.0 ** -39], dtype=torch.float64)
    return n * 2.0 ** -39


def bound(ref, e, key, H, W):
    """The device bound per entry: 2 * E32 + 2^-21 * max(1, |ref|) + the truncation"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref.abs(), min=1.0) + truncation(key, H, W)


def shape_e32(H, W):
    for (h, w), _, e in SHAPES:
        if (h, w) == (H, W):
            return e
    raise KeyError((H, W))


# ------------------------------------------------------------------------------------------------
# exact inputs: logits in {0, 40} have the fp32 weights 0.5 and 1 exactly, every sum of them is exact in fp64 and in the kernel's
# integers, and every share and CDF value is ONE correctly rounded fp64 quotient of the same two numbers on both sides, so col, row and
# pit of the device must be the fp32 roundings of the restatement's, bit for bit
# ------------------------------------------------------------------------------------------------
EXACT_SHAPES = [(5, 4), (6, 16), (17, 23), (9, 256), (256, 256)]


def exact_planes(H, W, channels=C):
    """-> (x [B, channels, H, W] of 0 / 40, a quarter of them 40; gt [B, channels, 2] inside the map, T = 1)"""
    return RC.exact_planes(H, W, channels)


# ------------------------------------------------------------------------------------------------
# closed forms: a one-hot plane (one pixel of weight, everything else -inf) and a plane of two equal masses
# ------------------------------------------------------------------------------------------------
CLOSED_MAP = (6, 16)             # (H, W)


def one_hot_planes():
    """-> (x [1, 5, H, W], gt, T = 1, a = (col, row) of the mass): the ground truth at a, right of / below it, left of / above it, and
    5 pixels outside the map on the left / 4 below it"""
    H, W = CLOSED_MAP
    a = (9, 2)
    gts = [(9.0, 2.0), (13.0, 4.0), (3.0, 0.0), (-5.0, 2.0), (9.0, H + 3.0)]
    x = torch.full((1, len(gts), H, W), float("-inf"))
    x[0, :, a[1], a[0]] = 0.3
    return x, torch.tensor(gts).view(1, len(gts), 2), 1.0, a


def two_mass_planes():
    """-> (x [1, 3, H, W], gt, T = 1, (a, b) columns of two equal masses in one row): g = a, between, and b"""
    H, W = CLOSED_MAP
    a, b, r = 3, 11, 4
    gts = [(float(a), float(r)), (6.0, float(r)), (float(b), float(r))]
    x = torch.full((1, len(gts), H, W), float("-inf"))
    x[0, :, r, a] = 0.0
    x[0, :, r, b] = 0.0
    return x, torch.tensor(gts).view(1, len(gts), 2), 1.0, (a, b, r)


# ------------------------------------------------------------------------------------------------
# the plane-level rules: planes of one launch on logits N(0, 2^2) (the radial table's planes)
# ------------------------------------------------------------------------------------------------
RULE_SHAPES = RC.RULE_SHAPES      # vector path / element-wise path (both in SHAPES)
RULE_PLANES = RC.RULE_PLANES
rule_planes = RC.rule_planes

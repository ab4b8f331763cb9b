"""Seeded inputs and the fp64 restatement for the tests of ynet_map_radial / ops.map_radial / utils/radial.py
(tests/test_radial_host.py checks this table on the CPU, tests/test_gpu_radial.py runs the kernel against it).

The reference is stock torch on .double() inputs (`radial_ref`), never the code under test.  Per plane, with z = x / T,
w = sigmoid(z), Z = sum w, g the ground truth rounded half-even ((x, y) = (column, row); it need not lie inside the map) and the
integer d2 = (col - g.x)^2 + (row - g.y)^2 with its ring k = floor(sqrt(d2)), corrected in integers:
    ring[k] = (sum over {ring == k} of w) / Z,  tail = (sum over {ring >= n_rings} of w) / Z,
    mean = (sum w sqrt(d2)) / Z,  mean_sq = (sum w d2) / Z.
Run in fp32 the same code is the yardstick of the device test: E32 is its largest error against its own fp64 run, and the device bound
is 2 * E32 + 2^-21 * max(1, |ref|), for ring and tail plus the truncation of the kernel's fixed-point sums, n * 2^-40 (n = H * W
pixels, each dropping less than 2^-40 of the plane's largest weight <= Z)."""
import functools
import math

import torch

import _likelihood_cases as LC

OUTPUTS = ("ring", "tail", "mean", "mean_sq")
B, C = LC.B, LC.C
KINDS = LC.KINDS                 # the five logit kinds of the likelihood table, with their temperatures
GT_MARGIN = 16384                # YNET_MAP_RADIAL_GT_MARGIN
MAX_RINGS = 1024                 # YNET_MAP_RADIAL_MAX_RINGS


def default_rings(H, W):
    """min(1024, ceil(hypot(H, W)) + 1): no in-map ground truth leaves a tail"""
    return min(MAX_RINGS, math.isqrt(H * H + W * W - 1) + 2)


# ------------------------------------------------------------------------------------------------
# (H, W) -> the walk of the kernel the shape exists for (the likelihood table's meaning).  Third field: E32 per output = the largest
# error of `radial_ref` run in fp32 against its own fp64 run over the logit kinds and ring counts below, measured on the CPU
# (tests/test_radial_host.py re-measures it and holds the table to it) and rounded up to three digits.
# ------------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 1), "scalar path, one element", {"ring": 0.0, "tail": 0.0, "mean": 1.92e-07, "mean_sq": 1.91e-06}),
    ((1, 3), "scalar path, one row", {"ring": 7.51e-08, "tail": 7.51e-08, "mean": 5.02e-07, "mean_sq": 4.04e-06}),
    ((5, 4), "5 vectors: idle threads", {"ring": 1.02e-07, "tail": 1.07e-07, "mean": 1.11e-06, "mean_sq": 5.41e-06}),
    ((17, 23), "W % 4 != 0, 391 elements: planes after the first start off a 16-byte boundary", {"ring": 1.47e-07, "tail": 1.92e-07, "mean": 2.57e-06, "mean_sq": 4.28e-05}),
    ((90, 12), "270 vectors: the tail loop only", {"ring": 3.31e-08, "tail": 2.20e-07, "mean": 6.04e-06, "mean_sq": 1.23e-03}),
    ((96, 160), "3840 vectors: the unrolled loop, then the tail", {"ring": 6.67e-08, "tail": 1.42e-07, "mean": 1.59e-05, "mean_sq": 1.40e-03}),
    ((256, 256), "the production size: unrolled loop only", {"ring": 9.90e-08, "tail": 9.98e-08, "mean": 3.76e-05, "mean_sq": 7.07e-03}),
    ((512, 512), "configuration C4", {"ring": 4.87e-07, "tail": 1.05e-07, "mean": 8.62e-05, "mean_sq": 4.26e-02}),
]


def ring_counts(H, W):
    """The n_rings every case runs at: 1, 3 (a tail wherever the map is larger), the default, and the cap on the largest map"""
    out = [1, 3, default_rings(H, W)]
    if (H, W) == (512, 512):
        out.append(MAX_RINGS)
    return list(dict.fromkeys(out))


logits = LC.logits


def positions(H, W):
    """Ground-truth positions (x, y) -> the pixel they round to (col, row): the four corners, the centre, the half-way roundings
    2.5 -> 2 and 3.5 -> 4 (half to even) where the map is wide enough, and (-3.4, H + 2): outside the map, and valid.  Duplicates of a
    tiny plane dropped, order kept."""
    pos = [((0.0, 0.0), (0, 0)), ((W - 1.0, 0.0), (W - 1, 0)), ((0.0, H - 1.0), (0, H - 1)), ((W - 1.0, H - 1.0), (W - 1, H - 1)),
           ((float(W // 2), float(H // 2)), (W // 2, H // 2))]
    if W >= 5:
        pos += [((2.5, min(2.5, H - 1.0)), (2, min(2, H - 1))), ((3.5, min(3.5, H - 1.0)), (4, min(4, H - 1)))]
    pos += [((-3.4, H + 2.0), (-3, H + 2))]
    seen, out = set(), []
    for xy, px in pos:
        if px not in seen:
            seen.add(px)
            out.append((xy, px))
    return out


def ground_truth(H, W, kind):
    """[B, C, 2] fp32 (x, y): plane p of kind k takes position (p + 3 k) of `positions`, so the kinds together visit every position"""
    pos = positions(H, W)
    gt = torch.empty(B, C, 2)
    for p in range(B * C):
        gt[p // C, p % C] = torch.tensor(pos[(p + 3 * kind) % len(pos)][0])
    return gt


def isqrt_tensor(d2):
    """floor(sqrt(d2)) of an int64 tensor, exact: the fp64 root is a first guess, corrected in integers"""
    k = torch.sqrt(d2.double()).long()
    k = k - (k * k > d2).long()
    return k + ((k + 1) * (k + 1) <= d2).long()


def squared_distances(gt, H, W):
    """-> (d2 [B, C, H, W] int64 from the rounded ground truth, valid [B, C]: finite and at most GT_MARGIN pixels outside the map)"""
    g = torch.round(gt.double())                            # half to even
    valid = torch.isfinite(g).all(dim=-1) & (g[..., 0] >= -GT_MARGIN) & (g[..., 0] <= W - 1 + GT_MARGIN) \
        & (g[..., 1] >= -GT_MARGIN) & (g[..., 1] <= H - 1 + GT_MARGIN)
    g = torch.where(valid[..., None], g, torch.zeros_like(g)).long()
    dy = torch.arange(H).view(1, 1, H, 1) - g[..., 1, None, None]
    dx = torch.arange(W).view(1, 1, 1, W) - g[..., 0, None, None]
    return dx * dx + dy * dy, valid


def radial_ref(x, gt, T, n_rings, dtype=torch.float64):
    """The four scores in stock torch at `dtype` -> {"ring" [B, C, n_rings], "tail", "mean", "mean_sq" [B, C]} at `dtype`.
    A NaN logit, or Z == 0, makes a plane NaN by itself (NaN sums, 0 / 0); a ground truth that is not finite or more than GT_MARGIN
    pixels outside the map makes it NaN by the rule."""
    raw = x.float()
    Bn, Cn, H, W = raw.shape
    w = torch.sigmoid(raw.to(dtype) / T)
    Z = w.sum(dim=(2, 3))
    d2, valid = squared_distances(gt, H, W)
    bins = isqrt_tensor(d2).clamp(max=n_rings)              # bin n_rings: the tail
    hist = torch.zeros(Bn, Cn, n_rings + 1, dtype=dtype).scatter_add_(2, bins.reshape(Bn, Cn, -1), w.reshape(Bn, Cn, -1))
    # (the tail as a masked sum, torch's pairwise one: with few rings it holds most of the map, and scatter_add's one-by-one fp32 sum of
    # 10^5 terms would make a yardstick of 10^-3 out of it)
    beyond = torch.where(bins == n_rings, w, torch.zeros((), dtype=dtype)).sum(dim=(2, 3))
    nan = torch.full((), float("nan"), dtype=dtype)
    out = {"ring": hist[..., :n_rings] / Z[..., None], "tail": beyond / Z,
           "mean": (w * torch.sqrt(d2.to(dtype))).sum(dim=(2, 3)) / Z, "mean_sq": (w * d2.to(dtype)).sum(dim=(2, 3)) / Z}
    return {k: torch.where(valid[..., None] if v.dim() == 3 else valid, v, nan) for k, v in out.items()}


def e32(x, gt, T, n_rings):
    """{output: the largest error of the fp32 restatement against its own fp64 run (finite entries)}"""
    r64, r32 = radial_ref(x, gt, T, n_rings), radial_ref(x, gt, T, n_rings, torch.float32)
    out = {}
    for k in r64:
        d = (r32[k].double() - r64[k]).abs()
        d = d[torch.isfinite(r64[k])]
        out[k] = float(d.max()) if d.numel() else 0.0
    return out


@functools.lru_cache(maxsize=None)
def case(si, kind):
    """-> (x [B, C, H, W], gt [B, C, 2], T, {n_rings: fp64 reference}) of SHAPES[si], KINDS[kind]; computed once, shared, never written to"""
    (H, W), _, _ = SHAPES[si]
    x, gt, T = logits(H, W, kind), ground_truth(H, W, kind), KINDS[kind][1]
    return x, gt, T, {R: radial_ref(x, gt, T, R) for R in ring_counts(H, W)}


def truncation(H, W):
    """What the kernel's fixed-point sums may drop from a share: n pixels, each less than 2^-40 of the largest weight"""
    return H * W * 2.0 ** -40


def bound(ref, e, key, H, W):
    """The device bound per entry: 2 * E32 + 2^-21 * max(1, |ref|), + n * 2^-40 for the shares"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref.abs(), min=1.0) + (truncation(H, W) if key in ("ring", "tail") else 0.0)


def shape_e32(H, W):
    for (h, w), _, e in SHAPES:
        if (h, w) == (H, W):
            return e
    raise KeyError((H, W))


# ------------------------------------------------------------------------------------------------
# exact inputs: logits in {0, 40} have the fp32 weights 0.5 and 1 exactly, every sum of them is exact in fp64 and in the kernel's
# integers, so ring, tail and mean_sq of the device must be the fp32 roundings of the restatement's, bit for bit
# ------------------------------------------------------------------------------------------------
def exact_planes(H, W, channels=C):
    """-> (x [B, channels, H, W] of 0 / 40, a quarter of them 40; gt [B, channels, 2] inside the map, T = 1)"""
    g = LC._gen(700, H, W, channels)
    x = torch.where(torch.rand(B, channels, H, W, generator=g) < 0.25, torch.tensor(40.0), torch.tensor(0.0))
    gt = torch.stack([torch.randint(0, W, (B, channels), generator=g), torch.randint(0, H, (B, channels), generator=g)], dim=-1).float()
    return x, gt, 1.0


# ------------------------------------------------------------------------------------------------
# ring edges: one pixel of weight, everything else -inf, at an offset (dx, dy) from g -> the ring that must hold all the mass.
# d2 = 25, 36, 49, 50 as given; 24, 35 and 48 are not sums of two squares (each has a prime factor = 3 mod 4 to an odd power), so no
# pixel is at those distances: the largest d2 below each square that IS one stands in (20, 34, 45).  The rings asked for are the same.
# ------------------------------------------------------------------------------------------------
RING_EDGES = [((2, 4), 20, 4), ((3, 4), 25, 5), ((3, 5), 34, 5), ((0, 6), 36, 6), ((3, 6), 45, 6), ((7, 0), 49, 7), ((1, 7), 50, 7)]
EDGE_MAP = (12, 16)              # (H, W); g = (2, 1)


def ring_edge_planes():
    """-> (x [1, len(RING_EDGES), H, W], gt, T = 1): plane i holds its only finite logit at g + RING_EDGES[i][0]"""
    H, W = EDGE_MAP
    x = torch.full((1, len(RING_EDGES), H, W), float("-inf"))
    gt = torch.empty(1, len(RING_EDGES), 2)
    for i, ((dx, dy), d2, _) in enumerate(RING_EDGES):
        assert dx * dx + dy * dy == d2
        gt[0, i] = torch.tensor([2.0, 1.0])
        x[0, i, 1 + dy, 2 + dx] = 0.3
    return x, gt, 1.0


# ------------------------------------------------------------------------------------------------
# the plane-level rules: planes of one launch on logits N(0, 2^2)
# ------------------------------------------------------------------------------------------------
RULE_SHAPES = [(5, 4), (17, 23)]          # vector path / element-wise path (both in SHAPES)
RULE_PLANES = ["plain", "nan_logit", "all_minus_inf", "gt_outside_valid", "gt_nan", "gt_inf", "gt_20000_away", "gt_at_the_margin"]


def rule_planes(H, W):
    """-> (x [1, P, H, W], gt [1, P, 2], T, which planes must raise the status flag)"""
    P = len(RULE_PLANES)
    x = torch.randn(1, P, H, W, generator=LC._gen(800, H, W)) * 2.0
    gt = torch.empty(1, P, 2)
    gt[0, :] = torch.tensor([1.0, 2.0])
    x[0, 1, H - 1, W - 2] = float("nan")
    x[0, 2] = float("-inf")
    gt[0, 3] = torch.tensor([-3.4, H + 2.0])
    gt[0, 4] = torch.tensor([float("nan"), 1.0])
    gt[0, 5] = torch.tensor([1.0, float("inf")])
    gt[0, 6] = torch.tensor([W - 1 + 20000.0, 0.0])
    gt[0, 7] = torch.tensor([-float(GT_MARGIN), H - 1.0 + GT_MARGIN])      # the farthest valid corner: d2 just below 2^31
    return x, gt, 1.5, [False, False, False, False, True, True, True, False]

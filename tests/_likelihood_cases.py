"""Seeded inputs and the fp64 restatement for the tests of ynet_map_likelihood / ops.map_likelihood (tests/test_likelihood_host.py
checks this table on the CPU, tests/test_gpu_likelihood.py runs the kernel against it).

The reference is stock torch on .double() inputs (`like_ref`), never the code under test.  Per plane, with z = x / T,
w = sigmoid(z), Z = sum w and g the ground-truth pixel (rounded half-even, (x, y) = (column, row)):
    nll = log Z - log_sigmoid(z_g),   entropy = log Z - (sum w log_sigmoid(z)) / Z,   hpd = (sum over {x >= x_g} of w) / Z
with membership decided on the raw fp32 logits.  Run in fp32 the same code is the yardstick of the device test: E32 is its largest
error against its own fp64 run, and the device bound is 2 * E32 + 2^-21 * max(1, |ref|) (four fp32 ulps of the stored result)."""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20241123
OUTPUTS = ("nll", "entropy", "hpd")
B, C = 2, 3


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


# ------------------------------------------------------------------------------------------------
# (H, W) -> the walk of the kernel the shape exists for.  Third field: E32 per output = the largest error of `like_ref` run in fp32
# against its own fp64 run over the logit kinds below, measured on the CPU (tests/test_likelihood_host.py re-measures it and holds
# the table to it) and rounded up to three digits.
# ------------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 1), "scalar path, one element", {"nll": 5.97e-08, "entropy": 5.97e-08, "hpd": 0.0}),
    ((1, 3), "scalar path, one row", {"nll": 8.35e-07, "entropy": 5.42e-07, "hpd": 7.51e-08}),
    ((5, 4), "5 vectors: idle threads", {"nll": 5.73e-07, "entropy": 3.32e-07, "hpd": 6.62e-08}),
    ((17, 23), "W % 4 != 0, 391 elements: planes after the first start off a 16-byte boundary", {"nll": 1.08e-06, "entropy": 4.40e-07, "hpd": 1.59e-07}),
    ((90, 12), "270 vectors: the tail loop only", {"nll": 7.27e-07, "entropy": 3.87e-07, "hpd": 1.49e-07}),
    ((96, 160), "3840 vectors: the unrolled loop, then the tail", {"nll": 1.02e-06, "entropy": 8.30e-07, "hpd": 1.57e-07}),
    ((256, 256), "the production size: unrolled loop only", {"nll": 1.71e-06, "entropy": 8.22e-07, "hpd": 1.70e-07}),
    ((512, 512), "configuration C4", {"nll": 1.60e-06, "entropy": 1.06e-06, "hpd": 1.03e-07}),
]
KINDS = [          # (name, temperature)
    ("N(0, 0.5^2)", 1.0),
    ("N(0, 8^2)", 1.0),
    ("N(0, 3^2) - 10", 1.8),
    ("N(0, 3^2) + 20, saturated", 0.7),
    ("trained-looking: background -12, a Gaussian bump of +14, noise 0.05", 1.0),
]


def logits(H, W, kind):
    """[B, C, H, W] fp32 logits of KINDS[kind]"""
    g = _gen(100 + kind, H, W)
    n = torch.randn(B, C, H, W, generator=g)
    if kind == 0:
        return n * 0.5
    if kind == 1:
        return n * 8.0
    if kind == 2:
        return n * 3.0 - 10.0
    if kind == 3:
        return n * 3.0 + 20.0
    cy = torch.rand(B, C, 1, 1, generator=g) * (H - 1)
    cx = torch.rand(B, C, 1, 1, generator=g) * (W - 1)
    yy = torch.arange(H, dtype=torch.float32).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float32).view(1, 1, 1, W)
    s = max(1.0, 0.04 * max(H, W))
    return -12.0 + 14.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.05 * n


def positions(H, W):
    """Ground-truth positions (x, y) -> the pixel they must hit (col, row): the four corners, the last 16-byte vector of row 0, the first
    vector of row 1, and the half-way roundings 2.5 -> 2 and 3.5 -> 4 (half to even) where the map is wide enough.  Duplicates of a tiny
    plane dropped, order kept."""
    pos = [((0.0, 0.0), (0, 0)), ((W - 1.0, 0.0), (W - 1, 0)), ((0.0, H - 1.0), (0, H - 1)), ((W - 1.0, H - 1.0), (W - 1, H - 1)),
           ((max(W - 4, 0) + 0.25, -0.25), (max(W - 4, 0), 0)), ((0.0, min(1, H - 1) + 0.0), (0, min(1, H - 1)))]
    if W >= 5:
        pos += [((2.5, min(2.5, H - 1.0)), (2, min(2, H - 1))), ((3.5, min(3.5, H - 1.0)), (4, min(4, H - 1)))]
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


def like_ref(x, gt, T, dtype=torch.float64):
    """The three scores in stock torch at `dtype` -> {"nll", "entropy", "hpd"}, each [B, C] at `dtype`.  gt None: entropy alone.
    A NaN logit, or Z == 0, makes a plane NaN by itself (NaN sums, -inf - -inf, 0 / 0); a ground truth outside the map (or NaN)
    makes nll and hpd NaN."""
    raw = x.float()
    xd = raw.to(dtype)
    z = xd / T
    w = torch.sigmoid(z)
    ls = F.logsigmoid(z)                                    # min(z, 0) - log1p(exp(-|z|))
    zero = torch.zeros((), dtype=dtype)
    Z = w.sum(dim=(2, 3))
    logZ = torch.log(Z)
    out = {"entropy": logZ - torch.where(w > 0, w * ls, zero).sum(dim=(2, 3)) / Z}      # (a weight of 0 adds 0, whatever its log)
    if gt is None:
        return out
    Bn, Cn, H, W = raw.shape
    g = torch.round(gt.double())                            # half to even
    inside = (g[..., 0] >= 0) & (g[..., 0] < W) & (g[..., 1] >= 0) & (g[..., 1] < H)
    gx = torch.where(inside, g[..., 0], torch.zeros_like(g[..., 0])).long()
    gy = torch.where(inside, g[..., 1], torch.zeros_like(g[..., 1])).long()
    bi, ci = torch.arange(Bn).view(-1, 1).expand(Bn, Cn), torch.arange(Cn).view(1, -1).expand(Bn, Cn)
    xg = raw[bi, ci, gy, gx]                                # the raw fp32 logit of the ground-truth pixel
    member = raw >= xg[:, :, None, None]                    # fp32 compare: the same set at every dtype
    nan = torch.full((), float("nan"), dtype=dtype)
    out["nll"] = torch.where(inside, logZ - F.logsigmoid(xg.to(dtype) / T), nan)
    out["hpd"] = torch.where(inside, torch.where(member, w, zero).sum(dim=(2, 3)) / Z, nan)
    return out


def e32(x, gt, T):
    """{"nll", "entropy", "hpd"} -> the largest error of the fp32 restatement against its own fp64 run (finite entries)"""
    r64, r32 = like_ref(x, gt, T), like_ref(x, gt, T, torch.float32)
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
    return x, gt, T, like_ref(x, gt, T)


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
def constant_plane(H, W, value=0.7):
    """-> (x [1, 1, H, W] constant, gt, T, closed form): every pixel has probability 1 / HW"""
    x = torch.full((1, 1, H, W), value)
    gt = torch.tensor([[[W - 1.0, 0.0]]])
    n = math.log(H * W)
    return x, gt, 1.3, {"nll": n, "entropy": n, "hpd": 1.0}


def spike_planes(H, W):
    """-> (x [1, 2, H, W]: one logit of +60 at the last pixel over a background of 0, gt [1, 2, 2]: plane 0 on the spike, plane 1 on
    pixel 0, T = 1, closed forms per plane) for a map of at least two pixels"""
    n = H * W
    assert n >= 2
    x = torch.zeros(1, 2, H, W)
    x[:, :, H - 1, W - 1] = 60.0
    gt = torch.tensor([[[W - 1.0, H - 1.0], [0.0, 0.0]]])
    s = 1.0 / (1.0 + math.exp(-60.0))
    ls = -math.log1p(math.exp(-60.0))
    Z = s + (n - 1) * 0.5
    ent = math.log(Z) - (s * ls + (n - 1) * 0.5 * math.log(0.5)) / Z
    want = {"nll": [math.log(Z) - ls, math.log(Z) - math.log(0.5)], "entropy": [ent, ent], "hpd": [s / Z, 1.0]}
    return x, gt, 1.0, want


# ------------------------------------------------------------------------------------------------
# the edge rules: planes of one launch, with what each must give
# ------------------------------------------------------------------------------------------------
EDGE_SHAPES = [(5, 4), (17, 23)]          # vector path / element-wise path (both in SHAPES)
EDGE_PLANES = ["nan", "minus_inf_elsewhere", "gt_on_minus_inf", "plus_and_minus_inf", "all_minus_inf", "gt_right_of_map", "gt_below_map",
               "gt_negative", "gt_nan", "gt_minus_0.4"]


def edge_planes(H, W):
    """-> (x [1, P, H, W], gt [1, P, 2], T) for EDGE_PLANES, on logits N(0, 2^2)"""
    P = len(EDGE_PLANES)
    x = torch.randn(1, P, H, W, generator=_gen(300, H, W)) * 2.0
    gt = torch.empty(1, P, 2)
    gt[0, :] = torch.tensor([1.0, 2.0])
    inf, nan = float("inf"), float("nan")
    x[0, 0, H - 1, W - 2] = nan                             # NaN anywhere: the whole plane is NaN
    x[0, 1, 0, :] = -inf                                    # a row of -inf, the ground truth elsewhere: ordinary results
    x[0, 2, 2, 1] = -inf                                    # the ground truth ON a -inf pixel: nll = +inf, hpd = 1
    x[0, 2, 0, 0] = -inf
    x[0, 3, 2, 1] = inf                                     # +inf is sigmoid = 1, also beside a -inf
    x[0, 3, 0, 0] = -inf
    x[0, 4] = -inf                                          # Z == 0: NaN
    gt[0, 5] = torch.tensor([W + 0.0, 0.0])                 # the first column right of the map
    gt[0, 6] = torch.tensor([0.0, H - 0.49])                # rounds to H: the first row below the map
    gt[0, 7] = torch.tensor([-0.6, 1.0])                    # rounds to -1
    gt[0, 8] = torch.tensor([nan, 1.0])
    gt[0, 9] = torch.tensor([-0.4, 1.0])                    # rounds to -0: inside
    return x, gt, 1.5


def edge_outside(H, W):
    """Which planes of `edge_planes` hold a ground truth outside the map"""
    out = [False] * len(EDGE_PLANES)
    out[5] = out[6] = out[7] = out[8] = True
    return out


# ------------------------------------------------------------------------------------------------
# other layouts
# ------------------------------------------------------------------------------------------------
def many_planes():
    """70000 planes of 2 x 2 (more than 65535 workgroups along blockIdx.x) -> (x [35000, 2, 2, 2], gt, T)"""
    g = _gen(400)
    x = torch.randn(35000, 2, 2, 2, generator=g) * 3.0
    gt = torch.randint(0, 2, (35000, 2, 2), generator=g).float()
    return x, gt, 1.8


def sliced(H, W):
    """A 5-channel tensor whose channels 1:3 are scored in place -> (x5 [2, 5, H, W], gt [2, 2, 2], T)"""
    g = _gen(500, H, W)
    x5 = torch.randn(2, 5, H, W, generator=g) * 4.0
    gt = torch.stack([torch.randint(0, W, (2, 2), generator=g), torch.randint(0, H, (2, 2), generator=g)], dim=-1).float()
    return x5, gt, 0.7

"""Seeded inputs and the fp64 restatement for the tests of ynet_map_credible / ops.map_credible (tests/test_credible_host.py checks this
table on the CPU, tests/test_gpu_credible.py runs the kernel against it).

The reference is numpy / stock torch in fp64 (`restate`, `share`), never the code under test.  Per plane, with z = x / T,
w = sigmoid(z), Z = sum w, and per level q (the fp32 level taken to fp64):
    threshold = the largest logit value t of the plane with (sum over {x >= t} of w) / Z >= q
    area = #{x >= threshold},   mass = (sum over {x >= threshold} of w) / Z
`restate` sorts the distinct values descending, takes the cumulative mass and count per value, and searches the first value whose
share reaches q.  The device bound on a share is
    delta = 2 * E32 + 2^-21 * max(1, |fp64|) + n * 2^-39
E32: the error of the same shares -- `share` at the restatement's thresholds -- taken in fp32 on the CPU against fp64, per shape;
2^-21: four fp32 ulps of the stored result (tests/_likelihood_cases.py, tests/_compliance_cases.py); n * 2^-39: the truncation of
the kernel's 40-bit fixed point over the n pixels of the plane, as include/ynet_hip.h derives it."""
import functools
import math

import numpy as np
import torch

SEED = 20250311
B, C = 2, 3
TEMPS = (1.0, 1.8)
LEVELS8 = (0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 0.999999)
LEVEL_SETS = {1: (0.9,), 5: (0.5, 0.9, 0.99, 0.999, 0.999999), 8: LEVELS8}      # (every set is part of LEVELS8: one restatement serves all)
MAX_LEVELS = 8
MAX_PIXELS = 1 << 22
FRAC_BITS = 40


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


# (H, W) -> E32, measured on one CPU over every kind, temperature and level of the table and rounded up to three digits
# (tests/test_credible_host.py re-measures it and holds the table to it, with the headroom the order of a stock-torch sum needs).
E32 = {
    (1, 1): 0.0,
    (1, 3): 8.13e-08,
    (5, 7): 1.53e-07,
    (17, 23): 1.72e-07,
    (64, 64): 1.64e-07,
    (255, 257): 2.00e-07,
    (256, 256): 1.63e-07,
    (512, 512): 2.04e-07,
}
SHAPES = [
    ((1, 1), "one pixel: the region is the plane"),
    ((1, 3), "one row, element-wise path"),
    ((5, 7), "35 pixels: idle threads, planes off a 16-byte boundary"),
    ((17, 23), "391 pixels, element-wise path"),
    ((64, 64), "1024 vectors: one per thread, the tail loop only"),
    ((255, 257), "odd size above the production size, element-wise path"),
    ((256, 256), "the production size: the unrolled loop"),
    ((512, 512), "Y-Net-Mod's maps"),
]
KINDS = ["N(0, 3^2)", "N(0, 8^2)", "N(-10, 3^2)", "integer grid -6 .. 6", "peaked bump with noise"]
CONTINUOUS = (0, 1, 2)      # kinds whose values are (nearly) all distinct: a level can fall near a boundary
GRID = 3


def logits(H, W, kind):
    """-> x [B, C, H, W] float32 of KINDS[kind]"""
    g = _gen(100 + kind, H, W)
    if kind == 0:
        return torch.randn(B, C, H, W, generator=g) * 3.0
    if kind == 1:
        return torch.randn(B, C, H, W, generator=g) * 8.0
    if kind == 2:
        return torch.randn(B, C, H, W, generator=g) * 3.0 - 10.0
    if kind == 3:
        return torch.randint(-6, 7, (B, C, H, W), generator=g).float()
    yy, xx = torch.arange(H).view(H, 1).float(), torch.arange(W).view(1, W).float()
    cy, cx = torch.rand(B, C, 1, 1, generator=g) * H, torch.rand(B, C, 1, 1, generator=g) * W
    s = max(1.0, 0.08 * max(H, W))
    return 14.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) - 8.0 + 0.5 * torch.randn(B, C, H, W, generator=g)


def levels32(levels):
    """the levels as the kernel takes them: fp32, then to fp64"""
    return np.asarray(levels, dtype=np.float32).astype(np.float64)


def _sigmoid64(z):
    with np.errstate(over="ignore"):
        return np.where(z >= 0, 1.0 / (1.0 + np.exp(-np.abs(z))), np.exp(-np.abs(z)) / (1.0 + np.exp(-np.abs(z))))


def restate_plane(x, levels, T):
    """One plane (any shape, float32) -> (area [L] int64, threshold [L] float32, mass [L] float64) in fp64."""
    q = levels32(levels)
    L = q.size
    x = np.asarray(x, dtype=np.float32).reshape(-1)
    nan = np.full(L, np.nan)
    if np.isnan(x).any():
        return np.full(L, -1, dtype=np.int64), nan.astype(np.float32), nan
    x = x + np.float32(0.0)      # -0.0 -> +0.0: one plateau
    w = _sigmoid64(x.astype(np.float64) / T)
    Z = w.sum()
    if not Z > 0:
        return np.zeros(L, dtype=np.int64), nan.astype(np.float32), nan
    vals, inv, cnt = np.unique(x, return_inverse=True, return_counts=True)      # ascending
    m = np.bincount(inv.reshape(-1), weights=w, minlength=vals.size)
    share = np.cumsum(m[::-1]) / Z      # descending values: the share of {x >= value}
    count = np.cumsum(cnt[::-1])
    area, thr, mass = np.empty(L, dtype=np.int64), np.empty(L, dtype=np.float32), np.empty(L)
    for l in range(L):
        hit = np.nonzero(share >= q[l])[0]
        i = int(hit[0]) if hit.size else int(np.nonzero(m[::-1] > 0)[0][-1])      # (rounding left the last share below q: every plateau with mass)
        area[l], thr[l], mass[l] = count[i], vals[::-1][i], share[i]
    return area, thr, mass


def restate(x, levels, T):
    """x [B, C, H, W] -> {"area" [B, C, L] int64, "threshold" float32, "mass" float64} (torch, host)"""
    xb = x.numpy()
    res = [[restate_plane(xb[b, c], levels, T) for c in range(xb.shape[1])] for b in range(xb.shape[0])]
    pick = lambda k: torch.from_numpy(np.stack([np.stack([r[k] for r in row]) for row in res]))
    return {"area": pick(0), "threshold": pick(1), "mass": pick(2)}


def share(x, thr, T, dtype=torch.float64, strict=False):
    """The share of {x >= thr} (strict: {x > thr}) in stock torch at `dtype`: x [B, C, H, W], thr [B, C, L] -> [B, C, L] at `dtype`"""
    w = torch.sigmoid(x.float().to(dtype) / T)
    Z = w.sum(dim=(2, 3))
    zero = torch.zeros((), dtype=dtype)
    out = []
    for l in range(thr.shape[-1]):
        t = thr[..., l, None, None]
        out.append(torch.where((x > t) if strict else (x >= t), w, zero).sum(dim=(2, 3)) / Z)
    return torch.stack(out, dim=-1)


def count_ge(x, thr):
    """#{x >= thr}: x [B, C, H, W], thr [B, C, L] -> [B, C, L] int64"""
    return torch.stack([(x >= thr[..., l, None, None]).sum(dim=(2, 3)) for l in range(thr.shape[-1])], dim=-1)


def is_logit_of(x, thr):
    """whether every threshold compares equal to a logit of its plane -> [B, C, L] bool"""
    return torch.stack([(x == thr[..., l, None, None]).any(dim=3).any(dim=2) for l in range(thr.shape[-1])], dim=-1)


def truncation(n):
    return n * 2.0 ** -39


def bound(ref, e, n):
    """delta per entry: 2 * E32 + 2^-21 * max(1, |ref|) + n * 2^-39"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref.abs(), min=1.0) + truncation(n)


def shape_e32(H, W):
    return E32[(H, W)]


@functools.lru_cache(maxsize=None)
def case(si, kind, ti):
    """-> (x [B, C, H, W], T, fp64 restatement at LEVELS8, fp64 share of {x >= threshold}, of {x > threshold}) of SHAPES[si], KINDS[kind],
    TEMPS[ti]; computed once, shared, never written to"""
    (H, W), _ = SHAPES[si]
    x = logits(H, W, kind)
    T = TEMPS[ti]
    ref = restate(x, LEVELS8, T)
    return x, T, ref, share(x, ref["threshold"], T), share(x, ref["threshold"], T, strict=True)


def case_e32(si, kind, ti):
    """the fp32 shares' error on `case(si, kind, ti)`"""
    x, T, ref, s64, _ = case(si, kind, ti)
    return float((share(x, ref["threshold"], T, torch.float32).double() - s64).abs().max())


def level_index(L):
    """where the levels of LEVEL_SETS[L] stand in LEVELS8"""
    return [LEVELS8.index(q) for q in LEVEL_SETS[L]]


def accept(x, T, levels, got, e32):
    """The acceptance of one launch, on host tensors: got = {"area", "threshold", "mass"} [B, C, L].  Asserts the properties that must
    hold for EVERY case and -> (fp64 share of {x >= threshold}, delta)."""
    q = torch.from_numpy(levels32(levels))
    n = x.shape[2] * x.shape[3]
    thr = got["threshold"]
    assert bool(is_logit_of(x, thr).all()), "a threshold is no logit of its plane"
    assert torch.equal(got["area"].long(), count_ge(x, thr)), "area != #{x >= threshold}"
    ge, gt = share(x, thr, T), share(x, thr, T, strict=True)
    d = bound(ge, e32, n)
    assert bool((ge >= q - d).all()), f"the region holds less than q: worst {float((q - ge).max()):.3e} against delta {float(d.max()):.3e}"
    assert bool((gt < q + d).all()), f"the region without its lowest plateau still holds q: worst {float((gt - q).max()):.3e}"
    err = (got["mass"].double() - ge).abs()
    assert bool((err <= d).all()), f"mass off by {float(err.max()):.3e} against delta {float(d.max()):.3e}"
    return ge, d


# ------------------------------------------------------------------------------------------------
# planted planes: (name, x [1, P, H, W], levels, T, expected {"area" [P, L], "threshold" [P, L]} or None where `restate` is the answer)
# ------------------------------------------------------------------------------------------------
def _f(bits):
    return np.array(bits, dtype=np.uint32).view(np.float32)


def two_valued(H, W, k, hi, lo, T=1.0):
    """k pixels at `hi`, the rest at `lo` -> (x [H, W], the share of the upper plateau in closed form)"""
    n = H * W
    x = torch.full((n,), float(lo))
    x[torch.randperm(n, generator=_gen(7, H, W, k))[:k]] = float(hi)
    s = lambda v: 1.0 / (1.0 + math.exp(-v / T))
    return x.view(H, W), k * s(hi) / (k * s(hi) + (n - k) * s(lo))


def planted():
    """-> list of (name, x [1, P, H, W], levels, T, closed-form areas [P, L] or None)"""
    out = []
    H, W = 17, 19      # 323 pixels: no level of LEVELS8 is a multiple of 1 / 323
    n = H * W
    g = _gen(300)
    # keys that differ only in the lowest digit: 256 neighbouring floats around 1.5, every one once, then repeated
    base = int(np.float32(1.5).view(np.uint32))
    lowest = torch.from_numpy(_f((base + (np.arange(n) % 256)).astype(np.uint32)).copy())[torch.randperm(n, generator=g)].view(1, 1, H, W)
    out.append(("lowest digit only", lowest, LEVELS8, 1.0, None))
    # keys that differ only in the highest digit: x and -x of one magnitude
    highest = torch.where(torch.rand(n, generator=g) < 0.3, 2.5, -2.5).view(1, 1, H, W)
    out.append(("highest digit only", highest, LEVELS8, 1.0, None))
    # keys that straddle a digit boundary: the floats just below and from 2.0 on (exponent change), and around +-0 / denormals
    b2 = int(np.float32(2.0).view(np.uint32))
    straddle = torch.from_numpy(_f((b2 - 160 + (np.arange(n) % 320)).astype(np.uint32)).copy())[torch.randperm(n, generator=g)].view(1, 1, H, W)
    out.append(("digit boundary", straddle, LEVELS8, 1.0, None))
    out.append(("constant", torch.full((1, 2, H, W), -3.25), LEVELS8, 1.8, np.full((2, 8), n)))
    # two values, the upper plateau just under / just over q = 0.5 at T = 1: hi = 0, lo = -log(3) => sigmoid 1/2 and 1/4; k upper pixels
    # hold 2k / (n + k) of the mass: k = n / 3 would be exactly q = 1/2, so k = 106 (0.4942) stays under and k = 109 (0.5046) goes over
    lo = -math.log(3.0)
    under, s_under = two_valued(H, W, 106, 0.0, lo)
    over, s_over = two_valued(H, W, 109, 0.0, lo)
    assert s_under < 0.5 - 1e-3 and s_over > 0.5 + 1e-3
    out.append(("two values around q", torch.stack([under, over])[None], (0.5,), 1.0, np.array([[n], [109]])))
    # one dominant pixel: sigmoid(40) against 322 pixels of sigmoid(-40): area 1 at every level
    dom = torch.full((n,), -40.0)
    dom[123] = 40.0
    out.append(("one dominant pixel", dom.view(1, 1, H, W), LEVELS8, 1.0, np.full((1, 8), 1)))
    # levels in one bin / in different bins of the first pass: values 1.0 .. 1.9 share sign and upper exponent bits, -1, 1, 40 do not
    same = (1.0 + 0.9 * torch.rand(n, generator=g)).view(1, 1, H, W)
    out.append(("levels in one first-pass bin", same, LEVELS8, 1.0, None))
    spread = torch.tensor([-1.0, 1.0, 3.0e-3, 40.0, -1.0e-3, 6.0e4, -7.0e5, 1.0e-20])[torch.randint(0, 8, (n,), generator=g)].view(1, 1, H, W)
    out.append(("levels in different first-pass bins", spread, LEVELS8, 30.0, None))
    # +-0.0 is one plateau: 100 of each over a background of -2 => sigmoid 1/2 x 200 against sigmoid(-2) x 123
    zeros = torch.full((n,), -2.0)
    idx = torch.randperm(n, generator=g)
    zeros[idx[:100]] = 0.0
    zeros[idx[100:200]] = -0.0
    out.append(("+-0.0", zeros.view(1, 1, H, W), (0.3, 0.8, 0.95), 1.0, np.array([[200, 200, n]])))
    # denormal logits are not flushed: three plateaus 1e-40 > 0 > -1e-40 of nearly equal weight
    den = torch.from_numpy(np.array([1e-40, 0.0, -1e-40], dtype=np.float32))[torch.arange(n) % 3].view(1, 1, H, W)
    c0 = int((torch.arange(n) % 3 == 0).sum())
    c1 = int((torch.arange(n) % 3 == 1).sum())
    out.append(("denormal logits", den, (0.2, 0.5, 0.9), 1.0, np.array([[c0, c0 + c1, n]])))
    # sigmoids in fp32's denormal range (z = -95: 5e-42) beside normal ones (z = -80): their share is below 1e-6 either way
    tiny = torch.where(torch.arange(n) % 2 == 0, -80.0, -95.0).view(1, 1, H, W)
    out.append(("sigmoid in the denormal range", tiny, (0.5, 0.9), 1.0, np.full((1, 2), (n + 1) // 2)))
    # +-inf pixels: +inf is weight 1 and the largest value, -inf is never a member
    infs = torch.randn(n, generator=g)
    infs[idx[:3]] = math.inf
    infs[idx[3:40]] = -math.inf
    out.append(("+-inf pixels", infs.view(1, 1, H, W), LEVELS8, 1.0, None))
    minus = torch.full((n,), -math.inf)
    minus[idx[:5]] = -3.0
    out.append(("-inf beside one plateau", minus.view(1, 1, H, W), (0.5, 0.999999), 1.0, np.full((1, 2), 5)))
    return out


def saturated():
    """a 512 x 512 plane of logits >= 30: every fp32 sigmoid rounds to 1, the integer sum is at its largest -> (x [1, 1, 512, 512], levels)"""
    x = 30.0 + 20.0 * torch.rand(1, 1, 512, 512, generator=_gen(400))
    return x, LEVELS8


def nan_among_clean(H=5, W=7):
    """-> x [2, 3, H, W]: plane (1, 0) holds one NaN, plane (0, 2) is all -inf, plane (1, 2) all -200 (every sigmoid is 0 in fp32)"""
    x = torch.randn(2, 3, H, W, generator=_gen(500)) * 3
    x[1, 0, H // 2, W // 3] = math.nan
    x[0, 2] = -math.inf
    x[1, 2] = -200.0
    return x


def many_planes():
    """70000 planes of 1 x 3 (more than 65535 workgroups along blockIdx.x) -> x [35000, 2, 1, 3]"""
    return torch.randn(35000, 2, 1, 3, generator=_gen(600)) * 3


def sliced(H=17, W=23):
    """A 5-channel tensor whose channels 1:3 are read in place: odd-sized planes off a 16-byte boundary -> x5 [2, 5, H, W]"""
    return torch.randn(2, 5, H, W, generator=_gen(700)) * 3

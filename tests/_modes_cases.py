"""Seeded inputs, planted planes and the CPU reference for the tests of ynet_map_modes / ops.map_modes / predict_modes
(tests/test_modes_host.py checks this table on the CPU, tests/test_gpu_modes.py runs the kernel against it).

The reference (`modes_ref`) is a plain greedy loop in NumPy / torch on the CPU, never the code under test.  Per plane: the candidates
are the pixels with x > -inf; mode m is the unsuppressed candidate with the largest raw fp32 logit (np.argmax: the first, i.e. the
smallest row * W + col, among equals; -0.0 == +0.0); it suppresses the disk drow^2 + dcol^2 <= radius^2 and claims
mass[m] = (sum of sigmoid(x / T) over the pixels it NEWLY suppressed) / (the sum over the plane).  The picks are made on the fp32 values,
so they are the same at every precision and are compared exactly; the sums are taken on .double() inputs.  Run on .float() inputs the
same sums are the yardstick of the device's masses: E32 is their largest error against the fp64 run, and the device bound is
2 * E32 + 2^-21 * max(1, |ref|) (the project's convention, tests/_likelihood_cases.py)."""
import functools

import numpy as np
import torch

import _likelihood_cases as LC

FILL_XY, FILL_LOGIT, FILL_MASS = -1.0, -np.inf, 0.0
N_MODES = [1, 2, 20, 64]
RADII = [0, 1, 3, 8]
M_MAX = 64


def over_radius(H, W):
    """a radius larger than the plane: the first disk holds every pixel, count must be 1"""
    return H + W


# ------------------------------------------------------------------------------------------------
# (H, W) -> the walk of the kernel the shape exists for, and E32 of the masses: the largest error of `modes_ref` run in fp32 against
# its own fp64 run over the logit kinds and radii below, measured on the CPU (tests/test_modes_host.py re-measures it and holds the
# table to it) and rounded up to three digits.  The first six shapes run every kind x radius; the last two once (kind 4, M 20, r 8).
# ------------------------------------------------------------------------------------------------
SHAPES = [
    ((1, 1), "one pixel", 0.0),
    ((1, 3), "one row, one partial segment", 9.33e-08),
    ((5, 4), "20 pixels: idle lanes", 1.31e-07),
    ((17, 23), "W % 4 != 0, 391 pixels: planes after the first start off a 16-byte boundary, two segments, the second partial", 2.26e-07),
    ((33, 70), "2310 pixels: ten segments, rows that straddle segments, ragged edges", 1.74e-07),
    ((96, 160), "60 segments: more than one pass of the waves over the table", 1.50e-07),
    ((256, 256), "the production size, once", 1.18e-07),
    ((512, 512), "configuration C4: the pixel cap, once", 2.68e-08),
]
FULL = 6                      # SHAPES[:FULL] run the whole cross of kinds and radii
ONCE = (4, 20, 8)             # (kind, n_modes, radius) of the two large shapes
KINDS = LC.KINDS              # the five logit kinds of the likelihood table, with their temperatures


def table():
    """-> [(shape index, kind, radius)]: every launch configuration of the table; n_modes runs over N_MODES for SHAPES[:FULL]"""
    out = []
    for si, ((H, W), _, _) in enumerate(SHAPES):
        if si < FULL:
            out += [(si, kind, r) for kind in range(len(KINDS)) for r in RADII + [over_radius(H, W)]]
        else:
            out.append((si, ONCE[0], ONCE[2]))
    return out


def table_modes(si):
    return N_MODES if si < FULL else [ONCE[1]]


# ------------------------------------------------------------------------------------------------
# the reference
# ------------------------------------------------------------------------------------------------
def _greedy(v, n_modes, radius):
    """One plane v [H, W] fp32 (NumPy) -> (count, [(row, col)], [flat indices of the pixels each mode newly suppressed]); count -1 for
    a plane that holds a NaN."""
    H, W = v.shape
    if np.isnan(v).any():
        return -1, [], []
    live = v > -np.inf
    sup = np.zeros((H, W), dtype=bool)
    picks, claimed = [], []
    r2 = int(radius) * int(radius)
    for _ in range(n_modes):
        cand = live & ~sup
        if not cand.any():
            break
        idx = int(np.argmax(np.where(cand, v, np.float32(-np.inf))))      # the first among equals: the smallest linear index
        row, col = divmod(idx, W)
        r0, r1, c0, c1 = max(row - radius, 0), min(row + radius, H - 1), max(col - radius, 0), min(col + radius, W - 1)
        rr = np.arange(r0, r1 + 1, dtype=np.int64)[:, None] - row
        cc = np.arange(c0, c1 + 1, dtype=np.int64)[None, :] - col
        disk = rr * rr + cc * cc <= r2
        new = disk & ~sup[r0:r1 + 1, c0:c1 + 1]
        nr, nc = np.nonzero(new)
        claimed.append((nr + r0) * W + (nc + c0))
        sup[r0:r1 + 1, c0:c1 + 1] |= disk
        picks.append((row, col))
    return len(picks), picks, claimed


def modes_ref(x, n_modes, radius, T, dtypes=(torch.float64,)):
    """x [B, C, H, W] fp32 -> {"xy" [B, C, M, 2] fp32 (column, row), "logit" [B, C, M] fp32, "count" [B, C] int32, "mass": one
    [B, C, M] tensor per entry of `dtypes`, the sums taken at that precision}; unfilled entries hold (-1, -1), -inf and 0."""
    x = x.float()
    B, C, H, W = x.shape
    xy = torch.full((B, C, n_modes, 2), FILL_XY)
    logit = torch.full((B, C, n_modes), FILL_LOGIT)
    count = torch.zeros((B, C), dtype=torch.int32)
    mass = [torch.zeros((B, C, n_modes), dtype=d) for d in dtypes]
    for b in range(B):
        for c in range(C):
            v = x[b, c].numpy()
            n, picks, claimed = _greedy(v, n_modes, radius)
            count[b, c] = n
            if n <= 0:
                continue
            for m, (row, col) in enumerate(picks):
                xy[b, c, m, 0], xy[b, c, m, 1] = float(col), float(row)
                logit[b, c, m] = x[b, c, row, col]
            for d, out in zip(dtypes, mass):
                w = torch.sigmoid(x[b, c].to(d) / T).reshape(-1)
                Z = w.sum()
                for m, idx in enumerate(claimed):
                    out[b, c, m] = w[torch.from_numpy(idx)].sum() / Z
    return {"xy": xy, "logit": logit, "count": count, "mass": mass}


def cut(ref, n_modes):
    """The reference for fewer modes: greedy picks do not depend on how many are still to come, so it is the prefix."""
    return {"xy": ref["xy"][:, :, :n_modes], "logit": ref["logit"][:, :, :n_modes], "count": ref["count"].clamp(max=n_modes),
            "mass": [m[:, :, :n_modes] for m in ref["mass"]]}


@functools.lru_cache(maxsize=None)
def case(si, kind, radius):
    """-> (x [B, C, H, W], T, reference at the largest n_modes of the shape with fp64 and fp32 masses); computed once, shared, never
    written to.  `cut` gives the reference of a smaller n_modes."""
    (H, W), _, _ = SHAPES[si]
    x, T = LC.logits(H, W, kind), KINDS[kind][1]
    return x, T, modes_ref(x, max(table_modes(si)), radius, T, (torch.float64, torch.float32))


def e32_of(ref):
    """the largest error of the fp32 masses of a reference against its fp64 masses"""
    return float((ref["mass"][1].double() - ref["mass"][0]).abs().max())


def bound(ref64, e):
    """The device bound per mass entry: 2 * E32 + 2^-21 * max(1, |ref|)"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref64.abs(), min=1.0)


def shape_e32(H, W):
    for (h, w), _, e in SHAPES:
        if (h, w) == (H, W):
            return e
    raise KeyError((H, W))


def bits(t):
    """fp32 values as their bit patterns: -0.0 and +0.0 differ, NaNs compare"""
    return t.detach().cpu().float().contiguous().view(torch.int32)


def disk_area(r):
    """A(r) = #{(dx, dy) : dx^2 + dy^2 <= r^2}, by counting"""
    d = np.arange(-r, r + 1, dtype=np.int64)
    return int((d[:, None] ** 2 + d[None, :] ** 2 <= r * r).sum())


# ------------------------------------------------------------------------------------------------
# planted planes: (name, x [1, P, H, W], n_modes, radius, T, what must come out: {"count": [...], "xy": {plane: [(col, row), ...]}})
# ------------------------------------------------------------------------------------------------
def _noise(H, W, key, scale=0.1, P=1):
    return torch.randn(1, P, H, W, generator=LC._gen(700, key, H, W)) * scale


def planted():
    out = []
    H, W = 17, 23
    inf = float("inf")
    # every pick a tie: pure row-major order under suppression.  After (0, 0) the first free pixel of row 0 is column r + 1.
    for r in (0, 3):
        out.append((f"constant r{r}", torch.full((1, 1, H, W), 0.7), 20, r, 1.3,
                    {"count": [20], "xy": {0: [(0, 0), (r + 1, 0), (2 * (r + 1), 0)]}}))
    # two equal maxima at distance^2 = r^2 (the second is suppressed) and at r^2 + 1 (it is kept)
    r = 3
    x = _noise(H, W, 1)
    x[0, 0, 5, 5] = x[0, 0, 5, 5 + r] = 5.0
    out.append(("equal maxima at r^2", x, 2, r, 1.0, {"count": [2], "xy": {0: [(5, 5)]}, "not_xy": {0: (5 + r, 5)}}))
    x = _noise(H, W, 2)
    x[0, 0, 5, 5] = x[0, 0, 6, 5 + r] = 5.0
    out.append(("equal maxima at r^2 + 1", x, 2, r, 1.0, {"count": [2], "xy": {0: [(5, 5), (5 + r, 6)]}}))
    # equal maxima on both sides of a 64-lane boundary, of a 256-pixel segment boundary and of a 16-column tile border: index order
    Hs, Ws = 33, 70
    x = _noise(Hs, Ws, 3)
    want = []
    for lin in (63, 64, 255, 256, 10 * Ws + 15, 10 * Ws + 16, 2303, 2304):
        x[0, 0, lin // Ws, lin % Ws] = 4.0
        want.append((lin % Ws, lin // Ws))
    out.append(("equal maxima across lane / segment / tile borders", x, 8, 0, 1.0, {"count": [8], "xy": {0: want}}))
    # ... and on both sides of the 64-entry boundary of the segment table (segments 63 | 64 of a 256 x 256 plane), and of its middle
    x = _noise(256, 256, 4)
    want = []
    for lin in (64 * 256 - 1, 64 * 256, 128 * 256 - 1, 128 * 256, 65535):
        x[0, 0, lin // 256, lin % 256] = 6.0
        want.append((lin % 256, lin // 256))
    out.append(("equal maxima across the table's wave boundary", x, 5, 0, 1.0, {"count": [5], "xy": {0: want}}))
    # +0.0 beside -0.0: a tie, the lower index wins, and the logit comes back with its own sign
    x = torch.full((1, 2, H, W), -1.0)
    x[0, 0, 2, 3], x[0, 0, 2, 4] = -0.0, 0.0
    x[0, 1, 2, 3], x[0, 1, 2, 4] = 0.0, -0.0
    out.append(("+0.0 beside -0.0", x, 2, 0, 1.0, {"count": [2, 2], "xy": {0: [(3, 2), (4, 2)], 1: [(3, 2), (4, 2)]}}))
    out.append(("negative logits only", _noise(H, W, 5, 1.0) - 10.0, 20, 1, 1.8, {"count": [20]}))
    # denormals: every value below fp32's normal range, both signs; flushed to zero they would all tie
    g = LC._gen(701)
    mag = torch.randint(1, 2 ** 22, (1, 1, H, W), generator=g, dtype=torch.int32)
    sign = torch.randint(0, 2, (1, 1, H, W), generator=g, dtype=torch.int32) * torch.tensor(-2 ** 31, dtype=torch.int32)
    out.append(("denormals", (mag | sign).view(torch.float32), 20, 1, 1.0, {"count": [20]}))
    x = _noise(H, W, 6, 1.0, P=2)
    x[0, 0, 9, 11] = inf
    x[0, 1, 12, 2] = x[0, 1, 3, 20] = inf
    out.append(("+inf, and two of them", x, 3, 3, 1.0, {"count": [3, 3], "xy": {0: [(11, 9)], 1: [(20, 3), (2, 12)]}}))
    x = _noise(H, W, 7, 1.0)
    x[0, 0, 0, :] = -inf
    out.append(("a row of -inf", x, 20, 3, 1.0, {"count": [20]}))
    # a mode whose disk crosses each border and each corner
    x = _noise(H, W, 8)
    spots = [(0, 0), (0, W - 1), (H - 1, 0), (H - 1, W - 1), (0, W // 2), (H - 1, W // 2), (H // 2, 0), (H // 2, W - 1)]
    for k, (row, col) in enumerate(spots):
        x[0, 0, row, col] = 9.0 - k
    out.append(("disks across every border and corner", x, 8, 3, 1.0, {"count": [8], "xy": {0: [(c, r_) for r_, c in spots]}}))
    out.append(("-inf only", torch.full((1, 1, H, W), -inf), 5, 1, 1.0, {"count": [0]}))
    # finite logits stop early only when the map is covered, and the masses then sum to 1
    out.append(("a covered map, r 3", _noise(5, 4, 9, 1.0), 20, 3, 0.7, {"covered": True}))
    out.append(("a covered map, r 1", _noise(5, 4, 10, 1.0), 20, 1, 0.7, {"covered": True}))
    # a NaN plane among clean ones: not ranked, flag set, the neighbours untouched
    x = _noise(H, W, 11, 1.0, P=3)
    x[0, 1, H - 1, W - 2] = float("nan")
    out.append(("a NaN plane among clean ones", x, 20, 3, 1.0, {"count": [20, -1, 20], "nan": True}))
    return out


def check_planted(name, ref, want):
    """the reference (or the device's result) of a planted plane against its closed form"""
    if "count" in want:
        assert ref["count"].view(-1).tolist() == want["count"], (name, ref["count"])
    for pl, pts in want.get("xy", {}).items():
        got = [tuple(int(v) for v in p) for p in ref["xy"][0, pl, :len(pts)].tolist()]
        assert got == pts, (name, pl, got, pts)
    for pl, pt in want.get("not_xy", {}).items():
        assert all(tuple(int(v) for v in p) != pt for p in ref["xy"][0, pl].tolist()), (name, pl)
    if want.get("covered"):
        assert bool((ref["count"] < ref["xy"].shape[2]).all()) and bool((ref["count"] >= 1).all()), (name, ref["count"])
        mass = ref["mass"][0] if isinstance(ref["mass"], list) else ref["mass"]
        assert float((mass.double().sum(dim=2) - 1).abs().max()) <= 1e-6, (name, mass)


# ------------------------------------------------------------------------------------------------
# other layouts
# ------------------------------------------------------------------------------------------------
def many_planes():
    """70000 planes of 2 x 2 (more than 65535 workgroups along blockIdx.x) -> (x [35000, 2, 2, 2], n_modes, radius, T)"""
    return torch.randn(35000, 2, 2, 2, generator=LC._gen(800)) * 3.0, 2, 1, 1.8


def many_planes_ref(x, n_modes, radius, T, dtypes=(torch.float64,)):
    """`modes_ref` of `many_planes`, vectorised (a Python loop over 70000 planes is slow): with radius 1 on 2 x 2 the first mode
    leaves the pixel diagonally across, which is the second mode.  Checked against `modes_ref` on the first planes by the host test."""
    assert (n_modes, radius) == (2, 1) and x.shape[2:] == (2, 2) and bool(torch.isfinite(x).all())
    B, C = x.shape[:2]
    flat = x.float().reshape(-1, 4)
    first = torch.from_numpy(np.argmax(flat.numpy(), axis=1))
    idx = torch.stack([first, 3 - first], dim=1)                                   # [P, 2]
    mass = []
    for d in dtypes:
        w = torch.sigmoid(flat.to(d) / T)
        rest = w.clone().scatter_(1, idx[:, 1:], 0.0)                              # the first disk: all but the opposite pixel
        mass.append((torch.stack([rest.sum(dim=1), w.gather(1, idx[:, 1:])[:, 0]], dim=1) / w.sum(dim=1, keepdim=True)).view(B, C, 2))
    return {"xy": torch.stack([idx % 2, idx // 2], dim=-1).float().view(B, C, 2, 2), "logit": flat.gather(1, idx).view(B, C, 2),
            "count": torch.full((B, C), 2, dtype=torch.int32), "mass": mass}


def sliced(H, W):
    """A 5-channel tensor whose channels 1:3 are ranked in place -> (x5 [2, 5, H, W], n_modes, radius, T)"""
    return torch.randn(2, 5, H, W, generator=LC._gen(900, H, W)) * 4.0, 20, 3, 0.7

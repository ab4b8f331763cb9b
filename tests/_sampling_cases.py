"""Seeded inputs and the restatements for the edge sweep of the evaluation samplers: ynet_multinomial and ynet_cws_prior (csrc/sample.hip)
and ynet_kmeans2d (csrc/glue.hip).  tests/test_sampling_cases_host.py proves this table on the CPU, tests/test_gpu_sampling_edges.py runs
the kernels against it.

The references are oracle.ynet_oracle.device_multinomial (draw for draw), `kmeans_rule` (the rule documented above kmeans2d_kernel, in
NumPy with every fp32 step rounded) and `cws_rule` (the formula of cws_prior_kernel's header and O.cws_gaussian, in NumPy float64).
This module never imports the package under test."""
import functools
import zlib

import numpy as np
import torch

from oracle import ynet_oracle as O

SEED = 20261020


def _key(name):
    return zlib.crc32(str(name).encode())


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


def _rs(*key):
    return np.random.RandomState(np.random.SeedSequence([SEED, *key]).generate_state(1)[0])


def _seed62(name):
    """A 62-bit sampler seed (both words of the Philox key are in use)."""
    lo, hi = (int(v) for v in np.random.SeedSequence([SEED, _key(name), 1]).generate_state(2))
    return ((hi << 32) | lo) & (2 ** 62 - 1)


# ------------------------------------------------------------------------------------------------
# 1. multinomial: rows (name, prob [rows, n] fp32, K, replacement, rel_threshold, seed)
# ------------------------------------------------------------------------------------------------
TOPK_THREADS = 256          # multinomial_topk_kernel: element i belongs to thread i % 256
EXACT_N, EXACT_K = 5000, 20


def _dense(rows, n, name):
    return torch.sigmoid(torch.randn(rows, n, generator=_gen(_key(name), rows, n)) * 3)


def _residues(n, residues, name, rows=2):
    """Positive only at indices = r (mod 256), r in `residues`: every winner of the race lives in those threads' lists."""
    p = torch.zeros(rows, n)
    for r in residues:
        p[:, r::TOPK_THREADS] = _dense(rows, len(range(r, n, TOPK_THREADS)), f"{name}/{r}")
    return p


def exact_positions():
    """The EXACT_K seeded positions of the `exactly_K` / `too_few` rows, sorted."""
    return np.sort(_rs(_key("exactly_K")).choice(EXACT_N, EXACT_K, replace=False))


def _exactly_k():
    p = torch.zeros(2, EXACT_N)
    pos = torch.from_numpy(exact_positions())
    p[:, pos] = _dense(2, EXACT_K, "exactly_K")
    return p


def _denormal():
    p = torch.zeros(2, 4096)
    pos = torch.from_numpy(np.sort(_rs(_key("denormal")).choice(4096, 30, replace=False)))
    p[:, pos] = 1e-40           # (below fp32's smallest normal number, 1.18e-38)
    return p


def _one_hot_mass(n, at):
    p = torch.zeros(2, n)
    p[:, at] = 0.3
    return p


_TOPK = {       # name -> (prob builder, K, rel_threshold)
    "n1_K1": (lambda: _dense(2, 1, "n1_K1"), 1, None),
    "n48_K48": (lambda: _dense(2, 48, "n48_K48"), 48, None),
    "n300_K48": (lambda: _dense(2, 300, "n300_K48"), 48, None),
    "one_thread": (lambda: _residues(256 * 60, (7,), "one_thread"), 48, None),
    "two_threads": (lambda: _residues(256 * 60, (7, 200), "two_threads"), 48, None),
    "exactly_K": (_exactly_k, EXACT_K, None),
    "denormal": (_denormal, 20, None),
    "thr_1.0": (lambda: _dense(3, 1000, "thr_1.0"), 1, 1.0),
    "many_rows": (lambda: _dense(3000, 64, "many_rows"), 3, None),
}
_CDF = {        # name -> (prob builder, K, rel_threshold)
    "rep_n1": (lambda: _dense(2, 1, "rep_n1"), 300, None),
    "rep_n5": (lambda: _dense(2, 5, "rep_n5"), 300, None),
    "rep_n255": (lambda: _dense(2, 255, "rep_n255"), 300, None),
    "rep_n256": (lambda: _dense(2, 256, "rep_n256"), 300, None),
    "rep_n257": (lambda: _dense(2, 257, "rep_n257"), 300, None),
    "rep_mass_first": (lambda: _one_hot_mass(1000, 0), 300, None),
    "rep_mass_last": (lambda: _one_hot_mass(1000, 999), 300, None),
    "rep_512x512": (lambda: _dense(2, 512 * 512, "rep_512x512"), 1000, None),
    "rep_K1": (lambda: _dense(3, 777, "rep_K1"), 1, None),
    "rep_K255": (lambda: _dense(3, 777, "rep_K255"), 255, None),
    "rep_K257": (lambda: _dense(3, 777, "rep_K257"), 257, None),
    "thr_keeps_max_only": (lambda: _dense(3, 1000, "thr_keeps_max_only"), 300, 1.0),
}
MULTI_NAMES = list(_TOPK) + list(_CDF)
STATUS_NAMES = ["too_few", "zero_last"]


@functools.lru_cache(maxsize=None)
def multi_row(name):
    """-> (name, prob, K, replacement, rel_threshold, seed) of a row of MULTI_NAMES or STATUS_NAMES."""
    if name == "too_few":           # `exactly_K` asked for one draw more than it has positive entries
        return (name, _exactly_k(), EXACT_K + 1, False, None, _seed62(name))
    if name == "zero_last":         # rows are numbered by position, so the oracle's rows 0 .. 2 are the device's: the zero row goes last
        p = torch.cat([_dense(3, 500, "zero_last"), torch.zeros(1, 500)])
        return (name, p, 40, True, None, _seed62(name))
    replacement = name in _CDF
    build, K, thr = (_CDF if replacement else _TOPK)[name]
    return (name, build(), K, replacement, thr, _seed62(name))


@functools.lru_cache(maxsize=None)
def multi_want(name):
    """The oracle's draws of a row (computed once per process and shared; `zero_last`: of its three valid rows)."""
    _, prob, K, replacement, thr, seed = multi_row(name)
    if name == "zero_last":
        prob = prob[:3]
    return O.device_multinomial(prob, K, replacement, thr, seed)


# ------------------------------------------------------------------------------------------------
# 2. k-means
# ------------------------------------------------------------------------------------------------
def kmeans_rule(points, init_idx, tol, iter_limit):
    """The rule documented above kmeans2d_kernel for ONE point set, in NumPy: points [N, 2] (integer valued), init_idx [K]
    -> (centres [K, 2] fp32, iterations, empty flag, number of points with a distance tie in the first assignment).
      assign:  d_j = fl(fl(dx*dx) + fl(dy*dy)) in fp32, the first minimum wins
      update:  c_j = sum_j / n_j, exact integer sums, one fp32 division per coordinate
      stop:    (sum_j sqrt(fl(fl(ddx^2) + fl(ddy^2))))^2 < tol with the sum carried in fp32 in the order of j, or iter_limit (0: none)
    An empty cluster ends the run (the device hands that set to the host path): the flag is set, the centres are not meaningful."""
    f32 = np.float32
    pts = np.rint(np.asarray(points, dtype=np.float64)).astype(np.int64)
    x, y = pts[:, 0].astype(f32), pts[:, 1].astype(f32)
    idx = np.asarray(init_idx, dtype=np.int64)
    K = len(idx)
    cx, cy = x[idx].copy(), y[idx].copy()
    tol = f32(tol)
    it, ties = 0, 0
    while True:
        dx, dy = x[:, None] - cx[None, :], y[:, None] - cy[None, :]
        d = dx * dx + dy * dy                       # fp32 arrays: every step is rounded to fp32
        assert d.dtype == np.float32
        assign = np.argmin(d, axis=1)               # the first minimum
        if it == 0:
            ties = int(((d == d.min(axis=1, keepdims=True)).sum(axis=1) > 1).sum())
        n = np.bincount(assign, minlength=K)
        it += 1
        if (n == 0).any():
            return np.stack([cx, cy], axis=1), it, True, ties
        sx, sy = np.zeros(K, dtype=np.int64), np.zeros(K, dtype=np.int64)
        np.add.at(sx, assign, pts[:, 0])
        np.add.at(sy, assign, pts[:, 1])
        nx, ny = sx.astype(f32) / n.astype(f32), sy.astype(f32) / n.astype(f32)
        ddx, ddy = nx - cx, ny - cy
        step = np.sqrt(ddx * ddx + ddy * ddy)
        shift = f32(0)
        for j in range(K):
            shift = f32(shift + step[j])
        cx, cy = nx, ny
        if f32(shift * shift) < tol or (iter_limit != 0 and it >= iter_limit):
            return np.stack([cx, cy], axis=1), it, False, ties


# name -> (P, N, K, max coordinate, tol, iter_limit, kind of points)
KMEANS_CASES = {
    "blobs_10000_19": (5, 10000, 19, 256, 1e-3, 1000, "blobs"),
    "below_1024_threads": (3, 700, 32, 64, 1e-3, 1000, "distinct"),
    "lds_limit_18000_32": (2, 18000, 32, 512, 1e-3, 1000, "uniform"),
    "K1": (4, 45, 1, 32, 1e-3, 1000, "distinct"),
    "N_equals_K": (3, 7, 7, 16, 1e-3, 1000, "distinct"),
    "many_workgroups": (300, 64, 4, 32, 1e-3, 1000, "distinct"),
    "iter_limit_1": (5, 10000, 19, 256, 1e-3, 1, "blobs"),
    "iter_limit_3": (5, 10000, 19, 256, 1e-3, 3, "blobs"),
    "lattice": (1, 45, 2, 9, 1e-3, 1000, "lattice"),
    "duplicate_centre": (2, 50, 3, 32, 1e-3, 1000, "duplicate"),
}
KMEANS_EMPTY = {"duplicate_centre": [True, False]}      # the only case with an empty cluster: its person 0
LATTICE_W, LATTICE_H = 9, 5
LATTICE_WANT = dict(ties=5, iterations=2, centres=[[2.0, 2.0], [6.5, 2.0]])


def _kmeans_seed(name):
    base = "blobs_10000_19" if name.startswith("iter_limit") else name      # the iter_limit cases run the first case's points again
    # (the blobs put many samples on one pixel, as TTST's draws do; the stream was picked so that no person's initial centres coincide --
    # tests/test_sampling_cases_host.py asserts it -- and the empty-cluster status has its own case)
    return int(np.random.SeedSequence([SEED, _key(base), 6]).generate_state(1)[0])


@functools.lru_cache(maxsize=None)
def kmeans_case(name):
    """-> (points [P, N, 2] fp32 tensor, init_idx [P, K] int32 tensor, tol, iter_limit, numpy seed).  The initial centres are what
    np.random.seed(seed) followed by one np.random.choice(N, K, replace=False) per person gives (O.kmeans_lloyd draws them so)."""
    P, N, K, maxc, tol, limit, kind = KMEANS_CASES[name]
    seed = _kmeans_seed(name)
    rs = np.random.RandomState(seed ^ 0x5bd1e995)
    if kind == "blobs":             # six Gaussian blobs per person (the existing device test's points)
        centres = rs.randint(0, maxc // 4, (P, 6, 2)).astype(np.float64)
        pts = centres[np.arange(P)[:, None], rs.randint(0, 6, (P, N))] + rs.randn(P, N, 2) * 3
        pts = np.clip(np.rint(pts), 0, maxc - 1)
    elif kind == "uniform":         # uniform over the map
        pts = rs.randint(0, maxc, (P, N, 2)).astype(np.float64)
    elif kind in ("distinct", "duplicate"):     # N different pixels: no two initial centres coincide
        cells = np.stack([rs.choice(maxc * maxc, N, replace=False) for _ in range(P)])
        pts = np.stack([cells % maxc, cells // maxc], axis=-1).astype(np.float64)
    else:                           # the 9 x 5 integer lattice, row-major
        yy, xx = np.meshgrid(np.arange(LATTICE_H), np.arange(LATTICE_W), indexing="ij")
        pts = np.stack([xx.reshape(-1), yy.reshape(-1)], axis=-1)[None].astype(np.float64)
    init_rs = np.random.RandomState(seed)       # the stream np.random.seed(seed) gives the global generator
    init = np.stack([init_rs.choice(N, K, replace=False) for _ in range(P)]).astype(np.int32)
    if kind == "lattice":           # centres at (2, 2) and (6, 2): the column x = 4 is equidistant from both
        init = np.array([[2 * LATTICE_W + 2, 2 * LATTICE_W + 6]], dtype=np.int32)
    if kind == "duplicate":         # person 0: two initial centres on one pixel -> the second cluster gets no point
        pts[0, 1] = pts[0, 0]
        init[0] = [0, 1, 5]
    return torch.from_numpy(pts.astype(np.float32)), torch.from_numpy(init), tol, limit, seed


@functools.lru_cache(maxsize=None)
def kmeans_want(name):
    """kmeans_rule per person -> (centres [P, K, 2] fp32 tensor, iterations [P], empty [P], first-assignment ties [P])."""
    pts, init, tol, limit, _ = kmeans_case(name)
    res = [kmeans_rule(pts[p].numpy(), init[p].numpy(), tol, limit) for p in range(pts.shape[0])]
    return (torch.from_numpy(np.stack([r[0] for r in res])), [r[1] for r in res], [r[2] for r in res], [r[3] for r in res])


# ------------------------------------------------------------------------------------------------
# 3. conditioned-waypoint-sampling prior
# ------------------------------------------------------------------------------------------------
def cws_rule(sig, mean, dist, sigma_factor, ratio, rot):
    """cws_prior_kernel's header formula / O.cws_gaussian x sig in NumPy float64: sig [H, W], mean (x, y), dist (x, y)
    -> (map [H, W] = sig k / sum(sig k), x, y) with (x, y) the expectation over pixel INDICES.
      grid   linspace(0, N, N) per axis, minus the mean
      T      = R cov R^T, R = rotation by atan2(dist_x, dist_y) [then 90 degrees], cov = diag((d / sf / ratio)^2, (d / sf)^2), d = |dist| + 5
      k      = exp(-0.5 m^T T^-1 m), T inverted numerically
    A map whose every term underflows in float64 is 0 / 0 = NaN, and so is its expectation (what the reference produces as well)."""
    sig = np.asarray(sig, dtype=np.float64)
    H, W = sig.shape
    mx, my = (float(v) for v in mean)
    dx, dy = (float(v) for v in dist)
    gx, gy = np.linspace(0, W, W) - mx, np.linspace(0, H, H) - my
    X, Y = np.meshgrid(gx, gy, indexing="xy")       # [H, W] each
    rad = np.arctan2(dx, dy)
    c, s = np.cos(rad), np.sin(rad)
    R = np.array([[c, s], [-s, c]])
    if rot:
        R = np.array([[0.0, -1.0], [1.0, 0.0]]) @ R
    d = np.sqrt(dx * dx + dy * dy) + 5.0
    cov = np.diag([(d / sigma_factor / ratio) ** 2, (d / sigma_factor) ** 2])
    Ti = np.linalg.inv(R @ cov @ R.T)
    q = X * (Ti[0, 0] * X + Ti[0, 1] * Y) + Y * (Ti[1, 0] * X + Ti[1, 1] * Y)
    v = sig * np.exp(-0.5 * q)
    S = v.sum()
    with np.errstate(invalid="ignore", divide="ignore"):
        m = v / S
        x = (v * np.arange(W, dtype=np.float64)[None, :]).sum() / S
        y = (v * np.arange(H, dtype=np.float64)[:, None]).sum() / S
    return m, x, y


CWS_SHAPES = [(64, 64), (64, 96), (1, 8), (8, 1), (37, 50), (512, 512)]

# (name, mean(H, W) -> (x, y), dist, sigma_factor, ratio, rot, fp32 pattern, e_ref).  `fp32 pattern`: what the fp32 oracle gives with an
# all-ones map -- "finite", or "nan" where its every term underflows; cws_rule is finite on all rows but `outside_60px`.  e_ref: the
# fp32 oracle's own relative error against cws_rule over the elements above 1e-6 of the map's maximum, the largest over CWS_SHAPES,
# measured on the CPU (tests/test_sampling_cases_host.py asserts twice that).
CWS_ROWS = [
    ("benign", lambda H, W: (0.4 * W, 0.55 * H), (20.0, -14.0), 6.0, 2.0, False, "finite", 3.25e-5),
    ("benign_rot", lambda H, W: (0.6 * W, 0.3 * H), (-9.0, 30.0), 6.0, 2.0, True, "finite", 2.36e-5),
    ("dist_0", lambda H, W: (0.5 * W, 0.5 * H), (0.0, 0.0), 6.0, 2.0, False, "finite", 7.47e-5),
    ("corner_pixel", lambda H, W: (W - 1.0, H - 1.0), (10.0, 5.0), 6.0, 2.0, True, "finite", 5.08e-5),
    ("outside_12px", lambda H, W: (-12.0, 0.5 * H), (0.0, 0.0), 6.0, 2.0, False, "nan", None),
    ("outside_60px", lambda H, W: (-60.0, 0.5 * H), (0.0, 0.0), 6.0, 2.0, False, "nan", None),
    ("dist_200", lambda H, W: (0.5 * W, 0.5 * H), (200.0, 200.0), 6.0, 2.0, False, "finite", 6.44e-6),
    ("traj_idx_2", lambda H, W: (0.45 * W, 0.5 * H), (-25.0, 8.0), 6.0 - 2, 2.0, True, "finite", 1.79e-5),
    ("negative_sigma_factor", lambda H, W: (0.5 * W, 0.4 * H), (12.0, 16.0), -6.0, 2.0, False, "finite", 4.61e-5),
]
CWS_RULE_NAN = {"outside_60px"}         # float64 underflows too: NaN in the map and in xy
CWS_SIGS = ("sigmoid_randn", "ones", "channel_view")
CWS_B = 2                               # persons; every call has 2 * CWS_B rows, so row % B is exercised


def cws_row(name):
    return next(r for r in CWS_ROWS if r[0] == name)


def cws_inputs(name, H, W, rows=2 * CWS_B):
    """-> (mean [rows, 2], dist [rows, 2]) fp32 tensors: row 0 is the table's row as written, the others move the mean by a fraction of a
    pixel each (dist stays as it is: `dist_0` keeps atan2(0, 0) on every row)."""
    _, mean, dist, _, _, _, _, _ = cws_row(name)
    m = torch.tensor([mean(H, W)] * rows, dtype=torch.float32)
    m = m + torch.arange(rows, dtype=torch.float32)[:, None] * torch.tensor([0.37, -0.21])
    return m, torch.tensor([dist] * rows, dtype=torch.float32)


def cws_sig(kind, H, W, device="cpu"):
    """The sigmoid maps of a variant on `device` -> (sig [B, H, W] as the call gets it (a view for `channel_view`), B).
    sigmoid_randn: CWS_B dense maps; ones: one all-ones map (utils/evaluate.cws_gaussians); channel_view: big[:, 1] of a [B, 3, H, W]
    tensor, what cws_waypoints passes (batch stride 3 H W; the slice is taken on `device`, a copy across devices would close the gaps)."""
    if kind == "ones":
        return torch.ones(1, H, W, device=device), 1
    if kind == "sigmoid_randn":
        return torch.sigmoid(torch.randn(CWS_B, H, W, generator=_gen(_key(kind), H, W))).to(device), CWS_B
    big = torch.sigmoid(torch.randn(CWS_B, 3, H, W, generator=_gen(_key(kind), H, W))).to(device)
    return big[:, 1], CWS_B


@functools.lru_cache(maxsize=4)
def cws_want(name, kind, H, W):
    """cws_rule on every row of cws_inputs(name, H, W) with the variant's maps -> (maps [rows, H, W], xy [rows, 2]) float64 arrays."""
    _, _, _, sf, ratio, rot, _, _ = cws_row(name)
    mean, dist = cws_inputs(name, H, W)
    sig, B = cws_sig(kind, H, W)
    sig = sig.double().numpy()
    out = [cws_rule(sig[r % B], mean[r].numpy(), dist[r].numpy(), sf, ratio, rot) for r in range(mean.shape[0])]
    return np.stack([o[0] for o in out]), np.array([[o[1], o[2]] for o in out])


def cws_oracle_error(name, H, W):
    """The fp32 oracle (O.cws_gaussian, all-ones map) against cws_rule on the table's row 0 -> (largest relative error over the elements
    above 1e-6 of the map's maximum, or None where the oracle is not finite; the oracle's map)."""
    _, _, _, sf, ratio, rot, _, _ = cws_row(name)
    mean, dist = cws_inputs(name, H, W, rows=1)
    got = O.cws_gaussian(mean[0], H, W, dist[0], sf, ratio, rot).double().numpy()
    ref, _, _ = cws_rule(np.ones((H, W)), mean[0].numpy(), dist[0].numpy(), sf, ratio, rot)
    if not np.isfinite(got).all() or not np.isfinite(ref).all():
        return None, got
    big = ref > 1e-6 * ref.max()
    return float((np.abs(got - ref)[big] / ref[big]).max()), got

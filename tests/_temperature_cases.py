"""Seeded inputs and yardsticks for the tests of ynet_map_likelihood_sweep / ops.map_likelihood_sweep / utils.calibrate
(tests/test_temperature_host.py checks this table on the CPU, tests/test_gpu_temperature.py runs the kernel against it).

The reference is tests/_likelihood_cases.like_ref on .double() inputs, called once per temperature: stock torch, never the code under
test.  Logits, ground truths, edge planes and layouts are that module's; this one adds the temperature grids, the E32 table of the
sweep (the largest error of like_ref in fp32 against its own fp64 run over the logit kinds AND the sweep's temperatures), the closed
forms per temperature and the planted calibration sets.  Device bound, as everywhere: 2 * E32 + 2^-21 * max(1, |ref|)."""
import functools
import math

import numpy as np
import torch

import _likelihood_cases as C

SWEEP_OUTPUTS = ("nll", "hpd")
N_TEMPS = [1, 2, 8, 9, 16, 17, 32]          # crosses every border between the kernel's forms (4 | 8 | 16 | 24 | 32 temperatures)


def _master():
    """32 temperatures, log-uniform over [0.25, 8], unsorted; entry 0 is 1.0 exactly (the kernel's z = x), entry 2 the lower end."""
    rng = np.random.default_rng(np.random.SeedSequence([C.SEED, 700]))
    t = np.exp(rng.uniform(math.log(0.25), math.log(8.0), 32)).astype(np.float32)
    t[0], t[2] = 1.0, 0.25
    assert np.unique(t).size == 32
    return t


MASTER = _master()


def grid(n):
    """The sweep grid of n temperatures: the first n - 1 of MASTER and, last, a repeat of entry 1 (n = 2: 1.0 twice; n = 1: 1.0 alone).
    Unsorted, holds 1.0 exactly, holds one value twice -- the two copies sit in different 8-temperature chunks from n = 10 on."""
    if n == 1:
        return MASTER[:1].copy()
    if n == 2:
        return np.array([1.0, 1.0], dtype=np.float32)
    return np.concatenate([MASTER[:n - 1], MASTER[1:2]])


def repeated(n):
    """(i, j): the two entries of grid(n) that hold the same temperature"""
    return (0, 1) if n == 2 else (1, n - 1)


def n_temps_for(H, W):
    return [3] if (H, W) == (512, 512) else N_TEMPS


def temps_for(H, W):
    """every distinct temperature the table test sweeps at this shape"""
    return np.unique(np.concatenate([grid(n) for n in n_temps_for(H, W)]))


# ------------------------------------------------------------------------------------------------
# (H, W) -> E32 per output over C.KINDS x temps_for(H, W), measured on the CPU (tests/test_temperature_host.py re-measures it and holds
# the table to it) and rounded up to three digits.  The shapes are C.SHAPES'.
# ------------------------------------------------------------------------------------------------
E32 = {
    (1, 1): {"nll": 4.77e-07, "hpd": 0.0},
    (1, 3): {"nll": 2.33e-06, "hpd": 1.06e-07},
    (5, 4): {"nll": 6.17e-06, "hpd": 2.06e-07},
    (17, 23): {"nll": 4.11e-06, "hpd": 1.98e-07},
    (90, 12): {"nll": 2.64e-06, "hpd": 2.84e-07},
    (96, 160): {"nll": 5.06e-06, "hpd": 2.53e-07},
    (256, 256): {"nll": 3.04e-06, "hpd": 2.23e-07},
    (512, 512): {"nll": 1.59e-06, "hpd": 2.32e-07},
}


@functools.lru_cache(maxsize=None)
def case(si, kind):
    """-> (x [B, C, H, W], gt [B, C, 2]) of C.SHAPES[si], C.KINDS[kind]: that module's tensors, shared, never written to"""
    x, gt, _, _ = C.case(si, kind)
    return x, gt


@functools.lru_cache(maxsize=None)
def ref(si, kind, T):
    """the fp64 restatement of case (si, kind) at temperature T -> {"nll", "hpd"} [B, C]; computed once per (case, T), shared"""
    x, gt = case(si, kind)
    r = C.like_ref(x, gt, float(T))
    return {k: r[k] for k in SWEEP_OUTPUTS}


def ref_sweep(si, kind, temps):
    """-> {"nll", "hpd"} [n_T, B, C] fp64"""
    rs = [ref(si, kind, float(T)) for T in temps]
    return {k: torch.stack([r[k] for r in rs]) for k in SWEEP_OUTPUTS}


def sweep_ref(x, gt, temps, dtype=torch.float64):
    """like_ref once per temperature on any input -> {"nll", "hpd"} [n_T, B, C] at `dtype`"""
    rs = [C.like_ref(x, gt, float(T), dtype) for T in temps]
    return {k: torch.stack([r[k] for r in rs]) for k in SWEEP_OUTPUTS}


def sweep_e32(x, gt, temps):
    """{"nll", "hpd"} -> the largest error of the fp32 restatement against its own fp64 run over `temps` (finite entries)"""
    out = {k: 0.0 for k in SWEEP_OUTPUTS}
    for T in temps:
        e = C.e32(x, gt, float(T))
        for k in SWEEP_OUTPUTS:
            out[k] = max(out[k], e[k])
    return out


def measure_e32(si):
    (H, W), _, _ = C.SHAPES[si]
    out = {k: 0.0 for k in SWEEP_OUTPUTS}
    for kind in range(len(C.KINDS)):
        x, gt = case(si, kind)
        e = sweep_e32(x, gt, temps_for(H, W))
        for k in SWEEP_OUTPUTS:
            out[k] = max(out[k], e[k])
    return out


# ------------------------------------------------------------------------------------------------
# known answers, per temperature
# ------------------------------------------------------------------------------------------------
def constant_answers(H, W, temps):
    """C.constant_plane at every temperature: every pixel has probability 1 / HW whatever T -> {"nll", "hpd"} [n_T, 1, 1]"""
    n = len(temps)
    return {"nll": torch.full((n, 1, 1), math.log(H * W), dtype=torch.float64), "hpd": torch.ones((n, 1, 1), dtype=torch.float64)}


def spike_answers(H, W, temps):
    """C.spike_planes (one logit of +60 at the last pixel over a background of 0; plane 0's ground truth on the spike, plane 1's on
    pixel 0) at every temperature -> {"nll", "hpd"} [n_T, 1, 2]: with s = sigmoid(60 / T), Z = s + (HW - 1) / 2,
    nll = (log Z - log s, log Z - log 1/2), hpd = (s / Z, 1)."""
    n = H * W
    nll, hpd = [], []
    for T in temps:
        a = 60.0 / float(T)
        s, ls = 1.0 / (1.0 + math.exp(-a)), -math.log1p(math.exp(-a))
        Z = s + (n - 1) * 0.5
        nll.append([[math.log(Z) - ls, math.log(Z) - math.log(0.5)]])
        hpd.append([[s / Z, 1.0]])
    return {"nll": torch.tensor(nll, dtype=torch.float64), "hpd": torch.tensor(hpd, dtype=torch.float64)}


# ------------------------------------------------------------------------------------------------
# the edge rules per temperature: C.edge_planes plus one plane whose mass vanishes at the small temperature alone
# ------------------------------------------------------------------------------------------------
EDGE_TEMPS = np.array([MASTER[2], MASTER[0], MASTER[1]], dtype=np.float32)          # 0.25, 1.0 and one more: all in temps_for(H, W)
NO_MASS_LOGIT = -40.0          # / 0.25 = -160: every sigmoid is below fp32's range (0 on the device), Z = 0; / 1.0 it is an ordinary 4e-18


def edge_planes(H, W):
    """-> (x [1, P + 1, H, W], gt [1, P + 1, 2]): C.edge_planes and, last, the plane "no_mass_at_small_T" (constant NO_MASS_LOGIT)"""
    x, gt, _ = C.edge_planes(H, W)
    extra = torch.full((1, 1, H, W), NO_MASS_LOGIT)
    return torch.cat([x, extra], dim=1), torch.cat([gt, torch.tensor([[[1.0, 2.0]]])], dim=1)


# ------------------------------------------------------------------------------------------------
# planted calibration sets: the truth is drawn from the distribution at T = 2.5, so the NLL over the grid has its minimum there
# ------------------------------------------------------------------------------------------------
PLANTED = [((5, 4), 512), ((17, 23), 256), ((96, 160), 64)]          # (H, W), planes
PLANTED_T = 2.5
PLANTED_BEST = 10          # the point of CAL_GRID next to 2.5 (2.5198)


def cal_grid(lo=0.25, hi=8.0, n=16):
    """n log-spaced temperatures over [lo, hi], fp64 then fp32, in stock NumPy (what utils.likelihood.temperature_grid must return)"""
    g = np.exp(np.linspace(math.log(lo), math.log(hi), n))
    g[0], g[-1] = lo, hi
    return g.astype(np.float32)


@functools.lru_cache(maxsize=None)
def planted(H, W, planes):
    """-> (x [planes, 1, H, W] = 2.5 * l, gt [planes, 1, 2]) with l = -8 + 10 * (a Gaussian bump, sigma = max(1, 0.08 max(H, W)), at a
    random centre) + 0.3 N(0, 1) and the ground truth drawn once, with a seeded generator, from sigmoid(l) / sum sigmoid(l).  (64 draws
    put the optimum of a finite sample at grid point 9 for some seeds; this key is one where the fp64 reference has it at point 10 for
    all three sets, which tests/test_temperature_host.py checks, with its margin.)"""
    g = C._gen(802, H, W, planes)
    cy = torch.rand(planes, 1, 1, 1, generator=g, dtype=torch.float64) * (H - 1)
    cx = torch.rand(planes, 1, 1, 1, generator=g, dtype=torch.float64) * (W - 1)
    yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    s = max(1.0, 0.08 * max(H, W))
    l = -8.0 + 10.0 * torch.exp(-((yy - cy) ** 2 + (xx - cx) ** 2) / (2 * s * s)) + 0.3 * torch.randn(planes, 1, H, W, generator=g, dtype=torch.float64)
    x = (PLANTED_T * l).float()
    p = torch.sigmoid(x.double() / PLANTED_T).flatten(1)          # the distribution of the fp32 logits at the planted temperature
    idx = torch.multinomial(p / p.sum(dim=1, keepdim=True), 1, generator=g)[:, 0]
    gt = torch.stack([(idx % W).float(), (idx // W).float()], dim=-1).view(planes, 1, 2)
    return x, gt


@functools.lru_cache(maxsize=None)
def planted_curve(H, W, planes, temps_key):
    """the fp64 mean NLL of the planted set at every temperature of the tuple `temps_key` -> np.float64 [n_T]"""
    x, gt = planted(H, W, planes)
    return sweep_ref(x, gt, temps_key)["nll"].mean(dim=(1, 2)).numpy()

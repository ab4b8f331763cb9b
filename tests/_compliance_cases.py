"""Seeded inputs and the fp64 restatement for the tests of ynet_map_class_mass / ops.map_class_mass (tests/test_compliance_host.py checks
this table on the CPU, tests/test_gpu_compliance.py runs the kernel against it).

The reference is stock torch on .double() inputs (`mass_ref`), never the code under test.  Per plane, with z = x / T, w = sigmoid(z)
and Z = sum w over the whole plane:
    mass[k] = (sum over {i : labels[i] == k} of w_i) / Z
Run in fp32 the same code is the yardstick of the device test: E32 is its largest error against its own fp64 run, and the device bound
is 2 * E32 + 2^-21 * max(1, |ref|) (four fp32 ulps of the stored result), as in tests/_likelihood_cases.py, whose shapes and logit kinds
(with their temperatures) this table takes."""
import functools
import math

import numpy as np
import torch

import _likelihood_cases as L

SEED = 20250217
B, C = L.B, L.C
KINDS = L.KINDS
MAX_CLASSES = 8


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


# ------------------------------------------------------------------------------------------------
# (H, W) -> E32 = the largest error of `mass_ref` run in fp32 against its own fp64 run over the logit kinds and the label patterns
# below, measured on the CPU (tests/test_compliance_host.py re-measures it and holds the table to it) and rounded up to three digits.
# The shapes are _likelihood_cases.SHAPES': each exists for a walk of the loop (see there).
# ------------------------------------------------------------------------------------------------
E32 = {
    (1, 1): 0.0,
    (1, 3): 9.34e-08,
    (5, 4): 1.07e-07,
    (17, 23): 2.07e-07,
    (90, 12): 7.19e-08,
    (96, 160): 1.35e-07,
    (256, 256): 1.21e-07,
    (512, 512): 7.18e-08,
}
SHAPES = [(hw, why, E32[hw]) for hw, why, _ in L.SHAPES]

# (name, K)
PATTERNS = [
    ("uniform random labels", 6),
    ("vertical stripes of width 1: every 16-byte vector holds four classes", 6),
    ("blocks of 32 x 32", 6),
    ("all one class (2 of 3)", 3),
    ("a class that occurs nowhere (3 of 6)", 6),
    ("one class asked for, two in the map", 1),
    ("eight classes", 8),
    ("labels 7 and 255 under six classes: the row sums to less than 1", 6),
]
ABSENT = 3      # the class pattern 4 leaves out


def applies(H, W, pat):
    """blocks of 32 x 32 need a map that holds more than one"""
    return pat != 2 or (H >= 32 and W >= 32 and H * W > 32 * 32)


def labels(H, W, pat):
    """-> ([H, W] uint8 labels of PATTERNS[pat], K)"""
    g = _gen(200 + pat, H, W)
    K = PATTERNS[pat][1]
    yy, xx = torch.arange(H).view(H, 1), torch.arange(W).view(1, W)
    if pat == 0:
        lab = torch.randint(0, 6, (H, W), generator=g)
    elif pat == 1:
        lab = (xx % 6).expand(H, W)
    elif pat == 2:
        lab = ((yy // 32) * 5 + xx // 32) % 6
    elif pat == 3:
        lab = torch.full((H, W), 2)
    elif pat == 4:
        lab = torch.tensor([0, 1, 2, 4, 5])[torch.randint(0, 5, (H, W), generator=g)]
    elif pat == 5:
        lab = torch.randint(0, 2, (H, W), generator=g)
    elif pat == 6:
        lab = torch.randint(0, 8, (H, W), generator=g)
    else:
        lab = torch.tensor([0, 1, 2, 3, 4, 5, 7, 255])[torch.randint(0, 8, (H, W), generator=g)]
    return lab.to(torch.uint8).contiguous(), K


def logits(H, W, kind):
    return L.logits(H, W, kind)


def weights(x, T, dtype=torch.float64):
    """-> (w = sigmoid(x / T) [B, C, H, W], Z [B, C]) at `dtype`"""
    w = torch.sigmoid(x.float().to(dtype) / T)
    return w, w.sum(dim=(2, 3))


def mass_from(w, Z, lab, K):
    """the class sums of `w` (any float dtype) over the label map [H, W] or [B, H, W], over Z -> [B, C, K].  A NaN logit, or Z == 0,
    makes a plane NaN by itself (NaN / NaN, 0 / 0)."""
    zero = torch.zeros((), dtype=w.dtype)
    lab = lab if lab.dim() == 2 else lab[:, None]
    return torch.stack([torch.where(lab == k, w, zero).sum(dim=(2, 3)) for k in range(K)], dim=-1) / Z[..., None]


def mass_ref(x, lab, K, T, dtype=torch.float64):
    """The class masses in stock torch at `dtype` -> [B, C, K] at `dtype`."""
    w, Z = weights(x, T, dtype)
    return mass_from(w, Z, lab, K)


def e32(x, lab, K, T):
    """-> the largest error of the fp32 restatement against its own fp64 run (finite entries)"""
    r64, r32 = mass_ref(x, lab, K, T), mass_ref(x, lab, K, T, torch.float32)
    d = (r32.double() - r64).abs()[torch.isfinite(r64)]
    return float(d.max()) if d.numel() else 0.0


@functools.lru_cache(maxsize=None)
def _weights_of(si, kind, dtype):
    (H, W), _, _ = SHAPES[si]
    x = logits(H, W, kind)
    return (x,) + weights(x, KINDS[kind][1], dtype)


@functools.lru_cache(maxsize=None)
def case(si, kind, pat):
    """-> (x [B, C, H, W], labels [H, W] uint8, K, T, fp64 reference [B, C, K]) of SHAPES[si], KINDS[kind], PATTERNS[pat]; computed
    once, shared, never written to"""
    (H, W), _, _ = SHAPES[si]
    x, w, Z = _weights_of(si, kind, torch.float64)
    lab, K = labels(H, W, pat)
    return x, lab, K, KINDS[kind][1], mass_from(w, Z, lab, K)


def case_e32(si, kind, pat):
    """the fp32 restatement's error on `case(si, kind, pat)`"""
    (H, W), _, _ = SHAPES[si]
    _, w, Z = _weights_of(si, kind, torch.float32)
    lab, K = labels(H, W, pat)
    r64 = case(si, kind, pat)[4]
    d = (mass_from(w, Z, lab, K).double() - r64).abs()[torch.isfinite(r64)]
    return float(d.max()) if d.numel() else 0.0


def cases(si):
    (H, W), _, _ = SHAPES[si]
    return [(kind, pat) for kind in range(len(KINDS)) for pat in range(len(PATTERNS)) if applies(H, W, pat)]


def bound(ref, e):
    """The device bound per entry: 2 * E32 + 2^-21 * max(1, |ref|)"""
    return 2.0 * e + 2.0 ** -21 * torch.clamp(ref.abs(), min=1.0)


def shape_e32(H, W):
    return E32[(H, W)]


# ------------------------------------------------------------------------------------------------
# known answers
# ------------------------------------------------------------------------------------------------
def constant_plane(H, W, value=0.7):
    """-> (x [1, 1, H, W] constant, labels, K, T, closed form [K]): every pixel has probability 1 / HW, so the mass is the class area"""
    lab, K = labels(H, W, 0)
    area = torch.bincount(lab.reshape(-1).long(), minlength=K).double() / (H * W)
    return torch.full((1, 1, H, W), value), lab, K, 1.3, area


def spike_planes(H, W):
    """-> (x [1, 2, H, W]: one logit of +60 over a background of 0, at the last pixel in plane 0 and at pixel 0 in plane 1; labels, K,
    T = 1, closed forms [2, K]) for a map of at least two pixels: with s = sigmoid(60), n_k pixels of class k and the spike on class j,
    Z = s + (n - 1) / 2, mass[j] = (s + (n_j - 1) / 2) / Z and mass[k] = (n_k / 2) / Z elsewhere"""
    n = H * W
    assert n >= 2
    lab, K = labels(H, W, 0)
    x = torch.zeros(1, 2, H, W)
    x[0, 0, H - 1, W - 1] = 60.0
    x[0, 1, 0, 0] = 60.0
    s = 1.0 / (1.0 + math.exp(-60.0))
    Z = s + (n - 1) * 0.5
    counts = torch.bincount(lab.reshape(-1).long(), minlength=K).double()
    want = torch.empty(2, K, dtype=torch.float64)
    for p, j in enumerate((int(lab[H - 1, W - 1]), int(lab[0, 0]))):
        want[p] = counts * 0.5 / Z
        want[p, j] = (s + (counts[j] - 1) * 0.5) / Z
    return x, lab, K, 1.0, want


# ------------------------------------------------------------------------------------------------
# the edge rules: planes of one launch, with what each must give
# ------------------------------------------------------------------------------------------------
EDGE_SHAPES = L.EDGE_SHAPES               # vector path / element-wise path
EDGE_PLANES = ["nan", "minus_inf_elsewhere", "minus_inf_pixels", "plus_and_minus_inf", "all_minus_inf"]


def edge_planes(H, W):
    """-> (x [1, 5, H, W], labels, K, T): the first five planes of _likelihood_cases.edge_planes -- a NaN logit, a row of -inf, two
    -inf pixels, +inf beside -inf, all -inf -- under uniform random labels"""
    x, _, T = L.edge_planes(H, W)
    assert L.EDGE_PLANES[:5] == ["nan", "minus_inf_elsewhere", "gt_on_minus_inf", "plus_and_minus_inf", "all_minus_inf"]
    lab, K = labels(H, W, 0)
    return x[:, :5].contiguous(), lab, K, T


# ------------------------------------------------------------------------------------------------
# other layouts
# ------------------------------------------------------------------------------------------------
def many_planes():
    """70000 planes of 2 x 2 (more than 65535 workgroups along blockIdx.x) -> (x [35000, 2, 2, 2], labels [2, 2], K, T)"""
    x, _, T = L.many_planes()
    return x, torch.tensor([[0, 1], [2, 0]], dtype=torch.uint8), 3, T


def sliced(H, W):
    """A 5-channel tensor whose channels 1:3 are read in place -> (x5 [2, 5, H, W], labels [H, W], K, T)"""
    x5, _, T = L.sliced(H, W)
    lab, K = labels(H, W, 0)
    return x5, lab, K, T

"""Seeded inputs and the fp64 restatements for the edge sweep of the read-out and element-wise kernels of csrc/glue.hip
(tests/test_glue_cases_host.py checks this table on the CPU, tests/test_gpu_glue_edges.py runs the kernels against it).

Every reference here is stock torch on .double() inputs or oracle.ynet_oracle -- never the code under test."""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import ynet_oracle as O

SEED = 20241016
EPS = 1e-6                       # SoftArgmax2D's denominator (utils/softargmax.py), part of the reference


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


def randn(*shape, key=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(key, *shape)) * scale


def uniform(*shape, key=0, lo=0.0, hi=1.0):
    return torch.rand(*shape, generator=_gen(key, *shape)) * (hi - lo) + lo


# ------------------------------------------------------------------------------------------------
# soft-argmax: (H, W) -> the walk of softargmax_plane the shape exists for.  The third field is the error of the fp32 oracle against
# its own fp64 run (max over the four logit kinds of `soft_logits`, measured on the CPU) for the planes wider or taller than 256, where
# the bound of the device test is twice the fp32 oracle's error alone; None: the 2e-5 floor of the 256 x 256 test applies as well.
# ------------------------------------------------------------------------------------------------
SOFT_SHAPES = [
    ((1, 1), "scalar path, one element", None),
    ((1, 3), "scalar path, one row", None),
    ((5, 4), "w4 = 1: step_r = 256, fewer than 256 vectors (idle threads keep m = -inf)", None),
    ((70, 8), "w4 = 2, fewer than 256 vectors", None),
    ((90, 12), "w4 = 3: step_c != 0 with 270 vectors (tail loop only)", None),
    ((1, 20), "H = 1, w4 = 5", None),
    ((96, 160), "unrolled loop, then the tail, step_c != 0 (w4 = 40)", None),
    ((160, 224), "unrolled loop, then the tail, step_c != 0 (w4 = 56)", None),
    ((256, 256), "the production size: step_c == 0, no tail", None),
    ((512, 512), "configuration C4: step_r = 2, step_c == 0", 1.07e-4),
    ((8, 1028), "w4 = 257 > 256: step_r == 0, one wrap per step", 2.25e-4),
    ((8, 2048), "w4 = 512: step_r == 0, a wrap every second step", 1.52e-4),
    ((17, 23), "W % 4 != 0 beyond 256 elements: scalar path with the division", None),
]
SOFT_KINDS = ("scale0.5", "scale8", "offset+1e4", "offset-1e4")
SOFT_B, SOFT_C = 2, 3


def soft_logits(H, W, kind):
    """[SOFT_B, SOFT_C, H, W] fp32 logits: N(0, 0.5^2), N(0, 8^2), and N(0, 3^2) shifted by +-1e4 (the running maximum absorbs the shift)."""
    k = SOFT_KINDS.index(kind)
    scale = (0.5, 8.0, 3.0, 3.0)[k]
    x = randn(SOFT_B, SOFT_C, H, W, key=100 + k, scale=scale)
    if k >= 2:
        x = x + (1e4 if k == 2 else -1e4)
    return x


def soft_planted(H, W):
    """The planted positions (col, row) of the known-answer planes: the four corners, the last 16-byte vector of row 0, the first vector of
    row 1, the last element (duplicates of a tiny plane dropped, order kept)."""
    pos = [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1), (max(W - 4, 0), 0), (0, min(1, H - 1)), (W - 1, H - 1)]
    return list(dict.fromkeys(pos))


def soft_known(H, W):
    """-> (x [1, P, H, W] fp32: one logit of +60 over a background of 0 per plane, positions [P, 2] (col, row))"""
    pos = soft_planted(H, W)
    x = torch.zeros(1, len(pos), H, W)
    for p, (c, r) in enumerate(pos):
        x[0, p, r, c] = 60.0
    return x, torch.tensor(pos, dtype=torch.float64)


def soft_ref(x):
    return O.softargmax2d(x.double(), EPS)


def soft_e_ref(x):
    """Error of the fp32 oracle against its own fp64 run: the yardstick of the device test."""
    return float((O.softargmax2d(x, EPS).double() - soft_ref(x)).abs().max())


def readout_ref(traj_map, goal_map, gt, rf):
    """utils/train_epoch.py:118-126 in fp64 from the fp64 coordinates -> (pred_traj, pred_goal, ade, fde)"""
    pt, pg = soft_ref(traj_map), soft_ref(goal_map[:, -1:])
    gt = gt.double()
    ade = ((((gt - pt) / rf) ** 2).sum(dim=2) ** 0.5).mean(dim=1)
    fde = ((((gt[:, -1:] - pg[:, -1:]) / rf) ** 2).sum(dim=2) ** 0.5).mean(dim=1)
    return pt, pg, ade, fde


# ------------------------------------------------------------------------------------------------
# max-pool: planes whose 2 x 2 blocks hold four pairwise distinct fp32 values (a random permutation of distinct multiples of 2^-10), so
# ties exist only where `pool_tie_planes` plants them
# ------------------------------------------------------------------------------------------------
POOL_EVEN = [(70000, 2, 2), (70000, 4, 6), (3, 2, 2), (5, 256, 256)]          # > 65535 planes: gridDim.y loops; the minimum; a big map
POOL_ODD = [(7, 3, 3), (6, 2, 3), (6, 3, 2), (5, 9, 7)]                       # the plain backward's zeroed trailing row / column


def pool_planes(N, H, W, key=0):
    n = N * H * W
    assert n < (1 << 24)
    perm = torch.randperm(n, generator=_gen(200 + key, N, H, W))
    return ((perm - n // 2).float() * 2.0 ** -10).view(N, H, W)


def pool_tie_planes():
    """[P, 4, 4]: every plane holds four 2 x 2 blocks; block (0, 0) .. (1, 1) of plane p are planted as listed, in window scan order."""
    inf, nan, z = float("inf"), float("nan"), -0.0
    blocks = [
        [(1.5, 1.5, 1.5, 1.5), (0.0, z, 0.0, z), (z, 0.0, z, 0.0), (-inf, -inf, -inf, -inf)],
        [(0.0, 0.0, z, z), (z, z, 0.0, 0.0), (2.0, 3.0, 3.0, 2.0), (-1.0, -1.0, -2.0, -1.0)],
        [(nan, 1.0, 2.0, 3.0), (1.0, nan, 5.0, 0.5), (4.0, 1.0, nan, 0.0), (9.0, 1.0, 2.0, nan)],
        [(nan, nan, nan, nan), (nan, 7.0, nan, 1.0), (-inf, -inf, 0.0, -inf), (inf, inf, 1.0, inf)],
    ]
    x = torch.empty(len(blocks), 4, 4)
    for p, bl in enumerate(blocks):
        for k, v in enumerate(bl):
            by, bx = 2 * (k // 2), 2 * (k % 2)
            x[p, by:by + 2, bx:bx + 2] = torch.tensor(v).view(2, 2)
    return x


def pool_blocks(x):
    """[N, H, W] -> [N, H/2, W/2, 4] in window scan order (floor sizes)"""
    N, H, W = x.shape
    Ho, Wo = H // 2, W // 2
    v = x[:, :2 * Ho, :2 * Wo].reshape(N, Ho, 2, Wo, 2)
    return v.permute(0, 1, 3, 2, 4).reshape(N, Ho, Wo, 4)


def pool_ref(x, dy, adds=(), relu_mask=False):
    """F.max_pool2d and its autograd on the CPU -> (y, dx, arg [N, Ho, Wo] in 0..3 from torch's return_indices).
    dx = (route(dy) + add0) + add1, then zeroed where x <= 0 (or NaN) under relu_mask: fp32, the order of the kernel's three adds."""
    N, H, W = x.shape
    xr = x.clone().unsqueeze(0).requires_grad_(True)
    y, idx = F.max_pool2d(xr, 2, 2, return_indices=True)
    y.backward(dy.unsqueeze(0))
    dx = xr.grad[0]
    for a in adds:
        dx = dx + a
    if relu_mask:
        dx = torch.where(x > 0, dx, torch.zeros_like(dx))
    idx = idx[0]
    yo = torch.arange(H // 2).view(1, -1, 1)
    xo = torch.arange(W // 2).view(1, 1, -1)
    arg = (idx // W - 2 * yo) * 2 + (idx % W - 2 * xo)
    return y.detach()[0], dx, arg


def pool_code(x, arg):
    """The byte per 2 x 2 block of ynet_conv2d_winograd_cat_pool_code (include/ynet_hip.h): bits 0..1 the arg-max, bits 2..5 "element is
    positive" in window scan order."""
    pos = (pool_blocks(x) > 0).to(torch.int64)
    code = arg + 4 * pos[..., 0] + 8 * pos[..., 1] + 16 * pos[..., 2] + 32 * pos[..., 3]
    return code.to(torch.uint8)


# ------------------------------------------------------------------------------------------------
# average-pool pyramid
# ------------------------------------------------------------------------------------------------
PYR_SHAPES = [(32, 32), (32, 96), (160, 224), (512, 512)]
PYR_PLANES = [(1, 1), (3, 100)]                                  # (B, C): 1 and 300 planes
PYR_BWD = [(1, 1, 32, 32), (3, 100, 32, 96), (1, 2, 160, 224)]


def pyramid_ref(x, n_levels):
    xd = x.double()
    return [F.avg_pool2d(xd, 2 ** i, 2 ** i) if i else xd for i in range(n_levels)]


def pyramid_bwd_ref(shape, grads):
    """fp64 autograd through the same avg_pool2d chain; grads[l] is the gradient of level l (level 0 = x itself, None = no gradient)."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    total = 0.0
    for l, g in enumerate(grads):
        if g is not None:
            total = total + ((F.avg_pool2d(x, 2 ** l, 2 ** l) if l else x) * g.double()).sum()
    total.backward()
    return x.grad


# ------------------------------------------------------------------------------------------------
# sigmoid(x[:, sel] / T): (B, C, H, W, sel, T).  9 and 17 channels take two and three launches of the 8-channel kernel.
# ------------------------------------------------------------------------------------------------
SIG_CASES = [
    (2, 5, 1, 1, [3], 1.0),
    (3, 4, 2, 3, [-1], 0.5),
    (1, 12, 2, 3, [0, 11, -1, 5, 5, -12, 7, 2], 0.5),
    (2, 10, 64, 64, [9, 0, -3, 4, 4, 8, -10, 1, 6], 1.8),
    (1, 6, 256, 256, [0, 1, 2, 3, 4, 5, -1, -2, -3, -4, -5, -6, 2, 2, 0, 5, 3], 1.0),
    (2, 30, 64, 64, [14, 29], 1.8),
    (1, 9, 1, 1, list(range(9)), 1.0),
    (2, 3, 256, 256, [1], 0.5),
]
SIG_RTOL, SIG_ATOL = 1e-6, 1e-7


def sig_input(B, C, H, W):
    return uniform(B, C, H, W, key=300, lo=-90.0, hi=90.0)


def sig_ref(x, sel, T):
    return torch.sigmoid(x.double()[:, sel] / T)


# ------------------------------------------------------------------------------------------------
# batch_sum: (B, n, batch stride).  n = 9 M lies beyond the 8192-block cap (8192 * 256 * 4 elements); B = 1 copies.
# ------------------------------------------------------------------------------------------------
BSUM_N_BIG = 9 * 1024 * 1024
BSUM_CASES = [(1, 4, 4), (2, 4, 8), (33, 4, 4), (1, 1028, 1040), (2, 1028, 1028), (33, 1028, 1032), (33, 4, 12),
              (1, BSUM_N_BIG, BSUM_N_BIG), (2, BSUM_N_BIG, BSUM_N_BIG + 64)]


def bsum_input(B, n, stride):
    """-> the [B, stride] buffer (the gap behind each row holds NaN: it must not be read into the sum)"""
    buf = torch.full((B, stride), float("nan"))
    buf[:, :n] = randn(B, n, key=400, scale=3.0)
    return buf


def bsum_ref(buf, n):
    """-> (fp64 sum, bound): the kernel adds the rows in batch order in fp32, at most B - 1 roundings of a running sum that never exceeds
    sum_b |x_b|, half an ulp (2^-24 relative) each."""
    x = buf[:, :n].double()
    return x.sum(dim=0), (buf.shape[0] - 1) * 2.0 ** -24 * x.abs().sum(dim=0)


# ------------------------------------------------------------------------------------------------
# pad2d / add_relu / relu_bwd: bit-exact, on both sides of grid_for's cap (8192 blocks * 256 threads = 2,097,152 elements)
# ------------------------------------------------------------------------------------------------
GRID_CAP = 8192 * 256
PAD_CASES = [(3, 50, 70, 32), (1, 1, 1, 32), (2, 64, 96, 32), (33, 250, 250, 32), (40, 225, 256, 32), (2, 5, 7, 4)]      # (N, H, W, division factor)
ELEM_N = [1, 3, 1000, GRID_CAP - 1, GRID_CAP + 77, 5 * 1024 * 1024 + 3]


def elem_inputs(n):
    """a, b for add_relu; (dy, y) for relu_bwd: y carries exact zeros, -0.0 and NaN."""
    a, b = randn(n, key=500), randn(n, key=501)
    dy, y = randn(n, key=502), randn(n, key=503)
    special = torch.tensor([0.0, -0.0, float("nan"), 1e-45, -1e-45])
    for k in range(min(n, 5)):
        y[(k * 7919) % n] = special[k]
    if n >= 3:
        a[0], b[0] = float("nan"), 1.0
        a[1], b[1] = -0.0, -0.0
        a[2], b[2] = 2.5, -2.5
    return a, b, dy, y


def add_relu_ref(a, b, relu):
    v = (a.double() + b.double()).float()          # (the fp64 sum of two fp32 values rounds to the fp32 sum)
    return torch.where(v < 0, torch.zeros_like(v), v) if relu else v


def relu_bwd_ref(dy, y):
    return torch.where(y.double() > 0, dy, torch.zeros_like(dy))


# ------------------------------------------------------------------------------------------------
# BCE-with-logits (mean): n x target kind; logits uniform over +-40
# ------------------------------------------------------------------------------------------------
BCE_N = [1, 2, 3, 5, 1027, 4 * 2 ** 20 + 3]
BCE_TARGETS = ("zeros", "ones", "uniform")
BCE_LOSS_RTOL, BCE_GRAD_RTOL = 2e-6, 1e-5


BCE_SMALL_LOGITS = (38.5, -40.0, 3.25, -0.5, 17.0)


def bce_inputs(n, target):
    """Logits uniform over +-40; for n <= 5 the first n of BCE_SMALL_LOGITS (both signs, both ends of the range).  A handful of random logits
    can all fall on the side where an element's loss is exp(-|x|), computed as the difference of two terms of size |x| by torch's fp32 kernel
    and by bce_element alike: such a mean has no relative accuracy in fp32 and the relative bound of the loss is out of reach for both."""
    x = uniform(1, 1, 1, n, key=600, lo=-40.0, hi=40.0) if n > 5 else torch.tensor(BCE_SMALL_LOGITS[:n]).view(1, 1, 1, n)
    t = {"zeros": torch.zeros, "ones": torch.ones}[target](1, 1, 1, n) if target != "uniform" else uniform(1, 1, 1, n, key=601)
    return x, t


def bce_ref(x, t, grad_out=1.0):
    xd = x.double().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xd, t.double())
    (loss * grad_out).backward()
    return loss.detach(), xd.grad


def bce_grad_atol(n, grad_out=1.0):
    """dx = (sigmoid(x) - t) * g / n: an fp32 sigmoid next to 1 is off by up to an ulp of 1 (2^-23), which survives the subtraction of t = 1
    whole -- the relative bound alone cannot hold where sigmoid(x) - t cancels."""
    return 2.0 ** -23 * abs(grad_out) / n


# ------------------------------------------------------------------------------------------------
# upsample2x: the shapes of tests/test_gpu_kernels.py (every kernel variant), handed over at 0-, 4- and 8-byte offsets
# ------------------------------------------------------------------------------------------------
UP_SHAPES = [(2, 3, 8, 16), (1, 2, 1, 1), (1, 4, 5, 3), (2, 16, 32, 32), (1, 2, 3, 6), (2, 2, 1, 4), (1, 3, 7, 12), (2, 2, 2, 128), (1, 2, 64, 64),
             (1, 1, 68, 62), (1, 2, 6, 10)]
UP_MANY = (70000, 1, 2, 2)
# float offsets of (x, y) forward and of (dy, dx, act) backward: 1 = 4 bytes, 2 = 8 bytes
UP_FWD_OFFSETS = [(0, 0), (1, 0), (2, 0), (0, 1), (0, 2), (1, 1), (2, 2)]
UP_BWD_OFFSETS = [(0, 0, 0), (1, 0, 0), (2, 0, 0), (0, 1, 0), (0, 2, 0), (0, 0, 1), (0, 0, 2), (1, 1, 1), (2, 2, 2)]


def up_ref(x, gy, act=None):
    xd = x.double().requires_grad_(True)
    y = F.interpolate(xd, scale_factor=2, mode="bilinear", align_corners=False)
    y.backward(gy.double())
    dx = xd.grad
    return y.detach(), dx, (None if act is None else torch.where(act > 0, dx, torch.zeros_like(dx)))


# ------------------------------------------------------------------------------------------------
# BatchNorm2d, training mode: channel c has mean BN_MEANS[c // 2] and std BN_STDS[c % 2].  BN_TORCH_ERR[case][tensor][c]: the error of
# torch's own fp32 CPU batch norm against the two-pass fp64 reference, per channel (max |.|), measured on the CPU; the device test allows the
# kernel twice torch's error on the same input.
# ------------------------------------------------------------------------------------------------
BN_MEANS, BN_STDS = (0.0, 1e2, 1e4), (1.0, 1e-2)
BN_CASES = [(4, 6, 32, 40), (2, 6, 64, 64)]
BN_EPS = 1e-5
BN_TENSORS = ("save_mean", "save_invstd", "y", "dx")
BN_TORCH_ERR = {
    (4, 6, 32, 40): {"save_mean": (8.89e-10, 8.89e-13, 8.60e-07, 3.13e-06, 3.68e-05, 1.55e-04),
                     "save_invstd": (1.53e-08, 1.69e-06, 3.87e-08, 1.07e-06, 2.56e-08, 1.04e-02),
                     "y": (2.50e-07, 1.39e-07, 4.98e-07, 7.80e-04, 2.91e-07, 3.94e-02),
                     "dx": (3.49e-07, 1.68e-05, 4.19e-07, 2.38e-04, 3.71e-09, 7.64e-02)},
    (2, 6, 64, 64): {"save_mean": (1.27e-10, 2.62e-12, 1.09e-06, 2.55e-06, 4.03e-04, 1.75e-04),
                     "save_invstd": (1.18e-08, 2.16e-06, 3.58e-09, 3.06e-06, 1.01e-07, 1.31e-02),
                     "y": (2.17e-07, 1.21e-07, 7.88e-07, 3.23e-04, 4.81e-07, 2.83e-02),
                     "dx": (3.48e-07, 1.49e-05, 3.53e-07, 6.51e-04, 2.48e-09, 1.80e-01)},
}


def bn_inputs(B, C, H, W):
    x = randn(B, C, H, W, key=700)
    for c in range(C):
        x[:, c] = x[:, c] * BN_STDS[c % 2] + BN_MEANS[c // 2]
    gamma, beta = randn(C, key=701) * 0.5 + 1.0, randn(C, key=702)
    return x, gamma, beta, randn(B, C, H, W, key=703)


def bn_ref(x, gamma, beta, gy, dtype=torch.float64):
    """dtype fp64: the two-pass reference (mean, then the mean of the squared deviations); fp32: torch's own CPU kernels on the same input.
    -> dict of save_mean, save_invstd, y, dx"""
    if dtype == torch.float64:
        xd = x.double().requires_grad_(True)
        mean = xd.mean(dim=(0, 2, 3), keepdim=True)
        var = ((xd - mean) ** 2).mean(dim=(0, 2, 3), keepdim=True)
        invstd = 1.0 / torch.sqrt(var + BN_EPS)
        y = (xd - mean) * invstd * gamma.double().view(1, -1, 1, 1) + beta.double().view(1, -1, 1, 1)
        y.backward(gy.double())
        return {"save_mean": mean.detach().flatten(), "save_invstd": invstd.detach().flatten(), "y": y.detach(), "dx": xd.grad}
    xf = x.clone().requires_grad_(True)
    y, mean, invstd = torch.native_batch_norm(xf, gamma, beta, None, None, True, 0.1, BN_EPS)
    y.backward(gy)
    return {"save_mean": mean.detach(), "save_invstd": invstd.detach(), "y": y.detach(), "dx": xf.grad}


def bn_channel_err(got, want):
    """max |got - want| per channel -> dict of [C] fp64 tensors"""
    out = {}
    for k in BN_TENSORS:
        e = (got[k].detach().cpu().double() - want[k]).abs()
        out[k] = e if e.dim() == 1 else e.amax(dim=(0, 2, 3))
    return out

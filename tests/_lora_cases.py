"""The adapter (LoRA / MoSA) kernels of csrc/lora.hip and csrc/lora_wgrad.hip at every dispatch edge: the shapes, the seeded inputs and the fp64 restatements
(tests/test_lora_cases_host.py checks this module on the CPU, tests/test_gpu_lora_edges.py runs the kernels against it).

The restatements are written from the algebra in the two files' header comments, in float64, and never call the package:
    compose_rule   W + s (B @ A).reshape(W.shape)
    pack_rule      the two packed filter layouts of a [cout][cin][K][K] filter, with the map of the positions they write
    grad_rule      dA = s B^T dWm,  dB = s dWm A^T,  dWm = dW.reshape(cout k, cin k)
    wgrad_rule     dA, dB of conv(cat(xs), W + s (B @ A).view) for an output gradient that is masked where the activation is <= 0 (fp64 autograd through
                   stock F.conv2d; W drops out of both)

Two kinds of input per shape:
  exact   values on a small integer grid -- x, dy in {-2 .. 2} with half of them zero, A, B, w, dw in {-1, 0, 1}, the mask activation in {0, 1}, s in {0.5, 1,
          2}.  Every product is an integer and every partial sum an integer multiple of s below 2^24 (the "abs bound": the same expression on absolute values;
          the host test asserts it), so fp32 is exact in ANY summation order and a kernel must reproduce the fp64 rule bit for bit.  A dropped or doubled term
          is at least 0.5 off.
  gauss   the generators and scales of tests/test_gpu_kernels.py (randn, A x 0.3, B x 0.1, w x 1 / sqrt(k k cin)) against fp64 at the project's tolerances
          below.  A ReLU mask is taken from the fp64 pre-activation and the SAME tensor is handed to the device: no sign flip near zero can enter.

Tolerances.  The host test measures the fp32 CPU evaluation of each rule against fp64 and requires it to stay within HALF of the tolerance; a case that does
not gets 4 x its measured fp32-CPU error in TOL_OVERRIDE, with the measurement next to it (the margin is for another summation order).  None needed one:
the worst fp32-CPU error / tolerance is 0.05 for compose, 0.09 for grad and 0.10 for wgrad (on the MI355X: 0.06, 0.05, 0.04)."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20261020

TOL_COMPOSE = dict(rtol=1e-5, atol=1e-6)            # tests/test_gpu_kernels.py::test_lora_compose_and_grad
TOL_GRAD = dict(rtol=1e-4, scale_rel=2e-6)
TOL_WGRAD = dict(rtol=2e-4, scale_rel=5e-6)          # ::test_lora_conv2d_wgrad_without_the_filter_gradient
TOL_OVERRIDE = {}                                    # (family, case name) -> tolerance from the 4 x rule (none was needed)

SCALES = (0.5, 1.0, 2.0)


# ------------------------------------------------------------------------------------------------
# the restatements
# ------------------------------------------------------------------------------------------------
def compose_rule(w, A, B, s):
    w, A, B = w.double(), A.double(), B.double()
    return w + s * (B @ A).reshape(w.shape)


def ceil64(n):
    return (n + 63) // 64 * 64


def pack_rule(w_eff, mode, n_floats, flip=True):
    """(values [n_floats] float64, written [n_floats] bool) of the packed layout: mode 0 (forward) fwd[(ci KK + t) ceil64(cout) + co] = w[co][ci][t], mode 1
    (dgrad) dgrad[(co KK + (KK - 1 - t)) ceil64(cin) + ci] = w[co][ci][t]; everything else is padding (zero, never written).  flip False: the wrong dgrad
    layout whose taps are not flipped (the host test shows that the data tells the two apart)."""
    w = np.asarray(w_eff.double())
    cout, cin, K, _ = w.shape
    KK = K * K
    co, ci, t = np.meshgrid(np.arange(cout), np.arange(cin), np.arange(KK), indexing="ij")
    if mode == 0:
        pos = (ci * KK + t) * ceil64(cout) + co
    else:
        pos = (co * KK + ((KK - 1 - t) if flip else t)) * ceil64(cin) + ci
    values, written = np.zeros(n_floats, dtype=np.float64), np.zeros(n_floats, dtype=bool)
    assert int(pos.max()) < n_floats
    values[pos.reshape(-1)] = w.reshape(-1)
    written[pos.reshape(-1)] = True
    assert int(written.sum()) == w.size
    return torch.from_numpy(values), torch.from_numpy(written)


def packed_floats(cout, cin, K, mode):
    """ynet_packed_weight_floats as include/ynet_hip.h documents it: rows padded to 16 plus one chunk of 16 slack rows, columns to 64 (the host test compares
    it with the library's answer)."""
    rows, cols = (cin, cout) if mode == 0 else (cout, cin)
    return ((rows + 15) // 16 * 16 + 16) * K * K * ceil64(cols)


def grad_rule(dw, A, B, s):
    cout, cin, k, _ = dw.shape
    dwm = dw.double().reshape(cout * k, cin * k)
    return s * B.double().t() @ dwm, s * dwm @ A.double().t()


def masked(dy, y):
    return dy.double() if y is None else dy.double() * (y > 0)


def wgrad_rule(xs, dy, y, A, B, s, dtype=torch.float64):
    """dA, dB of conv(cat(xs), W + s (B @ A).view(W.shape)) (3 x 3, rank 1, padding 1) for the output gradient dy, zeroed where the activation y is <= 0.
    The base filter W drops out of both gradients, so it is not an argument.  dtype float32: the same evaluation in fp32 (the host test's yardstick)."""
    x = torch.cat([t.to(dtype).expand(dy.shape[0], -1, -1, -1) for t in xs], 1)
    a, b = A.to(dtype).clone().requires_grad_(True), B.to(dtype).clone().requires_grad_(True)
    cout, cin = B.shape[0] // 3, A.shape[1] // 3
    out = F.conv2d(x, s * (b @ a).view(cout, cin, 3, 3), None, padding=1)
    out.backward(masked(dy, y).to(dtype))
    return a.grad, b.grad


def filter_grad_rule(xs, dy, y):
    """dW [cout][cin][3][3] of the same convolution in fp64 (what the two-call chain forms in between)."""
    x = torch.cat([t.double().expand(dy.shape[0], -1, -1, -1) for t in xs], 1)
    return torch.nn.grad.conv2d_weight(x, (dy.shape[1], x.shape[1], 3, 3), masked(dy, y), padding=1)


def straddling_columns(cin):
    """Filter columns u = 9 ci + tap that the kernel's XP loop takes one by one: those of the input channels whose nine taps straddle a boundary between
    the thirds [ii 3 cin, (ii + 1) 3 cin) of the 9 cin columns (lora_wgrad_kernel, `head_end` / `tail_begin`).  Empty iff cin % 3 == 0."""
    n3, cols = 3 * cin, []
    for ii in range(3):
        lo, hi = ii * n3, (ii + 1) * n3
        ci_lo, ci_hi = (lo + 8) // 9, hi // 9
        head_end = min(9 * ci_lo, hi)
        tail_begin = max(9 * ci_hi, head_end)
        cols += list(range(lo, head_end)) + list(range(tail_begin, hi))
    return cols


# the dispatch of ynet_lora_conv2d_wgrad, restated (lw_tile_rows; NTG = ceil(ceil(9 cin / 16) / 4) <= 2 iff cin <= 14)
def tile_rows(cin, cout):
    return 4 if (cin <= 32 and cout <= 32) else (2 if (cin <= 64 and cout <= 64) else 0)


SPECIALISED = {(14, 32), (32, 32), (32, 64), (64, 64)}


def instantiation(cin, cout):
    th = tile_rows(cin, cout)
    if (cin, cout) in SPECIALISED:
        return f"specialised_{th}row"
    if th == 4:
        return "generic_4row_ntg2" if cin <= 14 else "generic_4row_ntg5"
    return "generic_2row"


# ------------------------------------------------------------------------------------------------
# seeded inputs
# ------------------------------------------------------------------------------------------------
def _rs(*key):
    return np.random.RandomState(np.random.SeedSequence([SEED, *[int(k) for k in key]]).generate_state(4))


def _f32(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32))


def grid_pm2(rs, *shape):
    """{-2, -1, 1, 2}, half of the entries (each with probability 1 / 2) zero."""
    return _f32(rs.choice([-2, -1, 1, 2], size=shape) * rs.randint(0, 2, size=shape))


def grid_pm1(rs, *shape):
    return _f32(rs.randint(-1, 2, size=shape))


def gauss(rs, *shape, scale=1.0):
    return _f32(rs.standard_normal(size=shape) * scale)


# ------------------------------------------------------------------------------------------------
# ynet_lora_conv2d_wgrad: (B, H, W, [source channels], cout) by the instantiation the shape reaches
# ------------------------------------------------------------------------------------------------
WGRAD_GROUPS = {
    "generic_4row_ntg2": [(1, 4, 4, [1], 1), (2, 5, 8, [3], 5), (2, 3, 4, [2], 7), (2, 9, 36, [2, 5, 7], 20), (1, 1, 4, [4], 3)],
    "generic_4row_ntg5": [(2, 6, 40, [15], 32), (3, 7, 12, [9, 16, 7], 31), (1, 8, 32, [32], 16), (2, 2, 64, [18], 1)],
    "specialised_4row": [(33, 1, 4, [6, 8], 32), (2, 5, 36, [32], 32)],
    "generic_2row": [(2, 3, 68, [33], 33), (2, 5, 32, [1], 64), (1, 4, 8, [16, 16, 16, 15], 64), (1, 2, 4, [64], 1), (2, 1, 100, [40], 48)],
    "specialised_2row": [(2, 3, 36, [32], 64), (3, 1, 100, [64], 64)],
    # more tiles than the workspace's 1024 slabs / than 3 x 256 resident workgroups: 800 four-row tiles on the 512 slots two 65 KB workgroups per CU leave,
    # 1600 two-row tiles on 768 -- the persistent workgroups walk 2 or 3 tiles each
    "grid_wrap": [(50, 64, 4, [32], 32), (50, 64, 4, [64], 64)],
}
# sources that are views: `expand` -- source i is a [1, c, H, W] tensor expanded to the batch (batch stride 0); `slice` -- source i is big[:, c0:c0 + c] of a
# [B, c_big, H, W] tensor (16-byte aligned, batch stride c_big H W)
WGRAD_VIEWS = {
    "bcast_first_ragged": dict(shape=(3, 5, 12, [3, 4], 9), expand=0),
    "slice_second": dict(shape=(2, 3, 36, [8, 25], 40), slice=(1, 8, 36)),
}


def _shape_name(shape):
    B, H, W, cs, cout = shape
    return f"{B}x{H}x{W}_{'+'.join(map(str, cs))}to{cout}"


WGRAD_SHAPES = {_shape_name(s): s for g in WGRAD_GROUPS.values() for s in g}
WGRAD_SHAPES.update({n: v["shape"] for n, v in WGRAD_VIEWS.items()})
WGRAD_GROUP_OF = {_shape_name(s): g for g, ss in WGRAD_GROUPS.items() for s in ss}
WGRAD_VARIANTS = [(n, kind, m) for n in WGRAD_SHAPES for kind in ("exact", "gauss") for m in (False, True)]
ZERO_FRACTION = 0.02      # of the expected entries of an exact case
SALTS = 256               # seeds tried per exact case until its expected entries meet ZERO_FRACTION (a condition on the inputs)


class WgradCase:
    """Inputs (fp32, CPU) and the fp64 dA / dB of one variant.  xs[i] has batch 1 where WGRAD_VIEWS says `expand`.  y: the mask activation (or None)."""

    def __init__(self, name, kind, with_mask, salt):
        B, H, W, cs, cout = WGRAD_SHAPES[name]
        cin = sum(cs)
        self.name, self.kind, self.shape, self.cin, self.cout, self.salt = name, kind, (B, H, W, tuple(cs), cout), cin, cout, salt
        self.view = WGRAD_VIEWS.get(name, {})
        idx = list(WGRAD_SHAPES).index(name)
        rs = _rs(1, idx, kind == "exact", with_mask, salt)
        batch = [1 if self.view.get("expand") == i else B for i in range(len(cs))]
        if kind == "exact":
            self.xs = [grid_pm2(rs, b, c, H, W) for b, c in zip(batch, cs)]
            self.dy = grid_pm2(rs, B, cout, H, W)
            self.a, self.b, self.w = grid_pm1(rs, 3, 3 * cin), grid_pm1(rs, 3 * cout, 3), grid_pm1(rs, cout, cin, 3, 3)
            self.s = SCALES[idx % 3]
            self.y = _f32(rs.randint(0, 2, size=(B, cout, H, W))) if with_mask else None
        else:
            self.xs = [gauss(rs, b, c, H, W) for b, c in zip(batch, cs)]
            self.dy = gauss(rs, B, cout, H, W)
            self.a, self.b = gauss(rs, 3, 3 * cin, scale=0.3), gauss(rs, 3 * cout, 3, scale=0.1)
            self.w = gauss(rs, cout, cin, 3, 3, scale=1.0 / (9 * cin) ** 0.5)
            self.s = 1.0
            self.y = None
            if with_mask:      # the fp64 pre-activation decides; the fp32 tensor handed to the device has the same sign pattern (a positive double stays positive)
                x = torch.cat([t.double().expand(B, -1, -1, -1) for t in self.xs], 1)
                self.y = F.relu(F.conv2d(x, compose_rule(self.w, self.a, self.b, self.s), None, padding=1)).float()
                assert bool(((self.y > 0) == (F.conv2d(x, compose_rule(self.w, self.a, self.b, self.s), None, padding=1) > 0)).all())
        self.recompute()

    def tensors(self):
        return [*self.xs, self.dy, self.a, self.b] + ([self.y] if self.y is not None else [])

    def recompute(self):
        self.da, self.db = wgrad_rule(self.xs, self.dy, self.y, self.a, self.b, self.s)

    def abs_bound(self):
        """The largest value of the same expressions on absolute values: no partial sum of either gradient, in any order, exceeds it (times s)."""
        da, db = wgrad_rule([x.abs() for x in self.xs], self.dy.abs(), self.y, self.a.abs(), self.b.abs(), self.s)
        dw = filter_grad_rule([x.abs() for x in self.xs], self.dy.abs(), self.y)
        return max(float(da.max()), float(db.max()), self.s * float(dw.max()))

    def zero_fraction(self):
        return (int((self.da == 0).sum()) + int((self.db == 0).sum())) / (self.da.numel() + self.db.numel())

    def blind_spots(self):
        """How many of the image's edges carry nothing: the last pixel row and the last four pixel columns of the masked output gradient, the last input
        channel (a case with one of them empty could not show that a kernel drops it)."""
        g = masked(self.dy, self.y)
        return int(not g[:, :, -1, :].any()) + int(not g[:, :, :, -4:].any()) + int(not self.xs[-1][:, -1].any())


@functools.lru_cache(maxsize=None)
def wgrad_case(name, kind, with_mask):
    """The variant's case; for an exact one, the first salt whose expected entries are non-zero but for ZERO_FRACTION of them (so that a missing term shows
    in almost every entry)."""
    if kind != "exact":
        return WgradCase(name, kind, with_mask, 0)
    for salt in range(SALTS):
        c = WgradCase(name, kind, with_mask, salt)
        if c.zero_fraction() <= ZERO_FRACTION and not c.blind_spots():
            return c
    return _rearranged(WgradCase(name, kind, with_mask, 0), (1, list(WGRAD_SHAPES).index(name), with_mask))


def _rearranged(c, key, steps=20000):
    """The smallest cases (a 1 x 4 image behind a mask leaves three or four products per sum; a 1 x 1 filter of three channels as few) meet ZERO_FRACTION in
    no draw: there, seeded swaps of two elements inside one input tensor -- the values, and the share of them that is zero, stay what they were -- are kept
    while the number of zero entries does not grow."""
    rs = _rs(5, *key)
    tensors = c.tensors()
    n_out = c.da.numel() + c.db.numel()
    zeros = lambda: int((c.da == 0).sum()) + int((c.db == 0).sum()) + n_out * c.blind_spots()      # noqa: E731
    have = zeros()
    for _ in range(steps):
        if have <= ZERO_FRACTION * n_out:
            c.salt = -1
            return c
        t = tensors[rs.randint(len(tensors))].view(-1)
        i, j = rs.randint(t.numel(), size=2)
        if float(t[i]) == float(t[j]):
            continue
        t[i], t[j] = float(t[j]), float(t[i])
        c.recompute()
        now = zeros()
        if now <= have:
            have = now
        else:
            t[i], t[j] = float(t[j]), float(t[i])
            c.recompute()
    raise AssertionError(f"{key}: the zero fraction is not met")


# ------------------------------------------------------------------------------------------------
# compose / grad / pack: (cout, cin, k, r)
# ------------------------------------------------------------------------------------------------
GEMM_SHAPES = [(1, 1, 1, 1), (5, 3, 1, 8), (17, 33, 3, 2), (7, 9, 5, 1), (33, 7, 5, 3), (65, 130, 3, 4), (130, 65, 1, 2), (16, 16, 5, 8), (64, 64, 3, 5)]
GEMM_VARIANTS = [(s, kind) for s in GEMM_SHAPES for kind in ("exact", "gauss")]


class GemmCase:
    """w, A, B, dw (fp32, CPU), s and the fp64 results: w_eff, dA, dB."""

    def __init__(self, shape, kind, salt):
        cout, cin, k, r = shape
        self.shape, self.kind, self.salt = shape, kind, salt
        idx = GEMM_SHAPES.index(shape)
        rs = _rs(2, idx, kind == "exact", salt)
        if kind == "exact":
            self.w, self.dw = grid_pm1(rs, cout, cin, k, k), grid_pm1(rs, cout, cin, k, k)
            self.a, self.b = grid_pm1(rs, r * k, cin * k), grid_pm1(rs, cout * k, r * k)
            self.s = SCALES[(idx + 1) % 3]
        else:
            self.w, self.dw = gauss(rs, cout, cin, k, k), gauss(rs, cout, cin, k, k)      # (test_lora_compose_and_grad: unit-variance weights)
            self.a, self.b = gauss(rs, r * k, cin * k), gauss(rs, cout * k, r * k, scale=0.1)
            self.s = 1.0 / r
        self.recompute()

    def tensors(self):
        return [self.dw, self.a, self.b]

    def recompute(self):
        self.w_eff = compose_rule(self.w, self.a, self.b, self.s)
        self.da, self.db = grad_rule(self.dw, self.a, self.b, self.s)

    def abs_bound(self):
        da, db = grad_rule(self.dw.abs(), self.a.abs(), self.b.abs(), self.s)
        return max(float(da.max()), float(db.max()), float(compose_rule(self.w.abs(), self.a.abs(), self.b.abs(), self.s).max()))

    def blind_spots(self):
        return 0

    def zero_fraction(self):
        """Of dA and dB (W_eff = w + s B A is compared whole; its zeros are as informative as its other entries)."""
        return (int((self.da == 0).sum()) + int((self.db == 0).sum())) / (self.da.numel() + self.db.numel())


@functools.lru_cache(maxsize=None)
def gemm_case(shape, kind):
    if kind != "exact":
        return GemmCase(shape, kind, 0)
    for salt in range(SALTS):
        c = GemmCase(shape, kind, salt)
        if c.zero_fraction() <= ZERO_FRACTION:
            return c
    return _rearranged(GemmCase(shape, kind, 0), (2, GEMM_SHAPES.index(shape)))


# ------------------------------------------------------------------------------------------------
# ops.refresh_filters: 50 tiny convolutions, more than one ynet_lora_compose_pack_multi launch holds (48)
# ------------------------------------------------------------------------------------------------
def refresh_layers():
    """[(cin, cout, K, r)]: K in {1, 3, 5} and r in {0 .. 3} in every combination, one 130 -> 65 layer whose tile count makes the workgroups of every other
    layer of its launch return early; r == 0 is a plain convolution."""
    rs = _rs(3)
    layers = []
    for i in range(50):
        K, r = (1, 3, 5)[i % 3], (0, 1, 2, 3)[(i // 3) % 4]
        layers.append((int(rs.randint(1, 20)), int(rs.randint(1, 20)), K, r))
    layers[7] = (130, 65, 3, 2)
    layers[49] = (9, 70, 1, 1)      # the second launch's largest layer; cout pads to 128 columns
    return layers


def refresh_values(i, shape, kind):
    """(w, A or None, B or None) of layer i, fp32 CPU."""
    cin, cout, K, r = shape
    rs = _rs(4, i, kind == "exact")
    if kind == "exact":
        return grid_pm1(rs, cout, cin, K, K), (grid_pm1(rs, r * K, cin * K) if r else None), (grid_pm1(rs, cout * K, r * K) if r else None)
    return gauss(rs, cout, cin, K, K), (gauss(rs, r * K, cin * K, scale=0.3) if r else None), (gauss(rs, cout * K, r * K, scale=0.1) if r else None)


# ------------------------------------------------------------------------------------------------
# comparison
# ------------------------------------------------------------------------------------------------
def mismatch(got, want, rtol, atol=0.0, scale_rel=None):
    """(bad elements, largest error / its bound) of got against the fp64 want; NaN-safe (an error that is not <= its bound is bad)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    assert got.shape == want.shape, (got.shape, want.shape)
    if scale_rel is not None:
        atol = max(atol, scale_rel * float(want.abs().max()))
    err = (got - want).abs()
    bound = atol + rtol * want.abs()
    bad = ~(err <= bound)
    ratio = float(torch.nan_to_num(err / bound, nan=float("inf")).max()) if err.numel() else 0.0
    return int(bad.sum()), ratio


def tol(family, name):
    return TOL_OVERRIDE.get((family, name), {"compose": TOL_COMPOSE, "grad": TOL_GRAD, "wgrad": TOL_WGRAD}[family])

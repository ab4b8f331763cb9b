"""Operands off a 16-byte boundary for the convolution family: the placements, the builder of offset views, the case tables and the fp64
references (tests/test_align_cases_host.py checks this module on the CPU, tests/test_gpu_conv_alignment.py runs the kernels against it).

Every fast path of ynet_conv2d / ynet_conv2d_wgrad / ynet_conv2d_auto is gated on operand alignment (pointer % 16, batch stride % 4 for the
LDS-DMA and streaming kernels; 16 / 8 bytes for the Winograd families).  Torch allocations are 256-byte aligned and a channel slice of a map with
W % 4 == 0 stays aligned, so only a view built on purpose reaches the other side of those gates: `offset_view`.

Every reference here is stock torch on .double() inputs on the CPU -- never the code under test."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

SEED = 20261019

# (off, pad) in floats: the view starts `off` floats into a 16-byte aligned buffer, its batch stride is C*H*W + pad
PLACEMENTS = [
    (1, 0),     # 4 bytes off
    (3, 0),     # 12 bytes off
    (2, 0),     # 8 bytes off: passes every 8-byte gate, fails every 16-byte gate
    (0, 2),     # image 0 aligned, batch stride = 2 mod 4: passes the `& 1` gates, fails the `& 3` gates
    (0, 1),     # odd batch stride
    (2, 2),     # both
]
OFFSETS_ONLY = [(1, 0), (2, 0), (3, 0)]      # for operands whose batch stride the wrapper fixes (dy)
TAIL = 64                                    # floats of slack behind the last image (a quad read past the end stays inside the buffer)

# the project's tolerances against fp64 (tests/test_gpu_kernels.py::test_conv2d_dispatch_sweep)
TOL_Y = dict(rtol=2e-5, atol=2e-5)
TOL_DX = dict(rtol=1e-4, scale_rel=2e-6)
TOL_DW = dict(rtol=1e-4, scale_rel=1e-5)
TOL_LORA = dict(rtol=2e-4, scale_rel=5e-6)   # dA / dB (test_lora_conv2d_wgrad_without_the_filter_gradient)
# |pre-activation| (and, behind a max-pool, the gap between a block's two largest elements) below which the fp32 kernels and the fp64 reference may
# disagree on a ReLU mask / an arg-max: 5 x the forward tolerance at |y| = 1, 2.5 x at the largest outputs of these cases (|y| < 6).  The gradient fed to the
# backward pass is zero there, so the device's own mask decides nothing the comparison sees -- what test_conv2d_dispatch_sweep achieves by driving
# the reference with the device's mask, with one reference per shape instead of one per run.
AMBIGUOUS = 2e-4


def _gen(*key):
    return torch.Generator().manual_seed(int(np.random.SeedSequence([SEED, *key]).generate_state(1)[0]))


def randn(*shape, key=0, scale=1.0):
    return torch.randn(*shape, generator=_gen(key, *shape)) * scale


def offset_view(t, off, pad, poison=float("nan"), alloc=None):
    """-> (view, buffer): `view` has the values and shape of t [B, C, H, W] and lives `off` floats into the flat fp32 `buffer` on t's device,
    with batch stride C*H*W + pad and contiguous planes; everything else in the buffer (before the view, between images, TAIL floats behind it) holds
    `poison`.  The buffer's base is 16-byte aligned (asserted), so view.data_ptr() % 16 == 4 * off % 16.  alloc(n): the flat buffer (tests)."""
    assert t.dim() == 4 and t.dtype == torch.float32 and off >= 0 and pad >= 0
    B, C, H, W = t.shape
    img = C * H * W
    n = off + B * (img + pad) + TAIL
    buf = alloc(n) if alloc is not None else torch.empty(n, device=t.device, dtype=torch.float32)
    assert buf.dim() == 1 and buf.numel() == n and buf.is_contiguous()
    assert buf.data_ptr() % 16 == 0, "offset_view: the buffer's base must be 16-byte aligned"
    buf.fill_(poison)
    view = buf.as_strided((B, C, H, W), (img + pad, H * W, W, 1), off)
    view.copy_(t)
    return view, buf


def slack_mask(shape, off, pad, device="cpu"):
    """Boolean mask over the flat buffer of offset_view(t of `shape`, off, pad): True where the buffer is slack."""
    B, C, H, W = shape
    img = C * H * W
    m = torch.ones(off + B * (img + pad) + TAIL, dtype=torch.bool, device=device)
    m.as_strided((B, img), (img + pad, 1), off).fill_(False)
    return m


def bits(t):
    return t.contiguous().view(torch.int32)


def slack_intact(buf, shape, off, pad, poison=float("nan")):
    """Is every slack float of the buffer still bit-identical to the poison?"""
    m = slack_mask(shape, off, pad, buf.device)
    want = bits(torch.full((1,), poison, dtype=torch.float32, device=buf.device))
    return bool((bits(buf)[m] == want).all())


def same_bits(a, b):
    return a.shape == b.shape and bool(torch.equal(bits(a), bits(b)))


def mismatch(got, want, rtol=2e-5, atol=2e-5, scale_rel=None):
    """(bad elements, largest error, atol used) of got against want, both on one device, in fp64.  NaN-safe: an error that is not <= the bound
    is bad, an element that is not finite in `got` where `want` is finite is bad."""
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (got.shape, want.shape)
    if scale_rel is not None:
        atol = max(atol, scale_rel * float(want.abs().max()))
    err = (got - want).abs()
    bad = ~(err <= atol + rtol * want.abs()) | (torch.isfinite(want) & ~torch.isfinite(got))
    return int(bad.sum()), float(torch.nan_to_num(err, nan=float("inf")).max()) if err.numel() else 0.0, atol


# ------------------------------------------------------------------------------------------------
# (a) ops.conv2d through autograd: every shape has W % 4 == 0, so alignment alone decides the path.
#   family: what the ALIGNED run takes; B, H, W, sources, cout, K, relu
#   fwd: the kernel the aligned forward launch must note (ynet_conv2d_last_launch(0)); wino: the Winograd family's tag instead.  The aligned filter gradient
#   takes an LDS-DMA / streaming kernel (noted 2, 3 or 4) unless wgrad_staged says that the register-staged tiles are all there is
# ------------------------------------------------------------------------------------------------
AUTOGRAD_CASES = {
    "dma_two_row": dict(shape=(2, 64, 64, [32], 32, 3, True), fwd=2, rows=2),
    "dma_two_row_cat": dict(shape=(4, 32, 64, [32, 16, 1], 32, 3, True), fwd=2, rows=2),      # (B 2 has too few two-row units: one-row tiles)
    "fold_4x8": dict(shape=(4, 8, 8, [65], 130, 3, True), fwd=3, rows=1),
    "fold_2x16": dict(shape=(4, 16, 16, [64, 2], 64, 3, True), fwd=3, rows=1),
    # (split: the input-channel loop is split over workgroups and conv_split_reduce_kernel writes the destination.  At B 8 the 32^2 map has the 64 two-row
    #  units of the LDS-DMA tile; one-row tiles -- register-staged at any alignment -- are what is left below that)
    "dma_split_k": dict(shape=(8, 32, 32, [64], 64, 3, True), fwd=2, rows=2, split=True),
    "one_row_split_k": dict(shape=(2, 32, 32, [64], 64, 3, True), fwd=1, rows=1, split=True),
    "stream_1x1_12": dict(shape=(2, 32, 32, [32], 12, 1, False), fwd=4),
    "stream_1x1_30": dict(shape=(2, 32, 32, [32], 30, 1, False), fwd=4),
    "k5": dict(shape=(1, 16, 16, [7], 9, 5, True), fwd=1, wgrad_staged=True),      # (5x5 has no DMA form: alignment only moves its epilogue stores)
    "winograd": dict(shape=(8, 128, 128, [32], 32, 3, True), wino="winograd:"),
    "winograd_cat": dict(shape=(8, 128, 128, [32, 16, 1], 32, 3, True), wino="winograd_cat:"),
    "slice_form": dict(shape=(10, 64, 64, [64], 64, 3, True), wino="winograd16:"),
    "pool_epilogue": dict(shape=(8, 128, 128, [6, 8], 32, 3, True), wino="winograd_cat:", pool=True),
}
CHAIN_CASE = (8, 128, 128, 32, 32, 32)            # conv -> ReLU -> conv: B, H, W, c0 -> c1 -> c2
LORA_CASE = (2, 32, 32, [32], 64)                 # a rank-1 loralib Conv2d, no ReLU (LORA_WGRAD_CASES)
UPCONV_CASE = (8, 64, 64, 32, 16)                 # bilinear x2 + conv: B, low-resolution H, W, cin -> cout

# (c) ops.conv2d_wgrad_raw: family -> (B, H, W, sources, cout, K, masked), the kernel noted when aligned (which = 1)
WGRAD_CASES = {
    "rolling_row": ((8, 64, 128, [32, 16], 32, 3, True), 3),      # (B 8: the 256 strip segments its persistent workgroups need)
    "dma_two_row": ((2, 64, 64, [64], 64, 3, False), 2),
    "stream_1x1": ((3, 16, 24, [32], 12, 1, False), 4),
    "k5": ((1, 16, 16, [7], 9, 5, False), 1),
}

# ynet_conv2d_auto_plan on stand-in pointers: the descriptors of tests/test_gpu_kernels.py::AUTO_CASES that a Winograd family, the pooled copy or the
# up-convolution serves, with the family (YnetConvTaken.family) the aligned descriptor plans
PLAN_CASES = {
    # name: (B, H, W, sources, destinations, relu, operands, family)
    "plain_32_32": (8, 256, 256, [32], [32], True, {}, 1),
    "plain_16_32_no_relu": (16, 128, 128, [16], [32], False, {}, 1),
    "dgrad_relu_of": (8, 256, 256, [32], [32], False, {"relu_of": True}, 1),
    "cat_48": (4, 256, 256, [32, 16], [32], True, {}, 2),
    "cat_49": (4, 256, 256, [32, 16, 1], [32], True, {}, 2),
    "split_65": (16, 128, 128, [64, 1], [32], True, {}, 2),
    "pool_code_first_layer": (4, 256, 256, [6, 8], [32], True, {"pooled": True}, 2),
    "pool_64_slice_form": (10, 64, 64, [64], [64], True, {"pooled": True}, 3),
    "slice_64_64": (10, 64, 64, [64], [64], True, {}, 3),
    "slice_dgrad_32_64_relu_of": (16, 128, 128, [32], [64], False, {"relu_of": True}, 3),
    "slice_cat_97_64": (10, 64, 64, [32, 64, 1], [64], True, {}, 3),
    "up_32_16": (8, 256, 256, [32], [16], False, {"upsample2x": True}, 4),
    "up_64_32": (16, 128, 128, [64], [32], False, {"upsample2x": True}, 5),
}


class ConvRef:
    """Seeded fp32 inputs of relu?(conv(cat(xs), w) + b) and its fp64 results: y, pre (the pre-activation), and -- for the output gradient `gy`, which is
    zero wherever the ReLU mask is AMBIGUOUS -- dxs, dw, db.  pooled / gp: the 2 x 2 max-pooled output and the gradient fed to it (then gy is None)."""

    def __init__(self, B, H, W, cs, cout, K, relu, pool=False, seed=0):
        cin = sum(cs)
        self.shape = (B, H, W, tuple(cs), cout, K, relu)
        self.xs = [randn(B, c, H, W, key=(seed, 1 + i)) for i, c in enumerate(cs)]
        self.w = randn(cout, cin, K, K, key=(seed, 10), scale=1.0 / (cin * K * K) ** 0.5)
        self.b = randn(cout, key=(seed, 11), scale=0.1)
        xs64 = [x.double().requires_grad_(True) for x in self.xs]
        w64, b64 = self.w.double().requires_grad_(True), self.b.double().requires_grad_(True)
        pre = F.conv2d(torch.cat(xs64, 1), w64, b64, padding=K // 2)
        y = F.relu(pre) if relu else pre
        self.pre, self.y = pre.detach(), y.detach()
        clear = (self.pre.abs() >= AMBIGUOUS) if relu else torch.ones_like(self.pre, dtype=torch.bool)
        self.gy = self.gp = self.pooled = None
        if pool:
            blocks = self.y.view(B, cout, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, cout, H // 2, W // 2, 4)
            top = blocks.topk(2, dim=-1).values
            sure = ((top[..., 0] - top[..., 1]) >= 5 * AMBIGUOUS) & (top[..., 0] >= 5 * AMBIGUOUS)      # (two elements, each off by the forward tolerance)
            self.gp = randn(B, cout, H // 2, W // 2, key=(seed, 12)) * sure
            p = F.max_pool2d(y, 2, 2)
            self.pooled = p.detach()
            p.backward(self.gp.double())
        else:
            self.gy = randn(B, cout, H, W, key=(seed, 12)) * clear
            y.backward(self.gy.double())
        self.dxs, self.dw, self.db = [x.grad for x in xs64], w64.grad, b64.grad


@functools.lru_cache(maxsize=None)
def conv_ref(B, H, W, cs, cout, K, relu, pool=False):
    return ConvRef(B, H, W, list(cs), cout, K, relu, pool)


class ChainRef:
    """conv0 -> ReLU -> conv1 (3 x 3, no bias, no second ReLU: conv1's backward carries no mask of its own, so its data gradient may take conv0's) in fp64.
    gy is zero in the 3 x 3 neighbourhood (all channels) of every position where conv0's mask is ambiguous: the gradient that reaches such an element of
    conv0's output is then exactly zero on the device and in the reference, whichever way the device's mask fell."""

    def __init__(self, B, H, W, c0, c1, c2):
        self.x = randn(B, c0, H, W, key=(7, 1))
        self.w0 = randn(c1, c0, 3, 3, key=(7, 2), scale=1.0 / (c0 * 9) ** 0.5)
        self.w1 = randn(c2, c1, 3, 3, key=(7, 3), scale=1.0 / (c1 * 9) ** 0.5)
        x64, w0, w1 = (t.double().requires_grad_(True) for t in (self.x, self.w0, self.w1))
        pre0 = F.conv2d(x64, w0, padding=1)
        y = F.conv2d(F.relu(pre0), w1, padding=1)
        self.y = y.detach()
        near = (pre0.detach().abs() < AMBIGUOUS).any(1, keepdim=True).double()
        near = F.max_pool2d(near, 3, 1, 1) > 0
        self.gy = randn(B, c2, H, W, key=(7, 4)) * ~near
        y.backward(self.gy.double())
        self.dx, self.dw0, self.dw1 = x64.grad, w0.grad, w1.grad


@functools.lru_cache(maxsize=None)
def chain_ref():
    return ChainRef(*CHAIN_CASE)


class LoraRef:
    """conv(cat(xs), W + s (B @ A).view(W.shape)), rank 1, no bias, no ReLU: fp64 y, dxs, dA, dB."""

    def __init__(self, B, H, W, cs, cout):
        cin, k, r = sum(cs), 3, 1
        self.scale = 1.0 / r
        self.xs = [randn(B, c, H, W, key=(8, 1 + i)) for i, c in enumerate(cs)]
        self.w = randn(cout, cin, k, k, key=(8, 10), scale=1.0 / (cin * 9) ** 0.5)
        self.a, self.bm = randn(r * k, cin * k, key=(8, 11), scale=0.3), randn(cout * k, r * k, key=(8, 12), scale=0.1)
        self.gy = randn(B, cout, H, W, key=(8, 13))
        xs64 = [x.double().requires_grad_(True) for x in self.xs]
        a64, b64 = self.a.double().requires_grad_(True), self.bm.double().requires_grad_(True)
        y = F.conv2d(torch.cat(xs64, 1), self.w.double() + (b64 @ a64).view(self.w.shape) * self.scale, None, padding=1)
        y.backward(self.gy.double())
        self.y, self.dxs, self.da, self.db = y.detach(), [x.grad for x in xs64], a64.grad, b64.grad


@functools.lru_cache(maxsize=None)
def lora_ref():
    return LoraRef(*LORA_CASE)


@functools.lru_cache(maxsize=None)
def upconv_ref():
    """x (a post-ReLU map), w, b and conv3x3(bilinear x2 of x) + b in fp64."""
    B, Hl, Wl, cin, cout = UPCONV_CASE
    x = torch.relu(randn(B, cin, Hl, Wl, key=(9, 1)))
    w, b = randn(cout, cin, 3, 3, key=(9, 2), scale=1.0 / (cin * 9) ** 0.5), randn(cout, key=(9, 3), scale=0.1)
    y = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False), w.double(), b.double(), padding=1)
    return x, w, b, y


def plan_desc(L, name, base=4096):
    """The YnetConvAuto of PLAN_CASES[name] on 16-byte aligned stand-in pointers (ynet_conv2d_auto_plan looks at pointers for alignment and NULL only)."""
    B, H, W, cs, couts, relu, opts, _ = PLAN_CASES[name]
    d = L.ConvAuto()
    d.nsrc, d.ndst = len(cs), len(couts)
    up = bool(opts.get("upsample2x"))
    hw_src = (H // 2) * (W // 2) if up else H * W
    for i, c in enumerate(cs):
        d.src[i], d.src_c[i], d.src_bs[i] = base * (1 + i), c, c * hw_src
    for i, c in enumerate(couts):
        d.dst[i], d.dst_c[i], d.dst_bs[i] = base * (8 + i), c, c * H * W
    d.wp, d.B, d.H, d.W, d.K, d.relu, d.upsample2x = base * 16, B, H, W, 3, int(relu), int(up)
    if opts.get("relu_of"):
        d.relu_of, d.relu_of_bs = base * 17, sum(couts) * H * W
    if opts.get("pooled"):
        d.pooled, d.pooled_bs = base * 18, sum(couts) * (H // 2) * (W // 2)
    return d

"""Per-kernel parity on the MI355X: every entry point of the C ABI against the CPU oracle / stock
torch ops on the same seeded inputs, plus the reference-generated vectors in golden/kernels.npz.

Tolerances (fp32): activations rtol 2e-5 / atol 2e-5 (different accumulation order than MKL-DNN);
gradients rtol 2e-4 relative to the tensor's scale; integer-like ops (max-pool, gather) bit-exact.
"""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import Golden, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def close(got, want, rtol=2e-5, atol=2e-5, scale_rel=None, msg=""):
    got, want = got.detach().cpu().double(), want.detach().cpu().double()
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    if scale_rel is not None:
        atol = max(atol, scale_rel * float(want.abs().max()))
    err = (got - want).abs()
    # (NaN-safe: an error that is not <= the bound is bad -- `err > bound` is False for a NaN; an element that is NaN on both sides counts as equal)
    bad = ~(err <= atol + rtol * want.abs()) & ~(torch.isnan(got) & torch.isnan(want))
    assert not bool(bad.any()), f"{msg}: max err {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e} (atol {atol:.2e}), {int(bad.sum())} bad of {bad.numel()}"


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


CONV_CASES = [
    # B, H, W, [source channels], cout, K, relu
    (2, 16, 32, [14], 32, 3, True),
    (1, 64, 64, [32], 32, 3, True),
    (2, 32, 64, [32, 16, 1], 32, 3, True),      # decoder conv: up + skip + waypoint map
    (2, 8, 8, [65], 130, 3, True),              # trajectory-decoder centre (odd channels, tiny map)
    (3, 24, 40, [5, 3], 16, 3, False),          # ragged tile edges, no ReLU
    (2, 32, 32, [32], 12, 1, False),            # 1x1 predictor
    (1, 16, 16, [7], 9, 5, True),               # 5x5 (adapter kernels)
    (2, 16, 16, [64, 33], 64, 3, True),
    (1, 40, 72, [16, 16, 8, 2], 48, 3, True),   # 4 sources
]


@pytest.mark.parametrize("B,H,W,cs,cout,K,relu", CONV_CASES)
def test_conv2d_forward_backward(dev, B, H, W, cs, cout, K, relu):
    ops = pkg("ops")
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=i + 1) for i, c in enumerate(cs)]
    w = rnd(cout, cin, K, K, seed=10, scale=1.0 / (cin * K * K) ** 0.5)
    b = rnd(cout, seed=11, scale=0.1)
    gy = rnd(B, cout, H, W, seed=12)
    # oracle: stock torch on CPU
    xc = [x.clone().requires_grad_(True) for x in xs]
    wc, bc = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(torch.cat(xc, 1), wc, bc, padding=K // 2)
    y = F.relu(y) if relu else y
    y.backward(gy)
    # HIP
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    yd = ops.conv2d(ops.lazy_cat(xd), wd, bd, relu, {})
    yd.backward(gy.to(dev))
    close(yd, y, msg="y")
    for i, (a, c) in enumerate(zip(xd, xc)):
        close(a.grad, c.grad, rtol=1e-4, scale_rel=2e-6, msg=f"dx{i}")
    close(wd.grad, wc.grad, rtol=1e-4, scale_rel=5e-6, msg="dW")
    close(bd.grad, bc.grad, rtol=1e-4, scale_rel=5e-6, msg="db")


def _sweep_cases():
    """Seeded shapes that walk the dispatcher: every tile-row count, folded tiles of the 8 / 16 wide maps, split-K on small
    maps, 16- and 32-wide output tiles, ragged widths that fall back to the register-staged kernels, 1..4 sources."""
    rs = np.random.RandomState(1234)
    cases = [
        # B, H, W, sources, cout, K, relu        (targeted: the production tile shapes at reduced batch)
        (8, 256, 256, [14], 32, 3, True),       # 4-row tiles, 1024+ workgroups
        (4, 256, 256, [32, 16], 32, 3, True),   # decoder level 4 (48 -> 32)
        (8, 128, 128, [64, 1], 32, 3, False),
        (16, 64, 64, [64, 32], 64, 3, True),    # 2-row tiles
        (32, 32, 32, [64], 64, 3, True),        # 1-row tiles + split-K
        (32, 16, 16, [128, 2], 64, 3, True),    # folded 2 x 16
        (32, 8, 8, [65], 130, 3, True),         # folded 4 x 8, odd channels
        (4, 256, 256, [32], 12, 1, False),      # streaming 1x1 predictor
        (4, 128, 128, [12], 32, 1, False),
    ]
    widths = [4, 8, 12, 16, 20, 28, 32, 36, 48, 64, 72, 100, 128]
    for _ in range(27):
        W = int(widths[rs.randint(len(widths))])
        H = int(rs.choice([1, 2, 3, 5, 8, 16, 17, 32, 40, 64]))
        K = int(rs.choice([1, 3, 3, 3, 5]))
        nsrc = int(rs.randint(1, 5))
        cs = [int(rs.choice([1, 2, 3, 5, 8, 16, 17, 32, 33, 64])) for _ in range(nsrc)]
        if K == 5:
            cs = [min(c, 8) for c in cs]
        cout = int(rs.choice([1, 3, 12, 16, 17, 32, 33, 48, 64, 65, 96, 130]))
        B = int(rs.choice([1, 2, 3, 5, 9]))
        cases.append((B, H, W, cs, cout, K, bool(rs.randint(2))))
    # widths that are NOT multiples of 4 (odd ones included): no 16-byte DMA / stores -> the register-staged conv and
    # wgrad kernels with scalar epilogue stores (real scenes are padded to multiples of 32, but their deep levels and
    # any direct caller of the C ABI are not)
    rs2 = np.random.RandomState(4321)
    for W in [1, 2, 3, 5, 6, 7, 9, 13, 15, 18, 30, 33, 37, 50, 63, 65, 129]:
        H = int(rs2.choice([1, 2, 3, 5, 8, 16, 17, 33]))
        K = int(rs2.choice([1, 3, 3, 3, 5]))
        nsrc = int(rs2.randint(1, 4))
        cs = [int(rs2.choice([1, 3, 8, 16, 17, 32, 33, 64])) for _ in range(nsrc)]
        if K == 5:
            cs = [min(c, 8) for c in cs]
        cout = int(rs2.choice([1, 12, 16, 17, 32, 48, 64, 65, 130]))
        B = int(rs2.choice([1, 2, 3, 5]))
        cases.append((B, H, W, cs, cout, K, bool(rs2.randint(2))))
    # the benchmarked batch (B = 32 per GPU; B = 16 at 512^2): persistent grids, rows-per-wave and split-K choices at
    # the sizes bench.py runs
    cases += [
        (32, 256, 256, [32, 16], 32, 3, True),      # decoder.4.0 (48 -> 32), the dominant launch
        (32, 256, 256, [32], 16, 3, False),         # upsample_conv.4
        (32, 128, 128, [64], 32, 3, False),         # upsample_conv.3
        (32, 64, 64, [64, 32, 1], 64, 3, True),     # trajectory decoder.2.0 (97 -> 64)
        (32, 8, 8, [128], 128, 3, True),            # goal centre, split-K
        (16, 512, 512, [6], 16, 3, True),           # C4 scene stage 0
        (32, 256, 256, [32], 12, 1, False),         # predictor
    ]
    return cases


@pytest.mark.parametrize("case", _sweep_cases(), ids=lambda c: "B{}_{}x{}_c{}_o{}_k{}_{}".format(
    c[0], c[1], c[2], "+".join(map(str, c[3])), c[4], c[5], "relu" if c[6] else "lin"))
def test_conv2d_dispatch_sweep(dev, case):
    """Forward, dgrad (all sources), wgrad and bias gradient of every dispatch path against stock torch on the CPU."""
    B, H, W, cs, cout, K, relu = case
    ops = pkg("ops")
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=i + 1) for i, c in enumerate(cs)]
    w = rnd(cout, cin, K, K, seed=10, scale=1.0 / (cin * K * K) ** 0.5)
    b = rnd(cout, seed=11, scale=0.1)
    gy = rnd(B, cout, H, W, seed=12)
    xc = [x.clone().requires_grad_(True) for x in xs]
    wc, bc = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    pre = F.conv2d(torch.cat(xc, 1), wc, bc, padding=K // 2)
    y = F.relu(pre) if relu else pre
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    wd, bd = w.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
    yd = ops.conv2d(ops.lazy_cat(xd), wd, bd, relu, {})
    yd.backward(gy.to(dev))
    close(yd, y, msg="y")
    # The ReLU gradient is discontinuous at 0: among 10^7..10^8 outputs a handful of pre-activations round to opposite
    # sides of 0 on the CPU and on the GPU (|pre| ~ 1e-8) and each such element changes 9 * Cin input gradients by O(1).
    # The backward pass is therefore checked against stock torch driven with the DEVICE's own mask (y > 0).
    pre.backward(gy * (yd.detach().cpu() > 0).float() if relu else gy)
    for i, (a, c) in enumerate(zip(xd, xc)):
        close(a.grad, c.grad, rtol=1e-4, scale_rel=2e-6, msg=f"dx{i}")
    close(wd.grad, wc.grad, rtol=1e-4, scale_rel=1e-5, msg="dW")
    close(bd.grad, bc.grad, rtol=1e-4, scale_rel=1e-5, msg="db")


def test_conv2d_broadcast_source_and_partial_grads(dev):
    """Semantic map shared by the batch (stride-0 expand) + only some inputs wanting gradients."""
    ops = pkg("ops")
    B, H, W = 3, 32, 32
    sem = rnd(1, 6, H, W, seed=1)
    mot = rnd(B, 8, H, W, seed=2)
    w, b = rnd(32, 14, 3, 3, seed=3, scale=0.1), rnd(32, seed=4, scale=0.1)
    y = F.relu(F.conv2d(torch.cat([sem.expand(B, -1, -1, -1), mot], 1), w, b, padding=1))
    motd = mot.to(dev).requires_grad_(True)
    yd = ops.conv2d(ops.lazy_cat([sem.to(dev).expand(B, -1, -1, -1), motd]), w.to(dev), b.to(dev), True, {})
    close(yd, y, msg="broadcast")
    yd.sum().backward()            # first source wants no gradient, second does
    mc = mot.clone().requires_grad_(True)
    F.relu(F.conv2d(torch.cat([sem.expand(B, -1, -1, -1), mc], 1), w, b, padding=1)).sum().backward()
    close(motd.grad, mc.grad, rtol=1e-4, scale_rel=2e-6, msg="partial grad")


def test_conv2d_is_deterministic(dev):
    ops = pkg("ops")
    x, w, b = rnd(2, 33, 40, 40, seed=1).to(dev), rnd(40, 33, 3, 3, seed=2).to(dev).requires_grad_(True), rnd(40, seed=3).to(dev)
    outs = []
    for _ in range(2):
        w.grad = None
        y = ops.conv2d(x, w, b, True, {})
        y.square().sum().backward()
        outs.append((y.detach().clone(), w.grad.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("cout,cin,r", [(32, 14, 1), (64, 32, 4), (16, 6, 3), (64, 64, 1)])
def test_lora_compose_and_grad(dev, cout, cin, r):
    ops = pkg("ops")
    k = 3
    w, a, bm = rnd(cout, cin, k, k, seed=1), rnd(r * k, cin * k, seed=2), rnd(cout * k, r * k, seed=3, scale=0.1)
    sd = {"l.weight": w, "l.lora_A": a, "l.lora_B": bm}
    want = O.effective_weight(sd, "l")
    got = ops.lora_compose(w.to(dev), a.to(dev), bm.to(dev), 1.0 / r)
    close(got, want, rtol=1e-5, atol=1e-6, msg="w_eff")
    dw = rnd(cout, cin, k, k, seed=4)
    ac, bc = a.clone().requires_grad_(True), bm.clone().requires_grad_(True)
    ((bc @ ac).view(w.shape) * (1.0 / r) * dw).sum().backward()
    d_a, d_b = ops.lora_grad(dw.to(dev), a.to(dev), bm.to(dev), 1.0 / r)
    close(d_a, ac.grad, rtol=1e-4, scale_rel=2e-6, msg="dA")
    close(d_b, bc.grad, rtol=1e-4, scale_rel=2e-6, msg="dB")


ROLL_WGRAD_CASES = [
    # B, H, W, [source channels], cout, ReLU mask, bias -- maps with enough 32-column strips for the rolling-row kernel
    (4, 128, 256, [6, 8], 32, True, True),      # encoder.stages.0.0: two sources, 14 channels (spare waves take K-step residues)
    (8, 64, 128, [32, 16], 32, True, False),    # 48 input channels = a full and a half channel block, segments of 4 steps
    (8, 64, 64, [64], 64, False, True),         # 2 x 2 blocks without a mask: 192 workgroups want 192 segments, B 8 has 128 -- the two-row LDS-DMA tiles (kernel 2)
    (4, 256, 128, [32], 16, True, True),        # half an output block
    (2, 256, 256, [32], 32, False, False),      # one block without a mask: 768 workgroups want 768 segments, B 2 has 512 -- the two-row LDS-DMA tiles (kernel 2)
    (12, 64, 64, [64], 64, False, True),        # 2 x 2 blocks on the unmasked rolling-row kernel: 192 segments of 4 steps, first and last tile column only
    (3, 256, 256, [32], 32, False, False),      # one block on the unmasked rolling-row kernel: 768 segments of 4 steps; interior tile columns
]
ROLL_WGRAD_KERNEL = [3, 3, 2, 3, 2, 3, 3]        # what ynet_conv2d_last_launch(1) must note for each (tests/test_wgrad_cases_host.py asks the plan the same)


@pytest.mark.parametrize("B,H,W,cs,cout,relu,bias", ROLL_WGRAD_CASES)
def test_conv2d_wgrad_rolling_rows(dev, B, H, W, cs, cout, relu, bias):
    """wgrad_roll_kernel (x rows kept in an LDS ring while a workgroup walks down a strip): dW / db against stock autograd at
    shapes that take it (image top / bottom pairs, first / last tile columns, segment starts), bitwise reproducible."""
    ops = pkg("ops")
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=i + 1) for i, c in enumerate(cs)]
    w = rnd(cout, cin, 3, 3, seed=10, scale=1.0 / (cin * 9) ** 0.5)
    b = rnd(cout, seed=11, scale=0.1)
    gy = rnd(B, cout, H, W, seed=12)
    wc, bc = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    y = F.conv2d(torch.cat(xs, 1), wc, bc, padding=1)
    y = F.relu(y) if relu else y
    y.backward(gy)
    xd, yd, gyd = [x.to(dev) for x in xs], y.detach().to(dev), gy.to(dev)
    mask = (yd.data_ptr(), cout * H * W) if relu else None
    ops._lib().ynet_conv2d_last_launch(1)
    dw, db = ops.conv2d_wgrad_raw(xd, gyd, mask, w.to(dev), bias)
    assert ops._lib().ynet_conv2d_last_launch(1) == ROLL_WGRAD_KERNEL[ROLL_WGRAD_CASES.index((B, H, W, cs, cout, relu, bias))]
    close(dw, wc.grad, rtol=1e-4, scale_rel=1e-5, msg="dW")
    if bias:
        close(db, bc.grad, rtol=1e-4, scale_rel=1e-5, msg="db")
    dw2, db2 = ops.conv2d_wgrad_raw(xd, gyd, mask, w.to(dev), bias)
    assert torch.equal(dw, dw2) and (not bias or torch.equal(db, db2))


@pytest.mark.parametrize("B,H,W,cout,bias", [(3, 16, 24, 12, True), (2, 64, 64, 30, True), (5, 8, 8, 32, False), (1, 4, 4, 7, True), (33, 32, 32, 12, True)])
def test_conv1x1_wgrad_streaming_kernel(dev, B, H, W, cout, bias):
    """wgrad1x1_stream_kernel (the predictors' filter / bias gradient, 32 -> pred_len): against stock autograd, for one and
    two output-channel tiles, maps smaller than the grid and chunk walks that cross image borders; reproducible."""
    ops = pkg("ops")
    x, w, b = rnd(B, 32, H, W, seed=1), rnd(cout, 32, 1, 1, seed=2, scale=0.3), rnd(cout, seed=3, scale=0.1)
    gy = rnd(B, cout, H, W, seed=4)
    wc, bc = w.clone().requires_grad_(True), b.clone().requires_grad_(True)
    F.conv2d(x, wc, bc).backward(gy)
    dw, db = ops.conv2d_wgrad_raw([x.to(dev)], gy.to(dev), None, w.to(dev), bias)
    close(dw, wc.grad, rtol=1e-4, scale_rel=1e-5, msg="dW 1x1")
    if bias:
        close(db, bc.grad, rtol=1e-4, scale_rel=1e-5, msg="db 1x1")
    dw2, _ = ops.conv2d_wgrad_raw([x.to(dev)], gy.to(dev), None, w.to(dev), bias)
    assert torch.equal(dw, dw2)
    # a batch-strided view of a wider tensor as the source (the decoder's last activation inside a larger buffer)
    big = rnd(B, 40, H, W, seed=5).to(dev)
    dw3, _ = ops.conv2d_wgrad_raw([big[:, 8:40]], gy.to(dev), None, w.to(dev), False)
    F.conv2d(big[:, 8:40].cpu(), wc2 := w.clone().requires_grad_(True)).backward(gy)
    close(dw3, wc2.grad, rtol=1e-4, scale_rel=1e-5, msg="dW 1x1 strided")


LORA_WGRAD_CASES = [
    # B, H, W, [source channels], cout, ReLU mask
    (2, 16, 32, [14], 32, True),            # tiny; W = one tile
    (2, 32, 64, [6, 8], 32, True),          # two sources (scene + motion maps of encoder.stages.0.0), 4-row tiles
    (3, 24, 40, [32], 32, True),            # ragged tile edges (H % 4 != 0 rows past the image, W not a multiple of 32)
    (2, 16, 16, [64], 64, True),            # 2-row tiles, a map narrower than the tile
    (2, 32, 32, [32], 64, False),           # no ReLU
    (1, 8, 8, [64], 64, True),
    (4, 64, 64, [33], 17, True),            # odd channel counts: 2-row tiles, partial column / channel blocks
]


@pytest.mark.parametrize("B,H,W,cs,cout,relu", LORA_WGRAD_CASES)
def test_lora_conv2d_wgrad_without_the_filter_gradient(dev, B, H, W, cs, cout, relu):
    """ynet_lora_conv2d_wgrad (dA / dB of a rank-1 loralib Conv2d from projected planes) against stock autograd through
    W + (B @ A).view(W.shape) * s, and against the two-call chain ynet_conv2d_wgrad -> ynet_lora_grad it replaces."""
    ops = pkg("ops")
    cin, r, k = sum(cs), 1, 3
    xs = [rnd(B, c, H, W, seed=i + 1) for i, c in enumerate(cs)]
    w = rnd(cout, cin, k, k, seed=10, scale=1.0 / (cin * 9) ** 0.5)
    a, bm = rnd(r * k, cin * k, seed=11, scale=0.3), rnd(cout * k, r * k, seed=12, scale=0.1)
    gy = rnd(B, cout, H, W, seed=13)
    scale = 1.0 / r
    ac, bc = a.clone().requires_grad_(True), bm.clone().requires_grad_(True)
    y = F.conv2d(torch.cat(xs, 1), w + (bc @ ac).view(w.shape) * scale, None, padding=1)
    y = F.relu(y) if relu else y
    y.backward(gy)
    xd = [x.to(dev) for x in xs]
    yd, gyd = y.detach().to(dev), gy.to(dev)
    mask = (yd.data_ptr(), cout * H * W) if relu else None
    assert ops.lora_conv2d_wgrad_supported(xd, gyd, w.to(dev), a.to(dev))
    d_a, d_b = ops.lora_conv2d_wgrad_raw(xd, gyd, mask, w.to(dev), a.to(dev), bm.to(dev), scale)
    close(d_a, ac.grad, rtol=2e-4, scale_rel=5e-6, msg="dA vs autograd")
    close(d_b, bc.grad, rtol=2e-4, scale_rel=5e-6, msg="dB vs autograd")
    dw, _ = ops.conv2d_wgrad_raw(xd, gyd, mask, w.to(dev), False)
    e_a, e_b = ops.lora_grad(dw, a.to(dev), bm.to(dev), scale)
    close(d_a, e_a, rtol=2e-4, scale_rel=5e-6, msg="dA vs the two-call chain")
    close(d_b, e_b, rtol=2e-4, scale_rel=5e-6, msg="dB vs the two-call chain")
    # bitwise reproducible (fixed-order reductions, no atomics)
    f_a, f_b = ops.lora_conv2d_wgrad_raw(xd, gyd, mask, w.to(dev), a.to(dev), bm.to(dev), scale)
    assert torch.equal(d_a, f_a) and torch.equal(d_b, f_b)


def test_lora_conv2d_wgrad_at_the_production_shapes(dev):
    """The encoder's adapted convs at the benchmarked batch (B = 32: 14 -> 32 @ 256^2 with the batch-broadcast scene as
    first source, 32 -> 32 @ 128^2, 64 -> 64 @ 64^2 and @ 16^2): against the two-call chain on the device."""
    ops = pkg("ops")
    gen = torch.Generator(device="cpu").manual_seed(5)
    for (cs, cout, HW, bcast) in (([6, 8], 32, 256, True), ([32], 32, 128, False), ([64], 64, 64, False), ([64], 64, 16, False)):
        B, cin = 32, sum(cs)
        xs = []
        for i, c in enumerate(cs):
            if bcast and i == 0:
                xs.append(torch.randn(1, c, HW, HW, generator=gen).to(dev).expand(B, -1, -1, -1))
            else:
                xs.append(torch.randn(B, c, HW, HW, generator=gen).to(dev))
        yact = torch.randn(B, cout, HW, HW, generator=gen).to(dev).relu_()
        gy = torch.randn(B, cout, HW, HW, generator=gen).to(dev)
        w = torch.randn(cout, cin, 3, 3, generator=gen).to(dev)
        a = (torch.randn(3, 3 * cin, generator=gen) * 0.3).to(dev)
        bm = (torch.randn(3 * cout, 3, generator=gen) * 0.1).to(dev)
        mask = (yact.data_ptr(), cout * HW * HW)
        assert ops.lora_conv2d_wgrad_supported(xs, gy, w, a)
        d_a, d_b = ops.lora_conv2d_wgrad_raw(xs, gy, mask, w, a, bm, 1.0)
        dw, _ = ops.conv2d_wgrad_raw(xs, gy, mask, w, False)
        e_a, e_b = ops.lora_grad(dw, a, bm, 1.0)
        close(d_a, e_a, rtol=5e-4, scale_rel=2e-5, msg=f"dA {cs}->{cout} @ {HW}")
        close(d_b, e_b, rtol=5e-4, scale_rel=2e-5, msg=f"dB {cs}->{cout} @ {HW}")


def test_lora_conv_end_to_end_and_identity_at_init(dev):
    """loralib semantics through the conv: grads of lora_A/B; zero lora_B == base conv bit-exactly
    (the reference's --init_check, train.py:46-59)."""
    ops = pkg("ops")
    B, cin, cout, H, W, r = 2, 14, 32, 32, 32, 2
    x = rnd(B, cin, H, W, seed=1)
    w, b = rnd(cout, cin, 3, 3, seed=2, scale=0.1), rnd(cout, seed=3, scale=0.1)
    a, bm = rnd(r * 3, cin * 3, seed=4, scale=0.2), rnd(cout * 3, r * 3, seed=5, scale=0.05)
    ac, bc = a.clone().requires_grad_(True), bm.clone().requires_grad_(True)
    y = F.relu(F.conv2d(x, w + (bc @ ac).view(w.shape) / r, b, padding=1))
    gy = rnd(B, cout, H, W, seed=6)
    y.backward(gy)
    ad, bd = a.to(dev).requires_grad_(True), bm.to(dev).requires_grad_(True)
    yd = ops.conv2d(x.to(dev), w.to(dev), b.to(dev), True, {}, ad, bd, 1.0 / r)
    yd.backward(gy.to(dev))
    close(yd, y, msg="lora y")
    close(ad.grad, ac.grad, rtol=2e-4, scale_rel=5e-6, msg="dA")
    close(bd.grad, bc.grad, rtol=2e-4, scale_rel=5e-6, msg="dB")
    y0 = ops.conv2d(x.to(dev), w.to(dev), b.to(dev), True, {}, a.to(dev), torch.zeros_like(bm).to(dev), 1.0 / r)
    y1 = ops.conv2d(x.to(dev), w.to(dev), b.to(dev), True, {})
    assert torch.equal(y0, y1)


def test_refresh_filters_packs_every_changed_conv_in_one_launch(dev):
    """ops.refresh_filters (ynet_lora_compose_pack_multi, rank 0 = plain conv) == the per-layer routines, bit for bit;
    untouched layers are skipped, changed ones are written again into the same buffers."""
    ops, ynet = pkg("ops"), pkg("models.ynet")
    torch.manual_seed(3)

    class Net(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a = ynet.HipConv2d(14, 32, 3)
            self.b = ynet.LoRAConv2d(32, 64, 3, r=2)
            self.c = ynet.HipConv2d(64, 12, 1)
            self.d = ynet.HipConv2d(7, 9, 5, bias=False)
            self.e = ynet.LoRAConv2d(33, 16, 3, r=1)
    net = Net()
    with torch.no_grad():
        for m in (net.b, net.e):
            m.lora_B.normal_(0, 0.05)
    net.to(dev)
    ops.refresh_filters(net)
    for m in (net.a, net.c, net.d):
        w = m.weight.detach()
        assert torch.equal(m._packed["fwd"], ops.pack_weight(w, 0)) and torch.equal(m._packed["dgrad"], ops.pack_weight(w, 1))
    for m in (net.b, net.e):
        fwd, dgrad = ops.lora_compose_pack(m.weight.detach(), m.lora_A.detach(), m.lora_B.detach(), m.scaling)
        assert torch.equal(m._packed["fwd"], fwd) and torch.equal(m._packed["dgrad"], dgrad)
    ptrs = {n: (m._packed["fwd"].data_ptr(), m._packed["dgrad"].data_ptr()) for n, m in net.named_children()}
    old_c = net.c._packed["fwd"].clone()
    with torch.no_grad():
        net.a.weight.mul_(1.5)
        net.e.lora_A.add_(0.25)
    ops.refresh_filters(net)
    assert {n: (m._packed["fwd"].data_ptr(), m._packed["dgrad"].data_ptr()) for n, m in net.named_children()} == ptrs
    assert torch.equal(net.a._packed["fwd"], ops.pack_weight(net.a.weight.detach(), 0))
    fwd, dgrad = ops.lora_compose_pack(net.e.weight.detach(), net.e.lora_A.detach(), net.e.lora_B.detach(), net.e.scaling)
    assert torch.equal(net.e._packed["fwd"], fwd) and torch.equal(net.e._packed["dgrad"], dgrad)
    assert torch.equal(net.c._packed["fwd"], old_c)
    # the convs use what refresh_filters wrote
    x = rnd(2, 14, 16, 16, seed=5).to(dev)
    y = net.a(x, relu=True)
    close(y, F.relu(F.conv2d(x.cpu(), net.a.weight.detach().cpu(), net.a.bias.detach().cpu(), padding=1)), msg="conv after refresh")


@pytest.mark.parametrize("shape", [(2, 3, 16, 32), (1, 5, 10, 14), (2, 2, 7, 9)])
def test_maxpool(dev, shape):
    ops = pkg("ops")
    x = rnd(*shape, seed=1)
    x[0, 0, :2, :2] = 0.0                       # ties: the first maximum takes the gradient
    xc = x.clone().requires_grad_(True)
    y = F.max_pool2d(xc, 2, 2)
    gy = rnd(*y.shape, seed=2)
    y.backward(gy)
    xd = x.to(dev).requires_grad_(True)
    yd = ops.max_pool2(xd)
    yd.backward(gy.to(dev))
    assert torch.equal(yd.cpu(), y.detach())
    assert torch.equal(xd.grad.cpu(), xc.grad)


def test_skip_gradients_fold_into_maxpool_backward(dev):
    """A feature map consumed by a max-pool AND by two convolutions (the decoders' skip connections): the conv
    backwards hand their gradients to the pool's backward (ynet_maxpool2_bwd_add) instead of autograd adding them;
    the total must equal stock autograd, with folding on and off, and the pool-first order must fall back."""
    ops = pkg("ops")
    x = rnd(2, 6, 16, 32, seed=1)
    w0, w1, w2 = rnd(8, 6, 3, 3, seed=2, scale=0.2), rnd(4, 8, 3, 3, seed=3, scale=0.2), rnd(5, 10, 3, 3, seed=4, scale=0.2)
    extra = rnd(2, 2, 16, 32, seed=5)
    # stock torch
    xc = x.clone().requires_grad_(True)
    f = F.relu(F.conv2d(xc, w0, padding=1))
    loss = F.max_pool2d(f, 2, 2).square().sum() + F.conv2d(f, w1, padding=1).sum() * 0.5 \
        + F.conv2d(torch.cat([f, extra], 1), w2, padding=1).square().sum()
    loss.backward()
    import contextlib
    for fold in (True, False):
        with (ops.fold_skip_gradients() if fold else contextlib.nullcontext()):
            assert ops.skip_fold == fold
            xd = x.to(dev).requires_grad_(True)
            fd = ops.conv2d(xd, w0.to(dev), None, True, {})
            ld = ops.max_pool2(fd).square().sum() + ops.conv2d(fd, w1.to(dev), None, False, {}).sum() * 0.5 \
                + ops.conv2d(ops.lazy_cat([fd, extra.to(dev)]), w2.to(dev), None, False, {}).square().sum()
            ld.backward()
        assert not ops.skip_fold
        close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg=f"dx (fold={fold})")
    # pruned graph (the gradient of a decoder-side loss with respect to the feature map only: the pool's backward
    # never runs).  Outside fold_skip_gradients() nothing is handed over, so the gradient is complete.
    fc = F.relu(F.conv2d(x, w0, padding=1)).requires_grad_(True)
    (gc,) = torch.autograd.grad(F.conv2d(fc, w1, padding=1).square().sum() + F.max_pool2d(fc, 2, 2).sum() * 0.0, fc)
    xd = x.to(dev).requires_grad_(True)
    fd = ops.conv2d(xd, w0.to(dev), None, True, {})
    pooled = ops.max_pool2(fd)                 # registers nothing outside the context
    (gd,) = torch.autograd.grad(ops.conv2d(fd, w1.to(dev), None, False, {}).square().sum(), fd)
    close(gd, gc, rtol=1e-4, scale_rel=2e-6, msg="pruned graph")
    assert not ops._skip_registry
    del pooled
    # odd spatial size: never registered, plain path
    xo = rnd(1, 3, 7, 9, seed=6)
    xoc = xo.clone().requires_grad_(True)
    (F.max_pool2d(F.relu(F.conv2d(xoc, w0[:, :3], padding=1)), 2, 2).sum()).backward()
    xod = xo.to(dev).requires_grad_(True)
    ops.max_pool2(ops.conv2d(xod, w0[:, :3].to(dev).contiguous(), None, True, {})).sum().backward()
    close(xod.grad, xoc.grad, rtol=1e-4, scale_rel=2e-6, msg="odd size")


def test_relu_backward_applied_by_the_gradient_producers(dev):
    """the ReLU backward of a conv whose output gradient comes from a max-pool backward (with the
    decoders' skip gradients folded in) or from the fused predictor + criterion is applied by that producer
    (ynet_maxpool2_bwd_add relu_mask, ynet_pred_bce dx_relu_mask) and the conv runs its unmasked dgrad / wgrad kernels:
    same gradients as stock autograd, bit-identical to the consumer-side masks, and the unmasked path is really taken."""
    ops = pkg("ops")
    B, H, W = 2, 16, 32
    x = rnd(B, 6, H, W, seed=1)
    w0, w1, w2 = rnd(8, 6, 3, 3, seed=2, scale=0.2), rnd(8, 8, 3, 3, seed=3, scale=0.2), rnd(4, 8, 3, 3, seed=4, scale=0.2)
    wp, bp = rnd(5, 8, 1, 1, seed=5, scale=0.3), rnd(5, seed=6, scale=0.1)
    t = torch.rand(B, 5, H, W, generator=torch.Generator().manual_seed(7)) * 0.01
    # stock torch: conv-relu -> {max-pool branch, skip conv, conv-relu -> predictor -> BCE}
    xc, w0c, w1c = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), w1.clone().requires_grad_(True)
    f = F.relu(F.conv2d(xc, w0c, padding=1))
    g = F.relu(F.conv2d(f, w1c, padding=1))
    loss = F.max_pool2d(f, 2, 2).square().sum() + F.conv2d(f, w2, padding=1).sum() * 0.5 \
        + F.binary_cross_entropy_with_logits(F.conv2d(g, wp, bp), t) * 1000.0
    loss.backward()
    got = {}
    for on in (True, False):
        old = ops._premask_allowed
        ops._premask_allowed = on
        ops.premask_stats["unmasked_backwards"] = 0
        try:
            with ops.fold_skip_gradients():
                xd, w0d, w1d = x.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True), w1.to(dev).requires_grad_(True)
                fd = ops.conv2d(xd, w0d, None, True, {})
                pooled = ops.max_pool2(fd)          # (the model's order: the pool is created before the decoder-side consumers,
                gd = ops.conv2d(fd, w1d, None, True, {})      # so its backward runs after theirs and sees every skip gradient)
                _, ld = ops.pred_bce(gd, wp.to(dev), bp.to(dev), t.to(dev), 1000.0, {})
                total = pooled.square().sum() + ops.conv2d(fd, w2.to(dev), None, False, {}).sum() * 0.5 + ld * 1000.0
                total.backward()
        finally:
            ops._premask_allowed = old
        # with the producers masking: both ReLU convs (pool -> conv 0, pred_bce -> conv 1) ran unmasked backwards
        assert ops.premask_stats["unmasked_backwards"] == (2 if on else 0)
        assert not ops._premasked and not ops._relu_outputs
        close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg=f"dx (premask={on})")
        close(w0d.grad, w0c.grad, rtol=1e-4, scale_rel=1e-5, msg=f"dW0 (premask={on})")
        close(w1d.grad, w1c.grad, rtol=1e-4, scale_rel=1e-5, msg=f"dW1 (premask={on})")
        got[on] = (xd.grad.clone(), w0d.grad.clone(), w1d.grad.clone())
    for a, b in zip(got[True], got[False]):      # the mask is an exact zeroing wherever it is applied
        assert torch.equal(a, b)
    # outside the context nothing is registered and nothing is pre-masked
    xd = x.to(dev).requires_grad_(True)
    ops.max_pool2(ops.conv2d(xd, w0.to(dev), None, True, {})).square().sum().backward()
    assert not ops._premasked and not ops._relu_outputs


@pytest.mark.parametrize("B,H,W,cs,cout", [(8, 128, 128, [6, 8], 32), (8, 64, 128, [32], 64), (4, 128, 256, [32], 16), (2, 256, 256, [16, 16], 48)])
def test_conv2d_pool_epilogue(dev, B, H, W, cs, cout):
    """ynet_conv2d_pool: conv + bias + ReLU with the 2 x 2 max-pooled copy written by the same epilogue -- both outputs bit-identical
    to ynet_conv2d followed by ynet_maxpool2_fwd, NaN propagation included; through ops.conv2d(pool=True) + ops.max_pool2 the pool
    kernel is not launched and the gradients equal stock autograd."""
    ops, L = pkg("ops"), pkg("_lib")
    lib = ops._lib()
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=i + 1).to(dev) for i, c in enumerate(cs)]
    xs[0][0, 0, 5, 7] = float("nan")
    w, b = rnd(cout, cin, 3, 3, seed=10, scale=1.0 / (cin * 9) ** 0.5).to(dev), rnd(cout, seed=11, scale=0.1).to(dev)
    assert lib.ynet_conv2d_pool_supported(B, H, W, cout, 3)
    wp = ops.pack_weight(w, 0)
    descs = [(x.data_ptr(), x.shape[1], x.shape[1] * H * W) for x in xs]
    y0, y1 = torch.empty(B, cout, H, W, device=dev), torch.empty(B, cout, H, W, device=dev)
    p0, p1 = torch.empty(B, cout, H // 2, W // 2, device=dev), torch.full((B, cout, H // 2, W // 2), 7.0, device=dev)
    ops.conv2d_raw(descs, None, wp, b, [(y0.data_ptr(), cout, cout * H * W)], B, H, W, 3, True)
    L.check(lib.ynet_maxpool2_fwd(y0.data_ptr(), p0.data_ptr(), B * cout, H, W, ops._stream()), lib)
    ops.conv2d_raw(descs, None, wp, b, [(y1.data_ptr(), cout, cout * H * W)], B, H, W, 3, True, pooled=(p1.data_ptr(), cout * (H // 2) * (W // 2)))
    assert torch.equal(torch.nan_to_num(y0, nan=-1.0), torch.nan_to_num(y1, nan=-1.0))
    assert bool(torch.isnan(p0).any()) and torch.equal(torch.isnan(p0), torch.isnan(p1))
    assert torch.equal(torch.nan_to_num(p0, nan=-1.0), torch.nan_to_num(p1, nan=-1.0))
    # autograd path: conv2d(pool=True) -> max_pool2 (no pool kernel) against stock torch
    xs = [rnd(B, c, H, W, seed=i + 1) for i, c in enumerate(cs)]
    xc = [x.clone().requires_grad_(True) for x in xs]
    wc = w.cpu().clone().requires_grad_(True)
    F.max_pool2d(F.relu(F.conv2d(torch.cat(xc, 1), wc, b.cpu(), padding=1)), 2, 2).square().sum().backward()
    xd = [x.to(dev).requires_grad_(True) for x in xs]
    wd = w.clone().requires_grad_(True)
    # (the implicit GEMM's launch: this test is ynet_conv2d_pool's.  The loss routes every pooled gradient to its block's arg-max; the
    #  Winograd launches round differently from the CPU reference, and among 10^6 blocks one near-tie picks the other element -- a whole
    #  filter row of dW moves by O(dy * x).  The Winograd pooled copies have their own tests, against max_pool2d of the same launch's output.)
    old_w = ops._wino_allowed
    ops._wino_allowed = False
    try:
        yd = ops.conv2d(ops.lazy_cat(xd) if len(xd) > 1 else xd[0], wd, b, True, {}, pool=True)
    finally:
        ops._wino_allowed = old_w
    assert (yd.data_ptr() in ops._pooled_outputs) == ops._pool_epilogue_allowed      # (YNET_POOL_EPILOGUE=0: the pool kernel runs)
    ops.max_pool2(yd).square().sum().backward()
    assert not ops._pooled_outputs
    close(wd.grad, wc.grad, rtol=1e-4, scale_rel=1e-5, msg="dW through the pooled epilogue")
    for a, c in zip(xd, xc):
        close(a.grad, c.grad, rtol=1e-4, scale_rel=2e-6, msg="dx through the pooled epilogue")


@pytest.mark.parametrize("B,H,W,cs,relu_mask,adds", [(8, 256, 256, [6, 8], True, 2), (16, 128, 128, [32], True, 1), (10, 96, 160, [32, 16, 1], False, 2), (8, 128, 256, [32], True, 0)], ids=str)
def test_winograd_pool_epilogue_leaves_the_backward_its_arg_max_and_relu_bits(dev, B, H, W, cs, relu_mask, adds):
    """Round 5: ynet_conv2d_winograd_cat_pool_code -- the Winograd launch in front of a MaxPool2d(2, 2) writes, besides the output and its pooled copy, one
    byte per 2 x 2 block: bits 0..1 the arg-max by ynet_maxpool2_bwd's rule (first maximum in scan order, a NaN wins), bits 2..5 `element > 0`.
    ynet_maxpool2_bwd_add_code routes the pooled gradient (+ the folded skip gradients, + the ReLU backward) from that byte alone: dx bit-identical to
    ynet_maxpool2_bwd_add reading the full-resolution activation; output and pooled copy bit-identical to the launch without the code plane."""
    ops, L = pkg("ops"), pkg("_lib")
    lib = ops._lib()
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=i + 1).to(dev) for i, c in enumerate(cs)]
    xs[0][0, 0, 5, 7] = float("nan")                       # (a NaN spreads over a 3 x 3 neighbourhood of every output channel of image 0)
    w, b = rnd(32, cin, 3, 3, seed=10, scale=1.0 / (cin * 9) ** 0.5).to(dev), rnd(32, seed=11, scale=0.1).to(dev)
    wp = ops.pack_weight(w, 0)
    descs = [(x.data_ptr(), x.shape[1], x.shape[1] * H * W) for x in xs]
    y0, y1 = torch.empty(B, 32, H, W, device=dev), torch.empty(B, 32, H, W, device=dev)
    p0, p1 = torch.empty(B, 32, H // 2, W // 2, device=dev), torch.empty(B, 32, H // 2, W // 2, device=dev)
    code = torch.full((B, 32, H // 2, W // 2), 255, device=dev, dtype=torch.uint8)
    pst = 32 * (H // 2) * (W // 2)
    t0 = ops.conv2d_raw(descs, None, wp, b, [(y0.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, pooled=(p0.data_ptr(), pst), wino=({}, "fwd"))
    t1 = ops.conv2d_raw(descs, None, wp, b, [(y1.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, pooled=(p1.data_ptr(), pst), wino=({}, "fwd"), pool_code=code)
    assert t0 == "winograd_cat:2,3" and t1 == "winograd_cat:2,6|code", (t0, t1)
    assert torch.equal(torch.nan_to_num(y0, nan=-1.0), torch.nan_to_num(y1, nan=-1.0)) and torch.equal(torch.nan_to_num(p0, nan=-1.0), torch.nan_to_num(p1, nan=-1.0))
    assert bool(torch.isnan(y1).any())
    # the byte, recomputed from the output: window scan order (0, 0), (0, 1), (1, 0), (1, 1)
    blk = y1.view(B, 32, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, 32, H // 2, W // 2, 4)
    m, arg = blk[..., 0].clone(), torch.zeros_like(blk[..., 0], dtype=torch.int64)
    for e in (1, 2, 3):
        v = blk[..., e]
        take = (v > m) | torch.isnan(v)
        m, arg = torch.where(take, v, m), torch.where(take, torch.full_like(arg, e), arg)
    want = arg + sum(((blk[..., e] > 0).to(torch.int64) << (2 + e)) for e in range(4))
    assert torch.equal(code.to(torch.int64), want)
    assert int((code & 3 != 0).sum()) > 0 and int((code >> 2 == 0).sum()) > 0      # (every arg-max position occurs, and all-negative blocks do)
    # backward: from the byte against from the activation
    dy = rnd(B, 32, H // 2, W // 2, seed=20).to(dev)
    a = [rnd(B, 32, H, W, seed=21 + i).to(dev) for i in range(adds)]
    ap = [t.data_ptr() for t in a] + [None, None]
    dx0, dx1 = torch.empty(B, 32, H, W, device=dev), torch.full((B, 32, H, W), float("nan"), device=dev)
    L.check(lib.ynet_maxpool2_bwd_add(y1.data_ptr(), dy.data_ptr(), ap[0], ap[1], dx0.data_ptr(), B * 32, H, W, 1 if relu_mask else 0, ops._stream()), lib)
    L.check(lib.ynet_maxpool2_bwd_add_code(code.data_ptr(), dy.data_ptr(), ap[0], ap[1], dx1.data_ptr(), B * 32, H, W, 1 if relu_mask else 0, ops._stream()), lib)
    assert torch.equal(dx0, dx1)
    assert lib.ynet_maxpool2_bwd_add_code(None, dy.data_ptr(), None, None, dx1.data_ptr(), B * 32, H, W, 0, ops._stream()) != 0
    assert lib.ynet_maxpool2_bwd_add_code(code.data_ptr(), dy.data_ptr(), None, None, dx1.data_ptr(), B * 32, H + 1, W, 0, ops._stream()) != 0
    # through autograd: conv2d(pool=True) -> max_pool2 -> backward uses the byte, and gives what the path without it gives
    grads = []
    for on in (True, False):
        old, n0 = ops._pool_code_allowed, ops.pool_code_stats["launches"]
        ops._pool_code_allowed = on
        try:
            xd = [x.detach().clone().nan_to_num(0.0).requires_grad_(True) for x in xs]
            wd = w.clone().requires_grad_(True)
            with ops.fold_skip_gradients():
                yd = ops.conv2d(ops.lazy_cat(xd) if len(xd) > 1 else xd[0], wd, b, True, {}, pool=True)
                ops.max_pool2(yd).square().sum().backward()
        finally:
            ops._pool_code_allowed = old
        grads.append(([t.grad for t in xd], wd.grad, ops.pool_code_stats["launches"] - n0))
    if grads[0][2] > 0:      # (the Winograd launch served the layer: the byte was used)
        assert grads[1][2] == 0
    for g0, g1 in zip(grads[0][0], grads[1][0]):
        assert torch.equal(g0, g1)
    assert torch.equal(grads[0][1], grads[1][1])


def test_conv2d_pool_rejects_shapes_without_the_epilogue(dev):
    ops = pkg("ops")
    lib = ops._lib()
    assert not lib.ynet_conv2d_pool_supported(2, 16, 16, 32, 3) and not lib.ynet_conv2d_pool_supported(8, 128, 128, 32, 1)
    x, w = rnd(2, 8, 16, 16, seed=1).to(dev), rnd(32, 8, 3, 3, seed=2).to(dev)
    y, p = torch.empty(2, 32, 16, 16, device=dev), torch.empty(2, 32, 8, 8, device=dev)
    with pytest.raises(RuntimeError, match="pooling epilogue"):
        ops.conv2d_raw([(x.data_ptr(), 8, 8 * 256)], None, ops.pack_weight(w, 0), None, [(y.data_ptr(), 32, 32 * 256)], 2, 16, 16, 3, True,
                       pooled=(p.data_ptr(), 32 * 64))
    # ... and ops.conv2d(pool=True) simply does not use it there
    yd = ops.conv2d(x, w, None, True, {}, pool=True)
    assert yd.data_ptr() not in ops._pooled_outputs


# B, H, W, channels of dy (the layer's cout), channels of dx (its cin), dy masked too
DGRAD_RELU_CASES = [
    (8, 128, 128, 32, 16, False),       # two-row tiles, one 16-channel tile per workgroup: mask inside the conv kernel
    (8, 128, 128, 32, 32, True),        # ... with the consumer-side mask of dy on top (masked instantiation)
    (8, 64, 128, 16, 64, False),        # four 16-channel tiles
    (4, 64, 64, 64, 48, True),          # three tiles (64 two-row units: the smallest launch that takes them)
    (2, 16, 32, 8, 8, False),           # small map: the fall-back pass
    (4, 16, 16, 64, 64, False),         # folded tiles, split channel loop: the mask is applied by the reduction
    (3, 24, 40, 5, 7, True),            # ragged edges, register-staged kernel + fall-back pass
]


@pytest.mark.parametrize("case", DGRAD_RELU_CASES, ids=[str(c) for c in DGRAD_RELU_CASES])
def test_conv2d_dgrad_relu_writes_through_the_relu_backward_of_the_layer_below(dev, case):
    """ynet_conv2d_dgrad_relu: dx = relu_of > 0 ? conv(dy [masked], flipped filter) : 0 -- the same values as the plain data
    gradient with the mask applied afterwards (bit-identical: the arithmetic is the same), on every kernel family."""
    ops = pkg("ops")
    B, H, W, cout, cin, masked = case
    dy, w = rnd(B, cout, H, W, seed=1).to(dev), rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev)
    act = torch.relu(rnd(B, cin, H, W, seed=3)).to(dev)        # the input of the forward conv = post-ReLU output of the layer below
    y = torch.relu(rnd(B, cout, H, W, seed=4)).to(dev)
    wp = ops.pack_weight(w, 1)
    mask = (y.data_ptr(), cout * H * W) if masked else None
    plain, got = torch.empty(B, cin, H, W, device=dev), torch.full((B, cin, H, W), float("nan"), device=dev)
    ops.conv2d_raw([(dy.data_ptr(), cout, cout * H * W)], mask, wp, None, [(plain.data_ptr(), cin, cin * H * W)], B, H, W, 3, False)
    ops.conv2d_raw([(dy.data_ptr(), cout, cout * H * W)], mask, wp, None, [(got.data_ptr(), cin, cin * H * W)], B, H, W, 3, False,
                   relu_of=(act.data_ptr(), cin * H * W))
    want = torch.where(act > 0, plain, torch.zeros_like(plain))
    assert torch.equal(got, want), float((got - want).abs().max())
    ref = F.conv_transpose2d((dy * (y > 0)) if masked else dy, w, padding=1) * (act > 0)
    close(got, ref, rtol=1e-4, scale_rel=2e-6, msg="dgrad_relu vs torch")
    # (the first four cases are the ones the conv kernel itself masks; the others take the reduction / the fall-back pass)
    assert bool(ops._lib().ynet_conv2d_dgrad_relu_supported(B, H, W, cin, 3)) == (case in DGRAD_RELU_CASES[:4])


# B, H, W, cin, cout, ReLU, bias, packing mode (0 forward, 1 data gradient), destination = a channel slice of a wider tensor
WINOGRAD_CASES = [
    (16, 128, 128, 32, 32, True, True, 0, False),      # the decoders' 32 -> 32 layers
    (4, 256, 256, 32, 16, True, True, 0, True),        # the layer in front of the predictor, written into a wider tensor
    (4, 256, 256, 16, 32, False, False, 1, False),     # its data gradient (mode-1 packing: flipped taps, transposed roles)
    (48, 64, 96, 16, 16, False, True, 0, False),       # ragged tile counts: 4 x 3 tiles per image, 576 tiles over 256 workgroups
    (3, 304, 320, 32, 32, True, False, 0, False),      # edges everywhere: 19 x 10 tiles, a batch that is no multiple of anything
]


@pytest.mark.parametrize("case", WINOGRAD_CASES, ids=[str(c) for c in WINOGRAD_CASES])
def test_winograd_convolution_matches_the_direct_form(dev, case):
    """ynet_conv2d_winograd (F(2x2, 3x3) on the fp32 matrix cores): the same values as torch's convolution and as ynet_conv2d within fp32
    rounding -- tolerance 2e-6 of the largest output (the bound the implicit-GEMM kernels are held to), since the two forms round
    differently; its error against an fp64 reference is not larger than the direct kernel's."""
    ops = pkg("ops")
    B, H, W, cin, cout, relu, has_bias, mode, wide = case
    assert ops._lib().ynet_conv2d_winograd_supported(B, H, W, cin, cout, 3)
    x = torch.relu(rnd(B, cin, H, W, seed=1)).to(dev)
    w = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev) if mode == 0 else rnd(cin, cout, 3, 3, seed=2, scale=0.2).to(dev)
    bias = rnd(cout, seed=3).to(dev) if has_bias else None
    wp = ops.pack_weight(w, mode)
    u = ops.winograd_filter(wp, cin, cout)
    ctot = cout + 8 if wide else cout
    got = torch.full((B, ctot, H, W), float("nan"), device=dev)
    c0 = 8 if wide else 0
    ops.conv2d_winograd_raw((x.data_ptr(), cin * H * W), u, bias, (got[:, c0:].data_ptr(), ctot * H * W), cin, cout, B, H, W, relu)
    direct = torch.empty(B, cout, H, W, device=dev)
    assert ops.conv2d_raw([(x.data_ptr(), cin, cin * H * W)], None, wp, bias, [(direct.data_ptr(), cout, cout * H * W)], B, H, W, 3, relu) is None
    if mode == 0:
        ref64 = F.conv2d(x.double(), w.double(), bias.double() if has_bias else None, padding=1)
    else:
        ref64 = F.conv_transpose2d(x.double(), w.double(), padding=1)
    ref64 = torch.relu(ref64) if relu else ref64
    y = got[:, c0:]
    if wide:
        assert bool(torch.isnan(got[:, :c0]).all()), "the channels in front of the slice were written"
    close(y, ref64, rtol=1e-5, scale_rel=2e-6, msg="winograd vs fp64")
    close(y, direct, rtol=1e-5, scale_rel=2e-6, msg="winograd vs ynet_conv2d")
    e_w, e_d = float((y.double() - ref64).abs().max()), float((direct.double() - ref64).abs().max())
    assert e_w <= 1.5 * e_d + 1e-7, (e_w, e_d)


def test_winograd_on_production_like_inputs(dev):
    """the inputs the decoders really feed these launches -- bilinearly up-sampled post-ReLU planes (smooth: the
    Winograd input transform takes differences of nearly equal values), skip features, and the way-point distance map, a ramp over
    [0, 2] -- not relu(randn).  The Winograd launches (one source and concatenated) against fp64 and against the implicit GEMM: the same
    2e-6-of-the-largest-output bound, an error against fp64 not above 1.5x the direct kernel's."""
    ops = pkg("ops")
    B, H, W = 8, 256, 256
    up = F.interpolate(torch.relu(rnd(B, 32, H // 2, W // 2, seed=1)), scale_factor=2, mode="bilinear", align_corners=False).to(dev)
    skip = torch.relu(rnd(B, 16, H, W, seed=2)).to(dev)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    ramp = torch.stack([(((yy - 40.0 - 11 * b) ** 2 + (xx - 200.0 + 13 * b) ** 2).sqrt() / 742.0 * 2.0) for b in range(B)]).unsqueeze(1).to(dev)
    w, bias = rnd(32, 49, 3, 3, seed=4, scale=0.2).to(dev), rnd(32, seed=5).to(dev)
    wp = ops.pack_weight(w, 0)
    srcs = [(up.data_ptr(), 32, 32 * H * W), (skip.data_ptr(), 16, 16 * H * W), (ramp.data_ptr(), 1, H * W)]
    got, direct = torch.full((B, 32, H, W), float("nan"), device=dev), torch.empty(B, 32, H, W, device=dev)
    assert ops.conv2d_raw(srcs, None, wp, bias, [(got.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, wino=({}, "fwd")).startswith("winograd")
    assert ops.conv2d_raw(srcs, None, wp, bias, [(direct.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True) is None
    ref64 = torch.relu(F.conv2d(torch.cat([up, skip, ramp], 1).double(), w.double(), bias.double(), padding=1))
    close(got, ref64, rtol=1e-5, scale_rel=2e-6, msg="winograd (cat) vs fp64")
    close(got, direct, rtol=1e-5, scale_rel=2e-6, msg="winograd (cat) vs ynet_conv2d")
    e_w, e_d = float((got.double() - ref64).abs().max()), float((direct.double() - ref64).abs().max())
    assert e_w <= 1.5 * e_d + 1e-7, (e_w, e_d)
    # the smooth planes alone through the one-source kernel (32 -> 32 and 32 -> 16)
    for cout in (32, 16):
        w1 = rnd(cout, 32, 3, 3, seed=6, scale=0.2).to(dev)
        wp1 = ops.pack_weight(w1, 0)
        g1, d1 = torch.empty(B, cout, H, W, device=dev), torch.empty(B, cout, H, W, device=dev)
        assert ops.conv2d_raw([(up.data_ptr(), 32, 32 * H * W)], None, wp1, None, [(g1.data_ptr(), cout, cout * H * W)], B, H, W, 3, False,
                              wino=({}, "fwd")).startswith("winograd")
        ops.conv2d_raw([(up.data_ptr(), 32, 32 * H * W)], None, wp1, None, [(d1.data_ptr(), cout, cout * H * W)], B, H, W, 3, False)
        r1 = F.conv2d(up.double(), w1.double(), None, padding=1)
        close(g1, r1, rtol=1e-5, scale_rel=2e-6, msg=f"winograd 32 -> {cout} vs fp64")
        e_w, e_d = float((g1.double() - r1).abs().max()), float((d1.double() - r1).abs().max())
        assert e_w <= 1.5 * e_d + 1e-7, (cout, e_w, e_d)


@pytest.mark.parametrize("case", [(8, 256, 256, 32, [32, 16]), (16, 128, 128, 32, [64]), (8, 256, 256, 16, [32, None])], ids=str)
def test_winograd_launches_over_output_channel_slices(dev, case):
    """A data gradient with 48 or 64 output channels (the decoders' first convolutions: up-sampled part + skip part) runs as two
    Winograd launches over slices of the filter, each into its own destination / its own channels of the one destination; a
    destination nobody wants is not computed.  Same values as the one implicit-GEMM launch within fp32 rounding."""
    ops = pkg("ops")
    B, H, W, cin, couts = case
    sizes = [c if c is not None else 16 for c in couts]
    ctot = sum(sizes)
    dy = rnd(B, cin, H, W, seed=1).to(dev)
    w = rnd(cin, ctot, 3, 3, seed=2, scale=0.2).to(dev)          # the forward layer's filter [Cout_fwd = cin here][Cin_fwd = ctot]
    wp = ops.pack_weight(w, 1)
    want = [torch.empty(B, c, H, W, device=dev) for c in sizes]
    got = [torch.full((B, c, H, W), float("nan"), device=dev) for c in sizes]
    ops.conv2d_raw([(dy.data_ptr(), cin, cin * H * W)], None, wp, None, [(t.data_ptr(), t.shape[1], t.shape[1] * H * W) for t in want], B, H, W, 3, False)
    dsts = [(t.data_ptr() if c is not None else None, t.shape[1], t.shape[1] * H * W if c is not None else 0) for t, c in zip(got, couts)]
    n0 = ops.wino_stats["launches"]
    assert ops.conv2d_raw([(dy.data_ptr(), cin, cin * H * W)], None, wp, None, dsts, B, H, W, 3, False, wino=({}, "dgrad")).startswith("winograd")
    # (round 5: a destination of 64 channels is ONE launch of the slice form, ynet_conv2d_winograd16, not two 32-channel launches)
    assert ops.wino_stats["launches"] - n0 == (1 if None in couts or (64 in couts and ops._wino16_allowed) else 2)
    for g, t, c in zip(got, want, couts):
        if c is None:
            assert bool(torch.isnan(g).all())
        else:
            close(g, t, rtol=1e-5, scale_rel=2e-6, msg=f"slice of {c} channels")
    ref = F.conv_transpose2d(dy, w, padding=1)
    close(torch.cat([g for g, c in zip(got, couts) if c is not None], 1), ref[:, :sum(c for c in couts if c is not None)], rtol=1e-4, scale_rel=2e-6, msg="vs torch")


@pytest.mark.parametrize("case", [(8, 256, 256, 32, 32), (16, 128, 128, 32, 16), (16, 128, 128, 16, 32)], ids=str)
def test_winograd_data_gradient_through_the_relu_backward_of_the_layer_below(dev, case):
    """ynet_conv2d_winograd_dgrad_relu: dx = relu_of > 0 ? conv(dy, flipped filter) : 0 -- zero exactly where the activation is not
    positive, the plain Winograd data gradient elsewhere (bit-identical to it: the mask is an exact zeroing), and the implicit GEMM's
    ynet_conv2d_dgrad_relu within fp32 rounding."""
    ops = pkg("ops")
    B, H, W, dy_c, dx_c = case
    dy, w = rnd(B, dy_c, H, W, seed=1).to(dev), rnd(dy_c, dx_c, 3, 3, seed=2, scale=0.2).to(dev)
    act = torch.relu(rnd(B, dx_c, H, W, seed=3)).to(dev)
    wp = ops.pack_weight(w, 1)
    plain, got, direct = (torch.full((B, dx_c, H, W), float("nan"), device=dev) for _ in range(3))
    src, cache = [(dy.data_ptr(), dy_c, dy_c * H * W)], {}
    assert ops.conv2d_raw(src, None, wp, None, [(plain.data_ptr(), dx_c, dx_c * H * W)], B, H, W, 3, False, wino=(cache, "dgrad")).startswith("winograd")
    assert ops.conv2d_raw(src, None, wp, None, [(got.data_ptr(), dx_c, dx_c * H * W)], B, H, W, 3, False, relu_of=(act.data_ptr(), dx_c * H * W),
                          wino=(cache, "dgrad")).startswith("winograd")
    assert ops.conv2d_raw(src, None, wp, None, [(direct.data_ptr(), dx_c, dx_c * H * W)], B, H, W, 3, False, relu_of=(act.data_ptr(), dx_c * H * W)) is None
    assert torch.equal(got, torch.where(act > 0, plain, torch.zeros_like(plain)))
    close(got, direct, rtol=1e-5, scale_rel=2e-6, msg="winograd vs implicit GEMM, both through the ReLU backward")
    close(got, F.conv_transpose2d(dy, w, padding=1) * (act > 0), rtol=1e-4, scale_rel=2e-6, msg="vs torch")


@pytest.mark.parametrize("case", [(4, 256, 256, [32, 16, 1], True), (16, 128, 128, [32, 16], True), (8, 256, 256, [20, 7, 3], False), (16, 128, 128, [48], False),
                                  (16, 128, 128, [64], True), (16, 128, 128, [32, 32, 1], True), (16, 128, 128, [64, 1], False)], ids=str)
def test_winograd_convolution_over_concatenated_sources(dev, case):
    """ynet_conv2d_winograd_cat: conv(cat(sources)) -> 32 channels with every source padded to a multiple of 4 channels inside the kernel
    (zero planes, zero filters) -- the decoders' first convolutions, cat(up-sampled features, skip features[, way-point map]).  Same values
    as torch's convolution of the concatenation and as the multi-source implicit GEMM within fp32 rounding."""
    ops = pkg("ops")
    B, H, W, cs, relu = case
    cin = sum(cs)
    xs = [torch.relu(rnd(B, c, H, W, seed=10 + i)).to(dev) for i, c in enumerate(cs)]
    w, bias = rnd(32, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
    wp = ops.pack_weight(w, 0)
    srcs = [(x.data_ptr(), c, c * H * W) for x, c in zip(xs, cs)]
    if len(cs) == 2:       # the second source as ONE image shared by the batch (batch stride 0: Y-Net-Mod's scene features)
        xs[1] = xs[1][:1].expand(B, -1, -1, -1).contiguous()
        srcs[1] = (xs[1].data_ptr(), cs[1], 0)
    got, direct = torch.full((B, 32, H, W), float("nan"), device=dev), torch.empty(B, 32, H, W, device=dev)
    n0 = ops.wino_stats["launches"]
    assert ops.conv2d_raw(srcs, None, wp, bias, [(got.data_ptr(), 32, 32 * H * W)], B, H, W, 3, relu, wino=({}, "fwd")).startswith("winograd")
    # (57 .. 88 padded input channels: the first 32 channels into the destination, then the rest with the destination as additive term)
    # (round 5: ONE source of 64 channels takes the slice form, ynet_conv2d_winograd16, in one launch)
    assert ops.wino_stats["launches"] - n0 == (1 if cs == [64] and ops._wino16_allowed else (2 if cin > 56 else 1))
    assert ops.conv2d_raw(srcs, None, wp, bias, [(direct.data_ptr(), 32, 32 * H * W)], B, H, W, 3, relu) is None
    ref64 = F.conv2d(torch.cat(xs, 1).double(), w.double(), bias.double(), padding=1)
    ref64 = torch.relu(ref64) if relu else ref64
    close(got, ref64, rtol=1e-5, scale_rel=2e-6, msg="winograd (cat) vs fp64")
    close(got, direct, rtol=1e-5, scale_rel=2e-6, msg="winograd (cat) vs ynet_conv2d")
    e_w, e_d = float((got.double() - ref64).abs().max()), float((direct.double() - ref64).abs().max())
    assert e_w <= 1.5 * e_d + 1e-7, (e_w, e_d)


@pytest.mark.parametrize("case", [(8, 256, 256, [6, 8]), (16, 128, 128, [32])], ids=str)
def test_winograd_convolution_with_the_pooled_copy(dev, case):
    """ynet_conv2d_winograd_cat_pool: conv + ReLU and its 2 x 2 max-pooled copy from one launch (the encoder's layers in front of a
    MaxPool2d: cat(scene one-hot 6 -- one image for the batch --, observed maps 8) -> 32 at 256^2, 32 -> 32 at 128^2); the pooled copy is
    bit-identical to max_pool2d of the full-resolution output of the same launch."""
    ops = pkg("ops")
    B, H, W, cs = case
    cin = sum(cs)
    xs = [torch.relu(rnd(B if i else 1, c, H, W, seed=10 + i)).to(dev) if len(cs) > 1 else torch.relu(rnd(B, c, H, W, seed=10)).to(dev) for i, c in enumerate(cs)]
    srcs = [(x.data_ptr(), c, 0 if x.shape[0] == 1 and B > 1 else c * H * W) for x, c in zip(xs, cs)]
    w, bias = rnd(32, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
    wp = ops.pack_weight(w, 0)
    y, yp = torch.full((B, 32, H, W), float("nan"), device=dev), torch.full((B, 32, H // 2, W // 2), float("nan"), device=dev)
    assert ops.conv2d_raw(srcs, None, wp, bias, [(y.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, pooled=(yp.data_ptr(), 32 * (H // 2) * (W // 2)),
                          wino=({}, "fwd")).startswith("winograd_cat")
    ref = torch.relu(F.conv2d(torch.cat([x.expand(B, -1, -1, -1) for x in xs], 1), w, bias, padding=1))
    close(y, ref, rtol=1e-4, scale_rel=2e-6, msg="output vs torch")
    assert torch.equal(yp, F.max_pool2d(y, 2, 2))


def test_winograd_shared_skip_term_launch(dev):
    """evaluate()'s per-sample launch of a decoder level's first convolution, relu(conv(cat(up, way-point map), W_rest) + b + term[b % Bs])
    with the batch-shared skip-feature term precomputed (ops.conv2d_shared_term): the Winograd form (ynet_conv2d_winograd_cat_add) against
    the implicit GEMM (ynet_conv2d_add) and against torch's convolution of the full concatenation."""
    ops = pkg("ops")
    Bs, times, H, W = 4, 2, 256, 256
    B = Bs * times
    up, wmap = torch.relu(rnd(B, 32, H, W, seed=1)).to(dev), torch.relu(rnd(B, 1, H, W, seed=2)).to(dev)
    skip = torch.relu(rnd(Bs, 16, H, W, seed=3)).to(dev)
    w, bias = rnd(32, 49, 3, 3, seed=4, scale=0.2).to(dev), rnd(32, seed=5).to(dev)
    outs = []
    for allowed in (True, False):
        old, n0, cache = ops._wino_allowed, ops.wino_stats["launches"], {}
        ops._wino_allowed = allowed
        try:
            with torch.no_grad():
                term = ops.shared_conv_term(skip, w, 32, 48, cache)
                ops.rest_filter(w, 32, 48, cache)
                ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), Bs, H, W)
                n1 = ops.wino_stats["launches"]
                outs.append(ops.conv2d_shared_term(None, times, [up, wmap], w, bias, True, cache, term, 32, 48))
        finally:
            ops._wino_allowed = old
        assert ops.wino_stats["launches"] - n1 == (1 if allowed else 0), (n0, n1)
    ref = torch.relu(F.conv2d(torch.cat([up, skip.repeat(times, 1, 1, 1), wmap], 1), w, bias, padding=1))
    close(outs[0], outs[1], rtol=1e-5, scale_rel=2e-6, msg="winograd vs implicit GEMM")
    close(outs[0], ref, rtol=1e-4, scale_rel=2e-6, msg="vs torch")


def test_rest_filter_forms_coexist_in_the_layer_cache(dev):
    """The shared-term launch over (32, 1) channels -> 32 at 128^2 takes the slice form at B 4 and the concatenated-source form at B 8 (evaluate() on folds of
    different sizes): the two transformed filters are two entries of the layer's cache.  Making the second leaves the first where it is, bit for bit (a captured
    sweep reads it at that address), a later call finds both again, and each batch size launches its own form."""
    ops = pkg("ops")
    H = W = 128
    up, wmap = torch.relu(rnd(8, 32, H, W, seed=1)).to(dev), torch.relu(rnd(8, 1, H, W, seed=2)).to(dev)
    skip = torch.relu(rnd(8, 16, H, W, seed=3)).to(dev)
    w, bias = rnd(32, 49, 3, 3, seed=4, scale=0.2).to(dev), rnd(32, seed=5).to(dev)
    cache = {}
    kinds = lambda: sorted(k[0] for k in cache if isinstance(k, tuple))      # noqa: E731
    with torch.no_grad():
        u4 = ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), 4, H, W)
        assert u4 is not None and kinds() == ["wino16"]
        addr4, kept4 = u4.data_ptr(), u4.clone()
        u8 = ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), 8, H, W)
        assert u8 is not None and kinds() == ["cat", "wino16"] and u8.data_ptr() != addr4
        addr8, kept8 = u8.data_ptr(), u8.clone()
        again4, again8 = ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), 4, H, W), ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), 8, H, W)
        assert again4.data_ptr() == addr4 and again8.data_ptr() == addr8 and kinds() == ["cat", "wino16"]
        for B, slice_launches in ((8, 0), (4, 1)):
            term = ops.shared_conv_term(skip[:B], w, 32, 48, cache)
            n0, n16 = ops.wino_stats["launches"], ops.wino_stats.get("launches16", 0)
            y = ops.conv2d_shared_term(None, 1, [up[:B], wmap[:B]], w, bias, True, cache, term, 32, 48)
            assert ops.wino_stats["launches"] - n0 == 1 and ops.wino_stats.get("launches16", 0) - n16 == slice_launches, B
            ref = torch.relu(F.conv2d(torch.cat([up[:B], skip[:B], wmap[:B]], 1), w, bias, padding=1))
            close(y, ref, rtol=1e-4, scale_rel=2e-6, msg=f"shared term at B {B} vs torch")
    assert torch.equal(again4, kept4) and torch.equal(again8, kept8)


def test_winograd_path_of_the_model_layer_and_its_switch(dev):
    """ops.conv2d takes the Winograd kernel for a plain 32 -> 32 layer -- forward AND data gradient -- and the implicit GEMM with
    YNET_WINOGRAD off; outputs and input gradients of the two agree within fp32 rounding.  (A layer without ReLU: behind a ReLU
    the two forms' masks differ wherever a pre-activation rounds to the other side of zero -- 576 of 8.4 M elements here.)"""
    ops = pkg("ops")
    B, H, W = 16, 128, 128
    w = rnd(32, 32, 3, 3, seed=5, scale=0.2).to(dev)
    bias = rnd(32, seed=6).to(dev)
    outs = []
    for allowed in (True, False):
        x = rnd(B, 32, H, W, seed=7).to(dev).requires_grad_(True)
        old, n0 = ops._wino_allowed, ops.wino_stats["launches"]
        ops._wino_allowed = allowed
        try:
            y = ops.conv2d(x, w, bias, False, {})
            (y * rnd(B, 32, H, W, seed=8).to(dev)).sum().backward()
        finally:
            ops._wino_allowed = old
        assert ops.wino_stats["launches"] - n0 == (2 if allowed else 0)
        outs.append((y.detach(), x.grad))
    close(outs[0][0], outs[1][0], rtol=1e-5, scale_rel=2e-6, msg="forward")
    close(outs[0][1], outs[1][1], rtol=1e-5, scale_rel=2e-6, msg="input gradient")
    ref = F.conv2d(rnd(B, 32, H, W, seed=7).to(dev), w, bias, padding=1)
    close(outs[0][0], ref, rtol=1e-4, scale_rel=2e-6, msg="forward vs torch")


@pytest.mark.parametrize("case", [(8, 256, 256, "plain", 32), (16, 128, 128, "plain", 16), (8, 256, 256, "cat", 32), (16, 128, 128, "split", 32), (10, 96, 160, "cat", 16)], ids=str)
def test_winograd_native_one_bit_relu_mask(dev, case):
    """Round 5: conv -> ReLU -> conv with 32 channels in between, both launches Winograd ones.  The first convolution's FORWARD launch (one source,
    concatenated sources, or the two-launch form for 57..88 channels) also writes one bit per output element in the register layout of the tiling
    the second convolution's data gradient shares -- one 32-bit word per lane and unit --, and that data gradient is gated by it
    (ynet_conv2d_winograd_dgrad_relu_bits) instead of fetching the float activation: the forward output is unchanged (bit-identical to the
    launch without the mask), the masked gradient bit-identical to ynet_conv2d_winograd_dgrad_relu's, a NaN / -0 activation counts as not positive."""
    ops = pkg("ops")
    lib = ops._lib()
    B, H, W, kind, dyc = case
    cs = {"plain": [32], "cat": [32, 16, 1], "split": [64, 1]}[kind]
    cin = sum(cs)
    xs = [rnd(B, c, H, W, seed=10 + i).to(dev) for i, c in enumerate(cs)]
    w, bias = rnd(32, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
    wp = ops.pack_weight(w, 0)
    srcs = [(x.data_ptr(), c, c * H * W) for x, c in zip(xs, cs)]
    n_words = lib.ynet_winograd_relu_bits_words(B, H, W)
    assert n_words == B * (H // 2) * (W // 32) * 64
    y0, y1 = torch.empty(B, 32, H, W, device=dev), torch.empty(B, 32, H, W, device=dev)
    wbits = torch.full((n_words,), -1, device=dev, dtype=torch.int32)
    t0 = ops.conv2d_raw(srcs, None, wp, bias, [(y0.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, wino=({}, "fwd"))
    t1 = ops.conv2d_raw(srcs, None, wp, bias, [(y1.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, wino=({}, "fwd"), wbits_out=wbits)
    assert t0.startswith("winograd") and t1.endswith("|wbits") and not t0.endswith("|wbits"), (t0, t1)
    assert torch.equal(y0, y1)
    assert not bool((wbits == -1).all())
    # a NaN and a -0 in the activation: "not positive" either way
    y1[0, 3, 5, 7] = float("nan")
    y1[1, 4, 9, 11] = -0.0
    dy = rnd(B, dyc, H, W, seed=5).to(dev)
    w2 = rnd(dyc, 32, 3, 3, seed=6, scale=0.2).to(dev)          # the second layer's filter [Cout = dyc][Cin = 32]
    wp2 = ops.pack_weight(w2, 1)
    src, cache = [(dy.data_ptr(), dyc, dyc * H * W)], {}
    g_float, g_bits = torch.full((B, 32, H, W), float("nan"), device=dev), torch.full((B, 32, H, W), float("nan"), device=dev)
    ta = ops.conv2d_raw(src, None, wp2, None, [(g_float.data_ptr(), 32, 32 * H * W)], B, H, W, 3, False, relu_of=(y1.data_ptr(), 32 * H * W), wino=(cache, "dgrad"))
    tb = ops.conv2d_raw(src, None, wp2, None, [(g_bits.data_ptr(), 32, 32 * H * W)], B, H, W, 3, False, relu_of=(y1.data_ptr(), 32 * H * W), wino=(cache, "dgrad"),
                        relu_wbits=wbits)
    assert ta == "winograd:2,%d,1" % (dyc // 8) and tb == "winograd:2,%d,2" % (dyc // 8), (ta, tb)
    # the mask was written from the launch's own output, before the NaN / -0 were planted: those two elements may differ, nothing else
    same = torch.ones_like(g_float, dtype=torch.bool)
    same[0, 3, 5, 7] = False
    same[1, 4, 9, 11] = False
    assert torch.equal(g_float[same], g_bits[same])
    assert float(g_float[0, 3, 5, 7]) == 0.0 and float(g_float[1, 4, 9, 11]) == 0.0
    assert int((g_bits == 0).sum()) >= int((y0 <= 0).sum())


@pytest.mark.parametrize("case", [(8, 256, 256, 32, 16, True), (16, 128, 128, 32, 16, False), (12, 96, 160, 32, 16, True), (10, 256, 256, 32, 16, False),
                                  # the slice form (ynet_upsample2x_conv2d_winograd_supported == 2): the decoders' levels 3 and 2, and a ragged map
                                  (16, 128, 128, 64, 32, True), (32, 64, 64, 64, 32, False), (6, 96, 160, 64, 32, True), (256, 32, 32, 64, 32, True)], ids=str)
def test_upsample_and_up_convolution_in_one_launch(dev, case):
    """ynet_upsample2x_conv2d_winograd (round 5): conv3x3(bilinear x2 of x) + bias for 32 -> 16 channels without the up-sampled tensor --
    against torch's interpolate + conv2d in fp64 (2e-6 of the largest output) and against the two launches it replaces (ynet_upsample2x_fwd,
    then ynet_conv2d_winograd: the same values within fp32 rounding, the image borders -- bilinear clamp inside, the convolution's zero
    padding outside -- checked on their own); through autograd (ops.upsample2x_conv2d on a frozen HipConv2d): the input gradient equals
    the unfused graph's."""
    ops, ynet = pkg("ops"), pkg("models.ynet")
    B, H, W, cin, cout, has_bias = case
    Hl, Wl = H // 2, W // 2
    kind = ops._lib().ynet_upsample2x_conv2d_winograd_supported(B, H, W, cin, cout, 3)
    assert kind == (1 if (cin, cout) == (32, 16) else 2)
    x = torch.relu(rnd(B, cin, Hl, Wl, seed=1)).to(dev)
    w = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev)
    bias = rnd(cout, seed=3).to(dev) if has_bias else None
    wp = ops.pack_weight(w, 0)
    u = ops.winograd_filter(wp, cin, cout) if kind == 1 else ops._wino16_filter(({}, "fwd"), wp, 0, (cin,), cout, 0, cout).u
    got = torch.full((B, cout, H, W), float("nan"), device=dev)
    ops.upsample2x_conv2d_raw((x.data_ptr(), cin * Hl * Wl), u, bias, (got.data_ptr(), cout * H * W), cin, cout, B, H, W)
    up = ops.upsample2x(x)
    two = torch.empty(B, cout, H, W, device=dev)
    assert ops.conv2d_raw([(up.data_ptr(), cin, cin * H * W)], None, wp, bias, [(two.data_ptr(), cout, cout * H * W)], B, H, W, 3, False, wino=({}, "fwd")).startswith("winograd")
    ref64 = F.conv2d(F.interpolate(x.double(), scale_factor=2, mode="bilinear", align_corners=False), w.double(), bias.double() if has_bias else None, padding=1)
    assert not bool(torch.isnan(got).any())
    close(got, ref64, rtol=1e-5, scale_rel=2e-6, msg="fused vs fp64")
    close(got, two, rtol=1e-5, scale_rel=2e-6, msg="fused vs up-sample + convolution")
    scale = float(ref64.abs().max())
    for name, sl in (("top", (slice(None), slice(None), 0)), ("bottom", (slice(None), slice(None), -1)), ("left", (slice(None), slice(None), slice(None), 0)),
                     ("right", (slice(None), slice(None), slice(None), -1))):
        assert float((got[sl].double() - ref64[sl]).abs().max()) <= 2e-6 * scale + 2e-5, name
    e_f, e_t = float((got.double() - ref64).abs().max()), float((two.double() - ref64).abs().max())
    assert e_f <= 1.5 * e_t + 1e-7, (e_f, e_t)
    # autograd: a frozen up-convolution module
    conv = ynet.HipConv2d(cin, cout, kernel_size=3).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w)
        conv.bias.copy_(bias if has_bias else torch.zeros(cout, device=dev))
    conv.weight.requires_grad_(False)
    conv.bias.requires_grad_(False)
    g = rnd(B, cout, H, W, seed=5).to(dev)
    grads = []
    for fused in (True, False):
        old, n0 = ops._upconv_allowed, ops.upconv_stats["fused"]
        ops._upconv_allowed = fused
        try:
            xi = x.clone().requires_grad_(True)
            y = ops.upsample2x_conv2d(xi, conv)
            (y * g).sum().backward()
        finally:
            ops._upconv_allowed = old
        assert ops.upconv_stats["fused"] - n0 == (1 if fused else 0)
        grads.append((y.detach(), xi.grad))
    close(grads[0][0], grads[1][0], rtol=1e-5, scale_rel=2e-6, msg="module forward")
    close(grads[0][1], grads[1][1], rtol=1e-5, scale_rel=2e-6, msg="input gradient")


W16_CASES = [
    # B, H, W, [source channels], cout, relu, bias, mode (0 forward filter, 1 data gradient)
    (32, 64, 64, [64], 64, True, True, 0),          # the 64 -> 64 layers at 64^2 (4 slices, 2 tiles per team member)
    (32, 64, 64, [32], 64, True, True, 0),          # encoder stage 2's first layer
    (32, 64, 64, [64], 32, False, True, 0),         # the up-convolution 64 -> 32 at 64^2 (no ReLU)
    (8, 256, 256, [32], 16, False, True, 0),        # the up-convolution 32 -> 16 at 256^2 (one slice)
    (10, 64, 64, [64], 64, True, False, 1),         # batch 10: 40 tiles, teams smaller than 8
    (32, 64, 64, [32, 64], 64, True, True, 0),      # decoder level 2, first convolution: 96 channels = two launches (in-place add)
    (32, 64, 64, [32, 64, 1], 64, True, True, 0),   # ... + the way-point map: 97 channels
    (16, 128, 128, [64, 1], 64, True, True, 0),     # 65 -> 64 at 128^2 in ONE launch of four slices (17 chunks)
    (256, 32, 32, [64], 64, True, True, 0),         # evaluate()'s folded batch at 32^2
    (4, 96, 160, [20, 7], 16, False, False, 0),     # ragged channel counts (zero planes / zero filters), H = 3 tiles, W = 5 tiles
    (8, 64, 128, [32], 64, True, True, 0),          # H != W
]


@pytest.mark.parametrize("case", W16_CASES, ids=str)
def test_winograd_slice_form_matches_the_direct_form(dev, case):
    """ynet_conv2d_winograd16 (round 5: 16 output channels per workgroup, two row pairs per wave) through ops.conv2d_raw's dispatch: the
    same values as torch's convolution in fp64 and as ynet_conv2d within fp32 rounding (2e-6 of the largest output), its error against
    fp64 not above 1.5x the implicit GEMM's."""
    ops = pkg("ops")
    B, H, W, cs, cout, relu, has_bias, mode = case
    cin = sum(cs)
    xs = [torch.relu(rnd(B, c, H, W, seed=10 + i)).to(dev) for i, c in enumerate(cs)]
    w = (rnd(cout, cin, 3, 3, seed=2, scale=0.2) if mode == 0 else rnd(cin, cout, 3, 3, seed=2, scale=0.2)).to(dev)
    bias = rnd(cout, seed=3).to(dev) if has_bias else None
    wp = ops.pack_weight(w, mode)
    srcs = [(x.data_ptr(), c, c * H * W) for x, c in zip(xs, cs)]
    got, direct = torch.full((B, cout, H, W), float("nan"), device=dev), torch.empty(B, cout, H, W, device=dev)
    n0 = ops.wino_stats.get("launches16", 0)
    old = ops._wino16_for_16
    ops._wino16_for_16 = True
    try:
        tag = ops.conv2d_raw(srcs, None, wp, bias, [(got.data_ptr(), cout, cout * H * W)], B, H, W, 3, relu, wino=({}, "fwd" if mode == 0 else "dgrad"))
    finally:
        ops._wino16_for_16 = old
    assert tag is not None and tag.startswith("winograd16"), tag
    assert ops.wino_stats["launches16"] - n0 == (2 if cin > 84 else 1)
    assert ops.conv2d_raw(srcs, None, wp, bias, [(direct.data_ptr(), cout, cout * H * W)], B, H, W, 3, relu) is None
    x64 = torch.cat(xs, 1).double()
    ref64 = F.conv2d(x64, w.double(), bias.double() if has_bias else None, padding=1) if mode == 0 else F.conv_transpose2d(x64, w.double(), padding=1)
    ref64 = torch.relu(ref64) if relu else ref64
    close(got, ref64, rtol=1e-5, scale_rel=2e-6, msg="winograd16 vs fp64")
    close(got, direct, rtol=1e-5, scale_rel=2e-6, msg="winograd16 vs ynet_conv2d")
    e_w, e_d = float((got.double() - ref64).abs().max()), float((direct.double() - ref64).abs().max())
    assert e_w <= 1.5 * e_d + 1e-7, (e_w, e_d)


@pytest.mark.parametrize("B,H,W", [(32, 64, 64), (8, 64, 128)])
def test_winograd_slice_form_epilogues(dev, B, H, W):
    """The epilogue variants of ynet_conv2d_winograd16 at 64 channels, 64^2 (and a map with H != W): a data gradient over two destinations
    (32 + 64 channels, a third one nobody wants), the data gradient through the ReLU backward of the layer below (bit-identical to
    "plain, then mask"), the 2 x 2 max-pooled copy (bit-identical to max_pool2d of the same launch's output) and evaluate()'s
    shared-skip-term launch."""
    ops = pkg("ops")
    dy = rnd(B, 64, H, W, seed=1).to(dev)
    # ---- two wanted destinations + an unwanted one (decoder level 2's first convolution: up 32, skip 64, way-point map 1)
    w = rnd(64, 97, 3, 3, seed=2, scale=0.2).to(dev)
    wp = ops.pack_weight(w, 1)
    sizes = [32, 64, 1]
    want = [torch.empty(B, c, H, W, device=dev) for c in sizes]
    got = [torch.full((B, c, H, W), float("nan"), device=dev) for c in sizes]
    ops.conv2d_raw([(dy.data_ptr(), 64, 64 * H * W)], None, wp, None, [(t.data_ptr(), t.shape[1], t.shape[1] * H * W) for t in want], B, H, W, 3, False)
    dsts = [(got[0].data_ptr(), 32, 32 * H * W), (got[1].data_ptr(), 64, 64 * H * W), (None, 1, 0)]
    tag = ops.conv2d_raw([(dy.data_ptr(), 64, 64 * H * W)], None, wp, None, dsts, B, H, W, 3, False, wino=({}, "dgrad"))
    assert tag == "winograd16:0+0", tag
    close(got[0], want[0], rtol=1e-5, scale_rel=2e-6, msg="32-channel destination")
    close(got[1], want[1], rtol=1e-5, scale_rel=2e-6, msg="64-channel destination")
    assert bool(torch.isnan(got[2]).all())
    # ---- through the ReLU backward of the layer below
    w2 = rnd(64, 64, 3, 3, seed=3, scale=0.2).to(dev)
    wp2 = ops.pack_weight(w2, 1)
    act = torch.relu(rnd(B, 64, H, W, seed=4)).to(dev)
    plain, masked, direct = (torch.full((B, 64, H, W), float("nan"), device=dev) for _ in range(3))
    src, cache = [(dy.data_ptr(), 64, 64 * H * W)], {}
    assert ops.conv2d_raw(src, None, wp2, None, [(plain.data_ptr(), 64, 64 * H * W)], B, H, W, 3, False, wino=(cache, "dgrad")) == "winograd16:0"
    assert ops.conv2d_raw(src, None, wp2, None, [(masked.data_ptr(), 64, 64 * H * W)], B, H, W, 3, False, relu_of=(act.data_ptr(), 64 * H * W),
                          wino=(cache, "dgrad")) == "winograd16:1"
    assert ops.conv2d_raw(src, None, wp2, None, [(direct.data_ptr(), 64, 64 * H * W)], B, H, W, 3, False, relu_of=(act.data_ptr(), 64 * H * W)) is None
    assert torch.equal(masked, torch.where(act > 0, plain, torch.zeros_like(plain)))
    close(masked, direct, rtol=1e-5, scale_rel=2e-6, msg="through the ReLU backward: winograd16 vs implicit GEMM")
    # ---- the pooled copy
    x = torch.relu(rnd(B, 64, H, W, seed=5)).to(dev)
    w3, b3 = rnd(64, 64, 3, 3, seed=6, scale=0.2).to(dev), rnd(64, seed=7).to(dev)
    wp3 = ops.pack_weight(w3, 0)
    y, yp = torch.full((B, 64, H, W), float("nan"), device=dev), torch.full((B, 64, H // 2, W // 2), float("nan"), device=dev)
    assert ops.conv2d_raw([(x.data_ptr(), 64, 64 * H * W)], None, wp3, b3, [(y.data_ptr(), 64, 64 * H * W)], B, H, W, 3, True,
                          pooled=(yp.data_ptr(), 64 * (H // 2) * (W // 2)), wino=({}, "fwd")) == "winograd16:3"
    close(y, torch.relu(F.conv2d(x, w3, b3, padding=1)), rtol=1e-4, scale_rel=2e-6, msg="output vs torch")
    assert torch.equal(yp, F.max_pool2d(y, 2, 2))
    # ---- evaluate()'s shared-skip-term launch with 64 output channels: relu(conv(cat(up, way-point map), W_rest) + b + term[b % Bs])
    Bs, times = B // 2, 2
    up, wmap = torch.relu(rnd(Bs * times, 32, H, W, seed=8)).to(dev), torch.relu(rnd(Bs * times, 1, H, W, seed=9)).to(dev)
    skip = torch.relu(rnd(Bs, 64, H, W, seed=10)).to(dev)
    w4, b4 = rnd(64, 97, 3, 3, seed=11, scale=0.2).to(dev), rnd(64, seed=12).to(dev)
    outs = []
    for allowed in (True, False):
        old, cache = ops._wino_allowed, {}
        ops._wino_allowed = allowed
        try:
            with torch.no_grad():
                term = ops.shared_conv_term(skip, w4, 32, 96, cache)
                ops.rest_filter(w4, 32, 96, cache)
                ops.rest_filter_winograd(w4, 32, 96, cache, (32, 1), Bs * times, H, W)
                n1 = ops.wino_stats.get("launches16", 0)
                outs.append(ops.conv2d_shared_term(None, times, [up, wmap], w4, b4, True, cache, term, 32, 96))
                assert ops.wino_stats.get("launches16", 0) - n1 == (1 if allowed else 0)
        finally:
            ops._wino_allowed = old
    ref = torch.relu(F.conv2d(torch.cat([up, skip.repeat(times, 1, 1, 1), wmap], 1), w4, b4, padding=1))
    close(outs[0], outs[1], rtol=1e-5, scale_rel=2e-6, msg="shared term: winograd16 vs implicit GEMM")
    close(outs[0], ref, rtol=1e-4, scale_rel=2e-6, msg="shared term vs torch")


@pytest.mark.parametrize("case", [("plain", 520), ("dgrad_relu", 264), ("cat", 264), ("cat_add", 264)], ids=str)
def test_winograd_tensors_beyond_2_and_4_gib(dev, case):
    """the Winograd kernels address ONE image per buffer descriptor (base + b * batch stride in scalar registers), so a
    [B, 32, 256, 256] tensor of 2.2 GB (B = 264: the zero-fill offset 0x80000000 must stay out of range) or 4.4 GB (B = 520: beyond one
    32-bit descriptor) -- what evaluate() folds its K samples into on a real scene -- is served, borders included: every image against
    the implicit GEMM (per-image descriptors since round 1), the first / the 2-GiB-straddling / the last image against torch."""
    ops = pkg("ops")
    kind, B = case
    H = W = 256
    g = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, 32, H, W, device=dev, generator=g).relu_()
    assert x.numel() * 4 >= (1 << 31)
    w = rnd(32, 49 if kind.startswith("cat") else 32, 3, 3, seed=2, scale=0.2).to(dev)
    bias = rnd(32, seed=3).to(dev)
    got, direct = torch.full((B, 32, H, W), float("nan"), device=dev), torch.empty(B, 32, H, W, device=dev)
    dst = lambda t: [(t.data_ptr(), 32, 32 * H * W)]
    picks = [0, (1 << 31) // (32 * H * W * 4), B - 1]
    if kind == "plain":
        wp = ops.pack_weight(w, 0)
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, bias, dst(got), B, H, W, 3, True, wino=({}, "fwd")).startswith("winograd")
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, bias, dst(direct), B, H, W, 3, True) is None
        ref = lambda b: torch.relu(F.conv2d(x[b:b + 1], w, bias, padding=1))
    elif kind == "dgrad_relu":
        act = torch.randn(B, 32, H, W, device=dev, generator=g).relu_()
        wp = ops.pack_weight(w, 1)
        ro = (act.data_ptr(), 32 * H * W)
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, None, dst(got), B, H, W, 3, False, relu_of=ro, wino=({}, "dgrad")).startswith("winograd")
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, None, dst(direct), B, H, W, 3, False, relu_of=ro) is None
        ref = lambda b: F.conv_transpose2d(x[b:b + 1], w, padding=1) * (act[b:b + 1] > 0)
    else:
        skip = torch.randn(B if kind == "cat" else 4, 16, H, W, device=dev, generator=g).relu_()
        wmap = torch.rand(B, 1, H, W, device=dev, generator=g)
        if kind == "cat":
            wp = ops.pack_weight(w, 0)
            srcs = [(x.data_ptr(), 32, 32 * H * W), (skip.data_ptr(), 16, 16 * H * W), (wmap.data_ptr(), 1, H * W)]
            assert ops.conv2d_raw(srcs, None, wp, bias, dst(got), B, H, W, 3, True, wino=({}, "fwd")) == "winograd_cat:2,0"
            assert ops.conv2d_raw(srcs, None, wp, bias, dst(direct), B, H, W, 3, True) is None
            ref = lambda b: torch.relu(F.conv2d(torch.cat([x[b:b + 1], skip[b:b + 1], wmap[b:b + 1]], 1), w, bias, padding=1))
        else:       # evaluate()'s shared-skip-term launch: the term of image b % 4 added in front of the ReLU
            outs = []
            for allowed in (True, False):
                old, cache = ops._wino_allowed, {}
                ops._wino_allowed = allowed
                try:
                    with torch.no_grad():
                        term = ops.shared_conv_term(skip, w, 32, 48, cache)
                        ops.rest_filter(w, 32, 48, cache)
                        ops.rest_filter_winograd(w, 32, 48, cache, (32, 1), 4, H, W)
                        n1 = ops.wino_stats["launches"]
                        outs.append(ops.conv2d_shared_term(None, B // 4, [x, wmap], w, bias, True, cache, term, 32, 48))
                        assert ops.wino_stats["launches"] - n1 == (1 if allowed else 0)
                finally:
                    ops._wino_allowed = old
            got, direct = outs
            ref = lambda b: torch.relu(F.conv2d(torch.cat([x[b:b + 1], skip[b % 4:b % 4 + 1], wmap[b:b + 1]], 1), w, bias, padding=1))
    assert not bool(torch.isnan(got).any())
    scale = float(direct.abs().max())
    err = (got - direct).abs_()
    assert float(err.max()) <= 2e-6 * scale + 2e-5, (float(err.max()), scale)
    # the border rows / columns of every image (zero padding by the out-of-range offset) on their own
    for sl in (err[:, :, 0], err[:, :, -1], err[:, :, :, 0], err[:, :, :, -1]):
        assert float(sl.max()) <= 2e-6 * scale + 2e-5
    for b in picks:
        close(got[b:b + 1], ref(b), rtol=1e-4, scale_rel=2e-6, msg=f"image {b} vs torch")


@pytest.mark.parametrize("relu", [True, False])
def test_winograd_epilogue_propagates_nan(dev, relu):
    """a NaN convolution result stays a NaN through the epilogue's ReLU (torch: relu(NaN) = NaN), it is not turned into
    0 / -inf by a max against the floor.  One NaN input pixel: every output torch makes NaN is NaN here (the Winograd transforms spread
    it over the 2 x 2 blocks whose 4 x 4 patch holds the pixel, a superset), everything else finite and equal to the clean run's; the
    pooled copy carries it too."""
    ops = pkg("ops")
    B, H, W = 8, 128, 128
    x = torch.relu(rnd(B, 32, H, W, seed=1)).to(dev)
    w, bias = rnd(32, 32, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
    wp = ops.pack_weight(w, 0)
    clean = torch.empty(B, 32, H, W, device=dev)
    cache = {}
    ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, bias, [(clean.data_ptr(), 32, 32 * H * W)], B, H, W, 3, relu, wino=(cache, "fwd"))
    x[3, 5, 40, 77] = float("nan")
    got = torch.empty(B, 32, H, W, device=dev)
    assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, bias, [(got.data_ptr(), 32, 32 * H * W)], B, H, W, 3, relu, wino=(cache, "fwd")).startswith("winograd")
    want = F.conv2d(x, w, bias, padding=1)
    want = torch.relu(want) if relu else want
    nan_w, nan_g = torch.isnan(want), torch.isnan(got)
    assert int(nan_w.sum()) == 9 * 32 and bool((nan_g | ~nan_w).all()), "a NaN of the reference is missing"
    assert int(nan_g.sum()) <= 16 * 32 and bool(nan_g[3, :, 38:44, 74:80].any()) and not bool(torch.isinf(got).any())
    assert torch.equal(got[~nan_g], clean[~nan_g])
    if relu:       # the pooled copy of the same launch family (ynet_conv2d_winograd_cat_pool)
        y, yp = torch.empty(B, 32, H, W, device=dev), torch.empty(B, 32, H // 2, W // 2, device=dev)
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, wp, bias, [(y.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True,
                              pooled=(yp.data_ptr(), 32 * (H // 2) * (W // 2)), wino=({}, "fwd")).startswith("winograd_cat")
        assert bool(torch.isnan(y)[nan_w].all()) and torch.equal(torch.isnan(yp), torch.isnan(F.max_pool2d(y, 2, 2)))


# B, H, W, channels of the first layer's output (= of dx), channels of dy, dy masked too, input channels of the first layer
RELU_BITS_CASES = [
    (8, 128, 128, 32, 16, False, 14),     # two 16-channel tiles x 4 rows: 64 mask bits per lane
    (8, 128, 128, 32, 32, True, 32),      # ... with the consumer-side mask of dy on top
    (8, 64, 128, 64, 16, False, 48),      # four tiles x 2 rows
    (4, 128, 128, 48, 64, True, 20),      # three tiles x 2 rows: 48 bits, the second word half filled
    (8, 128, 128, 16, 32, False, 8),      # one tile: 32 bits or fewer, one word per lane
    (8, 204, 136, 32, 32, False, 16),     # ragged tile rows / columns (H % 8, W % 32 != 0)
]


@pytest.mark.parametrize("case", RELU_BITS_CASES, ids=[str(c) for c in RELU_BITS_CASES])
def test_one_bit_relu_mask_between_two_convolutions(dev, case):
    """conv -> ReLU -> conv.  The first layer's forward launch also writes one bit per output element (y > 0) in
    the register layout of its tiles (ynet_conv2d_relu_bits); the second layer's data gradient -- same output shape, same tiling --
    applies it to what it writes (ynet_conv2d_dgrad_relu_bits).  Bit-identical to the float-activation form (ynet_conv2d_dgrad_relu)
    and the forward output bit-identical to the plain launch; -0.0 and NaN activations count as "not positive" in both."""
    ops = pkg("ops")
    lib = ops._lib()
    B, H, W, c1, c2, masked, c0 = case
    n_words = lib.ynet_conv2d_relu_bits_words(B, H, W, c1, 3)
    assert n_words > 0 and lib.ynet_conv2d_dgrad_relu_supported(B, H, W, c1, 3)
    x, w1, b1 = rnd(B, c0, H, W, seed=1).to(dev), rnd(c1, c0, 3, 3, seed=2, scale=0.2).to(dev), rnd(c1, seed=3, scale=0.1).to(dev)
    x[0, 0, 3, 5] = float("nan")                         # a NaN activation patch: the bit must be 0 where y is NaN
    wp1 = ops.pack_weight(w1, 0)
    y_plain, y_bits = torch.empty(B, c1, H, W, device=dev), torch.full((B, c1, H, W), float("nan"), device=dev)
    bits = torch.full((n_words,), -1, device=dev, dtype=torch.int32)
    ops.conv2d_raw([(x.data_ptr(), c0, c0 * H * W)], None, wp1, b1, [(y_plain.data_ptr(), c1, c1 * H * W)], B, H, W, 3, True)
    ops.conv2d_raw([(x.data_ptr(), c0, c0 * H * W)], None, wp1, b1, [(y_bits.data_ptr(), c1, c1 * H * W)], B, H, W, 3, True,
                   bits_out=bits.data_ptr())
    assert torch.equal(torch.nan_to_num(y_bits, nan=-7.0), torch.nan_to_num(y_plain, nan=-7.0))
    assert bool(torch.isnan(y_plain).any())
    # the second layer's data gradient through the first layer's ReLU backward
    dy, w2 = rnd(B, c2, H, W, seed=4).to(dev), rnd(c2, c1, 3, 3, seed=5, scale=0.2).to(dev)
    y2 = torch.relu(rnd(B, c2, H, W, seed=6)).to(dev)
    wp2 = ops.pack_weight(w2, 1)
    mask = (y2.data_ptr(), c2 * H * W) if masked else None
    want, got = torch.empty(B, c1, H, W, device=dev), torch.full((B, c1, H, W), float("nan"), device=dev)
    ops.conv2d_raw([(dy.data_ptr(), c2, c2 * H * W)], mask, wp2, None, [(want.data_ptr(), c1, c1 * H * W)], B, H, W, 3, False,
                   relu_of=(y_plain.data_ptr(), c1 * H * W))
    ops.conv2d_raw([(dy.data_ptr(), c2, c2 * H * W)], mask, wp2, None, [(got.data_ptr(), c1, c1 * H * W)], B, H, W, 3, False,
                   relu_bits=bits.data_ptr())
    assert torch.equal(got, want), float((got - want).abs().max())
    assert float(got[torch.isnan(y_plain)].abs().sum()) == 0.0
    # a shape the bit-mask epilogues do not serve is refused, loudly
    assert lib.ynet_conv2d_relu_bits_words(2, 16, 16, 64, 3) == 0
    small = torch.zeros(2, 64, 16, 16, device=dev)
    with pytest.raises(RuntimeError, match="not served"):
        ops.conv2d_raw([(small.data_ptr(), 64, 64 * 256)], None, ops.pack_weight(rnd(64, 64, 3, 3, seed=7).to(dev), 0), None,
                       [(small.data_ptr(), 64, 64 * 256)], 2, 16, 16, 3, True, bits_out=bits.data_ptr())


def test_relu_backward_applied_by_upsampling_and_by_the_next_data_gradient(dev):
    """conv0-ReLU -> conv1-ReLU -> bilinear x2 -> conv2 (no ReLU): conv1's output gradient comes from the up-sampling backward
    (ynet_upsample2x_bwd_relu), conv0's from conv1's data gradient (ynet_conv2d_dgrad_relu); both then run unmasked dgrad /
    wgrad kernels.  Same gradients as stock autograd; the data gradient bit-identical to the consumer-side masks."""
    ops = pkg("ops")
    B, H, W = 8, 128, 128          # (large enough for the two-row tiles that mask inside the conv kernel)
    x = rnd(B, 6, H, W, seed=1)
    w0, w1, w2 = rnd(16, 6, 3, 3, seed=2, scale=0.2), rnd(16, 16, 3, 3, seed=3, scale=0.2), rnd(4, 16, 3, 3, seed=4, scale=0.2)
    xc, w0c, w1c = x.clone().requires_grad_(True), w0.clone().requires_grad_(True), w1.clone().requires_grad_(True)
    g = F.relu(F.conv2d(F.relu(F.conv2d(xc, w0c, padding=1)), w1c, padding=1))
    F.conv2d(F.interpolate(g, scale_factor=2, mode="bilinear", align_corners=False), w2, padding=1).square().sum().backward()
    got = {}
    # wino: with the Winograd generation (this shape is served by it) conv1's data gradient is ynet_conv2d_winograd_dgrad_relu, which reads conv0's
    # float activation -- no 1-bit mask --; without it the implicit GEMM takes the 1-bit form.  The producer-side masks work either way.
    for on, wino in ((True, False), (False, False), (True, True)):
        old, old_w = ops._premask_allowed, ops._wino_allowed
        ops._premask_allowed, ops._wino_allowed = on, wino
        ops.premask_stats["unmasked_backwards"] = 0
        ops.premask_stats["bit_masks"] = 0
        n_w = ops.wino_stats["launches"]
        try:
            with ops.fold_skip_gradients():
                xd, w0d, w1d = x.to(dev).requires_grad_(True), w0.to(dev).requires_grad_(True), w1.to(dev).requires_grad_(True)
                # (bits=True: what FusedSequential asks of the first conv of a conv -> ReLU -> conv chain -- conv1's data gradient
                # then takes conv0's ReLU mask in its 1-bit form)
                gd = ops.conv2d(ops.conv2d(xd, w0d, None, True, {}, bits=True), w1d, None, True, {})
                ops.conv2d(ops.upsample2x(gd), w2.to(dev), None, False, {}).square().sum().backward()
        finally:
            ops._premask_allowed, ops._wino_allowed = old, old_w
        assert ops.premask_stats["unmasked_backwards"] == (2 if on else 0)
        if wino:
            assert ops.premask_stats["bit_masks"] == 0 and ops.wino_stats["launches"] - n_w >= 2      # (conv1's forward and its masked data gradient at least)
            close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg="dx (Winograd launches)")
            close(w0d.grad, w0c.grad, rtol=1e-4, scale_rel=1e-5, msg="dW0 (Winograd launches)")
            close(w1d.grad, w1c.grad, rtol=1e-4, scale_rel=1e-5, msg="dW1 (Winograd launches)")
            continue
        assert ops.premask_stats["bit_masks"] == (1 if (on and ops._relu_bits_allowed) else 0)
        assert not ops._premasked
        close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg=f"dx (premask={on})")
        close(w0d.grad, w0c.grad, rtol=1e-4, scale_rel=1e-5, msg=f"dW0 (premask={on})")
        close(w1d.grad, w1c.grad, rtol=1e-4, scale_rel=1e-5, msg=f"dW1 (premask={on})")
        got[on] = (xd.grad.clone(), w0d.grad.clone(), w1d.grad.clone())
    # the data gradient is bit-identical (the mask is an exact zeroing wherever it is applied); the filter gradients of a map this
    # large come from differently split pixel sums (unmasked rolling-row kernel: 3 workgroups per CU, masked: 2) -> rounding only
    assert torch.equal(got[True][0], got[False][0])
    for a, b in zip(got[True][1:], got[False][1:]):
        close(a, b, rtol=1e-5, scale_rel=2e-6, msg="dW, masks at the producer vs at the consumer")


@pytest.mark.parametrize("cin,cout,relu", [(32, 12, False), (12, 32, False), (32, 30, True), (7, 16, True), (32, 33, False)])
def test_conv1x1_predictor_kernels(dev, cin, cout, relu):
    """The streaming 1x1 kernel (Cout <= 32: 16 x 4-pixel and 32 x 2-pixel variants) and the MFMA path beyond it."""
    ops = pkg("ops")
    B, H, W = 3, 16, 24
    x, w, b = rnd(B, cin, H, W, seed=1), rnd(cout, cin, 1, 1, seed=2, scale=0.3), rnd(cout, seed=3, scale=0.1)
    y = F.conv2d(x, w, b)
    y = F.relu(y) if relu else y
    yd = ops.conv2d(x.to(dev), w.to(dev), b.to(dev), relu, {})
    close(yd, y, msg="1x1")
    # batch-broadcast input (stride 0)
    y1 = F.conv2d(x[:1].expand(B, -1, -1, -1), w, b)
    y1 = F.relu(y1) if relu else y1
    close(ops.conv2d(x[:1].to(dev).expand(B, -1, -1, -1), w.to(dev), b.to(dev), relu, {}), y1, msg="1x1 broadcast")


@pytest.mark.parametrize("shape", [(2, 3, 8, 16), (1, 2, 1, 1), (1, 4, 5, 3), (2, 16, 32, 32), (1, 2, 3, 6), (2, 2, 1, 4), (1, 3, 7, 12), (2, 2, 2, 128), (1, 2, 64, 64), (1, 1, 68, 62), (1, 2, 6, 10)])
def test_upsample2x(dev, shape):
    ops = pkg("ops")
    x = rnd(*shape, seed=1)
    xc = x.clone().requires_grad_(True)
    y = F.interpolate(xc, scale_factor=2, mode="bilinear", align_corners=False)
    gy = rnd(*y.shape, seed=2)
    y.backward(gy)
    xd = x.to(dev).requires_grad_(True)
    yd = ops.upsample2x(xd)
    yd.backward(gy.to(dev))
    close(yd, y, rtol=1e-6, atol=1e-6, msg="up fwd")
    close(xd.grad, xc.grad, rtol=1e-5, atol=1e-5, msg="up bwd")


@pytest.mark.parametrize("shape", [(2, 3, 8, 16), (1, 4, 5, 3), (2, 16, 32, 32), (1, 2, 3, 6), (1, 3, 7, 12), (1, 2, 64, 64), (1, 1, 68, 62), (1, 2, 6, 10)])
def test_upsample2x_bwd_relu(dev, shape):
    """ynet_upsample2x_bwd_relu = ynet_upsample2x_bwd followed by the ReLU backward of the up-sampled activation (every kernel
    variant: 4-row, 2-row, quad, scalar), bit-identical to masking afterwards."""
    ops, L = pkg("ops"), pkg("_lib")
    lib = ops._lib()
    B, C, H, W = shape
    gy = rnd(B, C, 2 * H, 2 * W, seed=2).to(dev)
    act = torch.relu(rnd(B, C, H, W, seed=3)).to(dev)
    plain, got = torch.empty(B, C, H, W, device=dev), torch.full((B, C, H, W), float("nan"), device=dev)
    L.check(lib.ynet_upsample2x_bwd(gy.data_ptr(), plain.data_ptr(), B * C, H, W, ops._stream()), lib)
    L.check(lib.ynet_upsample2x_bwd_relu(gy.data_ptr(), got.data_ptr(), act.data_ptr(), B * C, H, W, ops._stream()), lib)
    torch.cuda.synchronize()
    assert torch.equal(got, torch.where(act > 0, plain, torch.zeros_like(plain)))


@pytest.mark.parametrize("cls,wd", [("Adam", 0.0), ("Adam", 0.01), ("AdamW", 0.05), ("Adam+decoupled", 0.05)])
def test_adam_step_kernel_matches_torch(dev, cls, wd):
    """ynet_adam_step (what a captured step launches instead of torch's fused multi-tensor Adam) against torch.optim.Adam / AdamW on the
    device: five steps over tensors of 1 .. 70,000 elements, one of them without a gradient; the step counters advance as torch's do."""
    sg = pkg("utils.step_graph")
    if not sg.ADAM_KERNEL:
        pytest.skip("YNET_ADAM_KERNEL=0")
    shapes = [(1,), (7, 3), (1025,), (64, 64, 3, 3), (70000,), (5,)]
    ps = [torch.nn.Parameter(rnd(*sh, seed=i).to(dev)) for i, sh in enumerate(shapes)]
    qs = [torch.nn.Parameter(p.detach().clone()) for p in ps]
    if cls == "Adam+decoupled":      # torch.optim.Adam(decoupled_weight_decay=True) IS AdamW's rule (the kernel must follow it)
        import inspect
        if "decoupled_weight_decay" not in inspect.signature(torch.optim.Adam.__init__).parameters:
            pytest.skip("this torch has no Adam(decoupled_weight_decay=)")
        make = lambda params, **kw: torch.optim.Adam(params, decoupled_weight_decay=True, **kw)      # noqa: E731
    else:
        make = getattr(torch.optim, cls)
    ref, mine = make(ps, lr=1e-3, weight_decay=wd), make(qs, lr=1e-3, weight_decay=wd, capturable=True, fused=True)
    for step in range(5):
        for i, (p, q) in enumerate(zip(ps, qs)):
            g = None if i == 5 else rnd(*shapes[i], seed=100 + 10 * step + i).to(dev) * (10.0 if i == 2 else 1.0)
            p.grad, q.grad = g, (None if g is None else g.clone())
        ref.step()
        if step == 0:
            mine.step()                      # (torch creates the state; from then on the kernel advances it)
            tabs = sg._AdamTables.prepare(mine)
            assert tabs is not None
        else:
            sg._AdamTables.fill(tabs, mine)  # (new gradient tensors every step here: refresh the pointers)
            sg._AdamTables.step(tabs)
    torch.cuda.synchronize()
    for i, (p, q) in enumerate(zip(ps, qs)):
        close(q, p, rtol=1e-5, scale_rel=1e-6, msg=f"param {i}")
        if i != 5:
            close(mine.state[q]["exp_avg"], ref.state[p]["exp_avg"], rtol=1e-5, scale_rel=1e-6, msg="exp_avg")      # (torch's default foreach path rounds its lerp differently by an ulp)
            close(mine.state[q]["exp_avg_sq"], ref.state[p]["exp_avg_sq"], rtol=1e-5, scale_rel=1e-6, msg="exp_avg_sq")
            assert float(mine.state[q]["step"]) == 5.0
    assert torch.equal(qs[5], ps[5]) and qs[5] not in mine.state or "step" not in mine.state.get(qs[5], {})


def test_batch_expand_gives_every_consumer_its_own_batch_sum(dev):
    """ops.BatchExpand: a one-image tensor read by two convolutions as a batch-broadcast source -- each conv expands it itself
    (_BatchExpandFn), so its gradient is two ynet_batch_sum launches + a one-image add; same gradient as stock autograd."""
    ops = pkg("ops")
    B, C, H, W = 6, 8, 16, 32
    x, w1, w2 = rnd(1, C, H, W, seed=1), rnd(12, C, 3, 3, seed=2, scale=0.2), rnd(4, C + 3, 3, 3, seed=3, scale=0.2)
    other = rnd(B, 3, H, W, seed=4)
    xc = x.clone().requires_grad_(True)
    xe = xc.expand(B, -1, -1, -1)
    (F.conv2d(xe, w1, padding=1).square().sum() + F.conv2d(torch.cat([xe, other], 1), w2, padding=1).sum() * 3.0).backward()
    xd = x.to(dev).requires_grad_(True)
    be = ops.BatchExpand(xd, B)
    total = ops.conv2d(be, w1.to(dev), None, False, {}).square().sum() \
        + ops.conv2d(ops.lazy_cat([be, other.to(dev)]), w2.to(dev), None, False, {}).sum() * 3.0
    total.backward()
    close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg="gradient of the broadcast image")
    got = ops.lazy_cat([be, other.to(dev)]).materialize()
    assert torch.equal(got.cpu(), torch.cat([x.expand(B, -1, -1, -1), other], 1))


def test_avgpool_pyramid(dev):
    ops = pkg("ops")
    x = rnd(3, 2, 64, 96, seed=1).abs()
    got = ops.avgpool_pyramid(x.to(dev), 6)
    want = O.waypoint_pyramid(x, 6)
    assert len(got) == 6
    for g, w in zip(got, want):
        close(g, w, rtol=1e-6, atol=1e-6, msg="pyramid")


def test_bce_with_logits(dev):
    ops = pkg("ops")
    x = rnd(2, 12, 32, 64, seed=1, scale=4.0)
    t = torch.rand(2, 12, 32, 64, generator=torch.Generator().manual_seed(2)) * 0.01
    xc = x.clone().requires_grad_(True)
    loss = F.binary_cross_entropy_with_logits(xc, t) * 1000
    loss.backward()
    xd = x.to(dev).requires_grad_(True)
    ld = ops.bce_with_logits(xd, t.to(dev)) * 1000
    ld.backward()
    close(ld, loss.detach(), rtol=2e-6, atol=1e-6, msg="loss")
    close(xd.grad, xc.grad, rtol=1e-5, atol=1e-9, msg="dlogits")
    # the gradient is written by the forward pass for an *expected* upstream gradient: right, wrong, and reused graphs
    for expected in (1000.0, 3.0):
        xe = x.to(dev).requires_grad_(True)
        le = ops.bce_with_logits(xe, t.to(dev), expected) * 1000
        le.backward(retain_graph=True)
        close(le, loss.detach(), rtol=2e-6, atol=1e-6, msg=f"loss (expected_grad {expected})")
        close(xe.grad, xc.grad, rtol=1e-5, atol=1e-9, msg=f"dlogits (expected_grad {expected})")
        xe.grad = None
        le.backward()
        close(xe.grad, xc.grad, rtol=1e-5, atol=1e-9, msg="dlogits, second backward")
    # ragged length (not a multiple of 4), wide range of logits, no-grad path
    xr = torch.linspace(-30, 30, 1027).view(1, 1, 13, 79)
    tr = torch.rand(1, 1, 13, 79, generator=torch.Generator().manual_seed(3))
    xrc = xr.clone().requires_grad_(True)
    lr_ = F.binary_cross_entropy_with_logits(xrc.double(), tr.double())
    lr_.backward()
    xrd = xr.to(dev).requires_grad_(True)
    lrd = ops.bce_with_logits(xrd, tr.to(dev))
    lrd.backward()
    close(lrd, lr_.detach().float(), rtol=1e-6, atol=0, msg="ragged loss")
    close(xrd.grad, xrc.grad, rtol=1e-5, atol=2e-10, msg="ragged dlogits")
    with torch.no_grad():
        close(ops.bce_with_logits(xr.to(dev), tr.to(dev)), lr_.detach().float(), rtol=1e-6, atol=0, msg="no-grad loss")
    zero = ops.bce_with_logits(torch.zeros(1, 1, 8, 8, device=dev), torch.zeros(1, 1, 8, 8, device=dev)) * 1000
    assert abs(float(zero) - 1000 * np.log(2)) < 1e-3      # known answer


def test_softargmax_golden_and_slices(dev):
    ops = pkg("ops")
    g = Golden("kernels")
    x = g.t("softargmax/x")
    got = ops.softargmax2d(x.to(dev))
    close(got, g.t("softargmax/out"), rtol=1e-5, atol=2e-5, msg="softargmax vs reference")
    assert abs(float(got[0, 0, 0]) - 7) < 1e-4 and abs(float(got[0, 0, 1]) - 5) < 1e-4   # known answer
    # channel slice without a copy, odd width (scalar path), and fp64 truth
    sl = ops.softargmax2d(x.to(dev)[:, -1:])
    close(sl, g.t("softargmax/out")[:, -1:], rtol=1e-5, atol=2e-5, msg="slice")
    y = rnd(2, 3, 17, 23, seed=3, scale=3.0)
    close(ops.softargmax2d(y.to(dev)), O.softargmax2d(y.double()).float(), rtol=1e-5, atol=2e-5, msg="odd width")
    # non-finite logits behave as in the reference: -inf has weight 0; a NaN or +inf logit makes its plane NaN
    z = rnd(1, 4, 16, 32, seed=4)
    z[0, 0, 3, 5] = float("-inf")
    z[0, 1, 2, 7] = float("nan")
    z[0, 2, 9, 9] = float("inf")
    want = O.softargmax2d(z)
    gotz = ops.softargmax2d(z.to(dev)).cpu()
    assert torch.isnan(want[0, 1]).all() and torch.isnan(want[0, 2]).all()
    assert torch.isnan(gotz[0, 1]).all() and torch.isnan(gotz[0, 2]).all()
    close(gotz[0, [0, 3]], want[0, [0, 3]], rtol=1e-5, atol=2e-5, msg="planes with -inf / finite logits")
    with pytest.raises(ValueError):
        ops.softargmax2d(torch.zeros(3, 4, 4, device=dev))
    with pytest.raises(TypeError):
        ops.softargmax2d([1, 2])


def test_softargmax_accuracy_vs_fp64(dev):
    """Closer to the fp64 truth than (or as close as) the fp32 reference on flat and peaky maps."""
    ops = pkg("ops")
    for scale in (0.5, 8.0):
        x = rnd(4, 12, 256, 256, seed=5, scale=scale)
        truth = O.softargmax2d(x.double())
        ref32 = O.softargmax2d(x)
        got = ops.softargmax2d(x.to(dev)).cpu()
        e_ref = float((ref32.double() - truth).abs().max())
        e_got = float((got.double() - truth).abs().max())
        assert e_got <= max(2 * e_ref, 2e-5), (scale, e_got, e_ref)


@pytest.mark.parametrize("B,cin,cout,H,W,scale", [(3, 32, 30, 64, 128, 1.0), (2, 32, 12, 256, 256, 3.0), (2, 8, 12, 32, 32, 2.0),
                                                  (2, 16, 1, 24, 32, 4.0), (1, 32, 30, 96, 160, 1.0)])
def test_pred_softargmax_is_conv1x1_then_softargmax(dev, B, cin, cout, H, W, scale):
    """ynet_pred_softargmax (predictor on the matrix cores, logits in registers only) against the fp64 truth of
    SoftArgmax2D(conv1x1(x)) and against the two launches it replaces (utils/evaluate.py:259-262)."""
    ops = pkg("ops")
    x = F.relu(rnd(B, cin, H, W, seed=1))
    w, b = rnd(cout, cin, 1, 1, seed=2, scale=scale / cin ** 0.5), rnd(cout, seed=3, scale=0.5)
    assert ops.pred_softargmax_supported(x.to(dev), w.to(dev))
    truth = O.softargmax2d(F.conv2d(x.double(), w.double(), b.double()))
    ref32 = O.softargmax2d(F.conv2d(x, w, b))
    got = ops.pred_softargmax(x.to(dev), w.to(dev), b.to(dev)).cpu()
    two = ops.softargmax2d(ops.conv2d(x.to(dev), w.to(dev), b.to(dev), False, {})).cpu()
    e_ref, e_got, e_two = (float((t.double() - truth).abs().max()) for t in (ref32, got, two))
    assert e_got <= max(2 * e_ref, 3e-5), (e_got, e_ref, e_two)
    close(got, two, rtol=0, atol=1e-4, msg="fused vs two launches")
    # no bias; a batch-strided input (channel slice of a wider tensor)
    wide = F.relu(rnd(B, cin + 8, H, W, seed=4)).to(dev)
    got2 = ops.pred_softargmax(wide[:, :cin], w.to(dev), None).cpu()
    want2 = O.softargmax2d(F.conv2d(wide[:, :cin].cpu().double(), w.double()))
    close(got2, want2.float(), rtol=0, atol=1e-4, msg="strided, no bias")


def test_pred_softargmax_nonfinite_and_unsupported(dev):
    ops = pkg("ops")
    # The reference is the composition itself, SoftArgmax2D(conv1x1(x)) in stock fp32 torch.  A non-finite INPUT reaches every plane of its pixel (0 * inf = NaN in
    # the predictor's product, on the matrix cores as in F.conv2d), so the -inf / +inf logits of single planes come from an overflowing product, and the NaN
    # input sits in an image of its own.  (Until close() counted NaN as a mismatch this test took the input channels for the logits and passed on NaN output.)
    x = F.relu(rnd(2, 32, 16, 32, seed=5))
    w = torch.zeros(4, 32, 1, 1)
    w[0, 0] = w[1, 1] = w[2, 2] = w[3, 3] = 2.0                      # logits of plane c = 2 * input channel c
    x[0, 0, 3, 5] = -3e38                                            # 2 * -3e38 = -inf in plane 0: its weight is 0, the plane stays finite
    x[0, 2, 9, 9] = 3e38                                             # +inf in plane 2: exp(inf - inf) = NaN, as in the reference
    x[1, 1, 2, 7] = float("nan")                                     # image 1: a NaN input -> every plane
    logits = F.conv2d(x, w)
    assert logits[0, 0, 3, 5] == float("-inf") and logits[0, 2, 9, 9] == float("inf") and bool(torch.isfinite(logits[0, [1, 3]]).all())
    want = O.softargmax2d(logits)
    got = ops.pred_softargmax(x.to(dev), w.to(dev), None).cpu()
    assert torch.isnan(got[0, 2]).all() and torch.isnan(want[0, 2]).all() and torch.isnan(got[1]).all() and torch.isnan(want[1]).all()
    assert bool(torch.isfinite(want[0, [0, 1, 3]]).all())
    close(got[0, [0, 1, 3]], want[0, [0, 1, 3]], rtol=1e-5, atol=2e-5, msg="planes with -inf / finite logits")
    # non-finite inputs in one image: every plane of that image is NaN, in the composition and in the kernel
    x = F.relu(rnd(1, 32, 16, 32, seed=5))
    x[0, 0, 3, 5], x[0, 1, 2, 7], x[0, 2, 9, 9] = float("-inf"), float("nan"), float("inf")
    assert torch.isnan(O.softargmax2d(F.conv2d(x, w))).all() and torch.isnan(ops.pred_softargmax(x.to(dev), w.to(dev), None)).all()
    assert not ops.pred_softargmax_supported(torch.zeros(1, 32, 17, 23, device=dev), w.to(dev))      # H*W % 128 != 0
    assert not ops.pred_softargmax_supported(torch.zeros(1, 24, 16, 32, device=dev), torch.zeros(4, 24, 1, 1, device=dev))
    assert not ops.pred_softargmax_supported(torch.zeros(1, 32, 16, 32, device=dev), torch.zeros(33, 32, 1, 1, device=dev))


def test_sigmoid_temp(dev):
    ops = pkg("ops")
    x = rnd(3, 30, 16, 32, seed=1, scale=3.0)
    for sel, T in (([14, 29], 1.8), ([11], 1.0)):
        got = ops.sigmoid_temp(x.to(dev), sel, T)
        want = torch.sigmoid(x[:, sel] / T)
        close(got, want, rtol=1e-6, atol=1e-7, msg="sigmoid")


def test_gather_patch_golden(dev):
    ops = pkg("ops")
    g = Golden("kernels")
    xy = g.t("patch/xy")
    for name, tmpl in (("dist", O.dist_template(210)), ("gauss", O.gaussian_template(210, 31, 4))):
        want = g.t("patch/" + name)
        for coords in (xy.numpy(), xy, xy.to(dev)):       # host array, host tensor, device tensor
            got = ops.gather_patches(tmpl.to(dev), coords, 24, 40)
            assert torch.equal(got.cpu(), want), name       # bit-exact incl. round-half-even (10.5 -> 10, 11.5 -> 12)
    with pytest.raises(ValueError):
        ops.gather_patches(O.dist_template(64).to(dev), np.array([[40.0, 0.0]], dtype=np.float32), 32, 32)


@pytest.mark.parametrize("rows,n,K,replacement,thr", [
    (6, 64 * 64, 20, False, None), (3, 256 * 256, 20, False, None), (5, 40 * 72, 1, False, 0.05), (2, 100, 48, False, None),
    (4, 64 * 64, 10000, True, 0.002), (2, 256 * 256, 10000, True, 0.01), (3, 777, 50, True, None)])
def test_device_multinomial_matches_its_cpu_restatement(dev, rows, n, K, replacement, thr):
    """ynet_multinomial (Philox4x32-10 exponential race / inverse CDF) == oracle.device_multinomial, draw for draw."""
    ops = pkg("ops")
    gen = torch.Generator().manual_seed(n + K)
    prob = torch.sigmoid(torch.randn(rows, n, generator=gen) * 3)
    prob[0, : n // 3] = 0.0                                  # zero-probability entries never win
    seed = 0x1234567 * (K + 1) + 0x9ABCDEF012345
    want = O.device_multinomial(prob, K, replacement, thr, seed)
    got = ops.multinomial(prob.to(dev), K, replacement, thr, seed).cpu()
    assert torch.equal(got, want), int((got != want).sum())
    if not replacement:
        assert all(len(set(r.tolist())) == K for r in got)  # without replacement: distinct
    assert bool((prob.gather(1, got) > 0).all())
    # a strided view (every second row of a wider matrix) is read in place
    wide = torch.stack([prob, prob.flip(0)], dim=1).reshape(2 * rows, n).to(dev)
    got2 = ops.multinomial(wide[::2], K, replacement, thr, seed).cpu()
    assert torch.equal(got2, want)
    # the seed as a DEVICE input (ynet_multinomial_devseed: what a captured evaluation sweep passes): the same draws
    seeds = torch.tensor([7, seed, 9], dtype=torch.int64, device=dev)
    got3 = ops.multinomial(prob.to(dev), K, replacement, thr, seeds[1:2]).cpu()
    assert torch.equal(got3, want)
    with pytest.raises(ValueError, match="one int64 element"):
        ops.multinomial(prob.to(dev), K, replacement, thr, seeds)


def test_device_multinomial_frequencies(dev):
    """Sanity of the sampler itself (not only of its restatement): empirical frequencies follow the probabilities."""
    ops = pkg("ops")
    p = torch.tensor([[0.05, 0.15, 0.0, 0.3, 0.5]]).to(dev)
    with_rep = ops.multinomial(p, 40000, True, None, 11).cpu().flatten()
    np.testing.assert_allclose(np.bincount(with_rep.numpy(), minlength=5) / 40000, p.cpu().numpy()[0], atol=0.01)
    first = torch.cat([ops.multinomial(p.expand(2000, -1).contiguous(), 1, False, None, s).cpu() for s in range(3)]).flatten()
    np.testing.assert_allclose(np.bincount(first.numpy(), minlength=5) / 6000, p.cpu().numpy()[0], atol=0.02)
    ops.check_patch_status()
    ops.multinomial(torch.zeros(1, 8, device=dev), 1, True, None, 1)      # an all-zero row is reported
    with pytest.raises(RuntimeError, match="invalid multinomial"):
        ops.check_patch_status()


@pytest.mark.parametrize("H,W,rot", [(64, 64, False), (64, 96, True), (256, 256, True)])
def test_cws_prior_matches_the_reference_gaussian(dev, H, W, rot):
    """ynet_cws_prior (fp64 per pixel) against the oracle's restatement of torch_multivariate_gaussian_heatmap
    (utils/evaluate.py:9-34) times the sigmoid map, normalised, and its expectation."""
    ops = pkg("ops")
    gen = torch.Generator().manual_seed(H + W)
    B, G = 3, 2
    sig = torch.sigmoid(torch.randn(B, H, W, generator=gen))
    mean = torch.rand(G * B, 2, generator=gen) * torch.tensor([W * 0.6, H * 0.6]) + torch.tensor([W * 0.2, H * 0.2])
    dist = (torch.rand(G * B, 2, generator=gen) - 0.5) * 60
    maps, xy = ops.cws_prior(sig.to(dev), mean.to(dev), dist.to(dev), 6.0, 2.0, rot, want_map=True, want_xy=True)
    for r in range(G * B):
        k = O.cws_gaussian(mean[r], H, W, dist[r], 6.0, 2.0, rot)
        mm = sig[r % B] * k
        mm = mm / mm.sum()
        want_xy = O.softargmax_on_map(mm[None, None])[0, 0]
        np.testing.assert_allclose(maps[r].cpu().numpy(), mm.numpy(), rtol=2e-4, atol=1e-9)
        np.testing.assert_allclose(xy[r].cpu().numpy(), want_xy.numpy(), rtol=0, atol=2e-5 * max(H, W) / 64)


@pytest.mark.parametrize("B,cin,cout,H,W,train_pred,scale,up", [
    (3, 32, 12, 16, 24, False, 1000.0, 1000.0), (2, 32, 30, 32, 32, True, 1000.0, 1000.0), (2, 8, 12, 8, 8, True, 1000.0, 250.0),
    (1, 16, 1, 4, 4, True, 1.0, 1.0)])
def test_fused_predictor_and_bce(dev, B, cin, cout, H, W, train_pred, scale, up):
    """ynet_pred_bce: 1x1 predictor + BCEWithLogitsLoss (mean) + the predictor's dgrad (+ dlogits for its wgrad) in
    one pass, against stock torch; `up` != scale exercises the rescale of the pre-computed gradients."""
    ops = pkg("ops")
    x = rnd(B, cin, H, W, seed=1).relu()
    w, b = rnd(cout, cin, 1, 1, seed=2, scale=0.3), rnd(cout, seed=3, scale=0.1)
    t = torch.rand(B, cout, H, W, generator=torch.Generator().manual_seed(4)) * 0.01
    xc, wc, bc = x.clone().requires_grad_(True), w.clone().requires_grad_(train_pred), b.clone().requires_grad_(train_pred)
    yc = F.conv2d(xc, wc, bc)
    lc = F.binary_cross_entropy_with_logits(yc, t) * scale
    lc.backward()
    xd, wd, bd = x.to(dev).requires_grad_(True), w.to(dev).requires_grad_(train_pred), b.to(dev).requires_grad_(train_pred)
    yd, ld = ops.pred_bce(xd, wd, bd, t.to(dev), up, {})
    (ld * scale).backward()
    close(yd, yc, msg="logits")
    ldv, lcv = float(ld.detach()), float(lc.detach())
    assert abs(ldv * scale - lcv) <= 2e-6 * abs(lcv), (ldv * scale, lcv)
    close(xd.grad, xc.grad, rtol=1e-4, scale_rel=2e-6, msg="dx")
    if train_pred:
        close(wd.grad, wc.grad, rtol=1e-4, scale_rel=1e-5, msg="dW")
        close(bd.grad, bc.grad, rtol=1e-4, scale_rel=1e-5, msg="db")
    assert not yd.requires_grad
    # twice in a row on the same stream: the workspace ticket was reset by the kernel
    y2, l2 = ops.pred_bce(x.to(dev), w.to(dev), b.to(dev), t.to(dev), up, {})
    assert torch.equal(y2, yd) and float(l2.detach()) == float(ld.detach())


@pytest.mark.parametrize("B,cout,H,W,S,device_xy", [(4, 12, 64, 96, 400, False), (3, 12, 128, 128, 300, True), (2, 30, 32, 64, 200, True), (2, 5, 64, 64, 160, False)])
def test_fused_predictor_and_bce_with_the_target_given_by_position(dev, B, cout, H, W, S, device_xy):
    """ynet_pred_bce_blob (round 5): the BCE target of a training step is get_patch(gt_template, gt_future, H, W) (utils/train_epoch.py:68-72) -- per plane
    the 31 x 31 Gaussian blob at the rounded position, zero elsewhere.  The fused predictor + criterion is handed such a tensor, recognises it (same storage,
    size, version as gather_patches left it) and computes the target from the positions instead of reading its planes: logits, loss, dx, dlogits
    bit-identical to the pass over the materialised target.  A target somebody wrote into, or a clone, is read as the tensor it is."""
    ops, iu = pkg("ops"), pkg("utils.image_utils")
    lib = ops._lib()
    tmpl = iu.analytic_gaussian_template(S, 31, 4, True, dev)
    gen = torch.Generator().manual_seed(B + cout)
    xy = torch.rand(B * cout, 2, generator=gen) * torch.tensor([W * 1.0, H * 1.0])
    xy[0] = torch.tensor([0.5, 1.5])                       # blobs cut by the window's corners, round-half-even
    xy[1] = torch.tensor([W - 0.5, H - 1.49])
    xy[2] = torch.tensor([W / 2.0, 0.0])
    if device_xy:
        xy[3] = torch.tensor([W + S * 1.0, 3.0])           # (device-side positions are not checked on the host: the window leaves the template -> an all-zero plane)
    x = rnd(B, 32, H, W, seed=1).relu().to(dev)
    w, b = rnd(cout, 32, 1, 1, seed=2, scale=0.3).to(dev), rnd(cout, seed=3, scale=0.1).to(dev)
    target = ops.gather_patches(tmpl, xy.to(dev) if device_xy else xy, H, W).view(B, cout, H, W)
    if device_xy:
        assert float(target[0, 3].abs().max()) == 0.0 and float(target[0, 2].max()) > 0.5
        with pytest.raises(ValueError, match="left the template"):      # (flagged by the heat-map kernel, raised -- and cleared -- at the next check)
            ops.check_patch_status()
    outs = []
    for how in ("blob", "tensor", "written"):
        t_in = target if how == "blob" else target.clone()
        if how == "written":
            t_in = target
            target[0, 0, 0, 0] += 0.0                          # (an in-place write, whatever it wrote: the version moved -> the planes are read)
        n0 = ops.bce_blob_stats["launches"]
        xd, wd, bd = x.clone().requires_grad_(True), w.clone().requires_grad_(True), b.clone().requires_grad_(True)
        y, loss = ops.pred_bce(xd, wd, bd, t_in, 1000.0, {})
        (loss * 1000.0).backward()
        assert ops.bce_blob_stats["launches"] - n0 == (1 if how == "blob" else 0), how
        outs.append((y, loss.detach().clone(), xd.grad, wd.grad, bd.grad))
    for o in outs[1:]:
        for got, want, name in zip(outs[0], o, ("logits", "loss", "dx", "dW", "db")):
            assert torch.equal(got, want), name
    assert float(outs[0][1]) > 0 and float(outs[0][2].abs().max()) > 0
    # the C ABI's argument checks
    ws = torch.zeros(lib.ynet_pred_bce_workspace_bytes() // 8 + 1, device=dev, dtype=torch.float64)
    yb, lb = torch.empty(B, cout, H, W, device=dev), torch.empty((), device=dev)
    wp = ops.pack_weight(w, 0)
    pos = xy.to(dev)
    assert lib.ynet_pred_bce_blob(x.data_ptr(), 32 * H * W, wp.data_ptr(), b.data_ptr(), pos.data_ptr(), tmpl.blob.data_ptr(), 31, 16, H, W, yb.data_ptr(),
                                  lb.data_ptr(), None, None, ws.data_ptr(), B, 32, cout, 1.0, 0, None) != 0          # template smaller than the window
    assert lib.ynet_pred_bce_blob(x.data_ptr(), 32 * H * W, wp.data_ptr(), b.data_ptr(), pos.data_ptr(), None, 31, S, H, W, yb.data_ptr(),
                                  lb.data_ptr(), None, None, ws.data_ptr(), B, 32, cout, 1.0, 0, None) != 0          # no blob table
    assert lib.ynet_pred_bce_blob(x.data_ptr(), 32 * H * W, wp.data_ptr(), b.data_ptr(), pos.data_ptr(), tmpl.blob.data_ptr(), 31, S, H, W, yb.data_ptr(),
                                  lb.data_ptr(), None, None, ws.data_ptr(), B, 32, cout, 1000.0, 0, None) == 0
    torch.cuda.synchronize()
    assert torch.equal(yb, outs[0][0]) and float(lb) == float(outs[0][1])


def test_scene_padding_and_label_one_hot_known_answers(dev):
    """SURVEY 8(f)-4, the part that needs neither OpenCV nor the segmentation backbone (utils/image_utils.py:74-81, 95-107):
    zero border at the bottom / right up to a multiple of 32, and the one-hot planes of a label map -- padded BEFORE the
    encoding, so the border is class 0.  Known answers written out by hand + the NumPy form of the reference's own lines."""
    ops, iu = pkg("ops"), pkg("utils.image_utils")
    lab = np.array([[0, 1, 2], [3, 4, 5], [5, 5, 0], [1, 1, 1], [2, 0, 2]], dtype=np.uint8)         # 5 x 3
    got = ops.seg_onehot_pad(torch.from_numpy(lab).to(dev), classes=6, division_factor=4).cpu().numpy()
    assert got.shape == (6, 8, 4)
    padded = np.zeros((8, 4), dtype=np.uint8)
    padded[:5, :3] = lab                                             # image_utils.pad: border = 0
    want = np.stack([(padded == v) for v in range(6)], axis=-1).transpose(2, 0, 1).astype("float32")   # image_utils.py:76-80
    assert np.array_equal(got, want)
    assert got[0, 7, 3] == 1.0 and got[1:, 5:, :].sum() == 0 and got[:, :5, :3].sum() == 15          # border is class 0 only
    # through the mirror's own functions (dict in, dict out, in place like the reference)
    images = {"s": lab.copy()}
    iu.pad(images, division_factor=4)
    assert images["s"].shape == (8, 4) and np.array_equal(images["s"], padded)
    iu.preprocess_image_for_segmentation(images, seg_mask=True, classes=6, device=dev)
    assert np.array_equal(images["s"].cpu().numpy(), want)
    # float planes [C, H, W] on the device
    x = rnd(3, 37, 50, seed=1)
    y = ops.pad_planes(x.to(dev), 32).cpu()
    assert y.shape == (3, 64, 64) and torch.equal(y[:, :37, :50], x) and float(y[:, 37:].abs().sum()) == 0 and float(y[:, :, 50:].abs().sum()) == 0
    assert ops.pad_planes(x[:, :32, :32].contiguous().to(dev), 32).shape == (3, 32, 32)             # already a multiple: unchanged
    with pytest.raises(ValueError, match="integer class labels"):
        ops.seg_onehot_pad(torch.rand(4, 4, device=dev), classes=6)


@pytest.mark.parametrize("H,W,f", [(16, 24, 0.25), (10, 6, 0.25), (100, 133, 0.33), (7, 5, 2.0), (50, 50, 0.5), (33, 65, 0.33)])
def test_label_map_nearest_resize_known_answers(dev, H, W, f):
    """resize(images, factor, seg_mask=True) = cv2.resize(im, (0, 0), fx=f, fy=f, interpolation=INTER_NEAREST)
    (utils/image_utils.py:83-87) restated from OpenCV's published rule -- output size cvRound(src * f) (halves to even: 10 * 0.25 ->
    2, 6 * 0.25 -> 2), source index min(floor(dst * (1 / f)), src - 1) with the product in double.  PARITY UNPINNED (cv2 is absent from
    the image, like loralib): known answers written from the rule, not reference outputs."""
    ops, iu = pkg("ops"), pkg("utils.image_utils")
    g = np.random.default_rng(H * 131 + W)
    lab = g.integers(0, 6, size=(H, W)).astype(np.uint8)
    Ho, Wo = int(np.rint(H * f)), int(np.rint(W * f))
    inv = 1.0 / f
    sy = np.minimum(np.floor(np.arange(Ho) * inv).astype(np.int64), H - 1)
    sx = np.minimum(np.floor(np.arange(Wo) * inv).astype(np.int64), W - 1)
    want = lab[sy][:, sx]
    got = ops.resize_nearest(torch.from_numpy(lab).to(dev), f)
    assert got.dtype == torch.uint8 and tuple(got.shape) == (Ho, Wo)
    assert np.array_equal(got.cpu().numpy(), want)
    if f == 0.25:
        assert np.array_equal(want, lab[::4, ::4][:Ho, :Wo])              # every fourth pixel, starting at 0
    if f == 2.0:
        assert np.array_equal(want, np.repeat(np.repeat(lab, 2, axis=0), 2, axis=1))
    images = {"s": lab.copy(), "t": torch.from_numpy(lab.astype(np.int64)).to(dev)}       # dict in, dict out, in place like the reference
    iu.resize(images, f, seg_mask=True)
    assert isinstance(images["s"], np.ndarray) and images["s"].dtype == np.uint8 and np.array_equal(images["s"], want)
    assert images["t"].is_cuda and images["t"].dtype == torch.int64 and np.array_equal(images["t"].cpu().numpy(), want)
    with pytest.raises(ValueError, match="integer class labels"):
        ops.resize_nearest(torch.rand(4, 4, device=dev), 0.5)


@pytest.mark.parametrize("B,P,H,W,rf", [(3, 12, 64, 64, 0.25), (2, 30, 32, 96, 0.33), (5, 1, 16, 16, 1.0)])
def test_train_readout_in_two_launches(dev, B, P, H, W, rf):
    """ynet_train_readout (utils/train_epoch.py:118-126): both soft-argmax calls and the ADE / FDE arithmetic against the
    module-by-module path (SoftArgmax2D + the reference's elementwise chain) and against the fp64 oracle."""
    ops = pkg("ops")
    tm, gm = rnd(B, P, H, W, seed=1, scale=3.0), rnd(B, P, H, W, seed=2, scale=3.0)
    gt = torch.rand(B, P, 2, generator=torch.Generator().manual_seed(3)) * torch.tensor([W * 1.0, H * 1.0])
    pt, pg, ade, fde = ops.train_readout(tm.to(dev), gm.to(dev), gt.to(dev), rf)
    want_t, want_g = ops.softargmax2d(tm.to(dev)), ops.softargmax2d(gm.to(dev)[:, -1:])
    assert torch.equal(pt, want_t) and torch.equal(pg, want_g)          # the same plane code
    gtd = gt.to(dev)
    want_ade = ((((gtd - want_t) / rf) ** 2).sum(dim=2) ** 0.5).mean(dim=1)
    want_fde = ((((gtd[:, -1:] - want_g[:, -1:]) / rf) ** 2).sum(dim=2) ** 0.5).mean(dim=1)
    close(ade, want_ade, rtol=1e-6, atol=1e-5, msg="ADE vs the elementwise chain")
    close(fde, want_fde, rtol=1e-6, atol=1e-5, msg="FDE vs the elementwise chain")
    o_t = O.softargmax2d(tm.double())
    close(pt, o_t.float(), rtol=0, atol=1e-4, msg="coordinates vs fp64")


@pytest.mark.parametrize("S,H,W", [(1050, 256, 256), (1386, 512, 512), (1050, 96, 160), (1386, 37, 50), (75, 16, 24)])
def test_analytic_heatmaps_are_bit_identical_to_template_slices(dev, S, H, W):
    """the windows get_patch slices out of create_dist_mat / create_gaussian_heatmap_template
    (utils/image_utils.py:15-63), computed in the kernel from the coordinate alone (fp64 sqrt / division rounded once to
    fp32; the 31 x 31 blob as a table) -- bit for bit the slices of the float64 NumPy templates cast to fp32."""
    ops, iu = pkg("ops"), pkg("utils.image_utils")
    gen = torch.Generator().manual_seed(S + H)
    xy = torch.rand(40, 2, generator=gen) * torch.tensor([W * 1.0, H * 1.0])
    xy[0] = torch.tensor([0.5, 1.5])                       # round-half-even corners
    xy[1] = torch.tensor([W - 0.5, H - 1.49])
    xy[2] = torch.tensor([2.5, 3.5])
    for kind, tmpl, ana in (
            ("dist", torch.Tensor(iu.create_dist_mat(size=S)), iu.analytic_dist_template(S, dev)),
            ("gauss", torch.Tensor(iu.create_gaussian_heatmap_template(size=S, kernlen=31, nsig=4, normalize=False)),
             iu.analytic_gaussian_template(S, 31, 4, False, dev)),
            ("gauss_norm", torch.Tensor(iu.create_gaussian_heatmap_template(size=S, kernlen=31, nsig=4, normalize=True)),
             iu.analytic_gaussian_template(S, 31, 4, True, dev))):
        want = ops.gather_patches(tmpl.to(dev), xy, H, W)
        got = ops.gather_patches(ana, xy, H, W)
        assert torch.equal(got, want), (kind, float((got - want).abs().max()))
        got_dev = ops.gather_patches(ana, xy.to(dev), H, W)          # device-side coordinates (captured steps)
        assert torch.equal(got_dev, want), kind
        assert torch.equal(ana.materialize().cpu(), tmpl), kind
    with pytest.raises(ValueError, match="leaves"):
        ops.gather_patches(iu.analytic_dist_template(S, dev), torch.tensor([[S * 1.0, 0.0]]), H, W)


@pytest.mark.parametrize("Bs,times,H,W,cx,cf,cw,cout", [(8, 4, 64, 64, 32, 64, 2, 64), (2, 10, 128, 128, 32, 32, 1, 32), (3, 1, 256, 256, 16, 32, 2, 32)])
def test_conv_with_batch_shared_term(dev, Bs, times, H, W, cx, cf, cw, cout):
    """ynet_conv2d_add: relu(conv(cat(x, repeat(feat), wp), W) + b) computed as the per-sample convolution over (x, wp) plus
    a term conv(feat, W[:, cx:cx+cf]) that is evaluated once for the Bs shared images (utils/evaluate.py's K goal samples)."""
    ops = pkg("ops")
    B = Bs * times
    x, feat, wp = rnd(B, cx, H, W, seed=1), rnd(Bs, cf, H, W, seed=2), rnd(B, cw, H, W, seed=3)
    cin = cx + cf + cw
    w, b = rnd(cout, cin, 3, 3, seed=4, scale=1.0 / (cin * 9) ** 0.5), rnd(cout, seed=5, scale=0.1)
    want = F.relu(F.conv2d(torch.cat([x, feat.repeat(times, 1, 1, 1), wp], 1), w, b, padding=1))
    assert ops.conv2d_add_supported(B, H, W, cout, 3)
    cache = {}
    with torch.no_grad():
        term = ops.shared_conv_term(feat.to(dev), w.to(dev), cx, cx + cf, cache)
        got = ops.conv2d_shared_term(None, times, [x.to(dev), wp.to(dev)], w.to(dev), b.to(dev), True, cache, term, cx, cx + cf)
        full = ops.conv2d(ops.lazy_cat([x.to(dev), ops.batch_repeat(feat.to(dev), times), wp.to(dev)]), w.to(dev), b.to(dev), True, {})
    close(got, want, msg="shared-term conv")
    close(got, full, rtol=2e-5, atol=1e-5, msg="vs the full conv on the same device")
    assert not ops.conv2d_add_supported(B, 8, 8, cout, 3)          # small maps keep the plain kernels


# ---- ynet_conv2d_auto: the dispatcher inside the library (round 6) -----------------------------------------------------------------------
AUTO_CASES = {
    # name: (B, H, W, [source channels], [destination channels, None = not wanted], K, relu, bias, operands)
    "plain_32_32": (8, 256, 256, [32], [32], 3, True, True, {}),
    "plain_16_32_no_relu": (16, 128, 128, [16], [32], 3, False, True, {}),
    "dgrad_pieces_32_16_unwanted": (8, 256, 256, [32], [32, 16, None], 3, False, False, {}),
    "dgrad_first_unwanted": (8, 256, 256, [16], [None, 32], 3, False, False, {}),
    "dgrad_relu_of": (8, 256, 256, [32], [32], 3, False, False, {"relu_of": True}),
    "dgrad_relu_wbits": (8, 256, 256, [32], [32], 3, False, False, {"relu_of": True, "relu_wbits": True}),
    "fwd_wbits_out": (8, 256, 256, [32], [32], 3, True, True, {"wbits_out": True}),
    "cat_48": (4, 256, 256, [32, 16], [32], 3, True, True, {}),
    "cat_49_wbits": (4, 256, 256, [32, 16, 1], [32], 3, True, True, {"wbits_out": True}),
    "split_65": (16, 128, 128, [64, 1], [32], 3, True, True, {"wbits_out": True}),
    "pool_code_first_layer": (4, 256, 256, [6, 8], [32], 3, True, True, {"pooled": True, "pool_code": True, "src0_shared": True}),
    "pool_64_slice_form": (10, 64, 64, [64], [64], 3, True, True, {"pooled": True}),
    "slice_64_64": (10, 64, 64, [64], [64], 3, True, True, {}),
    "slice_dgrad_32_64_relu_of": (16, 128, 128, [32], [64], 3, False, False, {"relu_of": True}),
    "slice_cat_97_64": (10, 64, 64, [32, 64, 1], [64], 3, True, True, {}),
    "small_map_workspace": (4, 16, 16, [64], [64], 3, True, True, {}),
    "small_map_dgrad_relu_of": (4, 32, 32, [64], [64], 3, False, False, {"relu_of": True}),
    "predictor_1x1": (4, 64, 64, [32], [12], 1, False, True, {}),
    "direct_bits_out": (8, 32, 32, [64], [64], 3, True, True, {"bits_out": True}),
    "masked_input": (4, 32, 32, [64], [32, 64], 3, False, False, {"mask": True}),
    "dgrad_s2d_16_of_16_32": (8, 256, 256, [32], [16, 32, None], 3, False, False, {"s2d": [1, 0, 0]}),      # (one launch: conv_wino_kernel<3, 4, 6, 4>)
    "dgrad_split_16_32": (8, 256, 256, [32], [16, 32], 3, False, False, {"split": True}),                  # (one launch: conv_wino_kernel<3, 4, 5, 4>)
    "dgrad_s2d_16_alone": (8, 256, 256, [32], [16, None], 3, False, False, {"s2d": [1, 0]}),               # (conv_wino_kernel<1, 4, 4, 8>)
    "dgrad_s2d_asked_of_two_pieces": (8, 256, 256, [32], [48], 3, False, False, {"s2d": [1]}),      # (not one launch: stays row-major)
}


@pytest.mark.parametrize("name", list(AUTO_CASES))
def test_conv2d_auto_takes_the_launches_of_the_python_dispatcher(dev, name):
    """the composition of a layer's launches (kernel family, destination pieces, two-launch forms, filter transforms and
    their cache) moved from ops.conv2d_raw into the library: ynet_conv2d_auto (csrc/conv_auto.cpp).  For every operand combination the
    model produces, the C dispatcher must take exactly the launches the round-5 Python dispatcher took -- same tag, same number of Winograd
    launches, optional outputs written in the same cases -- and give bit-identical results (they ARE the same kernels); a second call with the
    same cache does not transform the filter again, a new filter version does."""
    ops, L = pkg("ops"), pkg("_lib")
    B, H, W, cs, couts, K, relu, with_bias, opts = AUTO_CASES[name]
    lib = ops._lib()
    cin, sizes = sum(cs), [c if c is not None else 16 for c in couts]
    ctot = sum(sizes)
    xs = [rnd(1 if (i == 0 and opts.get("src0_shared")) else B, c, H, W, seed=20 + i).to(dev) for i, c in enumerate(cs)]
    srcs = [(x.data_ptr(), c, 0 if x.shape[0] == 1 and B > 1 else c * H * W) for x, c in zip(xs, cs)]
    dgrad = not with_bias and not relu
    w = rnd(cin, ctot, K, K, seed=2, scale=0.2).to(dev) if dgrad else rnd(ctot, cin, K, K, seed=2, scale=0.2).to(dev)
    wp = ops.pack_weight(w, 1 if dgrad else 0)
    bias = rnd(ctot, seed=3).to(dev) if with_bias else None
    act = torch.relu(rnd(B, ctot, H, W, seed=4)).to(dev) if opts.get("relu_of") else None
    mask_t = torch.relu(rnd(B, cin, H, W, seed=6)).to(dev) if opts.get("mask") else None
    n_words = lib.ynet_winograd_relu_bits_words(B, H, W)
    wb_in = None
    if opts.get("relu_wbits"):      # a mask word tensor as a forward launch leaves it
        wb_in = torch.empty(n_words, device=dev, dtype=torch.int32)
        y_prev = torch.empty(B, 32, H, W, device=dev)
        ops._conv2d_raw_py([(rnd(B, 32, H, W, seed=8).to(dev).data_ptr(), 32, 32 * H * W)], None, ops.pack_weight(rnd(32, 32, 3, 3, seed=9, scale=0.2).to(dev), 0), None,
                           [(y_prev.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, wino=({}, "fwd"), wbits_out=wb_in)
        act = y_prev

    def run(fn, tag_only=False, cache=None, s2d=True):
        outs = [torch.full((B, c, H, W), float("nan"), device=dev) for c in sizes]
        dsts = [(t.data_ptr() if c is not None else None, t.shape[1], t.shape[1] * H * W if c is not None else 0) for t, c in zip(outs, couts)]
        kw = {"wino": (cache if cache is not None else {}, "dgrad" if dgrad else "fwd")}
        extra = {}
        if act is not None:
            kw["relu_of"] = (act.data_ptr(), ctot * H * W)
        if wb_in is not None:
            kw["relu_wbits"] = wb_in
        if opts.get("wbits_out"):
            extra["wbits"] = kw["wbits_out"] = torch.full((n_words,), -1, device=dev, dtype=torch.int32)
        if opts.get("pooled"):
            extra["pooled"] = torch.full((B, ctot, H // 2, W // 2), float("nan"), device=dev)
            kw["pooled"] = (extra["pooled"].data_ptr(), ctot * (H // 2) * (W // 2))
        if opts.get("pool_code"):
            extra["code"] = kw["pool_code"] = torch.full((B, ctot, H // 2, W // 2), 255, device=dev, dtype=torch.uint8)
        if opts.get("bits_out"):
            words = lib.ynet_conv2d_relu_bits_words(B, H, W, ctot, K)
            assert words > 0
            extra["bits"] = torch.full((words,), -1, device=dev, dtype=torch.int32)
            kw["bits_out"] = extra["bits"].data_ptr()
            kw.pop("wino")
        if opts.get("s2d") and s2d:
            kw["dst_s2d"] = opts["s2d"]
        n0 = ops.wino_stats["launches"]
        tag = fn(srcs, (mask_t.data_ptr(), cin * H * W) if mask_t is not None else None, wp, bias, dsts, B, H, W, K, relu, **kw)
        return tag, ops.wino_stats["launches"] - n0, outs, extra

    t_py, n_py, o_py, e_py = run(ops._conv2d_raw_py)
    cache = {}
    t_c, n_c, o_c, e_c = run(lambda *a, **k: ops.conv2d_auto_raw(*a, **k)[0], cache=cache)
    assert t_c == t_py and n_c == n_py, (name, t_c, t_py, n_c, n_py)
    for a_, b_ in zip(o_py, o_c):
        assert torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(b_, nan=12345.0)), name      # (an unwanted destination stays NaN in both)
    assert set(e_py) == set(e_c)
    for k in e_py:
        assert torch.equal(torch.nan_to_num(e_py[k].float(), nan=12345.0), torch.nan_to_num(e_c[k].float(), nan=12345.0)), (name, k)
    if opts.get("s2d"):
        # a destination that asked for it AND is written whole by one plain launch holds its gradient space-to-depth (element (2 i + r, 2 j + c) of channel ch at
        # plane (2 r + c) * C + ch, position (i, j)): the same numbers as the row-major launch, bit for bit; every other destination is row-major as ever
        t_rm, _, o_rm, _ = run(ops._conv2d_raw_py, s2d=False)
        took = any(g.split(",")[2] in ("4", "6") for g in t_c.split(":")[1].split("|")[0].split("+"))
        assert took == (name != "dgrad_s2d_asked_of_two_pieces"), t_c
        assert t_c == {"dgrad_s2d_16_of_16_32": "winograd:3,4,6", "dgrad_s2d_16_alone": "winograd:1,4,4", "dgrad_s2d_asked_of_two_pieces": "winograd:2,4,0+1,4,0"}[name]
        for i, (a_, b_) in enumerate(zip(o_rm, o_c)):
            if couts[i] is None:
                continue
            if took and opts["s2d"][i]:
                C = a_.shape[1]
                a_ = a_.view(B, C, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * C, H // 2, W // 2)
                b_ = b_.view(B, 4 * C, H // 2, W // 2)
            assert torch.equal(a_, b_), (name, i)
    if opts.get("split") or name == "dgrad_s2d_16_of_16_32":
        # [16, 32] channels in ONE launch (three output blocks per wave): the numbers of the two launches it replaces, bit for bit
        assert n_c == 1 and t_c.startswith("winograd:3,4,")
        old = ops._split48_allowed
        ops._split48_allowed = False
        try:
            t_two, n_two, o_two, _ = run(ops._conv2d_raw_py)
            t_two_c, n_two_c, o_two_c, _ = run(lambda *a, **k: ops.conv2d_auto_raw(*a, **k)[0], cache={})
        finally:
            ops._split48_allowed = old
        assert n_two == 2 and n_two_c == 2 and t_two == t_two_c and "+" in t_two, (t_two, t_two_c)
        for a_, b_, c_ in zip(o_two, o_c, o_two_c):
            assert torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(b_, nan=12345.0)) and torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(c_, nan=12345.0)), name
    if t_c is not None:
        # the transformed filter is cached: the second call transforms nothing, a new version does
        kw = {"wino": (cache, "dgrad" if dgrad else "fwd")}
        if act is not None and wb_in is None:
            kw["relu_of"] = (act.data_ptr(), ctot * H * W)
        if opts.get("pooled"):
            kw["pooled"] = (e_c["pooled"].data_ptr(), ctot * (H // 2) * (W // 2))
        if opts.get("s2d"):
            kw["dst_s2d"] = opts["s2d"]
        dsts = [(t.data_ptr() if c is not None else None, t.shape[1], t.shape[1] * H * W if c is not None else 0) for t, c in zip(o_c, couts)]
        if wb_in is None and not opts.get("wbits_out") and not opts.get("pool_code"):
            _, tk = ops.conv2d_auto_raw(srcs, None, wp, bias, dsts, B, H, W, K, relu, **kw)
            assert tk.transformed == 0
            _, tk = ops.conv2d_auto_raw(srcs, None, wp, bias, dsts, B, H, W, K, relu, wp_version=2, **kw)
            assert tk.transformed == 1
            for a_, b_ in zip(o_py, o_c):
                assert torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(b_, nan=12345.0)), name


def test_conv2d_auto_reports_what_no_kernel_serves(dev):
    ops, L = pkg("ops"), pkg("_lib")
    import ctypes
    lib = ops._lib()
    x = rnd(2, 8, 16, 16, seed=1).to(dev)
    wp = ops.pack_weight(rnd(16, 8, 3, 3, seed=2).to(dev), 0)
    y = torch.empty(2, 16, 32, 32, device=dev)
    with pytest.raises(RuntimeError, match="upsample2x"):      # 8 -> 16 at 32^2 is below every up-convolution kernel's range
        ops.conv2d_auto_raw([(x.data_ptr(), 8, 8 * 256)], None, wp, None, [(y.data_ptr(), 16, 16 * 1024)], 2, 32, 32, 3, False, wino=({}, "fwd"), upsample2x=True)
    d = L.ConvAuto()
    assert lib.ynet_conv2d_auto(ctypes.byref(d), None, None) != 0 and b"conv2d_auto" in lib.ynet_last_error()
    assert lib.ynet_conv2d_auto(None, None, None) != 0


def test_a_decoder_level_through_the_c_abi_alone(dev):
    """A reference maintainer who binds include/ynet_hip.h with ctypes -- no ops.py -- reaches the benchmarked kernels: the last level of a decoder
    (models/ynet.py:463-467: bilinear x2 -> upsample_conv[4] (32 -> 16, no ReLU) -> cat with the skip features -> decoder[4] = two conv + ReLU)
    as THREE ynet_conv2d_auto calls on raw device pointers, against torch's fp64 result of the same modules, and at the Python path's speed."""
    import ctypes
    L = pkg("_lib")
    lib = L.load()
    B, H, W = 8, 256, 256
    stream = torch.cuda.current_stream().cuda_stream
    x_low = torch.relu(rnd(B, 32, H // 2, W // 2, seed=1)).to(dev)
    skip = torch.relu(rnd(B, 16, H, W, seed=2)).to(dev)
    ws = [rnd(16, 32, 3, 3, seed=3, scale=0.1).to(dev), rnd(32, 32, 3, 3, seed=4, scale=0.1).to(dev), rnd(32, 32, 3, 3, seed=5, scale=0.1).to(dev)]
    bs = [rnd(16, seed=6).to(dev), rnd(32, seed=7).to(dev), rnd(32, seed=8).to(dev)]

    def packed(w):
        cout, cin, k, _ = w.shape
        wp = torch.zeros(lib.ynet_packed_weight_floats(cout, cin, k, 0), device=dev)
        L.check(lib.ynet_pack_weight(w.data_ptr(), wp.data_ptr(), cout, cin, k, 0, stream), lib)
        return wp

    wps = [packed(w) for w in ws]
    up = torch.empty(B, 16, H, W, device=dev)
    h1, h2 = torch.empty(B, 32, H, W, device=dev), torch.empty(B, 32, H, W, device=dev)
    keep = []

    def call(srcs, wp, bias, dst, cout, relu, upsample2x=0):
        d = L.ConvAuto()
        d.nsrc, d.ndst = len(srcs), 1
        for i, (t, c) in enumerate(srcs):
            d.src[i], d.src_c[i], d.src_bs[i] = t.data_ptr(), c, t.stride(0)
        d.wp, d.bias = wp.data_ptr(), bias.data_ptr()
        d.dst[0], d.dst_c[0], d.dst_bs[0] = dst.data_ptr(), cout, dst.stride(0)
        d.B, d.H, d.W, d.K, d.relu, d.upsample2x = B, H, W, 3, relu, upsample2x
        need = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d))
        assert need > 0
        cache, tag = torch.empty(need, device=dev), (ctypes.c_ulonglong * 2)(0, 0)
        d.cache, d.cache_floats, d.cache_tag, d.wp_version = cache.data_ptr(), need, tag, 1
        keep.append((cache, tag))
        return d

    descs = [call([(x_low, 32)], wps[0], bs[0], up, 16, 0, upsample2x=1), call([(up, 16), (skip, 16)], wps[1], bs[1], h1, 32, 1), call([(h1, 32)], wps[2], bs[2], h2, 32, 1)]
    taken = [L.ConvTaken() for _ in descs]

    def level():
        for d, tk in zip(descs, taken):
            L.check(lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), stream), lib)

    level()
    assert [tk.family for tk in taken] == [4, 2, 1] and [tk.transformed for tk in taken] == [1, 1, 1]
    ref = F.interpolate(x_low.double(), scale_factor=2, mode="bilinear", align_corners=False)
    ref = F.conv2d(ref, ws[0].double(), bs[0].double(), padding=1)
    ref = torch.relu(F.conv2d(torch.cat([ref, skip.double()], 1), ws[1].double(), bs[1].double(), padding=1))
    ref = torch.relu(F.conv2d(ref, ws[2].double(), bs[2].double(), padding=1))
    close(h2, ref, rtol=1e-5, scale_rel=3e-6, msg="decoder level through ynet_conv2d_auto vs torch fp64")
    level()
    assert [tk.transformed for tk in taken] == [0, 0, 0]

    # the same level through the package's Python path (ops.upsample2x_conv2d_raw / conv2d_raw): the same kernels, the same speed
    ops = pkg("ops")
    cache_py = [{}, {}, {}]
    u0 = ops.winograd_filter(wps[0], 32, 16, 0, 16)

    def level_py():
        ops.upsample2x_conv2d_raw((x_low.data_ptr(), x_low.stride(0)), u0, bs[0], (up.data_ptr(), up.stride(0)), 32, 16, B, H, W)
        ops.conv2d_raw([(up.data_ptr(), 16, up.stride(0)), (skip.data_ptr(), 16, skip.stride(0))], None, wps[1], bs[1], [(h1.data_ptr(), 32, h1.stride(0))], B, H, W, 3, True,
                       wino=(cache_py[1], "fwd"))
        ops.conv2d_raw([(h1.data_ptr(), 32, h1.stride(0))], None, wps[2], bs[2], [(h2.data_ptr(), 32, h2.stride(0))], B, H, W, 3, True, wino=(cache_py[2], "fwd"))

    def timed(fn, n=20):
        for _ in range(3):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / n

    h2_c = h2.clone()
    level_py()
    assert torch.equal(h2, h2_c)
    # (interleaved rounds, the minimum of each: the chip's clock drifts by more than the bound between two back-to-back blocks of launches)
    rounds = [(timed(level), timed(level_py)) for _ in range(6)]
    t_c, t_py = min(r[0] for r in rounds), min(r[1] for r in rounds)
    assert abs(t_c - t_py) <= 0.03 * t_py + 0.005, (t_c, t_py, rounds)


@pytest.mark.parametrize("case", [(16, 128, 128, [16, 1], 32, 4, 2), (20, 64, 64, [32, 1], 64, 10, 3), (16, 128, 128, [16, 1], 32, 4, 0)], ids=str)
def test_conv2d_auto_with_an_additive_term(dev, case):
    """ynet_conv2d_auto's `addend` operand (the shared skip term of utils/evaluate.py:248-283: y = relu(conv(cat(rest)) + bias + term[b % modulus])) on its three
    routes -- the concatenated-source Winograd launch, the slice form, the implicit GEMM -- against torch in fp64."""
    ops = pkg("ops")
    B, H, W, cs, cout, mod, family = case
    xs = [rnd(B, c, H, W, seed=30 + i).to(dev) for i, c in enumerate(cs)]
    w, bias = rnd(cout, sum(cs), 3, 3, seed=2, scale=0.2).to(dev), rnd(cout, seed=3).to(dev)
    term = rnd(mod, cout, H, W, seed=4).to(dev)
    y = torch.full((B, cout, H, W), float("nan"), device=dev)
    tag, tk = ops.conv2d_auto_raw([(x.data_ptr(), c, c * H * W) for x, c in zip(xs, cs)], None, ops.pack_weight(w, 0), bias, [(y.data_ptr(), cout, cout * H * W)], B, H, W, 3, True,
                                  wino=({}, "fwd") if family else None, addend=(term.data_ptr(), cout * H * W, mod))
    assert tk.family == family, (tag, tk.family)
    with pytest.raises(RuntimeError, match="additive term is not served"):      # (the implicit GEMM takes an additive term on its large-map tiles only)
        ops.conv2d_auto_raw([(xs[0].data_ptr(), cs[0], cs[0] * 1024)], None, ops.pack_weight(w, 0), bias, [(y.data_ptr(), cout, cout * 1024)], 2, 32, 32, 3, True,
                            addend=(term.data_ptr(), cout * 1024, 1))
    ref = torch.relu(F.conv2d(torch.cat(xs, 1).double(), w.double(), bias.double(), padding=1) + term.double().repeat(B // mod + 1, 1, 1, 1)[:B])
    close(y, ref, rtol=1e-5, scale_rel=3e-6, msg="conv + additive term")


@pytest.mark.parametrize("kind", ["cat_pool_code", "relu_bits", "winograd16_addend", "winograd16_pooled", "up", "up16", "split48_s2d", "conv_pred_bce"])
def test_winograd_epilogue_and_up_paths_beyond_2_and_4_gib(dev, kind):
    """the one-image-per-descriptor addressing of round 5 was only exercised beyond 2 / 4 GiB on the plain, dgrad_relu, cat and cat_add
    paths.  The others -- the pooled copy's descriptor and the code byte index (EPI 3 / 6), the 1-bit mask word index, the slice form's auxiliary
    (addend) and pooled descriptors, both up-convolution kernels (low-resolution source descriptors) -- with batches whose tensors cross 2^31 and
    2^32 bytes: the first image, the images that straddle the two boundaries and the last one against torch (fp64)."""
    ops = pkg("ops")
    lib = ops._lib()
    g = torch.Generator(device=dev).manual_seed(5)

    def picks(bytes_per_image, B):
        return sorted({0, min(B - 1, (1 << 31) // bytes_per_image), min(B - 1, (1 << 32) // bytes_per_image), B - 1})

    if kind == "cat_pool_code":
        B, H, W = 520, 512, 512               # y 17 GB, pooled 4.4 GB (crosses 2^31 and 2^32), code 1.1 GB
        scene, obs = torch.rand(1, 6, H, W, device=dev, generator=g), torch.rand(B, 8, H, W, device=dev, generator=g)
        w, bias = rnd(32, 14, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
        y, pooled = torch.empty(B, 32, H, W, device=dev), torch.full((B, 32, H // 2, W // 2), float("nan"), device=dev)
        code = torch.full((B, 32, H // 2, W // 2), 255, device=dev, dtype=torch.uint8)
        tag = ops.conv2d_raw([(scene.data_ptr(), 6, 0), (obs.data_ptr(), 8, 8 * H * W)], None, ops.pack_weight(w, 0), bias, [(y.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True,
                             pooled=(pooled.data_ptr(), 32 * (H // 2) * (W // 2)), wino=({}, "fwd"), pool_code=code)
        assert tag == "winograd_cat:2,6|code"
        for b in picks(32 * (H // 2) * (W // 2) * 4, B):
            ref = torch.relu(F.conv2d(torch.cat([scene, obs[b:b + 1]], 1).double(), w.double(), bias.double(), padding=1))
            close(y[b:b + 1], ref, rtol=1e-4, scale_rel=2e-6, msg=f"image {b}")
            assert torch.equal(pooled[b:b + 1], F.max_pool2d(y[b:b + 1], 2)), b
            blk = y[b].view(32, H // 2, 2, W // 2, 2).permute(0, 1, 3, 2, 4).reshape(32, H // 2, W // 2, 4)
            eq = blk == blk.max(dim=3, keepdim=True)[0]
            first = ((eq.cumsum(3) == 1) & eq).long().argmax(dim=3)      # the first maximum in scan order (the backward's rule)
            assert torch.equal((code[b] & 3).long(), first) and torch.equal(((code[b] >> 2) & 15).long(), ((blk > 0).long() * torch.tensor([1, 2, 4, 8], device=dev)).sum(3)), b
        return
    if kind == "relu_bits":
        B, H, W = 520, 256, 256               # y 4.4 GB; the mask words of image 519 sit 136 MB into their tensor
        x = torch.randn(B, 32, H, W, device=dev, generator=g).relu_()
        w, bias = rnd(32, 32, 3, 3, seed=2, scale=0.2).to(dev), rnd(32, seed=3).to(dev)
        y = torch.empty(B, 32, H, W, device=dev)
        wbits = torch.full((lib.ynet_winograd_relu_bits_words(B, H, W),), -1, device=dev, dtype=torch.int32)
        assert ops.conv2d_raw([(x.data_ptr(), 32, 32 * H * W)], None, ops.pack_weight(w, 0), bias, [(y.data_ptr(), 32, 32 * H * W)], B, H, W, 3, True, wino=({}, "fwd"),
                              wbits_out=wbits).endswith("|wbits")
        dy, w2 = torch.randn(B, 16, H, W, device=dev, generator=g), rnd(16, 32, 3, 3, seed=6, scale=0.2).to(dev)
        dx = torch.full((B, 32, H, W), float("nan"), device=dev)
        assert ops.conv2d_raw([(dy.data_ptr(), 16, 16 * H * W)], None, ops.pack_weight(w2, 1), None, [(dx.data_ptr(), 32, 32 * H * W)], B, H, W, 3, False,
                              relu_of=(y.data_ptr(), 32 * H * W), wino=({}, "dgrad"), relu_wbits=wbits) == "winograd:2,2,2"
        for b in picks(32 * H * W * 4, B):
            close(y[b:b + 1], torch.relu(F.conv2d(x[b:b + 1].double(), w.double(), bias.double(), padding=1)), rtol=1e-4, scale_rel=2e-6, msg=f"image {b}")
            close(dx[b:b + 1], F.conv_transpose2d(dy[b:b + 1].double(), w2.double(), padding=1) * (y[b:b + 1] > 0), rtol=1e-4, scale_rel=2e-6, msg=f"masked gradient of image {b}")
        return
    if kind == "split48_s2d":
        # round 6: the [16, 32]-channel data gradient in one launch, the 16 channels space-to-depth -- dy 4.4 GB, the two destinations 2.2 and 4.4 GB
        B, H, W = 520, 256, 256
        dy = torch.randn(B, 32, H, W, device=dev, generator=g)
        w = rnd(32, 49, 3, 3, seed=2, scale=0.2).to(dev)          # a forward filter [cout 32][cin 49]: its data gradient maps 32 -> 49 (the 49th not wanted)
        d0, d1 = torch.full((B, 16, H, W), float("nan"), device=dev), torch.full((B, 32, H, W), float("nan"), device=dev)
        info = {}
        tag = ops.conv2d_raw([(dy.data_ptr(), 32, 32 * H * W)], None, ops.pack_weight(w, 1), None, [(d0.data_ptr(), 16, 16 * H * W), (d1.data_ptr(), 32, 32 * H * W), (None, 1, 0)],
                             B, H, W, 3, False, wino=({}, "dgrad"), dst_s2d=[1, 0, 0], info=info)
        assert tag == "winograd:3,4,6" and info["wrote_s2d"] == 1
        for b in picks(32 * H * W * 4, B) + picks(16 * H * W * 4, B):
            ref = F.conv_transpose2d(dy[b:b + 1].double(), w.double(), padding=1)
            got0 = d0[b].view(2, 2, 16, H // 2, W // 2).permute(2, 3, 0, 4, 1).reshape(1, 16, H, W)      # plane (2 r + c) * 16 + ch, position (i, j) -> (2 i + r, 2 j + c)
            close(got0, ref[:, :16], rtol=1e-4, scale_rel=2e-6, msg=f"space-to-depth part of image {b}")
            close(d1[b:b + 1], ref[:, 16:48], rtol=1e-4, scale_rel=2e-6, msg=f"row-major part of image {b}")
        assert not bool(torch.isnan(d0).any()) and not bool(torch.isnan(d1).any())
        return
    if kind == "conv_pred_bce":
        # round 6: the last decoder convolution with the predictor + criterion in its epilogue -- x, dX 4.3 GB each, the logits 1.5 GB; the table of target positions
        # (2 ints per plane in LDS) bounds the batch at 16 outputs to B <= 84, so the images are tall: 512 x 2048
        iu = pkg("utils.image_utils")
        B, H, W, pco, S = 66, 512, 2048, 12, 4200
        assert lib.ynet_conv2d_winograd_pred_bce_supported(B, H, W, 32, 32, pco, 31) == 1
        x = torch.randn(B, 32, H, W, device=dev, generator=g).relu_()
        w3, b3 = rnd(32, 32, 3, 3, seed=2, scale=0.1).to(dev), rnd(32, seed=3, scale=0.1).to(dev)
        w1, b1 = rnd(pco, 32, 1, 1, seed=4, scale=0.3).to(dev), rnd(pco, seed=5, scale=0.1).to(dev)
        tmpl = iu.analytic_gaussian_template(S, 31, 4, True, dev)
        pos = (torch.rand(B * pco, 2, generator=torch.Generator().manual_seed(7)) * torch.tensor([W * 1.0, H * 1.0])).to(dev)
        logits, dx, loss = torch.full((B, pco, H, W), float("nan"), device=dev), torch.full((B, 32, H, W), float("nan"), device=dev), torch.empty((), device=dev)
        ws = torch.zeros(lib.ynet_pred_bce_workspace_bytes() // 8 + 1, device=dev, dtype=torch.float64)
        assert x.numel() * 4 > (1 << 32) and dx.numel() * 4 > (1 << 32)
        ops.conv2d_winograd_pred_bce_raw((x.data_ptr(), 32, 32 * H * W), ops.winograd_filter(ops.pack_weight(w3, 0), 32, 32, 0, 32), b3, ops.pack_weight(w1, 0), b1, pco, pos, tmpl,
                                         logits, loss, dx, ws, B, H, W, 1000.0)
        n = B * pco * H * W
        tot = 0.0
        for b in range(B):
            yb = torch.relu(F.conv2d(x[b:b + 1].double(), w3.double(), b3.double(), padding=1))
            zb = F.conv2d(yb, w1.double(), b1.double())
            tb = ops.gather_patches(tmpl, pos[b * pco:(b + 1) * pco], H, W).view(1, pco, H, W).double()
            tot += float(F.binary_cross_entropy_with_logits(zb, tb, reduction="sum"))
            if b in picks(32 * H * W * 4, B) + picks(pco * H * W * 4, B):
                close(logits[b:b + 1], zb, rtol=1e-4, scale_rel=2e-6, msg=f"logits of image {b}")
                gz = (torch.sigmoid(zb) - tb) * (1000.0 / n)
                gx = F.conv_transpose2d(gz, w1.double()) * (yb > 0)
                bad = ((dx[b:b + 1].double() - gx).abs() > 1e-4 * float(gx.abs().max())).double().mean()
                assert float(bad) <= 1e-3, (b, float(bad))      # (isolated ReLU flips where the pre-activation is within fp32 rounding of zero)
        assert abs(float(loss) - tot / n) <= 2e-6 * tot / n and not bool(torch.isnan(dx).any()) and not bool(torch.isnan(logits).any())
        return
    if kind.startswith("winograd16"):
        B, H, W = 1040, 128, 128              # x, y 4.4 GB each
        x = torch.randn(B, 64, H, W, device=dev, generator=g).relu_()
        w, bias = rnd(64, 64, 3, 3, seed=2, scale=0.1).to(dev), rnd(64, seed=3).to(dev)
        y = torch.full((B, 64, H, W), float("nan"), device=dev)
        src, dst = [(x.data_ptr(), 64, 64 * H * W)], [(y.data_ptr(), 64, 64 * H * W)]
        if kind == "winograd16_addend":
            term = torch.randn(8, 64, H, W, device=dev, generator=g)
            _, tk = ops.conv2d_auto_raw(src, None, ops.pack_weight(w, 0), bias, dst, B, H, W, 3, True, wino=({}, "fwd"), addend=(term.data_ptr(), 64 * H * W, 8))
            assert tk.family == 3
            ref = lambda b: torch.relu(F.conv2d(x[b:b + 1].double(), w.double(), bias.double(), padding=1) + term[b % 8:b % 8 + 1].double())
        else:
            pooled = torch.full((B, 64, H // 2, W // 2), float("nan"), device=dev)
            assert ops.conv2d_raw(src, None, ops.pack_weight(w, 0), bias, dst, B, H, W, 3, True, pooled=(pooled.data_ptr(), 64 * (H // 2) * (W // 2)), wino=({}, "fwd")) == "winograd16:3"
            ref = lambda b: torch.relu(F.conv2d(x[b:b + 1].double(), w.double(), bias.double(), padding=1))
        for b in picks(64 * H * W * 4, B):
            close(y[b:b + 1], ref(b), rtol=1e-4, scale_rel=2e-6, msg=f"image {b}")
            if kind == "winograd16_pooled":
                assert torch.equal(pooled[b:b + 1], F.max_pool2d(y[b:b + 1], 2)), b
        assert not bool(torch.isnan(y).any())
        return
    # the up-convolutions: the LOW-resolution source and the destination both cross the boundaries
    cin, cout, H, W, B = (32, 16, 256, 256, 2100) if kind == "up" else (64, 32, 128, 128, 4200)
    assert lib.ynet_upsample2x_conv2d_winograd_supported(B, H, W, cin, cout, 3) == (1 if kind == "up" else 2)
    xl = torch.randn(B, cin, H // 2, W // 2, device=dev, generator=g).relu_()
    w, bias = rnd(cout, cin, 3, 3, seed=2, scale=0.2).to(dev), rnd(cout, seed=3).to(dev)
    y = torch.full((B, cout, H, W), float("nan"), device=dev)
    assert xl.numel() * 4 > (1 << 32) and y.numel() * 4 > (1 << 32)
    _, tk = ops.conv2d_auto_raw([(xl.data_ptr(), cin, xl.stride(0))], None, ops.pack_weight(w, 0), bias, [(y.data_ptr(), cout, y.stride(0))], B, H, W, 3, False, wino=({}, "fwd"),
                                upsample2x=True)
    assert tk.family == (4 if kind == "up" else 5)
    for b in sorted(set(picks(xl.stride(0) * 4, B) + picks(y.stride(0) * 4, B))):
        ref = F.conv2d(F.interpolate(xl[b:b + 1].double(), scale_factor=2, mode="bilinear", align_corners=False), w.double(), bias.double(), padding=1)
        close(y[b:b + 1], ref, rtol=1e-4, scale_rel=2e-6, msg=f"image {b}")
    assert not bool(torch.isnan(y[-8:]).any()) and not bool(torch.isnan(y[:8]).any())


@pytest.mark.parametrize("case", [(3, 16, 24, 40, True), (32, 8, 64, 64, True), (2, 5, 7, 9, False), (1, 64, 8, 8, True)], ids=str)
def test_batchnorm2d_and_add_relu_match_torch(dev, case):
    """Round 6 (VERDICT r5 missing 3): the serial adapters' nn.BatchNorm2d (models/ynet.py:24,64), the residual add and the ReLU behind the sum
    (ynet.py:66,117-131) as HIP launches: output, running statistics, num_batches_tracked, the three gradients -- training and evaluation mode --
    against torch's own CPU module in fp64 / fp32."""
    ynet, ops = pkg("models.ynet"), pkg("ops")
    B, C, H, W, affine_trains = case
    ref = torch.nn.BatchNorm2d(C)
    with torch.no_grad():
        ref.weight.copy_(rnd(C, seed=1) * 0.5 + 1.0)
        ref.bias.copy_(rnd(C, seed=2))
        ref.running_mean.copy_(rnd(C, seed=3) * 0.1)
        ref.running_var.copy_(rnd(C, seed=4).abs() + 0.5)
    mine = ynet.HipBatchNorm2d(C)
    mine.load_state_dict(ref.state_dict())
    mine.to(dev)
    assert list(mine.state_dict()) == list(ref.state_dict())
    for step, training in enumerate((True, True, False)):
        ref.train(training)
        mine.train(training)
        x = rnd(B, C, H, W, seed=10 + step) * 2 + 0.3
        gy = rnd(B, C, H, W, seed=20 + step)
        xr = x.clone().double().requires_grad_(True)
        refd = torch.nn.BatchNorm2d(C).double()
        refd.load_state_dict({k: (v.double() if v.is_floating_point() else v) for k, v in ref.state_dict().items()})
        refd.train(training)
        yr = refd(xr)
        yr.backward(gy.double())
        ref(x)                                                     # (advances the fp32 module's running statistics)
        xm = x.to(dev).requires_grad_(True)
        ym = mine(xm)
        ym.backward(gy.to(dev))
        close(ym, yr, rtol=1e-5, atol=2e-5, msg=f"y (training={training})")
        close(xm.grad, xr.grad, rtol=1e-4, scale_rel=2e-6, msg="dx")
        close(mine.weight.grad, refd.weight.grad, rtol=1e-4, scale_rel=5e-6, msg="dgamma")
        close(mine.bias.grad, refd.bias.grad, rtol=1e-4, scale_rel=5e-6, msg="dbeta")
        close(mine.running_mean, refd.running_mean, rtol=1e-6, atol=1e-6, msg="running_mean")
        close(mine.running_var, refd.running_var, rtol=1e-6, atol=1e-6, msg="running_var")
        assert int(mine.num_batches_tracked) == int(refd.num_batches_tracked)
        mine.zero_grad()
    # the residual add with and without the ReLU behind it
    a, b = rnd(B, C, H, W, seed=30), rnd(B, C, H, W, seed=31)
    for relu in (False, True):
        ad, bd = a.to(dev).requires_grad_(True), b.to(dev).requires_grad_(True)
        y = ops.add_relu(ad, bd, relu)
        want = torch.relu(a + b) if relu else a + b
        assert torch.equal(y.cpu(), want)
        g = rnd(B, C, H, W, seed=32)
        y.backward(g.to(dev))
        wg = g * (want > 0) if relu else g
        assert torch.equal(ad.grad.cpu(), wg) and torch.equal(bd.grad.cpu(), wg)
    nan = torch.tensor([float("nan"), -1.0, 2.0], device=dev).view(1, 3, 1, 1)
    out = ops.add_relu(nan, torch.zeros_like(nan), True)
    assert bool(torch.isnan(out[0, 0, 0, 0])) and float(out[0, 1, 0, 0]) == 0.0 and float(out[0, 2, 0, 0]) == 2.0


@pytest.mark.parametrize("B,Hl,Wl,wmap", [(8, 128, 128, True), (4, 128, 128, False), (6, 64, 160, True)], ids=str)
def test_up_convolution_backward_without_the_up_sampled_gradient(dev, B, Hl, Wl, wmap):
    """Round 6: the backward of `upsample_conv[4](F.interpolate(x, scale_factor=2))` (models/ynet.py:463-464) as a 3 x 3 convolution at the LOW
    resolution over the space-to-depth output gradient (effective filter per bilinear phase) + a correction on the outermost ring -- the up-sampled gradient
    [B, 32, 2 Hl, 2 Wl] is never written and the bilinear backward launch disappears.  A decoder's last level (conv -> ReLU below, up-convolution, cat with the skip
    features [and a way-point map], conv + ReLU above) inside fold_skip_gradients(): the gradient of the level's input with the hand-over on and off, and against
    torch's autograd in fp64; the hand-over is taken (the producer's 16-channel piece written space-to-depth), and only then."""
    ynet, ops = pkg("models.ynet"), pkg("ops")
    H, W = 2 * Hl, 2 * Wl
    below, up = ynet.HipConv2d(32, 32, 3).to(dev), ynet.HipConv2d(32, 16, 3).to(dev)
    top = ynet.FusedSequential(ynet.HipConv2d(49 if wmap else 48, 32, 3), torch.nn.ReLU(), ynet.HipConv2d(32, 32, 3), torch.nn.ReLU()).to(dev)      # decoder[4]
    for m in (below, up, top):
        for p_ in m.parameters():
            p_.requires_grad_(False)
    x0 = rnd(B, 32, Hl, Wl, seed=1).to(dev)
    skip = torch.relu(rnd(B, 32, H, W, seed=2)).to(dev)
    wm = torch.rand(B, 1, H, W, generator=torch.Generator().manual_seed(3)).to(dev) if wmap else None
    g = rnd(B, 32, H, W, seed=4).to(dev)

    def run(s2d):
        old = ops._upconv_s2d_allowed
        ops._upconv_s2d_allowed = s2d
        try:
            xi, sk = x0.clone().requires_grad_(True), skip.clone().requires_grad_(True)
            n0 = ops.upconv_stats_s2d["backwards"]
            with ops.fold_skip_gradients():
                h0 = below(xi, relu=True)                                   # a post-ReLU activation feeds the up-convolution, as in the decoder
                u_ = ops.upsample2x_conv2d(h0, up)
                y = top(ops.lazy_cat([u_, sk] + ([wm] if wmap else [])))
                (y * g).sum().backward()
            return y.detach(), xi.grad, sk.grad, ops.upconv_stats_s2d["backwards"] - n0
        finally:
            ops._upconv_s2d_allowed = old

    y1, gx1, gs1, n1 = run(True)
    y0, gx0, gs0, n0 = run(False)
    assert n1 == 1 and n0 == 0, (n1, n0)
    assert torch.equal(y1, y0) and torch.equal(gs1, gs0)                     # the forward pass and the skip features' gradient do not change
    xr, sr = x0.double().cpu().requires_grad_(True), skip.double().cpu().requires_grad_(True)
    dd = lambda m: (m.weight.detach().double().cpu(), m.bias.detach().double().cpu())      # noqa: E731
    h0 = torch.relu(F.conv2d(xr, *dd(below), padding=1))
    u_ = F.conv2d(F.interpolate(h0, scale_factor=2, mode="bilinear", align_corners=False), *dd(up), padding=1)
    yr = torch.relu(F.conv2d(torch.cat([u_, sr] + ([wm.double().cpu()] if wmap else []), 1), *dd(top[0]), padding=1))
    yr = torch.relu(F.conv2d(yr, *dd(top[2]), padding=1))
    (yr * g.double().cpu()).sum().backward()
    # the two device paths share every ReLU mask (the forward pass is bit-identical): they agree to fp32 rounding EVERYWHERE, the outermost ring included
    close(gx1, gx0, rtol=1e-4, scale_rel=5e-6, msg="low-resolution form vs up-sampled form")
    for sl in ((slice(None), slice(None), 0), (slice(None), slice(None), -1), (slice(None), slice(None), slice(None), 0), (slice(None), slice(None), slice(None), -1)):
        close(gx1[sl], gx0[sl], rtol=1e-4, scale_rel=5e-6, msg="ring")
    # against torch in fp64: a few pre-activations round to opposite sides of zero on the host and on the device, each flips the 9 x 32 gradients it gates --
    # all but a few per mille of the entries within rounding (the same entries on both device paths), and the low-resolution form no further from fp64 than the up-sampled one
    want = xr.grad
    tol = 5e-6 * float(want.abs().max()) + 1e-4 * want.abs()
    bad1, bad0 = (gx1.double().cpu() - want).abs() > tol, (gx0.double().cpu() - want).abs() > tol
    assert float(bad1.double().mean()) <= 5e-3 and int(bad1.sum()) <= int(bad0.sum()) + 16, (int(bad1.sum()), int(bad0.sum()))
    ok = ~(bad1 | bad0)
    e1, e0 = float((gx1.double().cpu() - want)[ok].abs().max()), float((gx0.double().cpu() - want)[ok].abs().max())
    assert e1 <= 2.0 * e0 + 1e-7 * float(want.abs().max()), (e1, e0)


def test_a_second_consumer_of_an_up_convolution_output_is_refused(dev):
    """The space-to-depth hand-over is between ONE producer and the up-convolution's backward.  If the up-convolution's output feeds two operations, autograd sums
    their gradients into a tensor the protocol never saw -- one of them in the other layout.  That must fail loudly, not return numbers."""
    ynet, ops = pkg("models.ynet"), pkg("ops")
    B, Hl, Wl = 4, 128, 128
    H, W = 2 * Hl, 2 * Wl
    below, up, other = ynet.HipConv2d(32, 32, 3).to(dev), ynet.HipConv2d(32, 16, 3).to(dev), ynet.HipConv2d(16, 16, 3).to(dev)
    top = ynet.FusedSequential(ynet.HipConv2d(48, 32, 3), torch.nn.ReLU(), ynet.HipConv2d(32, 32, 3), torch.nn.ReLU()).to(dev)
    for m in (below, up, other, top):
        for p_ in m.parameters():
            p_.requires_grad_(False)
    xi = rnd(B, 32, Hl, Wl, seed=1).to(dev).requires_grad_(True)
    skip = torch.relu(rnd(B, 32, H, W, seed=2)).to(dev)
    if not ops._upconv_s2d_allowed:
        pytest.skip("YNET_UPCONV_S2D=0")
    with pytest.raises(RuntimeError, match="second consumer"):
        with ops.fold_skip_gradients():
            u_ = ops.upsample2x_conv2d(below(xi, relu=True), up)
            loss = top(ops.lazy_cat([u_, skip])).sum() + other(u_).sum()
            loss.backward()
    assert not ops._s2d_produced and not ops._s2d_grads and not ops._s2d_wanted      # (the registries do not outlive the context)
    # ... and the same graph with the hand-over off is served as ever
    old = ops._upconv_s2d_allowed
    ops._upconv_s2d_allowed = False
    try:
        xi.grad = None
        with ops.fold_skip_gradients():
            u_ = ops.upsample2x_conv2d(below(xi, relu=True), up)
            (top(ops.lazy_cat([u_, skip])).sum() + other(u_).sum()).backward()
        assert torch.isfinite(xi.grad).all() and float(xi.grad.abs().max()) > 0
    finally:
        ops._upconv_s2d_allowed = old


@pytest.mark.parametrize("B,cin,cout,h,w", [(2, 3, 2, 5, 7), (1, 32, 16, 2, 2), (3, 8, 4, 16, 70), (2, 20, 16, 130, 9), (2, 32, 16, 64, 64)], ids=str)
def test_upconv_dgrad_ring_and_the_effective_filter_at_any_shape(dev, B, cin, cout, h, w):
    """ynet_upconv_dgrad_ring through the C ABI, away from the shapes the decoders use (odd sizes, a 2 x 2 map where every pixel is a corner, border lines longer
    and shorter than a 64-pixel segment, channel counts that are no multiple of 16): [data gradient of the effective filter over the space-to-depth gradient] +
    [ring] must be the gradient torch's fp64 autograd gives for conv2d(F.interpolate(x, scale_factor=2, mode='bilinear'), K) -- with and without a ReLU gate."""
    import torch.nn.functional as F
    ops = pkg("ops")
    lib = ops._lib()
    K = rnd(cout, cin, 3, 3, seed=1, scale=0.3)
    x = rnd(B, cin, h, w, seed=2).double().requires_grad_(True)
    dy = rnd(B, cout, 2 * h, 2 * w, seed=3)
    y = F.conv2d(F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False), K.double(), padding=1)
    (want,) = torch.autograd.grad(y, x, dy.double())
    D = dy.view(B, cout, h, 2, w, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * cout, h, w).contiguous().to(dev)      # plane (2 r + c) * cout + ch
    wp_eff, tables, _ = ops.upconv_s2d_tables(K.to(dev), {})
    assert tuple(tables.shape) == (16, 4 * cout, cin)
    gate = torch.relu(rnd(B, cin, h, w, seed=4)).to(dev)
    for masked in (False, True):
        dx = torch.full((B, cin, h, w), float("nan"), device=dev)
        fused_gate = masked and (cin * h * w) % 4 == 0      # (the convolution's ReLU-gated epilogue wants 16-byte aligned images; the ring kernel does not care)
        ops.conv2d_raw([(D.data_ptr(), 4 * cout, 4 * cout * h * w)], None, wp_eff, None, [(dx.data_ptr(), cin, cin * h * w)], B, h, w, 3, False,
                       relu_of=(gate.data_ptr(), cin * h * w) if fused_gate else None)
        if masked and not fused_gate:
            dx.mul_(gate > 0)
        pkg("_lib").check(lib.ynet_upconv_dgrad_ring(D.data_ptr(), 4 * cout * h * w, tables.data_ptr(), gate.data_ptr() if masked else None, cin * h * w,
                                                     dx.data_ptr(), cin * h * w, B, 4 * cout, cin, h, w, None), lib)
        ref = want * (gate.cpu() > 0) if masked else want
        err = (dx.double().cpu() - ref).abs()
        scale = float(want.abs().max())
        assert float(err.max()) <= 2e-5 * scale, (masked, float(err.max()), scale, [int(v) for v in torch.nonzero(err == err.max())[0]])
    # the interior alone (no ring) is NOT the gradient: the correction is doing something on every border line
    inner = torch.empty((B, cin, h, w), device=dev)
    ops.conv2d_raw([(D.data_ptr(), 4 * cout, 4 * cout * h * w)], None, wp_eff, None, [(inner.data_ptr(), cin, cin * h * w)], B, h, w, 3, False)
    diff = (inner.double().cpu() - want).abs()
    assert float(diff[:, :, 0, :].max()) > 1e-3 * scale and float(diff[:, :, :, -1].max()) > 1e-3 * scale
    if h > 2 and w > 2:
        assert float(diff[:, :, 1:-1, 1:-1].max()) <= 2e-5 * scale
    with pytest.raises(RuntimeError, match="upconv_dgrad_ring"):
        pkg("_lib").check(lib.ynet_upconv_dgrad_ring(D.data_ptr(), 4 * cout * h * w, tables.data_ptr(), None, 0, dx.data_ptr(), cin * h * w, B, 4 * cout + 2, cin, h, w, None), lib)


@pytest.mark.parametrize("B,cout,H,W,S", [(8, 12, 128, 128, 400), (13, 12, 64, 160, 400), (8, 5, 128, 128, 300), (2, 16, 256, 256, 600), (8, 30, 128, 128, 400), (2, 17, 256, 256, 600)], ids=str)
def test_last_decoder_convolution_inside_the_predictor_and_criterion(dev, B, cout, H, W, S):
    """Round 6: decoder[4][2] + ReLU, the 1 x 1 predictor, BCEWithLogitsLoss and the predictor's data gradient as ONE launch (ynet_conv2d_winograd_pred_bce_blob;
    models/ynet.py:467,469, utils/train_epoch.py:93-94) -- the 32 activation planes between the convolution and the predictor are never written.  Against the two
    launches it replaces (same kernels' arithmetic for the convolution; the predictor's products run on the matrix cores instead of an FMA chain: fp32 rounding
    differences only) and against torch autograd in fp64: logits, loss, the gradient of the level's input."""
    import torch.nn.functional as F
    ynet, ops, iu = pkg("models.ynet"), pkg("ops"), pkg("utils.image_utils")
    below = ynet.HipConv2d(32, 32, 3).to(dev)
    last = ynet.FusedSequential(ynet.HipConv2d(32, 32, 3), torch.nn.ReLU(), ynet.HipConv2d(32, 32, 3), torch.nn.ReLU()).to(dev)
    pred = ynet.HipConv2d(32, cout, 1).to(dev)
    for m in (below, last, pred):
        for p_ in m.parameters():
            p_.requires_grad_(False)
    tmpl = iu.analytic_gaussian_template(S, 31, 4, True, dev)
    gen = torch.Generator().manual_seed(B + cout)
    xy = torch.rand(B * cout, 2, generator=gen) * torch.tensor([W * 1.0, H * 1.0])
    xy[0] = torch.tensor([0.5, 1.5])
    xy[1] = torch.tensor([W - 0.5, H - 1.49])
    x0 = rnd(B, 32, H, W, seed=1).to(dev)
    scale = 1000.0
    expected = scale

    def run(fused):
        old = ops._conv_pred_bce_allowed
        ops._conv_pred_bce_allowed = fused
        try:
            xi = x0.clone().requires_grad_(True)
            n0, m0 = ops.conv_pred_bce_stats["fused"], ops.premask_stats["unmasked_backwards"]
            with ops.fold_skip_gradients():
                target = ops.gather_patches(tmpl, xy.to(dev), H, W).view(B, cout, H, W)
                h = last(below(xi, relu=True), defer_last=True)
                y, loss = ops.pred_bce(h, pred.weight, pred.bias, target, expected, pred._packed)
                (loss * scale).backward()
            return y.detach(), loss.detach().clone(), xi.grad, ops.conv_pred_bce_stats["fused"] - n0
        finally:
            ops._conv_pred_bce_allowed = old

    y1, l1, g1, n1 = run(True)
    y0, l0, g0, n0 = run(False)
    assert (n1, n0) == (1, 0)
    # fp64 autograd of the same graph
    xd = x0.double().cpu().requires_grad_(True)
    c = lambda m_, t: F.conv2d(t, m_.weight.double().cpu(), m_.bias.double().cpu(), padding=m_.kernel_size[0] // 2)
    hd = torch.relu(c(last[2], torch.relu(c(last[0], torch.relu(c(below, xd))))))
    zd = c(pred, hd)
    td = ops.gather_patches(tmpl, xy.to(dev), H, W).view(B, cout, H, W).double().cpu()
    ld = F.binary_cross_entropy_with_logits(zd, td)
    (ld * scale).backward()
    zs, gs = float(zd.detach().abs().max()), float(xd.grad.abs().max())
    e1, e0 = float((y1.double().cpu() - zd.detach()).abs().max()), float((y0.double().cpu() - zd.detach()).abs().max())
    assert e1 <= 2.0 * e0 + 1e-6 * zs, (e1, e0, zs)
    ld = ld.detach()
    assert abs(float(l1) - float(ld)) <= 2e-6 * abs(float(ld)) and abs(float(l1) - float(l0)) <= 2e-6 * abs(float(l0)), (float(l1), float(l0), float(ld))
    # the gradient: a ReLU whose pre-activation is within rounding of zero may flip between the two device paths -- isolated elements; everything else to fp32 rounding
    d1, d0 = (g1.double().cpu() - xd.grad).abs(), (g0.double().cpu() - xd.grad).abs()
    tol = 2e-4 * gs
    f1, f0 = float((d1 > tol).double().mean()), float((d0 > tol).double().mean())
    assert f1 <= max(5e-4, 1.25 * f0) and f0 <= 2e-3, (f1, f0)      # (the fused launch has no more of them than the two launches it replaces)
    assert float((g1 - g0).abs().median()) <= 1e-6 * gs and float(((g1 - g0).abs() > tol).double().mean()) <= 5e-4
    # a target that is not the blob form (a clone: no positions behind it) cannot take the fused launch: pred_bce launches the deferred convolution itself, then runs as ever
    with ops.fold_skip_gradients():
        xi = x0.clone().requires_grad_(True)
        target = ops.gather_patches(tmpl, xy.to(dev), H, W).view(B, cout, H, W).clone()
        f0, m0 = ops.conv_pred_bce_stats["fused"], ops.conv_pred_bce_stats["materialized"]
        h = last(below(xi, relu=True), defer_last=True)
        y2, loss2 = ops.pred_bce(h, pred.weight, pred.bias, target, expected, pred._packed)
        (loss2 * scale).backward()
        assert (ops.conv_pred_bce_stats["fused"] - f0, ops.conv_pred_bce_stats["materialized"] - m0) == (0, 1)
    assert torch.equal(y2.detach(), y0) and float(loss2) == float(l0) and torch.equal(xi.grad, g0)
    # a consumer that is not the fused criterion gets the tensor itself: the deferred convolution is launched for it
    with ops.fold_skip_gradients():
        xi = x0.clone().requires_grad_(True)
        h = last(below(xi, relu=True), defer_last=True)
        m0 = ops.conv_pred_bce_stats["materialized"]
        hm = ops.materialize_deferred(h)
        assert hm is h and ops.conv_pred_bce_stats["materialized"] == m0 + 1
        ref = last(below(x0, relu=True))
        assert torch.equal(h.detach(), ref.detach())

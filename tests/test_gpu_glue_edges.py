"""The read-out and element-wise kernels of csrc/glue.hip at their edges: every walk, loop and alignment fallback that the dispatchers
of that file can select, against a plain fp64 reference computed on the CPU (stock torch on .double() inputs, oracle.ynet_oracle) --
never against a second call into the code under test.  The inputs, the references and the reasons for each case are in
tests/_glue_cases.py; tests/test_glue_cases_host.py checks that table without a GPU.

Bit-exact operators (max-pool, pad, add, ReLU, the routed gradients) are compared with torch.equal; the others keep the bounds of
tests/test_gpu_kernels.py for the same kernel.  Soft-argmax: e_got <= max(2 e_ref, 2e-5), e_ref the fp32 oracle's own error on the same
input, without the floor for planes wider or taller than 256.  BatchNorm: twice the error of torch's fp32 CPU kernels, per channel."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _glue_cases as G
from conftest import pkg

pytestmark = pytest.mark.gpu


def _ops():
    ops = pkg("ops")
    return ops, ops._lib(), pkg("_lib")


def close(got, want, rtol, atol, msg=""):
    """|got - want| <= atol + rtol |want| in fp64, on the device that holds `got` (atol may be a tensor)."""
    g = got.detach().double()
    w = want.detach().double().to(g.device)
    a = atol.to(g.device) if torch.is_tensor(atol) else atol
    assert g.shape == w.shape, (msg, g.shape, w.shape)
    err = (g - w).abs()
    bad = ~(err <= a + rtol * w.abs())
    assert not bool(bad.any()), f"{msg}: max err {float(torch.nan_to_num(err, nan=float('inf')).max()):.3e}, {int(bad.sum())} bad of {bad.numel()}"


def same(got, want, msg=""):
    """Bit-exact up to the sign of zero; NaNs must sit in the same places."""
    got, want = got.detach().cpu(), want.detach().cpu()
    assert got.shape == want.shape, (msg, got.shape, want.shape)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), f"{msg}: NaN mask differs"
    assert torch.equal(torch.nan_to_num(got, nan=0.0), torch.nan_to_num(want, nan=0.0)), \
        f"{msg}: {int((torch.nan_to_num(got, nan=0.0) != torch.nan_to_num(want, nan=0.0)).sum())} elements differ of {got.numel()}"


def dview(t, off, dev):
    """A device copy of `t` that starts `off` floats (4 `off` bytes) into a 256-byte aligned buffer."""
    buf = torch.full((t.numel() + 8,), float("nan"), device=dev, dtype=t.dtype)
    v = buf[off:off + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 256 == 4 * off
    return v


def nan_out(shape, off, dev):
    return dview(torch.full(shape, float("nan")), off, dev)


# ------------------------------------------------------------------------------------------------
# 1. soft-argmax
# ------------------------------------------------------------------------------------------------
SOFT_IDS = ["{}x{}".format(*s) for s, _, _ in G.SOFT_SHAPES]


def _soft_bound(x, H, W):
    e_ref = G.soft_e_ref(x)
    return (2 * e_ref if (H > 256 or W > 256) else max(2 * e_ref, 2e-5)), e_ref


@pytest.mark.parametrize("shape", [s for s, _, _ in G.SOFT_SHAPES], ids=SOFT_IDS)
def test_softargmax_known_answers(dev, shape):
    """One logit of +60 over zeros at the corners, at the last vector of row 0, the first vector of row 1 and the last element: the row and
    column bookkeeping of the walk, independent of any random comparison.  The answer is the fp64 reference's (eps included); the device
    result is one fp32 rounding of an exact sum, so it is allowed one ulp (2^-23 relative, of 1 px at least)."""
    ops, _, _ = _ops()
    H, W = shape
    x, pos = G.soft_known(H, W)
    ref = G.soft_ref(x)
    got = ops.softargmax2d(x.to(dev)).cpu().double()
    tm = x.expand(2, -1, -1, -1).contiguous()
    pt, pg, _, _ = ops.train_readout(tm.to(dev), tm.to(dev), torch.zeros(2, x.shape[1], 2, device=dev), 1.0)
    atol = 2.0 ** -23 * ref.abs().clamp_min(1.0)
    print(f"known {H}x{W}: max |got - ref| = {float((got - ref).abs().max()):.3e} px over {x.shape[1]} positions")
    close(got, ref, 0.0, atol, "softargmax2d, planted maximum")
    close(pt.cpu(), ref.expand(2, -1, -1), 0.0, atol.expand(2, -1, -1), "train_readout trajectories, planted maximum")
    close(pg.cpu(), ref[:, -1:].expand(2, -1, -1), 0.0, atol[:, -1:].expand(2, -1, -1), "train_readout goal, planted maximum")


@pytest.mark.parametrize("kind", G.SOFT_KINDS)
@pytest.mark.parametrize("shape", [s for s, _, _ in G.SOFT_SHAPES], ids=SOFT_IDS)
def test_softargmax_and_readout_shape_sweep(dev, shape, kind):
    """ops.softargmax2d and ops.train_readout (coordinates, ADE, FDE) against the fp64 oracle on every walk of softargmax_plane.
    ADE / FDE: the norm moves by at most sqrt(2) times the coordinate bound, divided by the resize factor, plus the P + 8 fp32 roundings of
    the reference's own elementwise chain."""
    ops, _, _ = _ops()
    H, W = shape
    x = G.soft_logits(H, W, kind)
    gm = G.soft_logits(H, W, G.SOFT_KINDS[(G.SOFT_KINDS.index(kind) + 1) % 4])
    B, P = x.shape[:2]
    gt = G.uniform(B, P, 2, key=110) * torch.tensor([float(W), float(H)])
    rf = 0.25
    bound, e_ref = _soft_bound(x, H, W)
    bound_g, _ = _soft_bound(gm[:, -1:], H, W)
    truth = G.soft_ref(x)
    got = ops.softargmax2d(x.to(dev)).cpu().double()
    e_got = float((got - truth).abs().max())
    print(f"softargmax {H}x{W} {kind}: e_got {e_got:.3e} e_ref {e_ref:.3e} bound {bound:.3e}")
    assert e_got <= bound, (shape, kind, e_got, e_ref)
    pt, pg, ade, fde = ops.train_readout(x.to(dev), gm.to(dev), gt.to(dev), rf)
    wt, wg, wade, wfde = G.readout_ref(x, gm, gt, rf)
    e_t, e_g = float((pt.cpu().double() - wt).abs().max()), float((pg.cpu().double() - wg).abs().max())
    print(f"train_readout {H}x{W} {kind}: e_traj {e_t:.3e} (bound {bound:.3e}) e_goal {e_g:.3e} (bound {bound_g:.3e})")
    assert e_t <= bound and e_g <= bound_g, (shape, kind, e_t, e_g)
    close(ade.cpu(), wade, (P + 8) * 2.0 ** -24, 2.0 ** 0.5 * bound / rf, "ADE")
    close(fde.cpu(), wfde, (1 + 8) * 2.0 ** -24, 2.0 ** 0.5 * bound_g / rf, "FDE")


@pytest.mark.parametrize("shape", [(5, 4), (96, 160), (8, 1028), (17, 23)], ids=str)
def test_softargmax_views(dev, shape):
    """A channel slice and a batch-strided view go to the kernel without a copy; a view that starts 4 bytes into its buffer forces the
    .contiguous() branch of ops.softargmax2d (16-byte loads) -- all three against the fp64 oracle of the same values."""
    ops, _, _ = _ops()
    H, W = shape
    x = G.soft_logits(H, W, "scale8")
    B, C = x.shape[:2]
    wide = torch.full((B, C + 2, H, W), float("nan"), device=dev)
    wide[:, :C] = x.to(dev)
    views = {"channel slice": (x.to(dev)[:, 1:], x[:, 1:]), "batch-strided": (wide[:, :C], x), "misaligned": (dview(x, 1, dev), x)}
    for name, (v, src) in views.items():
        bound, e_ref = _soft_bound(src, H, W)
        if name != "misaligned":
            t, c, bs = ops._plane_desc(v, "softargmax")
            assert t.data_ptr() == v.data_ptr() and (name != "batch-strided" or bs == (C + 2) * H * W)          # no copy
        else:
            assert v.data_ptr() % 16 == 4
        e_got = float((ops.softargmax2d(v).cpu().double() - G.soft_ref(src)).abs().max())
        print(f"softargmax view {H}x{W} {name}: e_got {e_got:.3e} e_ref {e_ref:.3e}")
        assert e_got <= bound, (shape, name, e_got, e_ref)
    # the training read-out takes the same misaligned maps
    mis = views["misaligned"][0]
    pt, pg, _, _ = ops.train_readout(mis, mis, torch.zeros(B, C, 2, device=dev), 1.0)
    bound, _ = _soft_bound(x, H, W)
    assert float((pt.cpu().double() - G.soft_ref(x)).abs().max()) <= bound and float((pg.cpu().double() - G.soft_ref(x[:, -1:])).abs().max()) <= bound


# ------------------------------------------------------------------------------------------------
# 2. max-pool family: bit-exact against F.max_pool2d and its autograd on the CPU
# ------------------------------------------------------------------------------------------------
def _pool_fwd_bwd(dev, x, dy):
    ops, lib, L = _ops()
    N, H, W = x.shape
    xd, dyd = x.to(dev), dy.to(dev)
    y = torch.full((N, H // 2, W // 2), float("nan"), device=dev)
    dx = torch.full((N, H, W), float("nan"), device=dev)
    L.check(lib.ynet_maxpool2_fwd(xd.data_ptr(), y.data_ptr(), N, H, W, ops._stream()), lib)
    L.check(lib.ynet_maxpool2_bwd(xd.data_ptr(), dyd.data_ptr(), dx.data_ptr(), N, H, W, ops._stream()), lib)
    torch.cuda.synchronize()
    return y, dx


def _pool_all(dev, x, key):
    ops, lib, L = _ops()
    N, H, W = x.shape
    dy = G.randn(N, H // 2, W // 2, key=key)
    a0, a1 = G.randn(N, H, W, key=key + 1), G.randn(N, H, W, key=key + 2)
    wy, wdx, arg = G.pool_ref(x, dy)
    y, dx = _pool_fwd_bwd(dev, x, dy)
    same(y, wy, "forward")
    nn = ~torch.isnan(wy)
    assert torch.equal(torch.signbit(y.cpu()[nn]), torch.signbit(wy[nn])), "forward: sign of a zero maximum"
    same(dx, wdx, "plain backward")
    xd, dyd, a0d, a1d = x.to(dev), dy.to(dev), a0.to(dev), a1.to(dev)
    code = G.pool_code(x, arg).to(dev)
    for relu in (0, 1):
        for nadd in (0, 1, 2):
            adds = (a0, a1)[:nadd]
            p0, p1 = (a0d.data_ptr() if nadd > 0 else None), (a1d.data_ptr() if nadd > 1 else None)
            _, want, _ = G.pool_ref(x, dy, adds, bool(relu))
            got = torch.full((N, H, W), float("nan"), device=dev)
            L.check(lib.ynet_maxpool2_bwd_add(xd.data_ptr(), dyd.data_ptr(), p0, p1, got.data_ptr(), N, H, W, relu, ops._stream()), lib)
            same(got, want, f"bwd_add relu_mask={relu} addends={nadd}")
            got2 = torch.full((N, H, W), float("nan"), device=dev)
            L.check(lib.ynet_maxpool2_bwd_add_code(code.data_ptr(), dyd.data_ptr(), p0, p1, got2.data_ptr(), N, H, W, relu, ops._stream()), lib)
            same(got2, want, f"bwd_add_code relu_mask={relu} addends={nadd}")


@pytest.mark.parametrize("case", G.POOL_EVEN, ids=str)
def test_maxpool_family_even_shapes(dev, case):
    """Forward, plain backward, ynet_maxpool2_bwd_add (both mask settings, 0 / 1 / 2 addends) and ynet_maxpool2_bwd_add_code (the code bytes
    built on the host from the rule in include/ynet_hip.h): 70,000 planes make the kernels loop n += gridDim.y."""
    _pool_all(dev, G.pool_planes(*case), key=210)


@pytest.mark.parametrize("case", G.POOL_ODD, ids=str)
def test_maxpool_plain_backward_odd_shapes(dev, case):
    x = G.pool_planes(*case)
    N, H, W = x.shape
    dy = G.randn(N, H // 2, W // 2, key=220)
    wy, wdx, _ = G.pool_ref(x, dy)
    y, dx = _pool_fwd_bwd(dev, x, dy)
    same(y, wy, "forward")
    same(dx, wdx, "plain backward (the trailing row / column is zeroed)")


def test_maxpool_family_planted_ties(dev):
    """Equal values, +0 against -0, all -inf, one NaN, all NaN: the arg-max follows torch's (first in scan order, a NaN wins) and the
    gradient lands on that element only; NaN cases are compared on the NaN mask and on the values after nan_to_num."""
    _pool_all(dev, G.pool_tie_planes(), key=230)


# ------------------------------------------------------------------------------------------------
# 3. average-pool pyramid
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("planes", G.PYR_PLANES, ids=lambda p: f"{p[0] * p[1]}planes")
@pytest.mark.parametrize("shape", G.PYR_SHAPES, ids=lambda s: "{}x{}".format(*s))
def test_avgpool_pyramid_levels(dev, shape, planes):
    """n_levels 1..6 (the launch takes n_levels - 1 levels: below 5 the kernel returns between its barriers) against
    F.avg_pool2d(x.double(), 2**i)."""
    ops, _, _ = _ops()
    (B, C), (H, W) = planes, shape
    x = G.randn(B, C, H, W, key=310)
    want = [w.to(dev) for w in G.pyramid_ref(x, 6)[1:]]
    xd = x.to(dev)
    for n_levels in range(1, 7):
        got = ops.avgpool_pyramid(xd, n_levels)
        assert len(got) == n_levels and got[0].data_ptr() == xd.data_ptr()
        for i in range(1, n_levels):
            close(got[i], want[i - 1], 1e-6, 1e-6, f"{n_levels} levels, level {i}")


def test_avgpool_pyramid_refusals_write_nothing(dev):
    """The C ABI serves 1..5 pooled levels of maps whose sides are multiples of 32: 0 levels, 6 levels and a 48 x 64 map return non-zero
    and leave the outputs alone.  (5 is the largest served count -- it is what ops.avgpool_pyramid(x, 6) passes.)"""
    ops, lib, L = _ops()
    for nlev, H, W in ((0, 64, 64), (6, 64, 64), (3, 48, 64)):
        x = torch.ones(2, H, W, device=dev)
        outs = [torch.full((2, max(H >> i, 1), max(W >> i, 1)), float("nan"), device=dev) for i in range(1, 7)]
        ptrs = (ctypes.c_void_p * 6)(*[o.data_ptr() for o in outs])
        rc = lib.ynet_avgpool_pyramid(x.data_ptr(), ctypes.cast(ptrs, L.PP), nlev, 2, H, W, ops._stream())
        torch.cuda.synchronize()
        assert rc != 0 and lib.ynet_last_error(), (nlev, H, W)
        assert all(bool(torch.isnan(o).all()) for o in outs), (nlev, H, W)


@pytest.mark.parametrize("case", G.PYR_BWD, ids=str)
def test_avgpool_pyramid_backward(dev, case):
    """ynet_avgpool_pyramid_bwd against fp64 autograd through the same avg_pool2d chain: six levels with and without a gradient for level 0,
    and three levels."""
    ops, lib, L = _ops()
    B, C, H, W = case
    grads = [G.randn(B, C, H >> l, W >> l, key=320 + l) for l in range(6)]
    gd = [g.to(dev) for g in grads]
    for nlev, with0 in ((6, True), (6, False), (3, False), (1, True)):
        use = [g if (l > 0 or with0) else None for l, g in enumerate(grads[:nlev])]
        want = G.pyramid_bwd_ref((B, C, H, W), use)
        ptrs = (ctypes.c_void_p * nlev)(*[(gd[l].data_ptr() if use[l] is not None else None) for l in range(nlev)])
        dx = torch.full((B, C, H, W), float("nan"), device=dev)
        L.check(lib.ynet_avgpool_pyramid_bwd(ctypes.cast(ptrs, L.PP), nlev, dx.data_ptr(), B * C, H, W, ops._stream()), lib)
        close(dx, want, 1e-6, 1e-6, f"pyramid backward, {nlev} levels, level 0 {'given' if with0 else 'null'}")


# ------------------------------------------------------------------------------------------------
# 4. the remaining element-wise entries
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SIG_CASES, ids=lambda c: "B{}C{}_{}x{}_n{}_T{}".format(c[0], c[1], c[2], c[3], len(c[4]), c[5]))
def test_sigmoid_temp_cases(dev, case):
    ops, _, _ = _ops()
    B, C, H, W, sel, T = case
    x = G.sig_input(B, C, H, W)
    got = ops.sigmoid_temp(x.to(dev), sel, T)
    close(got, G.sig_ref(x, sel, T), G.SIG_RTOL, G.SIG_ATOL, "sigmoid_temp")


@pytest.mark.parametrize("case", G.BSUM_CASES, ids=str)
def test_batch_sum_cases(dev, case):
    ops, lib, L = _ops()
    B, n, stride = case
    buf = G.bsum_input(B, n, stride)
    ref, bound = G.bsum_ref(buf, n)
    bd = buf.to(dev)
    y = torch.full((n,), float("nan"), device=dev)
    L.check(lib.ynet_batch_sum(bd.data_ptr(), y.data_ptr(), B, n, stride, ops._stream()), lib)
    err = (y.double() - ref.to(dev)).abs()
    print(f"batch_sum {case}: max err {float(err.max()):.3e}, max bound {float(bound.max()):.3e}")
    assert bool((err <= bound.to(dev)).all())
    if B == 1:
        assert torch.equal(y.cpu(), buf[0, :n])


def test_batch_sum_refusals(dev):
    ops, lib, _ = _ops()
    x = torch.ones(2, 16, device=dev)
    y = torch.full((16,), float("nan"), device=dev)
    assert lib.ynet_batch_sum(x.data_ptr() + 4, y.data_ptr(), 2, 8, 8, ops._stream()) != 0          # a pointer 4 bytes off
    assert lib.ynet_batch_sum(x.data_ptr(), y.data_ptr() + 8, 2, 8, 8, ops._stream()) != 0
    assert lib.ynet_batch_sum(x.data_ptr(), y.data_ptr(), 2, 6, 8, ops._stream()) != 0              # n % 4 != 0
    assert lib.ynet_batch_sum(x.data_ptr(), y.data_ptr(), 2, 8, 10, ops._stream()) != 0             # stride % 4 != 0
    torch.cuda.synchronize()
    assert bool(torch.isnan(y).all())


@pytest.mark.parametrize("case", G.PAD_CASES, ids=str)
def test_pad_planes_cases(dev, case):
    ops, _, _ = _ops()
    N, H, W, d = case
    x = G.randn(N, H, W, key=510)
    Hp, Wp = -(-H // d) * d, -(-W // d) * d
    want = F.pad(x.double(), (0, Wp - W, 0, Hp - H)).float()
    same(ops.pad_planes(x.to(dev), d), want, "pad_planes")


@pytest.mark.parametrize("n", G.ELEM_N)
def test_add_relu_and_relu_backward_cases(dev, n):
    ops, lib, L = _ops()
    a, b, dy, yv = G.elem_inputs(n)
    ad, bd, dyd, yd = a.to(dev), b.to(dev), dy.to(dev), yv.to(dev)
    for relu in (0, 1):
        out = torch.full((n,), float("nan"), device=dev)
        L.check(lib.ynet_add_relu(ad.data_ptr(), bd.data_ptr(), out.data_ptr(), n, relu, ops._stream()), lib)
        same(out, G.add_relu_ref(a, b, bool(relu)), f"add_relu relu={relu}")
    dx = torch.full((n,), float("nan"), device=dev)
    L.check(lib.ynet_relu_bwd(dyd.data_ptr(), yd.data_ptr(), dx.data_ptr(), n, ops._stream()), lib)
    same(dx, G.relu_bwd_ref(dy, yv), "relu_bwd")


@pytest.mark.parametrize("target", G.BCE_TARGETS)
@pytest.mark.parametrize("n", G.BCE_N)
def test_bce_with_logits_cases(dev, n, target):
    """Loss and gradient against fp64 torch: lengths below one 16-byte vector, every n % 4, more elements than YNET_BCE_PARTS * 256 * 4,
    targets exactly 0 and 1, logits over +-40; the gradient written by the forward pass, the no-gradient launch, the recomputing
    backward, and (largest n) the expected-gradient / rescale path."""
    ops, _, _ = _ops()
    x, t = G.bce_inputs(n, target)
    loss, dx = G.bce_ref(x, t)
    xd = x.to(dev).requires_grad_(True)
    ld = ops.bce_with_logits(xd, t.to(dev))
    ld.backward(retain_graph=True)
    print(f"bce n={n} {target}: loss {float(ld.detach()):.9g} (fp64 {float(loss):.9g})")
    close(ld, loss, G.BCE_LOSS_RTOL, 0.0, "loss")
    close(xd.grad, dx, G.BCE_GRAD_RTOL, G.bce_grad_atol(n), "dlogits (forward pass)")
    xd.grad = None
    ld.backward()                                       # second backward: recomputed from the saved logits (ynet_bce_logits_bwd)
    close(xd.grad, dx, G.BCE_GRAD_RTOL, G.bce_grad_atol(n), "dlogits (recomputed)")
    with torch.no_grad():
        close(ops.bce_with_logits(x.to(dev), t.to(dev)), loss, G.BCE_LOSS_RTOL, 0.0, "loss, no-grad launch")
    if n == max(G.BCE_N):
        scale = 1000.0
        _, dxs = G.bce_ref(x, t, scale)
        for expected in (1000.0, 3.0):
            xe = x.to(dev).requires_grad_(True)
            le = ops.bce_with_logits(xe, t.to(dev), expected)
            (le * scale).backward()
            close(le, loss, G.BCE_LOSS_RTOL, 0.0, f"loss (expected_grad {expected})")
            # (the rescale multiplies by fl(g / expected): two more fp32 roundings on the gradient)
            close(xe.grad, dxs, G.BCE_GRAD_RTOL, G.bce_grad_atol(n, scale), f"dlogits (expected_grad {expected})")


def _up_call(dev, shape, fwd_off, bwd_off, x, gy, act):
    ops, lib, L = _ops()
    B, C, H, W = shape
    xo, yo = fwd_off
    xv, y = dview(x, xo, dev), nan_out((B, C, 2 * H, 2 * W), yo, dev)
    L.check(lib.ynet_upsample2x_fwd(xv.data_ptr(), y.data_ptr(), B * C, H, W, ops._stream()), lib)
    go, do, ao = bwd_off
    gv, av = dview(gy, go, dev), dview(act, ao, dev)
    dx, dxr = nan_out(shape, do, dev), nan_out(shape, do, dev)
    L.check(lib.ynet_upsample2x_bwd(gv.data_ptr(), dx.data_ptr(), B * C, H, W, ops._stream()), lib)
    L.check(lib.ynet_upsample2x_bwd_relu(gv.data_ptr(), dxr.data_ptr(), av.data_ptr(), B * C, H, W, ops._stream()), lib)
    torch.cuda.synchronize()
    return y, dx, dxr


@pytest.mark.parametrize("shape", G.UP_SHAPES, ids=str)
def test_upsample2x_alignment_fallbacks(dev, shape):
    """x / y / dy / dx / the activation handed over 0, 4 and 8 bytes into a larger buffer: every branch of the dispatchers that is chosen by
    pointer alignment (4-row, 2-row, quad and scalar kernels) against F.interpolate in fp64 and its autograd."""
    B, C, H, W = shape
    x, gy = G.randn(*shape, key=610), G.randn(B, C, 2 * H, 2 * W, key=611)
    act = torch.relu(G.randn(*shape, key=612))
    wy, wdx, wdxr = G.up_ref(x, gy, act)
    n = max(len(G.UP_FWD_OFFSETS), len(G.UP_BWD_OFFSETS))
    for k in range(n):
        fo, bo = G.UP_FWD_OFFSETS[k % len(G.UP_FWD_OFFSETS)], G.UP_BWD_OFFSETS[k % len(G.UP_BWD_OFFSETS)]
        y, dx, dxr = _up_call(dev, shape, fo, bo, x, gy, act)
        close(y, wy, 1e-6, 1e-6, f"forward, (x, y) offsets {fo}")
        close(dx, wdx, 1e-5, 1e-5, f"backward, (dy, dx, act) offsets {bo}")
        close(dxr, wdxr, 1e-5, 1e-5, f"backward + ReLU, (dy, dx, act) offsets {bo}")


def test_upsample2x_plane_loop(dev):
    """70,000 planes of 2 x 2: more planes than gridDim.y may hold, the kernels loop n += gridDim.y."""
    shape = G.UP_MANY
    B, C, H, W = shape
    x, gy = G.randn(*shape, key=620), G.randn(B, C, 2 * H, 2 * W, key=621)
    act = torch.relu(G.randn(*shape, key=622))
    wy, wdx, wdxr = G.up_ref(x, gy, act)
    y, dx, dxr = _up_call(dev, shape, (0, 0), (0, 0, 0), x, gy, act)
    close(y, wy, 1e-6, 1e-6, "forward")
    close(dx, wdx, 1e-5, 1e-5, "backward")
    close(dxr, wdxr, 1e-5, 1e-5, "backward + ReLU")


@pytest.mark.parametrize("case", G.BN_CASES, ids=str)
def test_batchnorm_training_with_large_offsets(dev, case):
    """Per-channel mean in {0, 1e2, 1e4} next to std in {1, 1e-2}: save_mean, save_invstd, y and dx against the two-pass fp64 reference.
    The kernel forms the variance as E[x^2] - m^2 in fp64; it is allowed twice the error of torch's own fp32 CPU kernels on the same input,
    per channel and per tensor."""
    ops, lib, L = _ops()
    B, C, H, W = case
    x, gamma, beta, gy = G.bn_inputs(B, C, H, W)
    r64 = G.bn_ref(x, gamma, beta, gy)
    e_torch = G.bn_channel_err(G.bn_ref(x, gamma, beta, gy, torch.float32), r64)
    xd, gd, bd, gyd = x.to(dev), gamma.to(dev), beta.to(dev), gy.to(dev)
    y, dx = torch.full_like(xd, float("nan")), torch.full_like(xd, float("nan"))
    mean, invstd = torch.empty(C, device=dev), torch.empty(C, device=dev)
    dg, db = torch.empty(C, device=dev), torch.empty(C, device=dev)
    ws = torch.empty(lib.ynet_batchnorm_workspace_doubles(C), device=dev, dtype=torch.float64)
    L.check(lib.ynet_batchnorm2d_fwd(xd.data_ptr(), y.data_ptr(), gd.data_ptr(), bd.data_ptr(), None, None, mean.data_ptr(), invstd.data_ptr(),
                                     ws.data_ptr(), B, C, H * W, 1, 0.1, G.BN_EPS, ops._stream()), lib)
    L.check(lib.ynet_batchnorm2d_bwd(gyd.data_ptr(), xd.data_ptr(), mean.data_ptr(), invstd.data_ptr(), gd.data_ptr(), dx.data_ptr(), dg.data_ptr(),
                                     db.data_ptr(), ws.data_ptr(), B, C, H * W, 1, ops._stream()), lib)
    e_got = G.bn_channel_err({"save_mean": mean, "save_invstd": invstd, "y": y, "dx": dx}, r64)
    for k in G.BN_TENSORS:
        print(f"batchnorm {case} {k}: kernel {['%.2e' % v for v in e_got[k].tolist()]} torch fp32 {['%.2e' % v for v in e_torch[k].tolist()]}")
    for k in G.BN_TENSORS:
        assert bool((e_got[k] <= 2 * e_torch[k]).all()), (k, e_got[k].tolist(), e_torch[k].tolist())

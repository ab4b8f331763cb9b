"""The adapter kernels (csrc/lora.hip, csrc/lora_wgrad.hip) against the fp64 restatements of tests/_lora_cases.py at every dispatch edge.

Exact cases (integer-grid inputs, every partial sum below 2^24: tests/test_lora_cases_host.py) must equal the fp64 rule BIT FOR BIT -- a dropped or doubled term
cannot hide in a tolerance; gauss cases stay within the project's tolerances against fp64.  ynet_lora_conv2d_wgrad is run at every instantiation of
lora_wgrad_kernel (generic 4-row with 2 and 5 column blocks per wave, generic 2-row, the specialised ones at ragged maps), on more tiles than resident workgroups,
on expanded and channel-sliced sources, with the shared scratch poisoned with NaN before every call, and beside the two-call chain (ynet_conv2d_wgrad ->
ynet_lora_grad), a second device path to the same integers.  The packed layouts are written into sentinel-filled buffers: every float outside pack_rule's map
keeps the sentinel.

The largest error / tolerance of the gauss cases per family is printed at the end of the module (pytest -s).  Measured on the MI355X: compose (and both
packed layouts) 0.057, lora_grad 0.053, lora_conv2d_wgrad 0.042; the 168 cases take 8 s."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _lora_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

SENTINEL = -7.5
_worst = {}


@pytest.fixture(scope="module", autouse=True)
def _report():
    yield
    print("\nlora edges, worst gauss error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(_worst.items())))


def _check(got, want, kind, family, name, what):
    """exact: the fp64 rule, which is representable in fp32, bit for bit; gauss: within the family's tolerance of it."""
    got = got.detach().cpu()
    assert got.shape == want.shape, (what, got.shape, want.shape)
    if kind == "exact":
        w32 = want.float()
        assert torch.equal(w32.double(), want)
        assert torch.equal(got, w32), f"{family} {name} {what}: {int((got != w32).sum())} of {got.numel()} entries differ from the exact rule, largest by {float(torch.nan_to_num((got.double() - want).abs(), nan=float('inf')).max())}"
        return
    bad, ratio = C.mismatch(got, want, **C.tol(family, name))
    _worst[family] = max(_worst.get(family, 0.0), ratio)
    assert bad == 0, f"{family} {name} {what}: {bad} of {got.numel()} entries outside the tolerance, worst error / tolerance {ratio:.3f}"


def _gemm_id(v):
    return f"{'x'.join(map(str, v[0]))}-{v[1]}"


# ------------------------------------------------------------------------------------------------
# ops.lora_compose
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", C.GEMM_VARIANTS, ids=map(_gemm_id, C.GEMM_VARIANTS))
def test_lora_compose_against_the_rule(dev, shape, kind):
    ops = pkg("ops")
    c = C.gemm_case(shape, kind)
    cout, cin, k, r = shape
    w, a, b = c.w.to(dev), c.a.to(dev), c.b.to(dev)
    got = ops.lora_compose(w, a, b, c.s)
    _check(got, c.w_eff, kind, "compose", shape, "w_eff")
    # lora_B = 0 (the adapter at its initialisation): the base weight, bit for bit
    assert torch.equal(ops.lora_compose(w, a, torch.zeros_like(b), c.s), w)
    # a NaN in A[q][n] reaches column n of the flat [cout k][cin k] product -- every row of it (0 * NaN is NaN) -- and nothing else
    q, n = (r * k) // 2, (cin * k) - 1 - (cin * k) // 3
    a_nan = a.clone()
    a_nan[q, n] = float("nan")
    planted = ops.lora_compose(w, a_nan, b, c.s).view(cout * k, cin * k)
    hit = torch.zeros(cout * k, cin * k, dtype=torch.bool, device=dev)
    hit[:, n] = True
    assert torch.equal(torch.isnan(planted), hit)
    assert torch.equal(planted[~hit], got.view(cout * k, cin * k)[~hit])


# ------------------------------------------------------------------------------------------------
# ops.lora_compose_pack
# ------------------------------------------------------------------------------------------------
def _packed_want(w_eff, cout, cin, k, lib):
    out = []
    for mode in (0, 1):
        n = lib.ynet_packed_weight_floats(cout, cin, k, mode)
        assert n == C.packed_floats(cout, cin, k, mode)
        out.append(C.pack_rule(w_eff, mode, n))
    return out


def _check_packed(buf, values, written, kind, name, what, rest):
    """The written positions against the rule; every other float bitwise equal to `rest`."""
    buf = buf.detach().cpu()
    _check(buf[written], values[written], kind, "compose", name, what)
    other = buf[~written]
    assert torch.equal(other.view(torch.int32), torch.full_like(other, rest).view(torch.int32)), f"{name} {what}: {int((other != rest).sum())} padding floats were written"


@pytest.mark.parametrize("shape,kind", C.GEMM_VARIANTS, ids=map(_gemm_id, C.GEMM_VARIANTS))
def test_lora_compose_pack_writes_the_rule_and_nothing_else(dev, shape, kind):
    ops = pkg("ops")
    lib = ops._lib()
    c = C.gemm_case(shape, kind)
    cout, cin, k, r = shape
    w, a, b = c.w.to(dev), c.a.to(dev), c.b.to(dev)
    want = _packed_want(c.w_eff, cout, cin, k, lib)
    # into sentinel-filled buffers: the padding is the caller's, the kernel leaves it alone
    bufs = tuple(torch.full((v.numel(),), SENTINEL, device=dev) for v, _ in want)
    ret = ops.lora_compose_pack(w, a, b, c.s, bufs)
    assert ret[0] is bufs[0] and ret[1] is bufs[1]
    for buf, (values, written), what in zip(bufs, want, ("fwd", "dgrad")):
        _check_packed(buf, values, written, kind, shape, what, SENTINEL)
    # into the zeroed buffers the wrapper makes: the whole buffer is the rule
    fresh = ops.lora_compose_pack(w, a, b, c.s)
    for buf, (values, written), what in zip(fresh, want, ("fwd", "dgrad")):
        assert buf.numel() == values.numel()
        _check_packed(buf, values, written, kind, shape, what + " (zeroed)", 0.0)
    # a changed adapter into the same buffers: same storage, new values, padding still zero
    a2 = torch.roll(c.a, 1, 1).neg()
    ptrs = [t.data_ptr() for t in fresh]
    again = ops.lora_compose_pack(w, a2.to(dev), b, c.s, fresh)
    assert [t.data_ptr() for t in again] == ptrs
    want2 = _packed_want(C.compose_rule(c.w, a2, c.b, c.s), cout, cin, k, lib)
    for buf, (values, written), what in zip(again, want2, ("fwd", "dgrad")):
        _check_packed(buf, values, written, kind, shape, what + " (second call)", 0.0)


# ------------------------------------------------------------------------------------------------
# ops.refresh_filters: 50 layers, two launches of ynet_lora_compose_pack_multi
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["exact", "gauss"])
def test_refresh_filters_across_the_48_layer_limit(dev, kind):
    ops, ynet = pkg("ops"), pkg("models.ynet")
    lib = ops._lib()
    layers = C.refresh_layers()
    assert len(layers) > ops.MULTI_PACK_MAX
    net = torch.nn.ModuleList()
    scales = []
    with torch.no_grad():
        for i, (cin, cout, K, r) in enumerate(layers):
            m = ynet.LoRAConv2d(cin, cout, K, r=r) if (r or i % 2) else ynet.HipConv2d(cin, cout, K, bias=bool(i % 4))
            w, a, b = C.refresh_values(i, layers[i], kind)
            m.weight.copy_(w)
            s = 0.0
            if r:
                m.lora_A.copy_(a)
                m.lora_B.copy_(b)
                if kind == "exact":
                    m.scaling = C.SCALES[i % 3]
                s = float(np.float32(m.scaling))      # (the scale crosses the C ABI as a float)
            scales.append(s)
            net.append(m)
    net.to(dev)
    ops.refresh_filters(net)
    for i, (m, (cin, cout, K, r)) in enumerate(zip(net, layers)):
        w, a, b = C.refresh_values(i, layers[i], kind)
        w_eff = C.compose_rule(w, a, b, scales[i]) if r else w.double()
        for (values, written), what in zip(_packed_want(w_eff, cout, cin, K, lib), ("fwd", "dgrad")):
            _check_packed(m._packed[what], values, written, kind, f"layer {i} {layers[i]}", what, 0.0)
    # nothing is left to do; a changed layer in each of the two launches' ranges is packed again into the same storage
    ptrs = [(m._packed["fwd"].data_ptr(), m._packed["dgrad"].data_ptr()) for m in net]
    with torch.no_grad():
        net[7].lora_A.neg_()
        net[49].weight.neg_()
    ops.refresh_filters(net)
    assert [(m._packed["fwd"].data_ptr(), m._packed["dgrad"].data_ptr()) for m in net] == ptrs
    for i in (7, 49, 8):
        cin, cout, K, r = layers[i]
        w, a, b = C.refresh_values(i, layers[i], kind)
        if i == 7:
            a = -a
        if i == 49:
            w = -w
        w_eff = C.compose_rule(w, a, b, scales[i]) if r else w.double()
        for (values, written), what in zip(_packed_want(w_eff, cout, cin, K, lib), ("fwd", "dgrad")):
            _check_packed(net[i]._packed[what], values, written, kind, f"layer {i} (again)", what, 0.0)


# ------------------------------------------------------------------------------------------------
# ops.lora_grad
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,kind", C.GEMM_VARIANTS, ids=map(_gemm_id, C.GEMM_VARIANTS))
def test_lora_grad_against_the_rule(dev, shape, kind):
    ops = pkg("ops")
    c = C.gemm_case(shape, kind)
    d_a, d_b = ops.lora_grad(c.dw.to(dev), c.a.to(dev), c.b.to(dev), c.s)
    _check(d_a, c.da, kind, "grad", shape, "dA")
    _check(d_b, c.db, kind, "grad", shape, "dB")


@pytest.mark.parametrize("shape,kind", C.GEMM_VARIANTS, ids=map(_gemm_id, C.GEMM_VARIANTS))
def test_lora_grad_with_operands_that_are_views(dev, shape, kind):
    """lora_A as the transposed view of a contiguous [cin k, r k] tensor, dW as the channel slice wide[:, :cin] of a [cout, cin + 3, k, k] tensor (the slack
    holds NaN): the gradients, read through their own strides, are the rule's.  Before ops.lora_grad made its operands contiguous the kernel wrote row-major
    into an output that had kept lora_A's strides and read dW as if it were dense: on the MI355X 16 of these 18 cases failed (all but 1 x 1 x 1 x 1, whose views
    are dense) -- e.g. 64 x 64 x 3 x 5 gauss with 2880 of 2880 entries of dA and 2880 of 2880 of dB outside the tolerance; with lora_A alone a view, 2878 of dA."""
    ops = pkg("ops")
    c = C.gemm_case(shape, kind)
    cout, cin, k, r = shape
    a_view = c.a.t().contiguous().to(dev).t()
    b_view = c.b.t().contiguous().to(dev).t()
    wide = torch.full((cout, cin + 3, k, k), float("nan"), device=dev)
    wide[:, :cin] = c.dw.to(dev)
    dw_view = wide[:, :cin]
    assert tuple(a_view.shape) == (r * k, cin * k) and a_view.stride() == (1, r * k) and dw_view.stride(0) == (cin + 3) * k * k
    d_a, d_b = ops.lora_grad(dw_view, a_view, b_view, c.s)
    assert tuple(d_a.shape) == tuple(c.da.shape) and tuple(d_b.shape) == tuple(c.db.shape)
    _check(d_a, c.da, kind, "grad", shape, "dA (views)")
    _check(d_b, c.db, kind, "grad", shape, "dB (views)")
    assert bool(torch.isnan(wide[:, cin:]).all())


# ------------------------------------------------------------------------------------------------
# ops.lora_conv2d_wgrad_raw
# ------------------------------------------------------------------------------------------------
def _device_sources(c, dev):
    """The case's sources on the device, as the views WGRAD_VIEWS asks for; -> (sources, buffers to keep alive and to find unchanged)."""
    B = c.shape[0]
    xs, keep = [], []
    for i, x in enumerate(c.xs):
        if c.view.get("expand") == i:
            base = x.to(dev)
            v = base.expand(B, -1, -1, -1)
            assert v.stride(0) == 0
        elif c.view.get("slice", (None,))[0] == i:
            _, c0, c_big = c.view["slice"]
            base = torch.full((B, c_big, *x.shape[2:]), float("nan"), device=dev)
            base[:, c0:c0 + x.shape[1]] = x.to(dev)
            v = base[:, c0:c0 + x.shape[1]]
            assert v.data_ptr() % 16 == 0 and v.stride(0) == c_big * x.shape[2] * x.shape[3] != x[0].numel()
        else:
            base = v = x.to(dev)
        xs.append(v)
        keep.append((base, base.clone()))
    return xs, keep


@pytest.fixture(scope="module")
def scratch(dev):
    """The shared scratch of ops.lora_conv2d_wgrad_raw at its largest (a 64 -> 64 call), so that every later call of this module reuses that buffer."""
    ops = pkg("ops")
    x, g = torch.zeros(1, 64, 2, 4, device=dev), torch.zeros(1, 64, 2, 4, device=dev)
    ops.lora_conv2d_wgrad_raw([x], g, None, torch.zeros(64, 64, 3, 3, device=dev), torch.zeros(3, 192, device=dev), torch.zeros(192, 3, device=dev), 1.0)
    key = (g.device, torch.cuda.current_stream().cuda_stream)
    ws = ops._lora_wg_ws[key]
    assert ws.numel() >= ops._lib().ynet_lora_conv2d_wgrad_workspace_floats(64, 64)
    return lambda: ops._lora_wg_ws[key]


def _wgrad_id(v):
    return f"{v[0]}-{v[1]}-{'mask' if v[2] else 'nomask'}"


@pytest.mark.parametrize("name,kind,with_mask", C.WGRAD_VARIANTS, ids=map(_wgrad_id, C.WGRAD_VARIANTS))
def test_lora_conv2d_wgrad_against_the_rule(dev, scratch, name, kind, with_mask):
    ops = pkg("ops")
    c = C.wgrad_case(name, kind, with_mask)
    B, H, W, cs, cout = c.shape
    xs, keep = _device_sources(c, dev)
    g, w, a, b = c.dy.to(dev), c.w.to(dev), c.a.to(dev), c.b.to(dev)
    y = c.y.to(dev) if with_mask else None
    mask = (y.data_ptr(), cout * H * W) if with_mask else None
    assert ops.lora_conv2d_wgrad_supported(xs, g, w, a)
    ws = scratch()
    ws.fill_(float("nan"))      # a stale slab of another call's grid must not enter the reduction
    d_a, d_b = ops.lora_conv2d_wgrad_raw(xs, g, mask, w, a, b, c.s)
    assert scratch() is ws
    _check(d_a, c.da, kind, "wgrad", name, "dA")
    _check(d_b, c.db, kind, "wgrad", name, "dB")
    # bitwise reproducible (fixed-order reductions, no atomics), whatever the scratch held
    ws.fill_(-3.0)
    f_a, f_b = ops.lora_conv2d_wgrad_raw(xs, g, mask, w, a, b, c.s)
    assert torch.equal(d_a, f_a) and torch.equal(d_b, f_b)
    if kind == "exact":      # the two-call chain: another device path to the same integers
        dw, _ = ops.conv2d_wgrad_raw(xs, g, mask, w, False)
        _check(dw, C.filter_grad_rule(c.xs, c.dy, c.y), kind, "wgrad", name, "dW of the chain")
        e_a, e_b = ops.lora_grad(dw, a, b, c.s)
        _check(e_a, c.da, kind, "wgrad", name, "dA of the chain")
        _check(e_b, c.db, kind, "wgrad", name, "dB of the chain")
    for base, snap in keep:
        assert torch.equal(base.view(torch.int32), snap.view(torch.int32)), "a source buffer changed"


# ------------------------------------------------------------------------------------------------
# through autograd
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["1x1x4_4to3", "2x6x40_15to32", "2x3x68_33to33"])
@pytest.mark.parametrize("relu", [False, True], ids=["linear", "relu"])
def test_adapter_gradients_through_autograd(dev, name, relu):
    """ops.conv2d with only the adapter requiring grad, on exact inputs: lora_A.grad / lora_B.grad are the rule's bits whichever path the backward takes (the
    projected kernel where ynet_lora_conv2d_wgrad_preferred says so -- 33 -> 33 -- and the two-call chain elsewhere).  With a ReLU the layer's own output is
    the mask: integers as well, so the fp64 convolution has exactly the device's sign pattern."""
    ops = pkg("ops")
    c = C.wgrad_case(name, "exact", False)
    B, H, W, cs, cout = c.shape
    x64 = torch.cat([t.double() for t in c.xs], 1)
    y64 = F.conv2d(x64, C.compose_rule(c.w, c.a, c.b, c.s), None, padding=1)
    assert float(y64.abs().max()) < 2 ** 24
    if relu:
        y64 = F.relu(y64)
        assert y64.numel() < 256 or 0.2 < float((y64 > 0).double().mean()) < 0.8
    da, db = C.wgrad_rule(c.xs, c.dy, y64 if relu else None, c.a, c.b, c.s)
    xs = [t.to(dev) for t in c.xs]
    a, b = c.a.to(dev).requires_grad_(True), c.b.to(dev).requires_grad_(True)
    y = ops.conv2d(ops.lazy_cat(xs) if len(xs) > 1 else xs[0], c.w.to(dev), None, relu, {}, a, b, c.s)
    _check(y, y64, "exact", "wgrad", name, "y")
    y.backward(c.dy.to(dev))
    _check(a.grad, da, "exact", "wgrad", name, "lora_A.grad")
    _check(b.grad, db, "exact", "wgrad", name, "lora_B.grad")

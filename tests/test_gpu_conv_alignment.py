"""The convolution family on operands off a 16-byte boundary (tests/_align_cases.py has the placements, the shapes and the fp64 references).

Every shape has W % 4 == 0, so alignment alone decides the path: the aligned run of a case takes the fast family the case names, the misaligned run must
leave it -- read from ynet_conv2d_last_launch, ops.wino_stats, ops.upconv_stats, ops.premask_stats, the dispatcher's tag -- and still be right against fp64
at the tolerances of test_conv2d_dispatch_sweep.  Source slack is NaN: a read past an image that reaches arithmetic shows as a non-finite output, which is
asserted on its own.  Slack of every buffer a call could write keeps its poison bit for bit; every input buffer is bitwise unchanged.

YNET_ALIGN_STATS=<file>: the largest error per family (aligned / misaligned) is written there as JSON.  Measured on the MI355X (largest absolute error against
fp64, aligned / misaligned runs; bounds: y 2e-5 + 2e-5 |y|, dx 2e-6 of the largest gradient + 1e-4 |dx|, dW / db 1e-5 of the largest + 1e-4 of the element):
    family              y                  dx                 dW                 db
    dma_two_row         1.7e-6 / 1.7e-6    9.1e-7 / 9.1e-7    3.7e-5 / 3.6e-5    1.5e-5 / 1.4e-5
    dma_two_row_cat     2.2e-6 / 2.2e-6    7.6e-7 / 7.6e-7    4.1e-5 / 3.4e-5    1.9e-5 / 1.2e-5
    fold_4x8            1.8e-6 / 1.8e-6    8.9e-7 / 8.9e-7    6.6e-6 / 6.8e-6    2.2e-6 / 2.9e-6
    fold_2x16           1.7e-6 / 1.7e-6    7.1e-7 / 7.1e-7    1.3e-5 / 1.3e-5    8.3e-6 / 5.4e-6
    dma_split_k         1.7e-6 / 1.7e-6    7.7e-7 / 7.7e-7    4.4e-5 / 4.4e-5    1.4e-5 / 2.0e-5
    one_row_split_k     1.7e-6 / 1.7e-6    8.2e-7 / 8.2e-7    1.9e-5 / 1.9e-5    7.5e-6 / 9.1e-6
    stream_1x1_12 / 30  1.2e-6 / 1.2e-6    8.0e-7 / 8.0e-7    1.8e-5 / 2.2e-5    1.3e-5 / 1.7e-5
    k5                  1.3e-6 / 1.3e-6    7.6e-7 / 7.6e-7    3.8e-6 / 3.8e-6    1.3e-6 / 1.3e-6
    winograd            1.4e-6 / 3.7e-6    2.3e-6 / 2.3e-6    2.7e-4 / 1.7e-4    6.4e-5 / 8.2e-5
    winograd_cat        1.6e-6 / 5.3e-6    1.9e-6 / 1.9e-6    3.5e-4 / 1.8e-4    6.8e-5 / 9.8e-5
    slice_form          1.8e-6 / 5.4e-6    2.9e-6 / 2.9e-6    1.7e-4 / 1.1e-4    4.7e-5 / 5.3e-5
    pool_epilogue       1.2e-6 / 2.5e-6    1.3e-6 / 1.3e-6    9.7e-5 / 9.3e-5    5.6e-5 / 5.6e-5      (pooled copy: as y)
    chain (Winograd)    1.3e-6 / 1.5e-6    1.4e-6 / 2.5e-6    3.0e-4 / 4.1e-4
    chain (implicit)    2.4e-6 / 2.4e-6    2.5e-6 / 2.5e-6    4.1e-4 / 4.1e-4
    lora                2.6e-6 / 2.6e-6    2.4e-6 / 2.4e-6    dA 3.1e-5 / 8.7e-5, dB 7.9e-5 / 1.1e-4
    wgrad_raw           rolling_row dW 1.7e-4 / 1.1e-4, dma_two_row 6.5e-5 / 5.8e-5, stream_1x1 1.4e-5 / 1.3e-5, k5 4.8e-6 / 4.8e-6
    raw dispatchers     forward 8e-7 .. 1.8e-6 / 8e-7 .. 5.3e-6, data gradients 3e-7 .. 3.2e-6 / 3e-7 .. 4.2e-6;  upconv y 8.8e-7 / 8.8e-7
The 53 cases take 7 s (tests/test_gpu_kernels.py: 61 s for 313).

What a broken gate looks like here (each read off the code, the third also run on the host against a scratch build):
  * conv2d_impl no longer clears vec_load for a misaligned source: every case of test_conv2d_autograd_with_operands_off_16_bytes fails at "register-staged, no 16-byte
    loads" (the launch noted is an LDS-DMA / streaming one), and so do its dy placements (dy is the data gradient's source);
  * ynet_conv2d_wgrad ignores misaligned(dy, dy_bs): the dy placements of test_conv2d_wgrad_raw_...[rolling_row, dma_two_row] and of every 3 x 3 autograd case note kernel 2 / 3, not 1;
  * make_plan accepts a source on 8 bytes: tests/test_align_cases_host.py::test_plan_leaves_the_winograd_families_...[plain_32_32, plain_16_32_no_relu, dgrad_relu_of,
    slice_64_64, slice_dgrad_32_64_relu_of] fail on the host, the source placement (2, 0) of the Winograd cases here on the device;
  * _Conv2dFn.backward hands a misaligned dy's layer the ReLU mask of the layer below: test_conv_relu_conv_chain_...[winograd] counts an unmasked backward that must not
    happen, [implicit_gemm] is refused by ynet_conv2d_dgrad_relu_bits ("source 0")."""
import ctypes
import functools
import json
import os

import pytest
import torch

import _align_cases as A
from conftest import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
_stats = {}


def _record(family, aligned, what, err):
    key = f"{family}|{'aligned' if aligned else 'misaligned'}|{what}"
    _stats[key] = max(_stats.get(key, 0.0), err)


@pytest.fixture(scope="module", autouse=True)
def _dump_stats():
    yield
    path = os.environ.get("YNET_ALIGN_STATS")
    if path:
        with open(path, "w") as f:
            json.dump(_stats, f, indent=1, sort_keys=True)


def _check(got, want, tol, family, aligned, what, ctx):
    """Finite everywhere (the references are), then parity; records the largest error."""
    assert bool(torch.isfinite(got).all()), f"{family} {ctx}: {what} has {int((~torch.isfinite(got)).sum())} non-finite elements"
    nbad, err, atol = A.mismatch(got, want, **tol)
    _record(family, aligned, what.rstrip("0123456789"), err)
    assert nbad == 0, f"{family} {ctx}: {what} max err {err:.3e} (atol {atol:.2e}), {nbad} bad of {want.numel()}"


def _kind(note):
    return note & 15


def _off_boundary(where, B):
    """Does the placement take the operand off 16 bytes?  (The batch stride of a single image is never used.)"""
    return where is not None and (where[0] % 4 != 0 or (B > 1 and where[1] % 4 != 0))


def _place(t, dev, where):
    """(tensor on the device, its buffer or None, (off, pad)): an offset view for a placement, a plain device tensor for None."""
    if where is None:
        return t.to(dev), None, None
    v, buf = A.offset_view(t.to(dev), *where)
    assert v.data_ptr() % 16 == (4 * where[0]) % 16 and v.stride(0) == t[0].numel() + where[1]
    return v, buf, where


class _Inputs:
    """Input buffers of a run: bitwise unchanged afterwards."""

    def __init__(self):
        self.items = []

    def add(self, t, buf):
        src = buf if buf is not None else t
        self.items.append((src, src.detach().clone()))

    def unchanged(self):
        return all(A.same_bits(a.detach(), b) for a, b in self.items)


# ---- (a) ops.conv2d through autograd ---------------------------------------------------------------------------------------------------
def _autograd_run(dev, name, ref, want, src_at, dy_at):
    """One forward + backward of the case with source i at src_at[i] and the output gradient at dy_at; checks the numbers, returns what was launched."""
    ops = pkg("ops")
    lib = ops._lib()
    case = A.AUTOGRAD_CASES[name]
    B, H, W, cs, cout, K, relu = case["shape"]
    pool = bool(case.get("pool"))
    aligned = not src_at and dy_at is None
    ctx = f"src {src_at} dy {dy_at}"
    keep = _Inputs()
    xd = []
    for i, x in enumerate(ref.xs):
        v, buf, _ = _place(x, dev, src_at.get(i))
        keep.add(v, buf)
        xd.append(v.requires_grad_(True))
    wd, bd = ref.w.to(dev).requires_grad_(True), ref.b.to(dev).requires_grad_(True)
    g, gbuf, _ = _place(ref.gp if pool else ref.gy, dev, dy_at)
    keep.add(g, gbuf)
    lib.ynet_conv2d_last_launch(0), lib.ynet_conv2d_last_launch(1)
    n0, n16 = ops.wino_stats["launches"], ops.wino_stats.get("launches16", 0)
    yd = ops.conv2d(ops.lazy_cat(xd) if len(xd) > 1 else xd[0], wd, bd, relu, {}, pool=pool)
    out = {"fwd": lib.ynet_conv2d_last_launch(0), "fwd_wino": ops.wino_stats["launches"] - n0, "fwd_wino16": ops.wino_stats.get("launches16", 0) - n16}
    if pool:
        out["pooled"] = yd.data_ptr() in ops._pooled_outputs
        pd = ops.max_pool2(yd)
        assert not ops._pooled_outputs
        pd.backward(g)
        _check(pd.detach(), want["pooled"], A.TOL_Y, name, aligned, "pooled", ctx)
    else:
        yd.backward(g)
    out["dgrad"], out["wgrad"] = lib.ynet_conv2d_last_launch(0), lib.ynet_conv2d_last_launch(1)
    _check(yd.detach(), want["y"], A.TOL_Y, name, aligned, "y", ctx)
    for i, x in enumerate(xd):
        _check(x.grad, want["dxs"][i], A.TOL_DX, name, aligned, f"dx{i}", ctx)
    _check(wd.grad, want["dw"], A.TOL_DW, name, aligned, "dW", ctx)
    _check(bd.grad, want["db"], A.TOL_DW, name, aligned, "db", ctx)
    assert keep.unchanged(), f"{name} {ctx}: an input buffer changed"
    return out


@pytest.mark.parametrize("name", list(A.AUTOGRAD_CASES))
def test_conv2d_autograd_with_operands_off_16_bytes(dev, name):
    """y, dx of every source, dW and db of ops.conv2d against fp64 with one operand misaligned at a time: each source in turn (every placement), then the
    dy handed to backward (offsets: backward makes a strided dy contiguous), then a source and dy together.  The aligned run takes the family the case names;
    a misaligned source moves the forward launch and the filter gradient to the register-staged tiles, a misaligned dy the data and the filter gradient."""
    case = A.AUTOGRAD_CASES[name]
    B, H, W, cs, cout, K, relu = case["shape"]
    pool = bool(case.get("pool"))
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu, pool)
    want = {"y": ref.y.to(dev), "dxs": [d.to(dev) for d in ref.dxs], "dw": ref.dw.to(dev), "db": ref.db.to(dev)}
    if pool:
        want["pooled"] = ref.pooled.to(dev)
    staged = bool(case.get("wgrad_staged"))

    got = _autograd_run(dev, name, ref, want, {}, None)
    if "wino" in case:
        assert got["fwd"] == 0 and got["fwd_wino"] >= 1, got
        assert (got["fwd_wino16"] >= 1) == (case["wino"] == "winograd16:"), got
    else:
        assert _kind(got["fwd"]) == case["fwd"] and got["fwd_wino"] == 0, got
        assert (got["fwd"] >> 12) & 3 == 3, got                                   # 16-byte loads and stores were legal
        if "rows" in case:
            assert (got["fwd"] >> 4) & 15 == case["rows"], got
        if case.get("split") and case["fwd"] == 1:
            assert (got["fwd"] >> 8) & 15 > 1, got                                # the input-channel loop was split: the reduce kernel wrote y
    if pool:
        assert got["pooled"] == pkg("ops")._pool_epilogue_allowed
    assert (got["dgrad"] >> 12) & 1 == 1, got
    assert _kind(got["wgrad"]) in ((1,) if staged else (2, 3, 4)), got

    for i in range(len(cs)):
        for where in A.PLACEMENTS:
            m = _autograd_run(dev, name, ref, want, {i: where}, None)
            if not _off_boundary(where, B):
                assert (m["fwd"], m["fwd_wino"], m["dgrad"], m["wgrad"]) == (got["fwd"], got["fwd_wino"], got["dgrad"], got["wgrad"]), (i, where, m)
                continue
            assert m["fwd_wino"] == 0 and _kind(m["fwd"]) == 1 and (m["fwd"] >> 12) & 1 == 0, (i, where, m)      # register-staged, no 16-byte loads
            assert _kind(m["wgrad"]) == 1, (i, where, m)
            assert (m["dgrad"] >> 12) & 1 == 1 and _kind(m["dgrad"]) == _kind(got["dgrad"]), (i, where, m)           # (dy and the gradients are aligned)
            if pool:
                assert not m["pooled"], (i, where)
    if pool:
        return      # (the gradient goes to the pool's backward; the convolution's dy is that kernel's fresh output)
    for where in A.OFFSETS_ONLY:
        m = _autograd_run(dev, name, ref, want, {}, where)
        assert m["fwd"] == got["fwd"] and m["fwd_wino"] == got["fwd_wino"], (where, m)
        assert _kind(m["dgrad"]) == 1 and (m["dgrad"] >> 12) & 1 == 0 and _kind(m["wgrad"]) == 1, (where, m)
    m = _autograd_run(dev, name, ref, want, {0: (1, 0)}, (3, 0))
    assert _kind(m["fwd"]) == 1 and _kind(m["dgrad"]) == 1 and _kind(m["wgrad"]) == 1 and m["fwd_wino"] == 0, m
    m = _autograd_run(dev, name, ref, want, {len(cs) - 1: (2, 2)}, (2, 0))
    assert _kind(m["fwd"]) == 1 and _kind(m["dgrad"]) == 1 and _kind(m["wgrad"]) == 1 and m["fwd_wino"] == 0, m


@pytest.mark.parametrize("wino", [True, False], ids=["winograd", "implicit_gemm"])
def test_conv_relu_conv_chain_with_operands_off_16_bytes(dev, wino):
    """conv -> ReLU -> conv under fold_skip_gradients(): the second layer's data gradient applies the first layer's ReLU backward (the float activation, its
    1-bit form, or the Winograd tiling's mask word) only when dy is on a 16-byte boundary; off it, the first layer masks for itself.  A misaligned network
    input costs the first layer its 1-bit masks (its launch leaves the kernels that write them), not the hand-over."""
    ops = pkg("ops")
    B, H, W, c0, c1, c2 = A.CHAIN_CASE
    ref = A.chain_ref()
    want = {k: getattr(ref, k).to(dev) for k in ("y", "dx", "dw0", "dw1")}
    family = "chain_winograd" if wino else "chain_implicit_gemm"
    runs = [(None, None)] + [(p, None) for p in A.PLACEMENTS] + [(None, p) for p in A.OFFSETS_ONLY] + [((1, 0), (3, 0))]
    old_w = ops._wino_allowed
    ops._wino_allowed = wino
    try:
        for x_at, dy_at in runs:
            ctx = f"x {x_at} dy {dy_at}"
            aligned = x_at is None and dy_at is None
            keep = _Inputs()
            xd, xbuf, _ = _place(ref.x, dev, x_at)
            g, gbuf, _ = _place(ref.gy, dev, dy_at)
            keep.add(xd, xbuf), keep.add(g, gbuf)
            xd.requires_grad_(True)
            w0, w1 = ref.w0.to(dev).requires_grad_(True), ref.w1.to(dev).requires_grad_(True)
            for k in ("unmasked_backwards", "bit_masks", "wino_bit_masks"):
                ops.premask_stats[k] = 0
            n0 = ops.wino_stats["launches"]
            with ops.fold_skip_gradients():
                h = ops.conv2d(xd, w0, None, True, {}, bits=c2)
                n_fwd0 = ops.wino_stats["launches"] - n0
                y = ops.conv2d(h, w1, None, False, {})
                y.backward(g)
            st = dict(ops.premask_stats)
            _check(y.detach(), want["y"], A.TOL_Y, family, aligned, "y", ctx)
            _check(xd.grad, want["dx"], A.TOL_DX, family, aligned, "dx", ctx)
            _check(w0.grad, want["dw0"], A.TOL_DW, family, aligned, "dW", ctx)
            _check(w1.grad, want["dw1"], A.TOL_DW, family, aligned, "dW", ctx)
            assert keep.unchanged(), ctx
            assert not ops._premasked, ctx
            handed = dy_at is None and ops._premask_allowed
            assert st["unmasked_backwards"] == (1 if handed else 0), (ctx, st)
            assert n_fwd0 == (1 if (wino and x_at is None) else 0), (ctx, n_fwd0)
            if wino:
                assert st["bit_masks"] == 0, (ctx, st)
                assert st["wino_bit_masks"] == (1 if (handed and x_at is None and ops._wino_relu_bits_allowed) else 0), (ctx, st)
            else:
                assert st["wino_bit_masks"] == 0 and ops.wino_stats["launches"] == n0, (ctx, st)
                assert st["bit_masks"] == (1 if (handed and x_at is None and ops._relu_bits_allowed) else 0), (ctx, st)
    finally:
        ops._wino_allowed = old_w


def test_lora_layer_with_operands_off_16_bytes(dev):
    """A rank-1 loralib Conv2d whose adapter alone trains: aligned, dA / dB come from ynet_lora_conv2d_wgrad; off a 16-byte boundary lora_conv2d_wgrad_supported
    answers False and the two-call chain (ynet_conv2d_wgrad -> ynet_lora_grad) serves them -- both against fp64 autograd through W + s (B @ A)."""
    ops = pkg("ops")
    lib = ops._lib()
    B, H, W, cs, cout = A.LORA_CASE
    ref = A.lora_ref()
    want = {"y": ref.y.to(dev), "dx": ref.dxs[0].to(dev), "da": ref.da.to(dev), "db": ref.db.to(dev)}
    w = ref.w.to(dev)
    runs = [(None, None)] + [(p, None) for p in A.PLACEMENTS] + [(None, p) for p in A.OFFSETS_ONLY] + [((2, 0), (2, 0))]
    for x_at, dy_at in runs:
        ctx = f"x {x_at} dy {dy_at}"
        aligned = x_at is None and dy_at is None
        keep = _Inputs()
        xd, xbuf, _ = _place(ref.xs[0], dev, x_at)
        g, gbuf, _ = _place(ref.gy, dev, dy_at)
        keep.add(xd, xbuf), keep.add(g, gbuf)
        a, bm = ref.a.to(dev).requires_grad_(True), ref.bm.to(dev).requires_grad_(True)
        assert ops.lora_conv2d_wgrad_supported([xd], g, w, a) == aligned, ctx
        assert ops.lora_conv2d_wgrad_supported([xd], g, w, a, preferred=True) == aligned, ctx
        xd.requires_grad_(True)
        lib.ynet_conv2d_last_launch(1)
        y = ops.conv2d(xd, w, None, False, {}, lora_a=a, lora_b=bm, scale=ref.scale)
        y.backward(g)
        note = lib.ynet_conv2d_last_launch(1)
        assert _kind(note) == (0 if aligned else 1), (ctx, note)      # no filter gradient at all / the register-staged one of the two-call chain
        _check(y.detach(), want["y"], A.TOL_Y, "lora", aligned, "y", ctx)
        _check(xd.grad, want["dx"], A.TOL_DX, "lora", aligned, "dx", ctx)
        _check(a.grad, want["da"], A.TOL_LORA, "lora", aligned, "dA", ctx)
        _check(bm.grad, want["db"], A.TOL_LORA, "lora", aligned, "dB", ctx)
        assert keep.unchanged(), ctx


# ---- (b) destinations the caller owns: both dispatchers on the same operands ---------------------------------------------------------------
RAW_CASES = [(n, "fwd_dst") for n in ("dma_two_row", "fold_4x8", "fold_2x16", "dma_split_k", "one_row_split_k", "stream_1x1_12", "winograd", "winograd_cat")]
RAW_CASES += [(n, "dgrad_dst") for n in ("dma_two_row", "fold_2x16", "dma_split_k", "winograd", "winograd_cat")]
RAW_CASES += [(n, "dgrad_mask") for n in ("dma_two_row", "dma_split_k", "winograd")]
RAW_CASES += [(n, "relu_of") for n in ("dma_two_row", "dma_split_k", "fold_4x8", "stream_1x1_12", "winograd")]
RAW_CASES += [("dma_two_row", "pooled"), ("winograd_cat", "pooled"), ("winograd_cat", "addend"), ("dma_two_row", "bits")]


class _Raw:
    """The operands of one raw call: every one lives in an offset_view buffer (placement (0, 0) unless named), destinations poisoned throughout."""

    def __init__(self, dev):
        self.dev, self.inputs, self.outputs = dev, _Inputs(), []

    def src(self, t, where=None):
        v, buf = A.offset_view(t.to(self.dev), *(where or (0, 0)))
        self.inputs.add(v, buf)
        return v

    def dst(self, shape, where=None):
        where = where or (0, 0)
        v, buf = A.offset_view(torch.full(shape, NAN, device=self.dev), *where)
        self.outputs.append((v, buf, where))
        return v

    def slack_ok(self):
        return all(A.slack_intact(buf, v.shape, *where) for v, buf, where in self.outputs)

    def untouched(self):
        return all(bool(torch.isnan(buf).all()) for _, buf, _ in self.outputs)


def _desc(v):
    return (v.data_ptr(), v.shape[1], v.stride(0))


def _raw_once(dev, name, what, fn_name, at, refused=None):
    """Builds the operands (operand -> placement in `at`), calls one dispatcher, returns (tag, outputs, the operands, launch note, Winograd launches, bits).
    refused: the call must raise with that word in its message and without having launched anything -- every destination keeps its fill."""
    ops = pkg("ops")
    lib = ops._lib()
    B, H, W, cs, cout, K, relu = A.AUTOGRAD_CASES[name]["shape"]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu)
    r = _Raw(dev)
    kw = {}
    if what in ("fwd_dst", "pooled", "addend", "bits"):
        srcs = [_desc(r.src(x, at.get(f"src{i}"))) for i, x in enumerate(ref.xs)]
        wp, bias, mask, do_relu = ops.pack_weight(ref.w.to(dev), 0), ref.b.to(dev), None, relu
        outs = [r.dst((B, cout, H, W), at.get("dst0"))]
        direction = "fwd"
        if what == "pooled":
            p = r.dst((B, cout, H // 2, W // 2), at.get("pooled"))
            kw["pooled"] = (p.data_ptr(), p.stride(0))
            outs.append(p)
        if what == "addend":
            ad = r.src(A.randn(B, cout, H, W, key=(5, 1)), at.get("addend"))
            kw["addend"] = (ad.data_ptr(), ad.stride(0), 0)
        if what == "bits":
            words = lib.ynet_conv2d_relu_bits_words(B, H, W, cout, K)
            assert words > 0
            kw["bits_out"] = torch.full((words,), -1, device=dev, dtype=torch.int32)
    else:      # a data gradient: the source is dy, one destination per forward source
        srcs = [_desc(r.src(ref.gy, at.get("src0")))]
        wp, bias, do_relu = ops.pack_weight(ref.w.to(dev), 1), None, False
        mask = None
        if relu and what == "dgrad_mask":      # (the consumer-side mask: dy counts where the layer's output is > 0)
            mk = r.src(ref.y.float(), at.get("mask"))
            mask = (mk.data_ptr(), mk.stride(0))
        outs = [r.dst((B, c, H, W), at.get(f"dst{i}")) for i, c in enumerate(cs)]
        direction = "dgrad"
        if what == "relu_of":
            act = r.src(torch.relu(A.randn(B, cs[0], H, W, key=(5, 2))), at.get("relu_of"))
            kw["relu_of"] = (act.data_ptr(), act.stride(0))
    dsts = [_desc(o) for o in outs[:len(outs) - (1 if what == "pooled" else 0)]]
    bits_t = kw.get("bits_out")
    if bits_t is not None:
        kw["bits_out"] = bits_t.data_ptr()
    else:
        kw["wino"] = ({}, direction)
    lib.ynet_conv2d_last_launch(0)
    n0 = ops.wino_stats["launches"]
    def call():
        if fn_name == "py":
            assert what != "addend"
            return ops._conv2d_raw_py(srcs, mask, wp, bias, dsts, B, H, W, K, do_relu, **kw)
        return ops.conv2d_auto_raw(srcs, mask, wp, bias, dsts, B, H, W, K, do_relu, **kw)[0]

    if refused is not None:
        with pytest.raises(RuntimeError, match=refused) as e:
            call()
        torch.cuda.synchronize()
        assert "launch failed" not in str(e.value), str(e.value)
        assert r.untouched() and r.inputs.unchanged(), (name, what, fn_name, at, "a refused call wrote something")
        assert bits_t is None or bool((bits_t == -1).all())
        assert lib.ynet_conv2d_last_launch(0) == 0 and ops.wino_stats["launches"] == n0, (name, what, fn_name, at, "a refused call launched a kernel")
        return None
    tag = call()
    return tag, outs, r, lib.ynet_conv2d_last_launch(0), ops.wino_stats["launches"] - n0, bits_t


@functools.lru_cache(maxsize=None)
def _unmasked_dx(name):
    B, H, W, cs, cout, K, relu = A.AUTOGRAD_CASES[name]["shape"]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu)
    dx = torch.nn.grad.conv2d_input((B, sum(cs), H, W), ref.w.double(), ref.gy.double(), padding=K // 2)
    return list(dx.split(list(cs), dim=1))


def _raw_want(dev, name, what):
    B, H, W, cs, cout, K, relu = A.AUTOGRAD_CASES[name]["shape"]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu)
    if what in ("fwd_dst", "bits"):
        return [ref.y.to(dev)]
    if what == "pooled":
        return [ref.y.to(dev), torch.nn.functional.max_pool2d(ref.y, 2, 2).to(dev)]
    if what == "addend":
        pre = ref.pre + A.randn(B, cout, H, W, key=(5, 1)).double()
        return [(torch.relu(pre) if relu else pre).to(dev)]
    if what == "dgrad_mask" or not relu:
        dxs = ref.dxs
    else:      # (no consumer-side mask in this call: the gradient of the pre-activation is gy itself)
        dxs = _unmasked_dx(name)
    if what == "relu_of":
        return [(dxs[0] * (torch.relu(A.randn(B, cs[0], H, W, key=(5, 2))) > 0)).to(dev)]
    return [d.to(dev) for d in dxs]


# operand -> placements that must be REFUSED before any launch (the word the message must carry), by (what, Winograd-eligible shape)
def _refusal(name, what, operand, where):
    off, pad = where
    wino = "wino" in A.AUTOGRAD_CASES[name]
    if operand == "relu_of":      # 16 bytes for ynet_conv2d_dgrad_relu; the Winograd launches read it in 8-byte pairs
        ok = (off % 2 == 0 and pad % 2 == 0) if wino else (off % 4 == 0 and pad % 4 == 0)
        return None if ok else "relu_of"
    if operand == "pooled":       # the Winograd launches store the pooled copy element by element; ynet_conv2d_pool in 8-byte pairs
        ok = True if wino else (off % 2 == 0 and pad % 2 == 0)
        return None if ok else "pooled"
    if operand == "addend":       # 8-byte pairs in the Winograd launches
        return None if (off % 2 == 0 and pad % 2 == 0) else "addend"
    if what in ("pooled", "addend", "bits") and operand.startswith("src"):
        return "source"           # the epilogue variants exist in the LDS-DMA kernels only
    if what in ("pooled", "addend", "bits") and operand == "dst0":
        if what != "bits" and wino and off % 2 == 0 and pad % 2 == 0:
            return None           # (8 bytes are enough for a Winograd destination)
        return "destination"
    return None


@pytest.mark.parametrize("name,what", RAW_CASES, ids=[f"{n}-{w}" for n, w in RAW_CASES])
def test_raw_dispatchers_with_caller_owned_operands_off_16_bytes(dev, name, what):
    """ops._conv2d_raw_py and ops.conv2d_auto_raw on the same operands, one of them misaligned: the same tag, bit-identical outputs, right against fp64, slack
    intact -- or, where the header documents a refusal, an error that names the operand and leaves every destination as it was (nothing was launched)."""
    case = A.AUTOGRAD_CASES[name]
    B, H, W, cs, cout, K, relu = case["shape"]
    want = _raw_want(dev, name, what)
    fns = ["auto"] if what == "addend" else ["py", "auto"]
    tol = A.TOL_Y if what in ("fwd_dst", "pooled", "addend", "bits") else A.TOL_DX
    operands = {"fwd_dst": ["dst0"], "dgrad_dst": [f"dst{len(cs) - 1}"], "dgrad_mask": ["mask"], "relu_of": ["relu_of", "dst0"],
                "pooled": ["pooled", "src0", "dst0"], "addend": ["addend", "src0", "dst0"], "bits": ["src0", "dst0"]}[what]

    def run(at):
        res = [_raw_once(dev, name, what, f, at) for f in fns]
        tags = [t for t, *_ in res]
        assert all(t == tags[0] for t in tags), (at, tags)
        for o_a, o_b in zip(res[0][1], res[-1][1]):
            assert A.same_bits(o_a, o_b), (at, "the two dispatchers disagree")
        if res[0][5] is not None:
            assert torch.equal(res[0][5], res[-1][5]) and int((res[0][5] == -1).sum()) < res[0][5].numel()
        for tag, outs, r, note, nw, _ in res:
            for i, (o, w_) in enumerate(zip(outs, want)):
                _check(o, w_, tol, f"raw_{name}_{what}", not at, f"out{i}", str(at))
            assert r.slack_ok(), (at, "slack of a destination was written")
            assert r.inputs.unchanged(), (at, "an input buffer changed")
        return res[-1]

    tag0, _, _, note0, nw0, _ = run({})
    if "wino" in case and what != "dgrad_mask" and not (what == "dgrad_dst" and len(cs) > 1):
        # (a masked data gradient is the implicit GEMM's, and so is one with a 1-channel destination)
        assert tag0 is not None and tag0.startswith("winograd") and nw0 >= 1, (tag0, nw0)
    elif "fwd" in case and what == "fwd_dst":
        assert _kind(note0) == case["fwd"] and (note0 >> 12) & 3 == 3, note0

    for operand in operands:
        for where in A.PLACEMENTS:
            word = _refusal(name, what, operand, where)
            at = {operand: where}
            if word is None:
                tag, _, _, note, nw, _ = run(at)
                off, pad = where
                if operand.startswith("dst") and what in ("fwd_dst", "dgrad_dst"):
                    if tag0 is not None and off % 2 == 0 and pad % 2 == 0:
                        assert tag == tag0 and nw == nw0, (at, tag, tag0)      # 8 bytes are enough for a Winograd destination
                    else:
                        assert tag is None and nw == 0 and _kind(note) == 1 and (note >> 13) & 1 == 0, (at, tag, note)      # register-staged, element stores
                        if case.get("split"):
                            assert (note >> 8) & 15 > 1, (at, note)      # ... with the split reduce writing the unaligned destination
                if operand == "mask":
                    assert _kind(note) == 1 and (note >> 12) & 1 == 0, (at, note)
                if operand == "relu_of" and "wino" in case:
                    assert tag == tag0, (at, tag)      # legal by the dispatcher's own gate: the Winograd launch stays
                continue
            for f in fns:
                _raw_once(dev, name, what, f, at, refused=word)


def test_refused_calls_leave_their_destinations_untouched(dev):
    """The documented refusals through the C ABI, with the destinations in our hands: non-zero status, the operand named, every destination (and the pooled
    copy) still bit-identical to its fill, no launch noted."""
    ops, L = pkg("ops"), pkg("_lib")
    lib = ops._lib()
    B, H, W, cs, cout, K, relu = A.AUTOGRAD_CASES["dma_two_row"]["shape"]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu)
    cin = cs[0]
    wp = ops.pack_weight(ref.w.to(dev), 0)
    wp_d = ops.pack_weight(ref.w.to(dev), 1)
    vp = ctypes.c_void_p
    assert lib.ynet_conv2d_pool_supported(B, H, W, cout, K) and lib.ynet_conv2d_relu_bits_words(B, H, W, cout, K) > 0

    def arrays(v):
        return ops._arrays([(v.data_ptr(), v.shape[1], v.stride(0))])

    for what, operand, where, word in [("pool", "src", (1, 0), b"source 0"), ("pool", "src", (0, 2), b"source 0"), ("pool", "pooled", (1, 0), b"pooled"),
                                       ("pool", "pooled", (0, 1), b"pooled"), ("pool", "dst", (2, 0), b"destination"), ("bits", "src", (2, 0), b"source 0"),
                                       ("relu_of", "relu_of", (2, 0), b"relu_of"), ("relu_of", "relu_of", (0, 2), b"relu_of")]:
        r = _Raw(dev)
        at = {operand: where}
        lib.ynet_conv2d_last_launch(0)
        if what == "relu_of":
            dy = r.src(ref.gy)
            act = r.src(torch.relu(A.randn(B, cin, H, W, key=(5, 2))), at.get("relu_of"))
            dx = r.dst((B, cin, H, W))
            rc = lib.ynet_conv2d_dgrad_relu(dy.data_ptr(), cout, dy.stride(0), None, 0, wp_d.data_ptr(), dx.data_ptr(), cin, dx.stride(0), act.data_ptr(), act.stride(0),
                                            B, H, W, K, None, 0, ops._stream())
        else:
            x = r.src(ref.xs[0], at.get("src"))
            y = r.dst((B, cout, H, W), at.get("dst"))
            sp, sc, sb = arrays(x)
            if what == "pool":
                p = r.dst((B, cout, H // 2, W // 2), at.get("pooled"))
                rc = lib.ynet_conv2d_pool(sp, sc, sb, 1, wp.data_ptr(), None, y.data_ptr(), cout, y.stride(0), p.data_ptr(), p.stride(0), B, H, W, K, 1, ops._stream())
            else:
                bits = torch.full((lib.ynet_conv2d_relu_bits_words(B, H, W, cout, K),), -1, device=dev, dtype=torch.int32)
                rc = lib.ynet_conv2d_relu_bits(sp, sc, sb, 1, wp.data_ptr(), None, y.data_ptr(), cout, y.stride(0), bits.data_ptr(), B, H, W, K, ops._stream())
                torch.cuda.synchronize()
                assert bool((bits == -1).all())
        msg = lib.ynet_last_error()
        torch.cuda.synchronize()
        assert rc != 0 and word in msg and b"launch failed" not in msg, (what, at, msg)
        assert r.untouched() and r.inputs.unchanged(), (what, at)
        assert lib.ynet_conv2d_last_launch(0) == 0, (what, at)


# ---- (c) ops.conv2d_wgrad_raw -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", list(A.WGRAD_CASES))
def test_conv2d_wgrad_raw_with_operands_off_16_bytes(dev, family):
    """dW and db of ynet_conv2d_wgrad against fp64 with a source, dy (offsets: the wrapper passes the contiguous stride) or the mask misaligned: the call leaves the
    rolling-row / two-row LDS-DMA / streaming kernel for the 4-row register-staged tiles, and two identical calls stay bitwise equal (fixed-order reductions)."""
    ops = pkg("ops")
    lib = ops._lib()
    (B, H, W, cs, cout, K, masked), kind = A.WGRAD_CASES[family]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, masked)
    want_w, want_b = ref.dw.to(dev), ref.db.to(dev)
    w = ref.w.to(dev)
    runs = [{}] + [{f"src{i}": p} for i in range(len(cs)) for p in A.PLACEMENTS] + [{"dy": p} for p in A.OFFSETS_ONLY]
    if masked:
        runs += [{"mask": p} for p in A.PLACEMENTS]
    runs += [{"src0": (3, 0), "dy": (1, 0)}]
    for at in runs:
        keep = _Inputs()
        xs = []
        for i, x in enumerate(ref.xs):
            v, buf, _ = _place(x, dev, at.get(f"src{i}"))
            keep.add(v, buf)
            xs.append(v)
        g, gbuf, _ = _place(ref.gy, dev, at.get("dy"))
        keep.add(g, gbuf)
        mask = None
        if masked:
            mk, mbuf, _ = _place(ref.y.float(), dev, at.get("mask"))
            keep.add(mk, mbuf)
            mask = (mk.data_ptr(), mk.stride(0))
        lib.ynet_conv2d_last_launch(1)
        dw, db = ops.conv2d_wgrad_raw(xs, g, mask, w, True)
        note = lib.ynet_conv2d_last_launch(1)
        assert note == (1 if any(_off_boundary(p, B) for p in at.values()) else kind), (family, at, note)
        _check(dw, want_w, A.TOL_DW, f"wgrad_{family}", not at, "dW", str(at))
        _check(db, want_b, A.TOL_DW, f"wgrad_{family}", not at, "db", str(at))
        dw2, db2 = ops.conv2d_wgrad_raw(xs, g, mask, w, True)
        assert torch.equal(dw, dw2) and torch.equal(db, db2), (family, at)
        assert keep.unchanged(), (family, at)


# ---- (d) ynet_lora_conv2d_wgrad called directly -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", A.PLACEMENTS, ids=str)
def test_lora_conv2d_wgrad_refuses_a_misaligned_source(dev, where):
    ops = pkg("ops")
    lib = ops._lib()
    B, H, W, cs, cout = A.LORA_CASE
    cin = sum(cs)
    ref = A.lora_ref()
    x, xbuf = A.offset_view(ref.xs[0].to(dev), *where)
    snap = xbuf.clone()
    g, a, bm = ref.gy.to(dev), ref.a.to(dev), ref.bm.to(dev)
    d_a, d_b = torch.full_like(a, -3.0), torch.full_like(bm, -5.0)
    ws = torch.full((lib.ynet_lora_conv2d_wgrad_workspace_floats(cin, cout),), -7.0, device=dev)
    sp, sc, sb = ops._arrays([(x.data_ptr(), cin, x.stride(0))])
    rc = lib.ynet_lora_conv2d_wgrad(sp, sc, sb, 1, g.data_ptr(), cout * H * W, None, 0, a.data_ptr(), bm.data_ptr(), 1.0, d_a.data_ptr(), d_b.data_ptr(), ws.data_ptr(),
                                    B, H, W, cout, 3, 1, ops._stream())
    msg = lib.ynet_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and b"aligned" in msg and b"source 0" in msg, msg
    assert bool((d_a == -3.0).all()) and bool((d_b == -5.0).all()) and bool((ws == -7.0).all())
    assert A.same_bits(xbuf, snap)


# ---- (e) ops.upsample2x_conv2d ----------------------------------------------------------------------------------------------------------------
def test_upsample2x_conv2d_with_a_misaligned_input(dev):
    """Under no_grad an aligned input takes the fused launch (bilinear x2 inside the Winograd convolution); 4 or 8 bytes off it takes ynet_upsample2x_fwd and the
    convolution.  Both match fp64 bilinear + conv."""
    ops, ynet = pkg("ops"), pkg("models.ynet")
    B, Hl, Wl, cin, cout = A.UPCONV_CASE
    x, w, b, y64 = A.upconv_ref()
    want = y64.to(dev)
    conv = ynet.HipConv2d(cin, cout, kernel_size=3).to(dev)
    with torch.no_grad():
        conv.weight.copy_(w.to(dev))
        conv.bias.copy_(b.to(dev))
        for where in (None, (1, 0), (2, 0), (3, 0)):
            xd, buf, _ = _place(x, dev, where)
            snap = (buf if buf is not None else xd).clone()
            n0 = ops.upconv_stats["fused"]
            y = ops.upsample2x_conv2d(xd, conv)
            assert ops.upconv_stats["fused"] - n0 == (1 if where is None and ops._upconv_allowed and ops._wino_allowed and ops._wino_eval else 0), where
            _check(y, want, A.TOL_Y, "upconv", where is None, "y", str(where))
            assert A.same_bits(buf if buf is not None else xd, snap), where

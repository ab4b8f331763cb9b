"""The up-convolution's data gradient at the low resolution from the C ABI alone (include/ynet_hip.h: ynet_upconv_tables and the YNET_AUTO_UPCONV_BWD form of
ynet_conv2d_auto; models/ynet.py:463-464): the tables kernel against the package's fp64 einsums, the one call against torch's fp64 autograd and against the
three-step path it replaces, its cache, a decoder level through ctypes alone, and a training step that never calls torch.einsum."""
import ctypes

import numpy as np
import pandas as pd
import pytest
import torch
import torch.nn.functional as F

from conftest import build_model, pkg
from oracle import ynet_oracle as O

pytestmark = pytest.mark.gpu


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def spread(*shape, seed=0):
    """Magnitudes spread over about 2^40 (and both signs)."""
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * torch.exp2(torch.randint(-20, 21, shape, generator=g).float())


def same_bits(a, b):
    """Bit-identical fp32 tensors (+0 and -0 taken as one value: the sign of an exactly cancelled sum depends on the order of the terms, nothing downstream sees it)."""
    a, b = a.detach().contiguous().view(-1), b.detach().contiguous().view(-1)
    assert a.shape == b.shape and a.dtype == b.dtype == torch.float32
    ok = (a.view(torch.int32) == b.view(torch.int32)) | ((a == 0) & (b == 0))
    return bool(ok.all()), int((~ok).sum())


def s2d(dy):
    """[B, cout, 2h, 2w] -> the space-to-depth layout [B, 4 cout, h, w], plane (2 r + c) * cout + ch."""
    B, cout, H, W = dy.shape
    return dy.view(B, cout, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * cout, H // 2, W // 2).contiguous()


class OneCall:
    """One layer's YNET_AUTO_UPCONV_BWD calls through ctypes: its own cache and tag."""

    def __init__(self, L, lib, dev, K, B, h, w, masked, flags=0):
        self.L, self.lib, self.K = L, lib, K
        cout, cin = K.shape[0], K.shape[1]
        d = L.ConvAuto()
        d.nsrc = d.ndst = 1
        d.src_c[0], d.src_bs[0] = 4 * cout, 4 * cout * h * w
        d.dst_c[0], d.dst_bs[0] = cin, cin * h * w
        d.relu_of_bs = cin * h * w if masked else 0
        d.B, d.H, d.W, d.K, d.flags = B, h, w, 3, flags | L.AUTO_UPCONV_BWD
        d.src[0], d.dst[0], d.wp = 256, 256, 256          # (stand-ins while sizing: the plan looks at alignment only)
        if masked:
            d.relu_of = 256
        need = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d))
        assert need > 0, lib.ynet_last_error()
        self.cache = torch.empty(need, device=dev)
        self.tag = (ctypes.c_ulonglong * 2)(0, 0)
        d.cache, d.cache_floats, d.cache_tag, d.wp_version = self.cache.data_ptr(), need, self.tag, 1
        self.d, self.masked = d, masked
        nws = lib.ynet_conv2d_auto_workspace_floats(ctypes.byref(d)) if B * h * w <= 65536 else 0
        self.ws = torch.empty(max(nws, 1), device=dev)
        if nws > 0:
            d.workspace, d.workspace_floats = self.ws.data_ptr(), nws

    def __call__(self, D, dx, relu_of=None, version=None):
        d = self.d
        d.src[0], d.dst[0], d.wp = D.data_ptr(), dx.data_ptr(), self.K.data_ptr()
        d.relu_of = relu_of.data_ptr() if self.masked else None
        if version is not None:
            d.wp_version = version
        tk = self.L.ConvTaken()
        self.L.check(self.lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), torch.cuda.current_stream().cuda_stream), self.lib)
        return tk


@pytest.mark.parametrize("cout,cin", [(16, 32), (32, 64), (8, 24), (16, 40), (1, 1)], ids=str)
@pytest.mark.parametrize("kind", ["normal", "spread"])
def test_tables_kernel_is_bit_identical_to_the_einsums(dev, cout, cin, kind):
    """ynet_upconv_tables (one launch, fp64 sums without contraction, one rounding) writes the packed effective filter and the 16 ring tables bit for bit as
    ops.upconv_s2d_tables (four fp64 torch.einsum calls, then ynet_pack_weight in mode 1), padding included."""
    L, ops = pkg("_lib"), pkg("ops")
    lib = L.load()
    for seed in range(3):
        K = (rnd(cout, cin, 3, 3, seed=seed, scale=0.2) if kind == "normal" else spread(cout, cin, 3, 3, seed=seed)).to(dev)
        wp_ref, tab_ref, _ = ops.upconv_s2d_tables(K, {})
        kf, tf = ctypes.c_longlong(0), ctypes.c_longlong(0)
        lib.ynet_upconv_tables_floats(cout, cin, ctypes.byref(kf), ctypes.byref(tf))
        keff = torch.full((kf.value,), float("nan"), device=dev)
        tab = torch.full((16, 4 * cout, cin), float("nan"), device=dev)
        L.check(lib.ynet_upconv_tables(K.data_ptr(), cout, cin, keff.data_ptr(), tab.data_ptr(), torch.cuda.current_stream().cuda_stream), lib)
        torch.cuda.synchronize()
        assert wp_ref.numel() == kf.value and tab_ref.shape == tab.shape
        ok, nbad = same_bits(keff, wp_ref)
        assert ok, f"effective filter: {nbad} entries differ (seed {seed})"
        ok, nbad = same_bits(tab, tab_ref)
        assert ok, f"ring tables: {nbad} entries differ (seed {seed})"


def _fp64_reference(x, K, dy, gate):
    xr = x.double().cpu().requires_grad_(True)
    y = F.conv2d(F.interpolate(xr, scale_factor=2, mode="bilinear", align_corners=False), K.double().cpu(), padding=1)
    (want,) = torch.autograd.grad(y, xr, dy.double().cpu())
    return want * (gate.cpu() > 0) if gate is not None else want


@pytest.mark.parametrize("cin", [24, 40])
@pytest.mark.parametrize("h,w", [(2, 2), (5, 7), (33, 17), (128, 128)], ids=str)
@pytest.mark.parametrize("B", [1, 3, 8])
def test_one_call_against_fp64_autograd(dev, B, h, w, cin):
    """dx of conv2d(F.interpolate(x, scale_factor=2, mode='bilinear'), K) with respect to x, from the space-to-depth output gradient, in ONE ynet_conv2d_auto call
    with the raw filter -- with and without the ReLU gate of the layer below; cin 24 / 40 put the ring kernel's corner loop over a partial group of 32 channels."""
    L = pkg("_lib")
    lib = L.load()
    cout = 16
    K = rnd(cout, cin, 3, 3, seed=B + cin, scale=0.3).to(dev)
    x = rnd(B, cin, h, w, seed=2)
    dy = rnd(B, cout, 2 * h, 2 * w, seed=3)
    gate = torch.relu(rnd(B, cin, h, w, seed=4)).to(dev)
    D = s2d(dy).to(dev)
    for masked in (False, True):
        call = OneCall(L, lib, dev, K, B, h, w, masked)
        dx = torch.full((B, cin, h, w), float("nan"), device=dev)
        tk = call(D, dx, gate)
        assert tk.transformed == 1 and tk.nlaunch >= 2
        want = _fp64_reference(x, K, dy, gate if masked else None)
        err = float((dx.double().cpu() - want).abs().max())
        scale = float(want.abs().max())
        assert err <= 1e-5 * scale, (masked, err, scale, tk.family, tk.variant)


@pytest.mark.parametrize("masked", [False, True])
def test_one_call_is_bit_equal_to_the_three_step_path(dev, masked):
    """At decoder level 4 of C2 (B 32, cout 16, cin 32, 128^2 low resolution): the one call equals, bit for bit, the path it replaces -- the einsum tables,
    ynet_conv2d_auto with the packed effective filter, ynet_upconv_dgrad_ring."""
    L, ops = pkg("_lib"), pkg("ops")
    lib = L.load()
    B, cout, cin, h, w = 32, 16, 32, 128, 128
    stream = torch.cuda.current_stream().cuda_stream
    K = rnd(cout, cin, 3, 3, seed=11, scale=0.1).to(dev)
    D = rnd(B, 4 * cout, h, w, seed=12).to(dev)
    gate = torch.relu(rnd(B, cin, h, w, seed=13)).to(dev)
    dx1 = torch.full((B, cin, h, w), float("nan"), device=dev)
    tk1 = OneCall(L, lib, dev, K, B, h, w, masked)(D, dx1, gate)
    # the three steps
    wp_eff, tables, _ = ops.upconv_s2d_tables(K, {})
    d = L.ConvAuto()
    d.nsrc = d.ndst = 1
    d.src[0], d.src_c[0], d.src_bs[0] = D.data_ptr(), 4 * cout, 4 * cout * h * w
    dx0 = torch.full((B, cin, h, w), float("nan"), device=dev)
    d.dst[0], d.dst_c[0], d.dst_bs[0] = dx0.data_ptr(), cin, cin * h * w
    if masked:
        d.relu_of, d.relu_of_bs = gate.data_ptr(), cin * h * w
    d.wp, d.B, d.H, d.W, d.K = wp_eff.data_ptr(), B, h, w, 3
    need = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d))
    cache, tag = torch.empty(max(need, 1), device=dev), (ctypes.c_ulonglong * 2)(0, 0)
    d.cache, d.cache_floats, d.cache_tag, d.wp_version = cache.data_ptr(), need, tag, 1
    tk0 = L.ConvTaken()
    L.check(lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk0), stream), lib)
    L.check(lib.ynet_upconv_dgrad_ring(D.data_ptr(), 4 * cout * h * w, tables.data_ptr(), gate.data_ptr() if masked else None, cin * h * w, dx0.data_ptr(),
                                       cin * h * w, B, 4 * cout, cin, h, w, stream), lib)
    torch.cuda.synchronize()
    assert (tk1.family, tk1.variant, tk1.nlaunch) == (tk0.family, tk0.variant, tk0.nlaunch + 1) and tk1.family != 0
    assert torch.equal(dx1, dx0)
    assert torch.equal(dx1.view(torch.int32), dx0.view(torch.int32))


def test_cache_follows_the_filter_version_and_belongs_to_its_layer(dev):
    L = pkg("_lib")
    lib = L.load()
    B, cout, cin, h, w = 8, 16, 32, 64, 64
    K1 = rnd(cout, cin, 3, 3, seed=21, scale=0.1).to(dev)
    K2 = rnd(cout, cin, 3, 3, seed=22, scale=0.1).to(dev)
    D = rnd(B, 4 * cout, h, w, seed=23).to(dev)
    gate = torch.relu(rnd(B, cin, h, w, seed=24)).to(dev)
    l1, l2 = OneCall(L, lib, dev, K1, B, h, w, True), OneCall(L, lib, dev, K2, B, h, w, True)
    out = lambda: torch.full((B, cin, h, w), float("nan"), device=dev)      # noqa: E731
    a1, a2 = out(), out()
    assert l1(D, a1, gate, version=1).transformed == 1 and l2(D, a2, gate, version=1).transformed == 1
    b1 = out()
    assert l1(D, b1, gate, version=1).transformed == 0                      # same version: the tables are not remade
    assert torch.equal(a1, b1)
    # K changes in place, the version is bumped: the tables are remade and the result follows the new K
    K1.mul_(-0.5).add_(0.01)
    c1 = out()
    assert l1(D, c1, gate, version=2).transformed == 1
    fresh = out()
    assert OneCall(L, lib, dev, K1, B, h, w, True)(D, fresh, gate).transformed == 1
    assert torch.equal(c1, fresh) and not torch.equal(c1, a1)
    # ... and without the bump the cache is trusted (the caller's contract): the old tables
    K1.mul_(2.0)
    e1 = out()
    assert l1(D, e1, gate, version=2).transformed == 0 and torch.equal(e1, c1)
    # the second layer, with its own cache, did not move
    b2 = out()
    assert l2(D, b2, gate, version=1).transformed == 0 and torch.equal(a2, b2)


def test_decoder_level_4_backward_through_the_c_abi_alone(dev):
    """The backward of decoder level 4's up-convolution (models/ynet.py:463-464) from the header's entry points alone -- the gradient the package hands to the
    up-convolution (written space-to-depth by the level's first convolution), the layer's raw filter and its input's activation go through ONE ctypes call, no
    ops function, no tables from Python -- equals the package's autograd gradient of the up-convolution's input bit for bit."""
    ynet, ops, L = pkg("models.ynet"), pkg("ops"), pkg("_lib")
    lib = L.load()
    if not ops._upconv_s2d_allowed:
        pytest.skip("YNET_UPCONV_S2D=0")
    B, Hl, Wl = 8, 128, 128
    H, W = 2 * Hl, 2 * Wl
    below, up = ynet.HipConv2d(32, 32, 3).to(dev), ynet.HipConv2d(32, 16, 3).to(dev)
    top = ynet.FusedSequential(ynet.HipConv2d(48, 32, 3), torch.nn.ReLU(), ynet.HipConv2d(32, 32, 3), torch.nn.ReLU()).to(dev)
    for m in (below, up, top):
        for p_ in m.parameters():
            p_.requires_grad_(False)
    xi = rnd(B, 32, Hl, Wl, seed=1).to(dev).requires_grad_(True)
    skip = torch.relu(rnd(B, 32, H, W, seed=2)).to(dev)
    g = rnd(B, 32, H, W, seed=4).to(dev)
    seen = {}
    n0 = ops.upconv_stats_s2d["backwards"]
    with ops.fold_skip_gradients():
        h0 = below(xi, relu=True)
        u_ = ops.upsample2x_conv2d(h0, up)
        u_.register_hook(lambda t: seen.__setitem__("D", t.detach().clone()))      # (the memory holds [B, 64, Hl, Wl] space-to-depth)
        h0.register_hook(lambda t: seen.__setitem__("dx", t.detach().clone()))
        (top(ops.lazy_cat([u_, skip])) * g).sum().backward()
    torch.cuda.synchronize()
    assert ops.upconv_stats_s2d["backwards"] - n0 == 1
    D = seen["D"].view(B, 64, Hl, Wl)
    dx = torch.full((B, 32, Hl, Wl), float("nan"), device=dev)
    tk = OneCall(L, lib, dev, up.weight.detach(), B, Hl, Wl, True)(D, dx, h0.detach())
    torch.cuda.synchronize()
    assert tk.transformed == 1 and tk.family != 0
    assert torch.equal(dx.view(torch.int32), seen["dx"].view(torch.int32))


def test_training_step_runs_without_einsum(dev, monkeypatch):
    """A C2-config training step -- eager, captured, replayed -- with torch.einsum made to raise: the up-convolutions' backward makes its tables in the library.
    Its loss, ADE / FDE and adapter gradients are bit-equal to the same steps with the tables injected from ops.upconv_s2d_tables (the three-step path)."""
    ops, te, trn, iu = pkg("ops"), pkg("utils.train_epoch"), pkg("models.trainer"), pkg("utils.image_utils")
    L = pkg("_lib")
    if not ops._upconv_s2d_allowed or not ops.conv_auto:
        pytest.skip("YNET_UPCONV_S2D=0 / YNET_CONV_AUTO=0")
    cfg, H, W, B = O.sdd_short(train_net="mosa_1", position=["0", "1", "2", "3", "4"]), 256, 256, 8
    sd = O.make_state_dict(cfg, seed=0, lora_b_std=0.05)
    scene, traj = O.synthetic_scene(cfg, H, W, 0), O.synthetic_trajectories(cfg, B, H, W, 21)
    S = cfg.template_size
    in_t, gt_t = iu.analytic_dist_template(S, dev), iu.analytic_gaussian_template(S, cfg.kernlen, cfg.nsig, False, dev)
    meta = pd.DataFrame({"metaId": np.arange(B)})
    loader = [(traj.clone(), [meta], "scene0") for _ in range(3)]      # eager (warm-up), capture, replay

    def three_step(D, weight, dx, relu_of, B_, cout, cin, h, w, cache):
        wp_eff, tables, wcache = ops.upconv_s2d_tables(weight, cache)
        ops.conv2d_raw([(D, 4 * cout, 4 * cout * h * w)], None, wp_eff, None, [(dx, cin, cin * h * w)], B_, h, w, 3, False,
                       relu_of=(relu_of, cin * h * w) if relu_of is not None else None, wino=(wcache, "dgrad"))
        lib = ops._lib()
        L.check(lib.ynet_upconv_dgrad_ring(D, 4 * cout * h * w, tables.data_ptr(), relu_of, cin * h * w, dx, cin * h * w, B_, 4 * cout, cin, h, w, ops._stream()), lib)

    def raise_(*a, **k):
        raise AssertionError("torch.einsum was called")

    runs = {}
    for mode in ("library", "einsum"):
        with monkeypatch.context() as mp:
            if mode == "library":
                mp.setattr(torch, "einsum", raise_)
            else:
                mp.setattr(ops, "upconv_dgrad_raw", three_step)
            n0 = ops.upconv_stats_s2d["backwards"]
            model = build_model(cfg, sd, dev)
            opt = torch.optim.SGD(model.parameters(), lr=0.0)
            res = te.train_epoch(model, loader, {"scene0": scene[0]}, opt, trn.HipBCEWithLogitsLoss(), cfg.loss_scale, dev, "sdd", None, gt_t, in_t,
                                 list(cfg.waypoints), 0, cfg.obs_len, cfg.pred_len, B, 10000, cfg.resize_factor, cfg.network, False, graph=True)
            torch.cuda.synchronize()
            used = ops.upconv_stats_s2d["backwards"] - n0
        runs[mode] = (res, {n: p.grad.detach().clone() for n, p in model.named_parameters() if p.grad is not None}, used)
    (r1, g1, u1), (r0, g0, u0) = runs["library"], runs["einsum"]
    assert u1 == u0 and u1 >= 2, (u1, u0)                # (both decoders' up-convolutions took the low-resolution backward)
    assert r1 == r0, (r1, r0)
    assert g1.keys() == g0.keys() and len(g1) == 18
    for n in g1:
        assert torch.equal(g1[n].view(torch.int32), g0[n].view(torch.int32)), n

"""The alignment sweep of the convolution family, the part that needs no GPU: the builder of offset views, the fp64 references against stock fp32
torch, the dispatcher's plan on stand-in pointers (ynet_conv2d_auto_plan looks at pointers for alignment and NULL only), the shapes of the case tables
against ynet_conv2d_plan, and the documented refusals -- answered on the host, before any launch."""
import ctypes

import pytest
import torch
import torch.nn.functional as F

import _align_cases as A
from conftest import pkg


# ---- offset_view ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off,pad", A.PLACEMENTS + [(0, 0)])
def test_offset_view_places_the_tensor_and_poisons_the_slack(off, pad):
    t = A.randn(3, 2, 4, 8, key=1)
    v, buf = A.offset_view(t, off, pad)
    assert torch.equal(v, t) and v.shape == t.shape
    assert buf.data_ptr() % 16 == 0 and v.data_ptr() % 16 == (4 * off) % 16 and v.data_ptr() == buf.data_ptr() + 4 * off
    assert v.stride() == (2 * 4 * 8 + pad, 32, 8, 1)
    assert buf.numel() == off + 3 * (64 + pad) + A.TAIL
    m = A.slack_mask(t.shape, off, pad)
    assert int(m.sum()) == off + 3 * pad + A.TAIL and bool(torch.isnan(buf[m]).all()) and not bool(torch.isnan(buf[~m]).any())
    assert A.slack_intact(buf, t.shape, off, pad)
    # one slack float changed -- before the view, between two images, behind the last one -- is seen; so is a NaN of another payload
    for i in [j for j in (off - 1, off + 64 + pad - 1, buf.numel() - 1) if j >= 0 and bool(m[j])]:
        old = buf[i].clone()
        buf[i] = 0.0
        assert not A.slack_intact(buf, t.shape, off, pad)
        A.bits(buf)[i] = 0x7FC00001
        assert not A.slack_intact(buf, t.shape, off, pad)
        buf[i] = old
    assert A.slack_intact(buf, t.shape, off, pad)
    v2, buf2 = A.offset_view(t, off, pad, poison=-7.5)
    assert bool((buf2[m] == -7.5).all()) and A.slack_intact(buf2, t.shape, off, pad, poison=-7.5)


def test_offset_view_insists_on_an_aligned_base():
    t = A.randn(1, 1, 4, 4, key=2)
    with pytest.raises(AssertionError, match="16-byte aligned"):
        A.offset_view(t, 1, 0, alloc=lambda n: torch.empty(n + 1)[1:])
    with pytest.raises(AssertionError):
        A.offset_view(t, 1, 0, alloc=lambda n: torch.empty(n + 4))      # (not the size asked for)


def test_mismatch_counts_nan_as_bad():
    want = torch.tensor([1.0, 2.0, float("nan")], dtype=torch.float64)
    assert A.mismatch(torch.tensor([1.0, 2.0, float("nan")]), want)[0] == 1      # (a NaN reference is never matched: the references here are finite)
    assert A.mismatch(torch.tensor([1.0, float("nan")]), want[:2])[0] == 1
    assert A.mismatch(torch.tensor([1.0, float("inf")]), want[:2])[0] == 1
    assert A.mismatch(torch.tensor([1.0, 2.0 + 1e-5]), want[:2], rtol=1e-5, atol=1e-6)[0] == 0


# ---- the fp64 references against stock fp32 torch -------------------------------------------------------------------------------------------
SMALL = [n for n, c in A.AUTOGRAD_CASES.items() if c["shape"][0] * c["shape"][1] * c["shape"][2] <= 8192]


@pytest.mark.parametrize("name", SMALL)
def test_fp64_reference_agrees_with_fp32_torch(name):
    B, H, W, cs, cout, K, relu = A.AUTOGRAD_CASES[name]["shape"]
    ref = A.conv_ref(B, H, W, tuple(cs), cout, K, relu)
    assert ref is A.conv_ref(B, H, W, tuple(cs), cout, K, relu)      # computed once
    xs = [x.clone().requires_grad_(True) for x in ref.xs]
    w, b = ref.w.clone().requires_grad_(True), ref.b.clone().requires_grad_(True)
    y = F.conv2d(torch.cat(xs, 1), w, b, padding=K // 2)
    y = F.relu(y) if relu else y
    y.backward(ref.gy)
    assert A.mismatch(y, ref.y, **A.TOL_Y)[0] == 0
    if relu:      # the gradient is zero wherever the two precisions could disagree on the mask, and only there and where the output is clearly negative
        assert bool(((y > 0) == (ref.pre > 0))[ref.gy != 0].all())
        assert float((ref.gy == 0).double().mean()) < 1e-3
    for got, want in zip(xs, ref.dxs):
        assert A.mismatch(got.grad, want, **A.TOL_DX)[0] == 0
    assert A.mismatch(w.grad, ref.dw, **A.TOL_DW)[0] == 0 and A.mismatch(b.grad, ref.db, **A.TOL_DW)[0] == 0


def test_lora_reference_agrees_with_fp32_torch():
    ref = A.lora_ref()
    a, bm = ref.a.clone().requires_grad_(True), ref.bm.clone().requires_grad_(True)
    y = F.conv2d(torch.cat(ref.xs, 1), ref.w + (bm @ a).view(ref.w.shape) * ref.scale, None, padding=1)
    y.backward(ref.gy)
    assert A.mismatch(y, ref.y, **A.TOL_Y)[0] == 0
    assert A.mismatch(a.grad, ref.da, **A.TOL_LORA)[0] == 0 and A.mismatch(bm.grad, ref.db, **A.TOL_LORA)[0] == 0


# ---- the shapes of the case tables take the family they name (ynet_conv2d_plan: aligned planes assumed) -----------------------------------------
@pytest.mark.parametrize("name", [n for n, c in A.AUTOGRAD_CASES.items() if "fwd" in c])
def test_case_shapes_plan_the_family_they_name(name):
    lib = pkg("_lib").load()
    case = A.AUTOGRAD_CASES[name]
    B, H, W, cs, cout, K, relu = case["shape"]
    assert W % 4 == 0
    plan = lib.ynet_conv2d_plan(B, H, W, cout, K)
    rows, dma, flog = plan & 255, (plan >> 17) & 1, (plan >> 19) & 3
    if case.get("split"):
        assert lib.ynet_conv2d_workspace_floats(B, H, W, cout) > 0      # (the partial sums of the split)
    if case["fwd"] == 2:
        assert dma == 1 and flog == 0 and rows == case["rows"]
    elif case["fwd"] == 3:
        assert dma == 1 and flog == {"fold_4x8": 2, "fold_2x16": 1}[name] and rows == 1
    elif case.get("split"):
        assert dma == 0 and rows == 1      # one-row tiles: register-staged
    else:
        assert dma == 0      # 1x1, 5x5: no LDS-DMA form
    assert not lib.ynet_conv2d_winograd_supported(B, H, W, sum(cs), cout, K)


def test_winograd_case_shapes_are_the_smallest_served():
    lib = pkg("_lib").load()
    assert lib.ynet_conv2d_winograd_supported(8, 128, 128, 32, 32, 3) and not lib.ynet_conv2d_winograd_supported(7, 128, 128, 32, 32, 3)
    c3 = (ctypes.c_int * 3)(32, 16, 1)
    assert lib.ynet_conv2d_winograd_cat_supported(8, 128, 128, c3, 3, 32, 3) and not lib.ynet_conv2d_winograd_cat_supported(7, 128, 128, c3, 3, 32, 3)
    c1 = (ctypes.c_int * 1)(64)
    assert lib.ynet_conv2d_winograd16_supported(10, 64, 64, c1, 1, 64, 3) and not lib.ynet_conv2d_winograd16_supported(9, 64, 64, c1, 1, 64, 3)
    assert lib.ynet_conv2d_pool_supported(8, 128, 128, 32, 3)
    B, Hl, Wl, cin, cout = A.UPCONV_CASE
    assert lib.ynet_upsample2x_conv2d_winograd_supported(B, 2 * Hl, 2 * Wl, cin, cout, 3) == 1
    B, H, W, cs, cout = A.LORA_CASE
    assert lib.ynet_lora_conv2d_wgrad_preferred(sum(cs), cout, 3, 1, W)


# ---- the dispatcher's plan on stand-in pointers -----------------------------------------------------------------------------------------
def _family(lib, L, d):
    tk = L.ConvTaken()
    rc = lib.ynet_conv2d_auto_plan(ctypes.byref(d), ctypes.byref(tk))
    return (tk.family if rc == 0 else None), lib.ynet_last_error()


@pytest.mark.parametrize("name", list(A.PLAN_CASES))
def test_plan_leaves_the_winograd_families_for_an_operand_off_its_boundary(name):
    L = pkg("_lib")
    lib = L.load()
    B, H, W, cs, couts, relu, opts, family = A.PLAN_CASES[name]
    up = bool(opts.get("upsample2x"))
    assert _family(lib, L, A.plan_desc(L, name))[0] == family
    for i in range(len(cs)):
        for byte_off in (4, 8, 12):      # a source off 16 bytes
            d = A.plan_desc(L, name)
            d.src[i] = d.src[i] + byte_off
            fam, msg = _family(lib, L, d)
            if up:      # no implicit-GEMM form of the up-convolution: refused, the caller runs ynet_upsample2x_fwd and the convolution
                assert fam is None and b"upsample2x" in msg and b"ynet_upsample2x_fwd" in msg, (name, byte_off, msg)
            else:
                assert fam == 0, (name, i, byte_off)
        if up:
            continue      # (the up-convolution's kernel addresses image b by src_bs in floats: ynet_upsample2x_conv2d_winograd checks it at the call)
        for extra in (1, 2, 3):      # its batch stride off a multiple of 4 floats
            d = A.plan_desc(L, name)
            d.src_bs[i] = d.src_bs[i] + extra
            assert _family(lib, L, d)[0] == 0, (name, i, extra)
    if not up:
        d = A.plan_desc(L, name)
        d.dst[0] = d.dst[0] + 4
        assert _family(lib, L, d)[0] == 0, name
        d = A.plan_desc(L, name)
        d.dst_bs[0] = d.dst_bs[0] + 1
        assert _family(lib, L, d)[0] == 0, name
        d = A.plan_desc(L, name)      # 8 bytes are enough for a destination
        d.dst[0] = d.dst[0] + 8
        assert _family(lib, L, d)[0] == family, name
        d = A.plan_desc(L, name)
        d.dst_bs[0] = d.dst_bs[0] + 2
        assert _family(lib, L, d)[0] == family, name
    if opts.get("relu_of"):
        d = A.plan_desc(L, name)
        d.relu_of = d.relu_of + 8
        assert _family(lib, L, d)[0] == family, name
        d = A.plan_desc(L, name)
        d.relu_of_bs = d.relu_of_bs + 2
        assert _family(lib, L, d)[0] == family, name
        for byte_off in (4, 12):
            d = A.plan_desc(L, name)
            d.relu_of = d.relu_of + byte_off
            assert _family(lib, L, d)[0] == 0, (name, byte_off)
        d = A.plan_desc(L, name)
        d.relu_of_bs = d.relu_of_bs + 1
        assert _family(lib, L, d)[0] == 0, name


def test_plan_with_an_additive_term_off_its_boundary():
    """The Winograd launches read the additive term in 8-byte pairs: 4 bytes off, or an odd image stride, plans the implicit GEMM (which then wants 16 bytes)."""
    L = pkg("_lib")
    lib = L.load()

    def desc():
        d = A.plan_desc(L, "cat_49")
        d.addend, d.addend_bs = 4096 * 20, 32 * 256 * 256
        return d

    assert _family(lib, L, desc())[0] == 2
    d = desc()
    d.addend = d.addend + 8
    assert _family(lib, L, d)[0] == 2
    for change in ("ptr4", "ptr12", "bs1"):
        d = desc()
        if change == "bs1":
            d.addend_bs = d.addend_bs + 1
        else:
            d.addend = d.addend + int(change[3:])
        assert _family(lib, L, d)[0] == 0, change


# ---- documented refusals: answered before any launch, so the host can ask -----------------------------------------------------------------------
def _arrays(L, ptrs, cs, bss):
    n = len(ptrs)
    vp = ctypes.c_void_p
    return (ctypes.cast((vp * n)(*[vp(p) for p in ptrs]), L.PP), (ctypes.c_int * n)(*cs), (ctypes.c_longlong * n)(*bss))


def test_epilogue_variants_refuse_operands_off_16_bytes_before_any_launch():
    L = pkg("_lib")
    lib = L.load()
    vp = ctypes.c_void_p
    B, H, W, cin, cout = 8, 128, 128, 32, 32
    img_in, img_out, img_p = cin * H * W, cout * H * W, cout * (H // 2) * (W // 2)
    assert lib.ynet_conv2d_pool_supported(B, H, W, cout, 3) and lib.ynet_conv2d_add_supported(B, H, W, cout, 3)
    assert lib.ynet_conv2d_relu_bits_words(B, H, W, cout, 3) > 0

    def pool(src=4096, src_bs=img_in, dst=8192, dst_bs=img_out, pooled=12288, pooled_bs=img_p):
        sp, sc, sb = _arrays(L, [src], [cin], [src_bs])
        rc = lib.ynet_conv2d_pool(sp, sc, sb, 1, vp(256), None, vp(dst), cout, dst_bs, vp(pooled), pooled_bs, B, H, W, 3, 1, None)
        return rc, lib.ynet_last_error()

    for kw, word in ((dict(src=4100), b"source 0"), (dict(src=4104), b"source 0"), (dict(src_bs=img_in + 2), b"source 0"), (dict(dst=8200), b"destination"),
                     (dict(dst_bs=img_out + 2), b"destination"), (dict(pooled=12292), b"pooled"), (dict(pooled_bs=img_p + 1), b"pooled")):
        rc, msg = pool(**kw)
        assert rc != 0 and word in msg and b"launch failed" not in msg, (kw, msg)

    def add(src=4096, dst=8192, addend=12288, addend_bs=img_out):
        sp, sc, sb = _arrays(L, [src], [cin], [img_in])
        rc = lib.ynet_conv2d_add(sp, sc, sb, None, 1, vp(256), None, vp(dst), cout, img_out, B, H, W, 3, 1, vp(addend), addend_bs, 0, None)
        return rc, lib.ynet_last_error()

    for kw, word in ((dict(addend=12292), b"addend"), (dict(addend=12296), b"addend"), (dict(addend_bs=img_out + 2), b"addend"), (dict(src=4104), b"source 0"),
                     (dict(dst=8200), b"destination")):
        rc, msg = add(**kw)
        assert rc != 0 and word in msg and b"launch failed" not in msg, (kw, msg)

    def dgrad_relu(relu_of=12288, relu_of_bs=img_in):
        rc = lib.ynet_conv2d_dgrad_relu(vp(4096), cout, img_out, None, 0, vp(256), vp(8192), cin, img_in, vp(relu_of), relu_of_bs, B, H, W, 3, None, 0, None)
        return rc, lib.ynet_last_error()

    for kw in (dict(relu_of=12292), dict(relu_of=12296), dict(relu_of=12300), dict(relu_of_bs=img_in + 1), dict(relu_of_bs=img_in + 2)):
        rc, msg = dgrad_relu(**kw)
        assert rc != 0 and b"relu_of" in msg and b"launch failed" not in msg, (kw, msg)

    sp, sc, sb = _arrays(L, [4104], [cin], [img_in])
    assert lib.ynet_conv2d_relu_bits(sp, sc, sb, 1, vp(256), None, vp(8192), cout, img_out, vp(16384), B, H, W, 3, None) != 0
    assert b"source 0" in lib.ynet_last_error()
    assert lib.ynet_conv2d_dgrad_relu_bits(vp(4100), cout, img_out, None, 0, vp(256), vp(8192), cin, img_in, vp(16384), B, H, W, 3, None) != 0
    assert b"source 0" in lib.ynet_last_error()
    assert lib.ynet_conv2d_dgrad_relu_bits(vp(4096), cout, img_out, vp(20484), img_out, vp(256), vp(8192), cin, img_in, vp(16384), B, H, W, 3, None) != 0
    assert b"mask" in lib.ynet_last_error()


def test_direct_winograd_entry_points_refuse_planes_off_their_boundary():
    """ynet_conv2d_auto never sends such operands there (the plan tests above); a direct caller is told."""
    L = pkg("_lib")
    lib = L.load()
    vp = ctypes.c_void_p
    B, H, W, c = 8, 128, 128, 32
    img = c * H * W
    for src, src_bs, dst, dst_bs in ((4100, img, 8192, img), (4104, img, 8192, img), (4096, img + 2, 8192, img), (4096, img, 8196, img), (4096, img, 8192, img + 1)):
        assert lib.ynet_conv2d_winograd(vp(src), src_bs, vp(256), None, vp(dst), dst_bs, c, c, B, H, W, 1, None) != 0
        assert b"16-byte (input, filters) / 8-byte (output) aligned" in lib.ynet_last_error()
    for relu_of, bs in ((12292, img), (12288, img + 1)):
        assert lib.ynet_conv2d_winograd_dgrad_relu(vp(4096), img, vp(256), vp(8192), img, vp(relu_of), bs, c, c, B, H, W, None) != 0
        assert b"activation must be 8-byte aligned" in lib.ynet_last_error()
    sp, sc, sb = _arrays(L, [4096, 8200], [32, 16], [img, img // 2])
    assert lib.ynet_conv2d_winograd_cat(sp, sc, sb, 2, vp(256), None, vp(16384), img, 32, B, H, W, 1, None) != 0
    assert b"source 1 must be 16-byte aligned" in lib.ynet_last_error()
    sp, sc, sb = _arrays(L, [4096, 8192], [32, 16], [img, img // 2])
    for addend, bs in ((20484, img), (20480, img + 1)):
        assert lib.ynet_conv2d_winograd_cat_add(sp, sc, sb, 2, vp(256), None, vp(16384), img, 32, B, H, W, 1, vp(addend), bs, 0, None) != 0
        assert b"additive term must be 8-byte aligned" in lib.ynet_last_error()
    assert lib.ynet_upsample2x_conv2d_winograd(vp(4104), 32 * 64 * 64, vp(256), None, vp(8192), 16 * H * W, 32, 16, B, H, W, 0, None) != 0
    assert b"aligned" in lib.ynet_last_error()


def test_lora_conv2d_wgrad_refuses_a_source_off_16_bytes_on_the_host():
    L = pkg("_lib")
    lib = L.load()
    vp = ctypes.c_void_p
    B, H, W, cs, cout = A.LORA_CASE
    cin = sum(cs)
    for src, bs in ((4100, cin * H * W), (4104, cin * H * W), (4096, cin * H * W + 2)):
        sp, sc, sb = _arrays(L, [src], [cin], [bs])
        rc = lib.ynet_lora_conv2d_wgrad(sp, sc, sb, 1, vp(8192), cout * H * W, None, 0, vp(256), vp(512), 1.0, vp(1024), vp(2048), vp(12288), B, H, W, cout, 3, 1, None)
        assert rc != 0 and b"source 0 is not 16-byte aligned" in lib.ynet_last_error()

"""The up-convolution's low-resolution data gradient through the C ABI alone (include/ynet_hip.h: ynet_upconv_tables, ynet_conv2d_auto with
YNET_AUTO_UPCONV_BWD): declared, bound, exported, and its argument checks answered on the host, before any launch."""
import ctypes
import os
import re

from conftest import ROOT, pkg


def _header():
    with open(os.path.join(ROOT, "include", "ynet_hip.h")) as f:
        return f.read()


def test_header_declares_the_tables_entries_and_the_form():
    h = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"long long ynet_upconv_tables_floats\(int cout, int cin, long long\* keff_floats, long long\* table_floats\);", h)
    assert re.search(r"int ynet_upconv_tables\(const float\* w, int cout, int cin, float\* keff_packed, float\* tables, void\* stream\);", h)
    m = re.search(r"#define YNET_AUTO_UPCONV_BWD (\d+)u", h)
    assert m and int(m.group(1)) == 64
    flags = [int(v) for v in re.findall(r"#define YNET_AUTO_\w+ (\d+)u", h)]
    assert len(set(flags)) == len(flags) and all(v & (v - 1) == 0 for v in flags)      # one bit each


def test_lib_binds_and_the_library_exports_them():
    L = pkg("_lib")
    for n in ("ynet_upconv_tables", "ynet_upconv_tables_floats"):
        assert n in L.SIGNATURES and n in L.header_symbols()
    assert L.AUTO_UPCONV_BWD == 64
    lib = ctypes.CDLL(L.LIB_PATH)
    assert hasattr(lib, "ynet_upconv_tables") and hasattr(lib, "ynet_upconv_tables_floats")


def test_table_sizes_follow_the_packed_layout():
    L = pkg("_lib")
    lib = L.load()
    for cout, cin in ((16, 32), (32, 64), (8, 24), (16, 40), (1, 1), (3, 70)):
        kf, tf = ctypes.c_longlong(-1), ctypes.c_longlong(-1)
        total = lib.ynet_upconv_tables_floats(cout, cin, ctypes.byref(kf), ctypes.byref(tf))
        assert kf.value == lib.ynet_packed_weight_floats(4 * cout, cin, 3, 1)      # ynet_pack_weight(Keff [4 cout][cin][3][3], mode 1)
        assert tf.value == 16 * 4 * cout * cin and total == kf.value + tf.value
        assert lib.ynet_upconv_tables_floats(cout, cin, None, None) == total
    assert lib.ynet_upconv_tables_floats(0, 4, None, None) < 0 and lib.ynet_upconv_tables_floats(4, 0, None, None) < 0


def test_tables_entry_checks_its_arguments_before_launching():
    L = pkg("_lib")
    lib = L.load()
    vp = ctypes.c_void_p
    assert lib.ynet_upconv_tables(None, 16, 32, vp(256), vp(256), None) != 0 and b"null" in lib.ynet_last_error()
    assert lib.ynet_upconv_tables(vp(256), 16, 32, None, vp(256), None) != 0 and b"null" in lib.ynet_last_error()
    assert lib.ynet_upconv_tables(vp(256), 0, 32, vp(256), vp(256), None) != 0 and b"cout 0" in lib.ynet_last_error()
    assert lib.ynet_upconv_tables(vp(256), 16, -1, vp(256), vp(256), None) != 0 and b"cin -1" in lib.ynet_last_error()


def _desc(L, B=32, h=128, w=128, cout=16, cin=32, relu_of=True, **extra):
    d = L.ConvAuto()
    d.nsrc = d.ndst = 1
    d.src[0], d.src_c[0], d.src_bs[0] = 256, 4 * cout, 4 * cout * h * w
    d.dst[0], d.dst_c[0], d.dst_bs[0] = 512, cin, cin * h * w
    if relu_of:
        d.relu_of, d.relu_of_bs = 768, cin * h * w
    d.wp, d.B, d.H, d.W, d.K, d.flags = 1024, B, h, w, 3, L.AUTO_UPCONV_BWD
    for k, v in extra.items():
        setattr(d, k, v)
    return d


def test_the_form_plans_on_the_host():
    """C2's decoder level 4 (B 32, cout 16, cin 32, 128^2 low resolution): the plan of the low-resolution data gradient is the one ynet_conv2d_auto_plan gives
    the same call with a packed effective filter, plus the ring launch; the cache covers Keff, the 16 tables and that plan's transforms."""
    L = pkg("_lib")
    lib = L.load()
    for B, h, w, relu_of in ((32, 128, 128, True), (32, 128, 128, False), (8, 5, 7, True), (3, 33, 17, False), (1, 2, 2, True)):
        d, tk = _desc(L, B, h, w, relu_of=relu_of), L.ConvTaken()
        assert lib.ynet_conv2d_auto_plan(ctypes.byref(d), ctypes.byref(tk)) == 0, lib.ynet_last_error()
        p, tp = _desc(L, B, h, w, relu_of=relu_of), L.ConvTaken()
        p.flags = 0
        assert lib.ynet_conv2d_auto_plan(ctypes.byref(p), ctypes.byref(tp)) == 0, lib.ynet_last_error()
        assert (tk.family, tk.variant, tk.nlaunch) == (tp.family, tp.variant, tp.nlaunch + 1)
        kf, tf = ctypes.c_longlong(0), ctypes.c_longlong(0)
        lib.ynet_upconv_tables_floats(16, 32, ctypes.byref(kf), ctypes.byref(tf))
        inner = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(p))
        assert lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d)) == (kf.value + 3) // 4 * 4 + (tf.value + 3) // 4 * 4 + inner
    d, tk = _desc(L), L.ConvTaken()
    assert lib.ynet_conv2d_auto_plan(ctypes.byref(d), ctypes.byref(tk)) == 0
    assert (tk.family, tk.variant, tk.nlaunch) == (3, 22, 2)      # (C2's shape: one slice-form launch over the 64 space-to-depth channels, then the ring)


def test_the_form_refuses_what_it_does_not_serve():
    L = pkg("_lib")
    lib = L.load()
    cache = (ctypes.c_ulonglong * 2)(0, 0)
    cases = {
        "two sources": dict(nsrc=2),
        "two destinations": dict(ndst=2),
        "upsample2x": dict(upsample2x=1),
        "pooled": dict(pooled=2048, pooled_bs=16),
        "addend": dict(addend=2048, addend_bs=16),
        "bias": dict(bias=2048),
        "relu": dict(relu=1),
        "mask": dict(mask=2048, mask_bs=16),
        "odd channels": dict(src_c=(ctypes.c_int * 4)(62, 0, 0, 0)),
        "1x1": dict(K=1),
        "one row": dict(H=1),
        "too wide for the ring": dict(src_c=(ctypes.c_int * 4)(128, 0, 0, 0), src_bs=(ctypes.c_longlong * 4)(128 * 128 * 128, 0, 0, 0),
                                      dst_c=(ctypes.c_int * 4)(64, 0, 0, 0), dst_bs=(ctypes.c_longlong * 4)(64 * 128 * 128, 0, 0, 0)),
    }
    for what, extra in cases.items():
        d, tk = _desc(L, **extra), L.ConvTaken()
        d.cache, d.cache_floats, d.cache_tag = 4096, 1 << 30, cache
        assert lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), None) != 0, what
        msg = lib.ynet_last_error()
        assert b"upconv_bwd" in msg, (what, msg)
        assert lib.ynet_conv2d_auto_plan(ctypes.byref(d), ctypes.byref(tk)) != 0, what
        assert lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d)) < 0, what
    assert tuple(cache) == (0, 0)      # nothing was made
    # a cache that is missing or too small is refused before the tables are made
    d, tk = _desc(L), L.ConvTaken()
    assert lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), None) != 0 and b"cache" in lib.ynet_last_error()
    need = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d))
    d.cache, d.cache_floats, d.cache_tag = 4096, need - 4, cache
    assert lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), None) != 0 and b"%d floats" % need in lib.ynet_last_error()
    d.wp = None
    d.cache_floats = need
    assert lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), None) != 0 and b"raw filter" in lib.ynet_last_error()
    assert tuple(cache) == (0, 0)

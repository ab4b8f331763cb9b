"""tests/_wgrad_cases.py on the CPU: every row's plan (ynet_conv2d_wgrad_plan is host code) is what the row claims, every edge of the sweep is reached, the workspace
formula covers what every plan writes, and the references are what the GPU test may hold the kernels to."""
import itertools

import pytest
import torch

import _align_cases as A
import _wgrad_cases as C
from conftest import pkg


@pytest.fixture(scope="module")
def libs():
    L = pkg("_lib")
    return L.load(), L


@pytest.fixture(scope="module")
def plans(libs):
    lib, L = libs
    return {name: C.case_plan(lib, L, name) for name in C.CASES}


@pytest.mark.parametrize("name", list(C.CASES))
def test_row_plans_what_it_claims(plans, name):
    shape, kernel, claims, edges, opts = C.CASES[name]
    p = plans[name]
    assert p["kernel"] == kernel, (name, p)
    for key, want in claims.items():
        got = C.cursor(p) if key == "cursor" else p[key]
        assert got == want, (name, key, got, want)
    assert p["rows"] == {1: 4, 2: 2, 3: 2, 4: 0}[kernel]
    if kernel != 3:
        assert p["seg"] == p["nseg_y"] == p["nsegs"] == 0
    else:
        assert p["nsplit"] <= p["nsegs"] and p["nseg_y"] == -(-p["tiles_y"] // p["seg"]) and p["tiles_y"] >= 2
    assert (p["ct"] != 0) == (kernel == 4)
    if kernel == 2:
        assert C.cursor_carries(p)[2], name      # (the cursor as the kernel walks it visits every tile once)
    for e in edges:
        assert C.EDGES[e](shape, p), (name, e, p)
        if e in C.OPTION_EDGES:
            assert C.OPTION_EDGES[e] in opts, (name, e)
    assert set(opts) <= {"shared", "slice", "misplace"}
    if len(shape[3]) > 1:
        assert "slice" in opts and opts["slice"] != opts.get("shared"), name      # one source of every multi-source row is a slice of a wider tensor
    if "misplace" in opts:
        assert C.aligned_of(name) == 0 and kernel == 1


def test_every_edge_is_reached_and_no_row_is_spare(plans):
    claimed = {e for _, _, _, edges, _ in C.CASES.values() for e in edges}
    assert claimed == set(C.EDGES), claimed ^ set(C.EDGES)
    per_kernel = {k: sum(1 for c in C.CASES.values() if c[1] == k) for k in (1, 2, 3, 4)}
    assert per_kernel == C.ROWS_PER_KERNEL
    # both carries of the two-row cursor, by walking it
    assert any(C.cursor_carries(p)[0] > 0 for p in plans.values() if p["kernel"] == 2)
    assert any(C.cursor_carries(p)[1] > 0 for p in plans.values() if p["kernel"] == 2)
    # reduce_partials_kernel: the split counts on both sides of its unrolled-by-32 loop, and an output longer than its grid covers in one pass
    ns = {p["nsplit"] for p in plans.values()}
    assert 1 in ns and ns & set(range(2, 8)) and ns & set(range(9, 25)) and ns & set(range(25, 33)) and any(n > 32 and n % 32 for n in ns)
    assert any(s[4] * sum(s[3]) * s[5] ** 2 > 4096 * 32 for s, *_ in C.CASES.values())
    assert sum(1 for c in C.CASES.values() if "shared" in c[4]) == 1 and sum(1 for c in C.CASES.values() if "misplace" in c[4]) == 1
    # the unmasked rolling-row kernel and its segment lengths
    rolls = [(C.shape_of(n), p) for n, p in plans.items() if p["kernel"] == 3]
    assert {p["seg"] for s, p in rolls if not s[6]} == {4, 8, 16}


def test_workspace_covers_every_plan(libs, plans):
    lib, L = libs
    exact = [n for n, p in plans.items() if p["partial_floats"] == p["workspace_floats"]]
    for n, p in plans.items():
        assert 0 < p["partial_floats"] <= p["workspace_floats"], (n, p)
        B, H, W, cs, cout, K, masked, bias = C.shape_of(n)
        p0 = C.case_plan(lib, L, n, want_bias=0)
        assert p["partial_floats"] - (p["nsplit"] * cout if bias else 0) == p0["partial_floats"] == p["nsplit"] * cout * sum(cs) * K * K
    assert {"roll_seg_8", "roll_unmasked_85", "roll_unmasked_768"} <= set(exact), exact
    # a wider grid of shapes: any alignment, mask and bias
    for B, H, W, (cs, cout), K in itertools.product([1, 2, 3, 5, 12, 16, 768], [1, 2, 4, 5, 10, 18, 34, 64], [1, 4, 32, 36, 64, 96, 100],
                                                    [([1], 1), ([5], 3), ([32], 16), ([32], 32), ([6, 8], 32), ([33], 17), ([64, 33], 64), ([65], 65), ([130], 130)], [1, 3, 5]):
        for masked, aligned in itertools.product([0, 1], [0, 1]):
            p = C.plan(lib, L, B, H, W, cs, cout, K, masked, aligned, 1)
            assert p["partial_floats"] <= p["workspace_floats"], (B, H, W, cs, cout, K, masked, aligned, p)
            # off a 16-byte boundary, and at K 5, the staged tiles are all there is; W % 4 != 0 keeps a 3 x 3 off the LDS-DMA kernels (the 1x1 streaming kernel
            # reads a plane as one run of 16-pixel chunks: it asks for H W % 16 == 0, which a map with W % 4 != 0 can meet)
            if not aligned or K == 5 or (W % 4 != 0 and (K == 3 or (H * W) % 16 != 0)):
                assert p["kernel"] == 1, (B, H, W, cs, cout, K, masked, aligned, p)
            assert p["kernel"] != 4 or (K == 1 and not masked and cs == [32] and cout <= 32 and (H * W) % 16 == 0)
            assert (p["kernel"] in (2, 3)) == (K == 3 and aligned == 1 and W % 4 == 0)


def test_plan_refuses_what_the_call_refuses(libs):
    import ctypes
    lib, L = libs
    p, one = L.WgradPlan(), (ctypes.c_int * 1)(4)
    assert lib.ynet_conv2d_wgrad_plan(1, 4, 4, 4, one, 1, 7, 0, 1, 1, ctypes.byref(p)) != 0 and b"kernel size" in lib.ynet_last_error()
    assert lib.ynet_conv2d_wgrad_plan(0, 4, 4, 4, one, 1, 3, 0, 1, 1, ctypes.byref(p)) != 0
    assert lib.ynet_conv2d_wgrad_plan(1, 4, 4, 4, one, 5, 3, 0, 1, 1, ctypes.byref(p)) != 0 and b"sources" in lib.ynet_last_error()
    assert lib.ynet_conv2d_wgrad_plan(1, 4, 4, 4, one, 1, 3, 0, 1, 1, None) != 0


def test_the_rolling_row_cases_of_the_kernel_suite(libs):
    """tests/test_gpu_kernels.py::ROLL_WGRAD_CASES names the kernel each shape takes: the plan agrees (the GPU test reads the launch note)."""
    import test_gpu_kernels as T
    lib, L = libs
    assert len(T.ROLL_WGRAD_CASES) == len(T.ROLL_WGRAD_KERNEL) == 7
    for (B, H, W, cs, cout, relu, bias), kernel in zip(T.ROLL_WGRAD_CASES, T.ROLL_WGRAD_KERNEL):
        assert C.plan(lib, L, B, H, W, cs, cout, 3, relu, 1, bias)["kernel"] == kernel, (B, H, W, cs, cout)
    unmasked = [c for c, k in zip(T.ROLL_WGRAD_CASES, T.ROLL_WGRAD_KERNEL) if k == 3 and not c[5]]
    assert (12, 64, 64, [64], 64, False, True) in unmasked and (3, 256, 256, [32], 32, False, False) in unmasked


@pytest.mark.parametrize("name", list(C.CASES))
def test_references(name):
    B, H, W, cs, cout, K, masked, bias = C.shape_of(name)
    assert 9 * B * H * W < 2 ** 24      # family (b): |x|, |dy| <= 3, so every partial sum of products is an integer below 2^24
    b = C.inputs(name, "b")
    for t in b.xs + [b.dy]:
        assert torch.equal(t, t.round()) and float(t.abs().max()) <= 3
    dw, db = C.ref64(name, "b")
    for t in (dw, db):
        assert torch.equal(t, t.round()) and float(t.abs().max()) < 2 ** 24
        assert torch.equal(t.float().double(), t)
    if masked:
        for fam in "ab":
            m = C.inputs(name, fam).mask
            flat = set(m.flatten().tolist())
            assert {-1.0, 0.0, C.FLT_MIN, 1.0, 2.0} <= flat, (name, fam)
            assert bool((torch.signbit(m) & (m == 0)).any()) and bool((~torch.signbit(m) & (m == 0)).any())      # -0.0 and +0.0
            assert 0.2 < float((m > 0).float().mean()) < 0.8
    # family (a): a correct fp32 implementation (stock conv2d backward on the CPU) reaches the project's tolerance against fp64 at these sizes
    a = C.inputs(name, "a")
    dw64, db64 = C.ref64(name, "a")
    dw32, db32 = C.reference(a, K, torch.float32)
    assert A.mismatch(dw32, dw64, **A.TOL_DW)[0] == 0 and A.mismatch(db32, db64, **A.TOL_DW)[0] == 0
    assert float(dw64.abs().max()) > 0 and dw64.shape == (cout, sum(cs), K, K)

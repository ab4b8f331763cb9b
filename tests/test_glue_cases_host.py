"""The case table of the glue-kernel edge sweep (tests/_glue_cases.py), checked on the CPU: the inputs are what the device tests assume
(ties only where planted, finite references, known answers that are known), and every stated bound is reachable by a correct fp32
implementation -- torch's own fp32 CPU kernels stay inside it."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import _glue_cases as G


def _within(got, want, rtol, atol):
    got, want = got.detach().double(), want.detach().double()
    err = (got - want).abs()
    return bool((err <= atol + rtol * want.abs()).all()), float(err.max())


# ---- soft-argmax -------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [s for s, _, _ in G.SOFT_SHAPES], ids=str)
def test_softargmax_known_answers_are_known(shape):
    """The fp64 reference lands on the planted (col, row).  Its eps = 1e-6 denominator is part of it: one logit of +60 over zeros gives
    (col, row) / (1 + eps) -- col * 1e-6 away from the integer, 2e-3 px at column 2047 -- so the condition is on reference * (1 + eps),
    which must be within 1e-6 px of the planted position (it is within 1e-12: the background weighs H W e^-60)."""
    H, W = shape
    x, pos = G.soft_known(H, W)
    assert x.shape[1] == len(G.soft_planted(H, W)) >= 1
    ref = G.soft_ref(x)[0]
    assert bool(torch.isfinite(ref).all())
    assert float((ref * (1.0 + G.EPS) - pos).abs().max()) <= 1e-6
    # every walk-relevant position is there: the corners, the end of row 0, the start of row 1, the last element
    for p in [(0, 0), (W - 1, 0), (0, H - 1), (W - 1, H - 1)]:
        assert p in G.soft_planted(H, W)


def test_softargmax_sweep_covers_every_walk_and_has_finite_references():
    shapes = {s: rec for s, _, rec in G.SOFT_SHAPES}
    for s in [(1, 1), (1, 3), (96, 160), (160, 224), (512, 512), (8, 1028), (8, 2048), (1, 20)]:
        assert s in shapes
    assert {W for (_, W) in shapes if W in (4, 8, 12)} == {4, 8, 12}
    assert any(W % 4 and H * W > 256 for (H, W) in shapes)
    for (H, W), rec in shapes.items():
        assert (rec is not None) == (H > 256 or W > 256), (H, W)
        worst = 0.0
        for kind in G.SOFT_KINDS:
            x = G.soft_logits(H, W, kind)
            assert x.dtype == torch.float32 and bool(torch.isfinite(G.soft_ref(x)).all())
            worst = max(worst, G.soft_e_ref(x))
        if rec is not None:         # the recorded yardstick is what this machine measures too (summation order may differ a little)
            assert rec / 4 <= worst <= rec * 4, ((H, W), worst, rec)
    assert float(G.soft_logits(8, 8, "offset+1e4").min()) > 9e3 and float(G.soft_logits(8, 8, "offset-1e4").max()) < -9e3


def test_readout_reference_is_the_elementwise_chain_in_fp64():
    tm, gm = G.randn(2, 3, 8, 12, key=1, scale=3.0), G.randn(2, 4, 8, 12, key=2, scale=3.0)
    gt = G.uniform(2, 3, 2, key=3) * 8
    pt, pg, ade, fde = G.readout_ref(tm, gm, gt, 0.25)
    assert pt.dtype == torch.float64 and pt.shape == (2, 3, 2) and pg.shape == (2, 1, 2)
    want = torch.stack([torch.stack([torch.linalg.norm((gt[b, p].double() - pt[b, p]) / 0.25) for p in range(3)]).mean() for b in range(2)])
    assert torch.allclose(ade, want, rtol=1e-14, atol=0)
    assert torch.allclose(fde, torch.stack([torch.linalg.norm((gt[b, -1].double() - pg[b, 0]) / 0.25) for b in range(2)]), rtol=1e-14, atol=0)


# ---- max-pool ----------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.POOL_EVEN + G.POOL_ODD, ids=str)
def test_maxpool_inputs_have_no_accidental_ties(case):
    """Outside the planted planes the four values of every 2 x 2 block are pairwise distinct in fp32: nothing is masked or skipped, the
    share of elements excluded from the bit-exact comparison is zero."""
    x = G.pool_planes(*case)
    assert x.dtype == torch.float32 and bool(torch.isfinite(x).all())
    b = G.pool_blocks(x)
    for i in range(4):
        for j in range(i + 1, 4):
            assert not bool((b[..., i] == b[..., j]).any()), (case, i, j)
    assert bool((x > 0).any()) and bool((x < 0).any())          # the ReLU mask has both sides to work on


def test_maxpool_planted_ties_and_the_reference_rule():
    """The planted planes hold what they claim, and torch's arg-max on them is the rule the kernels state: first maximum in scan order,
    a NaN wins (the last one of several)."""
    x = G.pool_tie_planes()
    b = G.pool_blocks(x)
    assert bool((b[0, 0, 0] == 1.5).all())
    zeros = [b[0, 0, 1], b[0, 1, 0], b[1, 0, 0], b[1, 0, 1]]
    signs = {tuple(torch.signbit(z).tolist()) for z in zeros}
    assert all(bool((z == 0).all()) for z in zeros) and len(signs) == 4          # +0 against -0 in four different orders
    assert bool(torch.isinf(b[0, 1, 1]).all()) and bool((b[0, 1, 1] < 0).all())
    assert [int(torch.isnan(b[2, i // 2, i % 2]).sum()) for i in range(4)] == [1, 1, 1, 1]
    assert bool(torch.isnan(b[3, 0, 0]).all())
    dy = G.randn(4, 2, 2, key=9)
    y, dx, arg = G.pool_ref(x, dy)
    assert arg.tolist() == [[[0, 0], [0, 0]], [[0, 0], [1, 0]], [[0, 1], [2, 3]], [[3, 2], [2, 0]]]
    assert torch.equal(torch.isnan(y), torch.tensor([[[False] * 2] * 2, [[False] * 2] * 2, [[True] * 2] * 2, [[True, True], [False, False]]]))
    # the gradient lands on that element only
    routed = G.pool_blocks(dx)
    for p in range(4):
        for i in range(2):
            for j in range(2):
                want = torch.zeros(4)
                want[arg[p, i, j]] = dy[p, i, j]
                assert torch.equal(routed[p, i, j], want)
    # the code byte restates the same arg-max next to the sign bits
    code = G.pool_code(x, arg)
    assert torch.equal(code & 3, arg.to(torch.uint8))
    assert int(code[0, 0, 0]) == 0 + 4 + 8 + 16 + 32 and int(code[0, 1, 1]) == 0 and int(code[2, 0, 0]) == 0 + 8 + 16 + 32


# ---- element-wise entries ----------------------------------------------------------------------
@pytest.mark.parametrize("case", G.SIG_CASES, ids=str)
def test_sigmoid_temp_bound_is_reachable_in_fp32(case):
    B, C, H, W, sel, T = case
    x = G.sig_input(B, C, H, W)
    ref = G.sig_ref(x, sel, T)
    assert ref.shape == (B, len(sel), H, W) and bool(torch.isfinite(ref).all())
    assert float(x.abs().max()) <= 90.0 and (x.numel() < 100 or float(x.abs().max()) > 80.0)
    ok, err = _within(torch.sigmoid(x[:, sel] / T), ref, G.SIG_RTOL, G.SIG_ATOL)
    assert ok, err


def test_sigmoid_temp_table_covers_the_launch_split():
    assert {len(c[4]) for c in G.SIG_CASES} >= {1, 8, 9, 17}
    assert {c[2] * c[3] for c in G.SIG_CASES} >= {1, 6, 4096, 65536}
    assert {c[5] for c in G.SIG_CASES} == {0.5, 1.0, 1.8}
    assert any(min(c[4]) < 0 for c in G.SIG_CASES) and any(len(set(c[4])) < len(c[4]) for c in G.SIG_CASES)


@pytest.mark.parametrize("n", G.BCE_N)
@pytest.mark.parametrize("target", G.BCE_TARGETS)
def test_bce_bounds_are_reachable_in_fp32(n, target):
    x, t = G.bce_inputs(n, target)
    assert float(x.abs().max()) <= 40.0
    loss, dx = G.bce_ref(x, t)
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(dx).all())
    xf = x.clone().requires_grad_(True)
    lf = F.binary_cross_entropy_with_logits(xf, t)
    lf.backward()
    ok, err = _within(lf, loss, G.BCE_LOSS_RTOL, 0.0)
    assert ok, ("loss", err)
    ok, err = _within(xf.grad, dx, G.BCE_GRAD_RTOL, G.bce_grad_atol(n))
    assert ok, ("gradient", err)
    if target != "uniform":
        assert set(t.unique().tolist()) == {0.0 if target == "zeros" else 1.0}


@pytest.mark.parametrize("case", G.BSUM_CASES, ids=str)
def test_batch_sum_bound_is_reachable_in_fp32(case):
    B, n, stride = case
    assert n % 4 == 0 and stride % 4 == 0 and stride >= n
    buf = G.bsum_input(B, n, stride)
    ref, bound = G.bsum_ref(buf, n)
    assert bool(torch.isfinite(ref).all()) and (stride == n or bool(torch.isnan(buf[:, n:]).all()))
    acc = buf[0, :n].clone()
    for b in range(1, B):
        acc += buf[b, :n]
    assert bool(((acc.double() - ref).abs() <= bound).all())
    if B == 1:
        assert float(bound.max()) == 0.0


def test_batch_sum_table_covers_the_issue():
    assert {c[0] for c in G.BSUM_CASES} == {1, 2, 33} and {c[1] for c in G.BSUM_CASES} == {4, 1028, G.BSUM_N_BIG}
    assert G.BSUM_N_BIG // 4 > 8192 * 256
    for n in (4, 1028, G.BSUM_N_BIG):
        assert {c[2] == n for c in G.BSUM_CASES if c[1] == n} == {True, False}


@pytest.mark.parametrize("n", G.ELEM_N)
def test_elementwise_inputs_and_references(n):
    a, b, dy, y = G.elem_inputs(n)
    for relu in (False, True):
        ref = G.add_relu_ref(a, b, relu)
        want = torch.relu(a + b) if relu else a + b
        assert torch.equal(torch.nan_to_num(ref, nan=12345.0), torch.nan_to_num(want, nan=12345.0))
        assert int(torch.isnan(ref).sum()) == (1 if n >= 3 else 0)
    ref = G.relu_bwd_ref(dy, y)
    assert bool(torch.isfinite(ref).all()) and torch.equal(ref, dy * (y > 0))
    if n >= 1000:
        assert bool((y == 0).any()) and bool(torch.isnan(y).any()) and bool(torch.signbit(y[y == 0]).any())
    assert min(G.ELEM_N) < G.GRID_CAP < max(G.ELEM_N)
    assert any(N * (-(-H // d) * d) * (-(-W // d) * d) > G.GRID_CAP for N, H, W, d in G.PAD_CASES)
    assert any(N * (-(-H // d) * d) * (-(-W // d) * d) < G.GRID_CAP for N, H, W, d in G.PAD_CASES)


@pytest.mark.parametrize("case", G.BN_CASES, ids=str)
def test_batchnorm_offset_cases_and_the_recorded_yardstick(case):
    """Every (mean, std) pair of the issue is a channel; the two-pass fp64 reference is finite; torch's own fp32 CPU batch norm against it
    is what the table records (within a factor of 4: thread count and vector width move an fp32 sum a little)."""
    B, C, H, W = case
    assert C == len(G.BN_MEANS) * len(G.BN_STDS)
    x, gamma, beta, gy = G.bn_inputs(B, C, H, W)
    m, s = x.double().mean(dim=(0, 2, 3)), x.double().std(dim=(0, 2, 3))
    for c in range(C):
        want_m, want_s = G.BN_MEANS[c // 2], G.BN_STDS[c % 2]
        assert abs(float(m[c]) - want_m) <= 0.1 * want_s + 1e-3 * abs(want_m) and 0.8 * want_s <= float(s[c]) <= 1.2 * want_s
    r64 = G.bn_ref(x, gamma, beta, gy)
    assert all(bool(torch.isfinite(v).all()) for v in r64.values())
    # the reference is two-pass: it agrees with torch's fp64 batch norm
    y64, m64, i64 = torch.native_batch_norm(x.double(), gamma.double(), beta.double(), None, None, True, 0.1, G.BN_EPS)
    assert torch.allclose(r64["save_invstd"], i64, rtol=1e-9, atol=0) and torch.allclose(r64["save_mean"], m64, rtol=1e-14, atol=0)
    live = G.bn_channel_err(G.bn_ref(x, gamma, beta, gy, torch.float32), r64)
    for k in G.BN_TENSORS:
        rec = torch.tensor(G.BN_TORCH_ERR[case][k], dtype=torch.float64)
        assert bool((live[k] <= 4 * rec + 1e-12).all()) and bool((rec <= 4 * live[k] + 1e-12).all()), (k, live[k].tolist(), rec.tolist())


def test_pyramid_and_upsample_tables():
    assert set(G.PYR_SHAPES) == {(32, 32), (32, 96), (160, 224), (512, 512)}
    assert sorted(b * c for b, c in G.PYR_PLANES) == [1, 300] and len(G.PYR_BWD) == 3
    for B, C, H, W in G.PYR_BWD:
        assert (H, W) in G.PYR_SHAPES
        grads = [None] + [G.randn(B, C, H >> l, W >> l, key=40 + l) for l in range(1, 6)]
        dx = G.pyramid_bwd_ref((B, C, H, W), grads)
        assert dx.shape == (B, C, H, W) and bool(torch.isfinite(dx).all())
        want = sum(F.interpolate(g.double(), scale_factor=2 ** l, mode="nearest") / 4 ** l for l, g in enumerate(grads) if g is not None)
        assert torch.allclose(dx, want, rtol=1e-13, atol=1e-15)
    x = G.randn(2, 1, 32, 96, key=41)
    ref = G.pyramid_ref(x, 6)
    assert [tuple(r.shape[2:]) for r in ref] == [(32 >> i, 96 >> i) for i in range(6)] and all(bool(torch.isfinite(r).all()) for r in ref)
    assert G.UP_MANY[0] > 65535
    offs = {o for t in G.UP_FWD_OFFSETS + G.UP_BWD_OFFSETS for o in t}
    assert offs == {0, 1, 2}
    for shape in G.UP_SHAPES[:4]:
        B, C, H, W = shape
        y, dx, dxr = G.up_ref(G.randn(*shape, key=42), G.randn(B, C, 2 * H, 2 * W, key=43), torch.relu(G.randn(*shape, key=44)))
        assert bool(torch.isfinite(y).all()) and bool(torch.isfinite(dx).all()) and bool((dxr == 0).any())

"""tests/_sampling_cases.py means what it says (CPU only): the multinomial rows plant what their names promise, kmeans_rule is the oracle's
Lloyd iteration bit for bit, cws_rule is the reference's Gaussian within the fp32 oracle's own error, and ynet_kmeans2d refuses on the host
the calls that could not end or would not fit (before any launch: nothing here touches a GPU)."""
import ctypes
import math

import numpy as np
import pytest
import torch

import _sampling_cases as S
from conftest import pkg
from oracle import ynet_oracle as O


# ------------------------------------------------------------------------------------------------
# multinomial
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.MULTI_NAMES)
def test_the_oracle_runs_on_every_row_and_draws_positive_entries(name):
    _, prob, K, replacement, thr, seed = S.multi_row(name)
    want = S.multi_want(name)
    assert want.shape == (prob.shape[0], K) and want.dtype == torch.int64
    assert bool((prob.gather(1, want) > 0).all())
    if not replacement:
        assert all(len(set(r.tolist())) == K for r in want)
    assert seed >> 32 != 0 and seed & 0xFFFFFFFF != 0       # both key words of the generator are in use


@pytest.mark.parametrize("name,residues", [("one_thread", {7}), ("two_threads", {7, 200})])
def test_planted_residues_hold_every_winner(name, residues):
    """All 48 winners sit in one (two) of the 256 per-thread lists: the list fills to depth 48 (at least 24) and its head advances as often."""
    _, prob, K, _, _, _ = S.multi_row(name)
    assert prob.shape[1] == 256 * 60 and K == 48
    pos = torch.nonzero(prob[0] > 0).flatten()
    assert set((pos % S.TOPK_THREADS).tolist()) == residues and len(pos) == 60 * len(residues)
    want = S.multi_want(name)
    assert set((want % S.TOPK_THREADS).flatten().tolist()) == residues
    for r in want:
        assert max(np.bincount((r % S.TOPK_THREADS).numpy())) >= K // len(residues)


def test_rows_with_exactly_K_positive_entries_return_that_set():
    pos = S.exact_positions().tolist()
    assert len(pos) == S.EXACT_K == len(set(pos))
    for r in S.multi_want("exactly_K"):
        assert sorted(r.tolist()) == pos
    _, prob, K, _, _, _ = S.multi_row("n48_K48")
    assert prob.shape[1] == K == 48 and bool((prob > 0).all())
    for r in S.multi_want("n48_K48"):
        assert sorted(r.tolist()) == list(range(48))
    assert S.multi_want("n1_K1").tolist() == [[0], [0]]


def test_denormal_row_is_positive_in_float32():
    _, prob, K, _, thr, _ = S.multi_row("denormal")
    assert prob.dtype == torch.float32 and thr is None
    pos = prob[prob != 0]
    assert pos.numel() == 2 * 30 and bool((pos > 0).all()) and bool((pos < torch.finfo(torch.float32).tiny).all())
    assert bool((pos.numpy().view(np.uint32) >> 23 == 0).all())      # exponent field 0: denormal
    for r, p in zip(S.multi_want("denormal"), prob):
        assert len(set(r.tolist())) == K and bool((p[r] > 0).all())


def test_threshold_rows_draw_the_argmax():
    for name in ("thr_1.0", "thr_keeps_max_only"):
        _, prob, K, _, thr, _ = S.multi_row(name)
        assert thr == 1.0
        assert torch.equal(S.multi_want(name), prob.argmax(dim=1, keepdim=True).expand(-1, K))


def test_mass_in_one_element_is_drawn_every_time():
    assert bool((S.multi_want("rep_mass_first") == 0).all()) and bool((S.multi_want("rep_mass_last") == 999).all())
    assert bool((S.multi_want("rep_n1") == 0).all())


def test_status_rows_make_the_oracle_raise():
    for name in S.STATUS_NAMES:
        _, prob, K, replacement, thr, seed = S.multi_row(name)
        with pytest.raises(RuntimeError, match="invalid multinomial"):
            O.device_multinomial(prob, K, replacement, thr, seed)
    _, prob, K, _, _, _ = S.multi_row("too_few")
    assert K == S.EXACT_K + 1 and all(int((p > 0).sum()) == S.EXACT_K for p in prob)
    _, prob, _, replacement, _, _ = S.multi_row("zero_last")
    assert replacement and prob.shape[0] == 4 and float(prob[3].abs().sum()) == 0.0 and bool((prob[:3] > 0).all())
    assert S.multi_want("zero_last").shape == (3, 40)


# ------------------------------------------------------------------------------------------------
# k-means
# ------------------------------------------------------------------------------------------------
def _from_the_numpy_stream(name):
    return S.KMEANS_CASES[name][6] not in ("lattice", "duplicate")


@pytest.mark.parametrize("name", [n for n in S.KMEANS_CASES if _from_the_numpy_stream(n)])
def test_kmeans_rule_is_the_oracle_bit_for_bit(name):
    """Same np.random.seed, same np.random.choice order.  K >= 2 (the oracle's .squeeze() breaks argmin at K = 1) and N * max coordinate
    < 2^24 (beyond that the reference's fp32 mean depends on its summation order)."""
    P, N, K, maxc, tol, limit, _ = S.KMEANS_CASES[name]
    pts, init, _, _, seed = S.kmeans_case(name)
    assert tuple(pts.shape) == (P, N, 2) and tuple(init.shape) == (P, K) and init.dtype == torch.int32
    assert float(pts.min()) >= 0 and float(pts.max()) < maxc and torch.equal(pts, pts.round())
    np.random.seed(seed)
    drawn = np.stack([np.random.choice(N, K, replace=False) for _ in range(P)])
    assert np.array_equal(drawn, init.numpy())
    want, _, empty, _ = S.kmeans_want(name)
    assert not any(empty)
    if K < 2:
        return
    assert N * maxc < 2 ** 24
    np.random.seed(seed)
    ref = torch.stack([O.kmeans_lloyd(pts[p], K, tol, limit) for p in range(P)])
    assert torch.equal(want, ref), float((want - ref).abs().max())


def test_kmeans_shapes_cover_the_edges():
    shapes = {n: c[:3] for n, c in S.KMEANS_CASES.items()}
    assert shapes["K1"][2] == 1 and shapes["lds_limit_18000_32"][1:] == (18000, 32) and shapes["below_1024_threads"][1] < 1024
    assert shapes["N_equals_K"][1] == shapes["N_equals_K"][2] and shapes["many_workgroups"][0] >= 256
    _, it, _, _ = S.kmeans_want("N_equals_K")
    assert it == [1, 1, 1]          # every point is its own centre: one iteration, shift 0
    want, _, _, _ = S.kmeans_want("K1")
    pts, _, _, _, _ = S.kmeans_case("K1")
    assert torch.equal(want[:, 0], (pts.double().sum(dim=1).float() / pts.shape[1]))


def test_only_the_dedicated_case_has_an_empty_cluster():
    for name in S.KMEANS_CASES:
        _, _, empty, _ = S.kmeans_want(name)
        assert empty == S.KMEANS_EMPTY.get(name, [False] * len(empty)), name


def test_lattice_has_ties_in_its_first_assignment():
    pts, init, _, _, _ = S.kmeans_case("lattice")
    assert pts[0, init[0, 0]].tolist() == [2.0, 2.0] and pts[0, init[0, 1]].tolist() == [6.0, 2.0]
    want, it, empty, ties = S.kmeans_want("lattice")
    assert ties[0] >= 1
    assert (ties[0], it[0], want[0].tolist()) == (S.LATTICE_WANT["ties"], S.LATTICE_WANT["iterations"], S.LATTICE_WANT["centres"])
    # with "last minimum wins" the column x = 4 would go to the right-hand cluster: the answer depends on the tie rule
    assert want[0].tolist() != [[1.5, 2.0], [6.0, 2.0]]


def test_iteration_limits_stop_exactly_there():
    _, free, _, _ = S.kmeans_want("blobs_10000_19")
    for name, limit in (("iter_limit_1", 1), ("iter_limit_3", 3)):
        assert S.KMEANS_CASES[name][5] == limit
        assert torch.equal(S.kmeans_case(name)[0], S.kmeans_case("blobs_10000_19")[0])
        _, it, _, _ = S.kmeans_want(name)
        assert it == [limit] * len(it)
        assert all(f > limit for f in free)
        assert not torch.equal(S.kmeans_want(name)[0], S.kmeans_want("blobs_10000_19")[0])


def _kmeans_call(lib, P=1, N=100, K=4, tol=1e-3, limit=1000):
    vp = ctypes.c_void_p
    rc = lib.ynet_kmeans2d(vp(256), vp(512), vp(768), vp(1024), P, N, K, tol, limit, None)
    return rc, lib.ynet_last_error()


def test_kmeans_entry_refuses_before_any_launch():
    """Dummy non-null pointers: every call below must return before it launches (a launch would read them)."""
    lib = pkg("_lib").load()
    for tol in (0.0, -1e-3, math.nan):
        rc, msg = _kmeans_call(lib, tol=tol, limit=0)       # `shift^2 < tol` can never hold: the loop could not end
        assert rc != 0 and b"tol" in msg and b"iter_limit" in msg, (tol, msg)
    for limit in (-1, -1000):
        rc, msg = _kmeans_call(lib, limit=limit)
        assert rc != 0 and b"iter_limit" in msg, (limit, msg)
    rc, msg = _kmeans_call(lib, tol=1e-3, limit=-1)
    assert rc != 0
    for kw in (dict(N=18001), dict(K=33), dict(N=5, K=6), dict(P=0), dict(N=0), dict(K=0)):
        rc, msg = _kmeans_call(lib, **kw)
        assert rc != 0 and b"bad shape" in msg, (kw, msg)
    vp = ctypes.c_void_p
    assert lib.ynet_kmeans2d(None, vp(512), vp(768), vp(1024), 1, 100, 4, 1e-3, 10, None) != 0 and b"null" in lib.ynet_last_error()


def test_header_documents_the_kmeans_refusals_and_the_status_bit():
    import os
    from conftest import ROOT
    with open(os.path.join(ROOT, "include", "ynet_hip.h")) as f:
        h = " ".join(f.read().split())
    doc = h[h.index("kmeans (utils/kmeans.py"):h.index("int ynet_kmeans2d(")]
    assert "iter_limit == 0" in doc and "tol > 0" in doc and "iter_limit < 0" in doc and "bit 1 (value 2)" in doc


# ------------------------------------------------------------------------------------------------
# conditioned-waypoint-sampling prior
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [r[0] for r in S.CWS_ROWS if r[6] == "finite"])
def test_cws_rule_agrees_with_the_fp32_oracle(name):
    """Bound: twice the fp32 oracle's own error against cws_rule over the elements above 1e-6 of the map's maximum, as recorded next to the
    row in CWS_ROWS (measured on the CPU: 6.4e-6 .. 7.5e-5, the largest at 512 x 512 where the fp32 grid has the coarsest spacing)."""
    e_ref = S.cws_row(name)[7]
    worst = 0.0
    for H, W in S.CWS_SHAPES:
        e, got = S.cws_oracle_error(name, H, W)
        assert e is not None and abs(float(got.sum()) - 1.0) <= 1e-4, (name, H, W)
        print(f"cws {name} {H}x{W}: fp32 oracle vs cws_rule {e:.3e} (recorded {e_ref:.3e})")
        worst = max(worst, e)
    assert worst <= 2 * e_ref, (name, worst, e_ref)
    assert worst >= e_ref / 8, (name, worst, e_ref)      # the recorded figure is a measurement, not a loose cap


def test_cws_nan_rows_have_the_listed_pattern():
    """12 px outside with dist = 0: every fp32 term underflows (oracle 0 / 0), float64 does not.  60 px outside: float64 underflows too, and
    the contract is NaN in the map and in the expectation."""
    assert {r[0] for r in S.CWS_ROWS if r[6] == "nan"} == {"outside_12px", "outside_60px"}
    for H, W in S.CWS_SHAPES:
        for name in ("outside_12px", "outside_60px"):
            e, oracle_map = S.cws_oracle_error(name, H, W)
            assert e is None and bool(np.isnan(oracle_map).all()), (name, H, W)
            maps, xy = S.cws_want(name, "ones", H, W)
            if name in S.CWS_RULE_NAN:
                assert bool(np.isnan(maps).all()) and bool(np.isnan(xy).all()), (name, H, W)
            else:
                assert bool(np.isfinite(maps).all()) and bool(np.isfinite(xy).all()), (name, H, W)
                np.testing.assert_allclose(maps.sum(axis=(1, 2)), 1.0, rtol=1e-12)
                assert float(np.abs(xy[:, 0]).max()) <= 1e-6      # the mass sits on column 0, next to the mean


def test_cws_rows_and_variants_cover_the_edges():
    rows = {r[0]: r for r in S.CWS_ROWS}
    assert rows["dist_0"][2] == (0.0, 0.0) and rows["dist_200"][2] == (200.0, 200.0)
    assert rows["traj_idx_2"][3:5] == (4.0, 2.0) and rows["negative_sigma_factor"][3] < 0
    assert rows["corner_pixel"][1](37, 50) == (49.0, 36.0)
    assert (1, 8) in S.CWS_SHAPES and (8, 1) in S.CWS_SHAPES and (512, 512) in S.CWS_SHAPES
    mean, dist = S.cws_inputs("dist_0", 64, 96)
    assert mean.shape == (2 * S.CWS_B, 2) and float(dist.abs().max()) == 0.0 and mean[0].tolist() == [48.0, 32.0]
    view, B = S.cws_sig("channel_view", 37, 50)
    assert B == S.CWS_B and view.stride() == (3 * 37 * 50, 50, 1) and not view.is_contiguous()
    ones, B1 = S.cws_sig("ones", 8, 1)
    assert B1 == 1 and bool((ones == 1).all())
    # the benign rows: the expectation of an all-ones map lies at the mean, in pixel indices (grid point i sits at i N / (N - 1))
    maps, xy = S.cws_want("benign", "ones", 64, 96)
    assert abs(xy[0, 0] - 0.4 * 96 * 95 / 96) < 0.05 and abs(xy[0, 1] - 0.55 * 64 * 63 / 64) < 0.05
    # persons differ: rows r and r + B of the dense variant use the same map, rows r and r + 1 do not
    dense, _ = S.cws_sig("sigmoid_randn", 8, 8)
    assert not torch.equal(dense[0], dense[1])

"""The evaluation samplers at their edges: ynet_multinomial and ynet_cws_prior (csrc/sample.hip) and ynet_kmeans2d (csrc/glue.hip) against
the restatements of tests/_sampling_cases.py (tests/test_sampling_cases_host.py proves that table without a GPU) -- never against a second
call into the code under test.

Multinomial: draw for draw (torch.equal) with oracle.device_multinomial.  k-means: centres, iteration count and flags equal to kmeans_rule.
CWS prior: the device computes in fp64 and rounds once to fp32, so the bounds follow from that and are not measured:
|map - ref| <= 2^-23 |ref| + 2^-126, |xy - ref| <= 2^-23 max(H, W), NaN exactly where cws_rule is NaN."""
import numpy as np
import pytest
import torch

import _sampling_cases as S
from conftest import pkg

pytestmark = pytest.mark.gpu


def _drain(ops):
    """Read and clear the sampler's device flag, whatever it holds: a failure here must not leak it into later tests."""
    try:
        ops.check_patch_status()
    except (RuntimeError, ValueError):
        pass


# ------------------------------------------------------------------------------------------------
# 1. multinomial
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", S.MULTI_NAMES)
def test_multinomial_rows_match_the_oracle(dev, name):
    """Every row of the table through the plain entry, through a [::2] row view (read in place) and through the device-seed entry; the
    status flag stays clean after each."""
    ops = pkg("ops")
    _, prob, K, replacement, thr, seed = S.multi_row(name)
    want = S.multi_want(name)
    rows, n = prob.shape
    _drain(ops)
    try:
        got = ops.multinomial(prob.to(dev), K, replacement, thr, seed).cpu()
        ops.check_patch_status()
        assert torch.equal(got, want), f"{name}: {int((got != want).sum())} of {want.numel()} draws differ"
        wide = torch.stack([prob, prob.flip(0)], dim=1).reshape(2 * rows, n).to(dev)
        view = wide[::2]
        assert view.stride(0) == 2 * n
        got2 = ops.multinomial(view, K, replacement, thr, seed).cpu()
        ops.check_patch_status()
        assert torch.equal(got2, want), f"{name}, row view: {int((got2 != want).sum())} draws differ"
        seeds = torch.tensor([7, seed, 9], dtype=torch.int64, device=dev)
        got3 = ops.multinomial(prob.to(dev), K, replacement, thr, seeds[1:2]).cpu()
        ops.check_patch_status()
        assert torch.equal(got3, want), f"{name}, device seed: {int((got3 != want).sum())} draws differ"
    finally:
        _drain(ops)


@pytest.mark.parametrize("name", S.STATUS_NAMES)
def test_multinomial_status_rows_are_reported(dev, name):
    """Fewer than K positive entries on the race without replacement, a row total of zero beside valid rows on the inverse-CDF path:
    check_patch_status raises once, then is clean; the valid rows of `zero_last` still equal the oracle."""
    ops = pkg("ops")
    _, prob, K, replacement, thr, seed = S.multi_row(name)
    _drain(ops)
    try:
        got = ops.multinomial(prob.to(dev), K, replacement, thr, seed).cpu()
        with pytest.raises(RuntimeError, match="invalid multinomial"):
            ops.check_patch_status()
        ops.check_patch_status()        # the flag was cleared by the report
        assert got.shape == (prob.shape[0], K) and int(got.min()) >= 0 and int(got.max()) < prob.shape[1]
        if name == "zero_last":
            assert torch.equal(got[:3], S.multi_want(name)), int((got[:3] != S.multi_want(name)).sum())
    finally:
        _drain(ops)


def test_multinomial_refusals(dev):
    ops = pkg("ops")
    p = torch.rand(2, 100, generator=torch.Generator().manual_seed(1)).to(dev) + 0.1
    _drain(ops)
    with pytest.raises(RuntimeError, match=r"K <= min\(48, n\)"):
        ops.multinomial(p, 49, False, None, 1)
    with pytest.raises(RuntimeError, match=r"K <= min\(48, n\)"):
        ops.multinomial(p[:, :10], 11, False, None, 1)
    with pytest.raises(RuntimeError, match="rel_threshold"):
        ops.multinomial(p, 4, False, 1.5, 1)
    with pytest.raises(RuntimeError, match="rel_threshold"):
        ops.multinomial(p, 4, True, 1.5, 1)
    ops.check_patch_status()            # a refused call launches nothing and reports nothing


# ------------------------------------------------------------------------------------------------
# 2. k-means
# ------------------------------------------------------------------------------------------------
def _kmeans_check(name, got, status, skip=()):
    want, its, empty, _ = S.kmeans_want(name)
    st = status.cpu()
    got = got.cpu()
    for p in range(want.shape[0]):
        if p in skip:
            continue
        assert int(st[p]) >> 8 == its[p], (name, p, int(st[p]) >> 8, its[p])
        assert int(st[p]) & 0xFF == int(empty[p]), (name, p, int(st[p]) & 0xFF, empty[p])
        if not empty[p]:
            assert torch.equal(got[p], want[p]), (name, p, float((got[p] - want[p]).abs().max()))


@pytest.mark.parametrize("name", list(S.KMEANS_CASES))
def test_kmeans_matches_the_rule(dev, name):
    """Centres bit for bit, status >> 8 the iteration count, status & 1 the empty flag (set only by the duplicate-centre case)."""
    ops = pkg("ops")
    pts, init, tol, limit, _ = S.kmeans_case(name)
    assert tol > 0 or limit > 0         # (the entry refuses the other calls: tests/test_sampling_cases_host.py)
    got, status = ops.kmeans2d(pts.to(dev), init, tol, limit)
    _kmeans_check(name, got, status)
    if name in S.KMEANS_EMPTY:
        assert (status.cpu() & 1).tolist() == [int(e) for e in S.KMEANS_EMPTY[name]] and any(S.KMEANS_EMPTY[name])


@pytest.mark.parametrize("name,person,slot,bad", [
    ("below_1024_threads", 1, 5, "N"), ("below_1024_threads", 2, 0, -1), ("below_1024_threads", 0, 31, 2 ** 31 - 1),
    ("K1", 3, 0, -2 ** 31), ("many_workgroups", 299, 2, "N")])
def test_kmeans_reports_an_initial_index_outside_the_points(dev, name, person, slot, bad):
    """An init_idx entry of N, -1 or an extreme value for ONE person: that person gets status 2 (no iteration) and NaN centres, the index is
    never used as an address, and every other person of the call equals the rule."""
    ops = pkg("ops")
    pts, init, tol, limit, _ = S.kmeans_case(name)
    init = init.clone()
    init[person, slot] = pts.shape[1] if bad == "N" else bad
    got, status = ops.kmeans2d(pts.to(dev), init, tol, limit)
    assert int(status[person].cpu()) == 2, int(status[person].cpu())
    assert bool(torch.isnan(got[person]).all())
    _kmeans_check(name, got, status, skip=(person,))


def test_ttst_goals_raises_on_the_bad_index_bit(dev, monkeypatch):
    """utils/evaluate.ttst_goals draws its indices on the host, so status bit 1 means a bug there: ValueError, not NaN goals."""
    ev = pkg("utils.evaluate")
    pts, _, _, _, _ = S.kmeans_case("N_equals_K")
    P, N, _ = pts.shape
    draw = pts.permute(1, 0, 2).unsqueeze(2).to(dev)            # [N, P, 1, 2]

    class Model:
        def softargmax(self, x):
            return torch.zeros(P, 1, 2, device=dev)
    np.random.seed(3)
    goals = ev.ttst_goals(Model(), None, None, 4, 0.01, draw=draw)
    assert goals.shape == (4, P, 1, 2) and bool(torch.isfinite(goals).all())
    monkeypatch.setattr(np.random, "choice", lambda n, k, replace=False: np.arange(n - k + 1, n + 1))      # the last index is N
    with pytest.raises(ValueError, match="outside 0"):
        ev.ttst_goals(Model(), None, None, 4, 0.01, draw=draw)


# ------------------------------------------------------------------------------------------------
# 3. conditioned-waypoint-sampling prior
# ------------------------------------------------------------------------------------------------
def _cws_compare(tag, maps, xy, want_maps, want_xy, H, W):
    worst_m = worst_xy = 0.0
    if maps is not None:
        got = maps.cpu().double().numpy()
        assert got.shape == want_maps.shape, (tag, got.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want_maps)), f"{tag}: NaN mask of the map differs"
        ok = ~np.isnan(want_maps)
        err, bound = np.abs(got - want_maps)[ok], (2.0 ** -23 * np.abs(want_maps) + 2.0 ** -126)[ok]
        if err.size:
            worst_m = float((err / bound).max())
        assert bool((err <= bound).all()), f"{tag}: map error {worst_m:.3f} x the bound, {int((err > bound).sum())} elements"
    if xy is not None:
        got = xy.cpu().double().numpy()
        assert got.shape == want_xy.shape, (tag, got.shape)
        assert np.array_equal(np.isnan(got), np.isnan(want_xy)), f"{tag}: NaN mask of xy differs"
        ok = ~np.isnan(want_xy)
        if ok.any():
            worst_xy = float(np.abs(got - want_xy)[ok].max())
        assert worst_xy <= 2.0 ** -23 * max(H, W), f"{tag}: xy error {worst_xy:.3e} px, bound {2.0 ** -23 * max(H, W):.3e}"
    return worst_m, worst_xy


@pytest.mark.parametrize("kind", S.CWS_SIGS)
@pytest.mark.parametrize("shape", S.CWS_SHAPES, ids=["{}x{}".format(*s) for s in S.CWS_SHAPES])
def test_cws_prior_matches_the_float64_rule(dev, shape, kind):
    """Every row of CWS_ROWS on 2 B rows (row % B picks the person), with want_map and want_xy together and each alone."""
    ops = pkg("ops")
    H, W = shape
    sig, B = S.cws_sig(kind, H, W, device=dev)
    if kind == "channel_view":
        assert sig.stride() == (3 * H * W, W, 1)        # the batch stride cws_waypoints passes: read in place
    for name, _, _, sf, ratio, rot, _, _ in S.CWS_ROWS:
        mean, dist = S.cws_inputs(name, H, W)
        want_maps, want_xy = S.cws_want(name, kind, H, W)
        assert bool(np.isnan(want_maps).all()) == (name in S.CWS_RULE_NAN) == bool(np.isnan(want_xy).all())
        both = ops.cws_prior(sig, mean.to(dev), dist.to(dev), sf, ratio, rot, want_map=True, want_xy=True)
        only_map = ops.cws_prior(sig, mean.to(dev), dist.to(dev), sf, ratio, rot, want_map=True, want_xy=False)
        only_xy = ops.cws_prior(sig, mean.to(dev), dist.to(dev), sf, ratio, rot, want_map=False, want_xy=True)
        assert only_map[1] is None and only_xy[0] is None
        tag = f"cws {name} {H}x{W} {kind}"
        wm, wx = _cws_compare(tag + " (map and xy)", both[0], both[1], want_maps, want_xy, H, W)
        print(f"{tag}: map error {wm:.3f} x (2^-23 |ref| + 2^-126), xy error {wx:.3e} px (bound {2.0 ** -23 * max(H, W):.3e})")
        _cws_compare(tag + " (map only)", only_map[0], None, want_maps, want_xy, H, W)
        _cws_compare(tag + " (xy only)", None, only_xy[1], want_maps, want_xy, H, W)

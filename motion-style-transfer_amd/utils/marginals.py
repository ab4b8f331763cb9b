"""Marginals of the goal-map distribution: the host side of ops.map_marginals.  The kernel gives, per plane, the
x- and the y-marginal of sigmoid(pred_goal_map / T) (its column and row sums), their CRPS against the ground truth and the two ends of
its PIT; here are the level handling of the drivers, quantiles and central intervals of a profile, the test whether a ground truth lies
inside an interval, the non-randomised PIT histogram, and the lines YNetTrainer.test prints.  Pure torch / NumPy on the small tensors
([..., side] per plane, hundreds of times smaller than the map), on whatever device they live, in fp64."""
import numpy as np
import torch

DEFAULT_LEVELS = (0.5, 0.9)


def marginal_levels(value, what="evaluate(return_marginals=...)"):
    """The drivers' flag -> None (off), or the levels of the central intervals as a tuple of floats: True means DEFAULT_LEVELS, anything
    else is a sequence of 1 .. 8 strictly ascending levels inside (0, 1) (checked as ops.map_credible checks its levels)."""
    if value is None or value is False:
        return None
    if value is True:
        return DEFAULT_LEVELS
    from .. import ops
    if np.ndim(value) != 1:
        raise ValueError(f"{what}: False, True or a sequence of levels is expected, got {value!r}")
    ops.credible_levels(value, what)
    return tuple(float(q) for q in value)


def profile_cdf(profile):
    """profile [..., side] -> its CDF [..., side] in fp64, divided by its own last value (the stored fp32 shares sum to 1 up to their
    roundings only: this way the CDF reaches 1 exactly and every quantile exists).  A NaN profile stays NaN."""
    cdf = torch.as_tensor(profile).double().cumsum(dim=-1)
    return cdf / cdf[..., -1:]


def quantiles(profile, qs):
    """The q-quantile of a marginal, per q in ``qs``: the smallest index whose CDF reaches q (CDF >= q; at an exact tie the index
    where it is reached, not the next) -> int64 [..., n_q]; -1 for a NaN profile."""
    cdf = profile_cdf(profile)
    q = torch.as_tensor([float(v) for v in qs], dtype=torch.float64, device=cdf.device)
    if q.numel() == 0 or bool(((q < 0) | (q > 1) | torch.isnan(q)).any()):
        raise ValueError(f"quantiles: qs {list(qs)!r}: one or more numbers in [0, 1] are expected")
    idx = (cdf[..., None, :] < q[:, None]).sum(dim=-1).clamp(max=cdf.shape[-1] - 1)
    return torch.where(torch.isnan(cdf[..., -1:]), torch.full_like(idx, -1), idx)


def central_intervals(profile, levels):
    """The central interval of a marginal per level q: from its (1 - q) / 2 quantile to its (1 + q) / 2 quantile, both ends included
    -> int64 [..., L, 2] (lo, hi) pixel indices; (-1, -1) for a NaN profile."""
    levels = [float(q) for q in levels]
    ends = quantiles(profile, [(1.0 - q) / 2.0 for q in levels] + [(1.0 + q) / 2.0 for q in levels])
    return torch.stack([ends[..., :len(levels)], ends[..., len(levels):]], dim=-1)


def inside_intervals(intervals, g):
    """Whether the rounded ground-truth coordinate lies inside each interval: intervals [..., L, 2] of central_intervals, g [...] (rounded
    half-even here) -> float64 [..., L]: 1.0 / 0.0, NaN where g is NaN or infinite or the profile had no interval (-1)."""
    intervals = torch.as_tensor(intervals)
    g = torch.round(torch.as_tensor(g, device=intervals.device).double())[..., None]
    lo, hi = intervals[..., 0].double(), intervals[..., 1].double()
    valid = torch.isfinite(g) & (lo >= 0)
    nan = torch.full((), float("nan"), dtype=torch.float64, device=intervals.device)
    return torch.where(valid, ((g >= lo) & (g <= hi)).double(), nan)


def profile_mean(profile):
    """The mean index of a marginal -> fp64 [...] (the expected pixel coordinate along that axis)"""
    p = torch.as_tensor(profile).double()
    t = torch.arange(p.shape[-1], dtype=torch.float64, device=p.device)
    return (p * t).sum(dim=-1) / p.sum(dim=-1)


def pit_histogram(pit, n_bins=10):
    """The deterministic (non-randomised) PIT histogram of a discrete forecast: pit [..., 2] (lower, upper) = F(g - 1), F(g) per plane
    -> float64 NumPy [n_bins] of masses.  Every plane spreads a unit mass uniformly over [lower, upper] across the bins of [0, 1] it
    overlaps; a zero-width PIT (a ground truth off the map, or on a bin without mass) goes whole into its bin (1.0 into the last).
    Rows with a NaN are left out.  A calibrated marginal gives a flat histogram; U: too narrow, a hump: too wide, a slope: biased."""
    n_bins = int(n_bins)
    if n_bins < 1:
        raise ValueError(f"pit_histogram: n_bins = {n_bins!r}, expected >= 1")
    p = np.asarray(torch.as_tensor(pit).detach().cpu().numpy() if torch.is_tensor(pit) else pit, dtype=np.float64).reshape(-1, 2)
    p = p[np.isfinite(p).all(axis=1)]
    lo, up = np.clip(p[:, 0], 0.0, 1.0), np.clip(p[:, 1], 0.0, 1.0)
    up = np.maximum(up, lo)
    edges = np.arange(n_bins + 1, dtype=np.float64) / n_bins
    hist = np.zeros(n_bins, dtype=np.float64)
    wide = up > lo
    if wide.any():
        l, u = lo[wide, None], up[wide, None]
        overlap = np.clip(np.minimum(u, edges[None, 1:]) - np.maximum(l, edges[None, :-1]), 0.0, None)
        hist += (overlap / (u - l)).sum(axis=0)
    if (~wide).any():
        hist += np.bincount(np.minimum((lo[~wide] * n_bins).astype(np.int64), n_bins - 1), minlength=n_bins)
    return hist


def marginals_report(levels, crps, inside, width, fde=None):
    """The lines YNetTrainer.test(return_marginals=...) prints per round for the last step: crps [N, 2] (x, y) and width [N, 2, L] in the
    units of FDE, inside [N, 2, L]; rows with a NaN (a plane that could not be scored) are left out of each average."""
    levels = [float(q) for q in levels]
    crps = np.asarray(crps, dtype=np.float64).reshape(-1, 2)
    inside = np.asarray(inside, dtype=np.float64).reshape(-1, 2, len(levels))
    width = np.asarray(width, dtype=np.float64).reshape(-1, 2, len(levels))
    avg = lambda v: float(v[np.isfinite(v)].mean()) if np.isfinite(v).any() else float("nan")
    both = crps.sum(axis=1)
    lines = [f"Marginal goal scores (no draw; n = {int(np.isfinite(both).sum())})",
             f"  mean CRPS x + y: {avg(both):.4f} (x {avg(crps[:, 0]):.4f}, y {avg(crps[:, 1]):.4f})"
             + (f"   (sampled FDE of this round: {float(fde):.4f})" if fde is not None else "")]
    for a, axis in enumerate("xy"):
        for l, q in enumerate(levels):
            lines.append(f"  {axis}, central {format(round(q * 100.0, 6), 'g')} % interval: coverage {avg(inside[:, a, l]):.4f} | "
                         f"mean width {avg(width[:, a, l]):.4f}")
    return "\n".join(lines)

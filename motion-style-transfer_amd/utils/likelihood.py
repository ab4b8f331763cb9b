"""Calibration of the goal-map distribution from the ``hpd`` values of ops.map_likelihood / evaluate(return_likelihood=True).

hpd is the mass of the smallest highest-density region of a forecast that still contains the ground truth.  Under a calibrated
model it is uniform on [0, 1]: the q-credible region (the most probable pixels, up to mass q) then holds the ground truth in a
fraction q of the cases.  Host code (NumPy): the inputs are a few numbers per agent.  The reference has nothing of the kind."""
import numpy as np

DEFAULT_LEVELS = np.linspace(0.05, 0.95, 19)


def calibration_curve(hpd, levels=DEFAULT_LEVELS):
    """-> (levels, coverage, ece): coverage[q] = the fraction of the finite entries of ``hpd`` with hpd <= levels[q] (how often the
    levels[q]-credible region held the ground truth), ece = mean |coverage - levels|.  NaN entries (a ground truth outside its map,
    a poisoned plane) are left out; an input without a finite entry is refused."""
    h = np.asarray(hpd.detach().cpu() if hasattr(hpd, "detach") else hpd, dtype=np.float64).reshape(-1)
    levels = np.asarray(levels, dtype=np.float64).reshape(-1)
    if levels.size == 0 or not np.isfinite(levels).all() or (levels < 0).any() or (levels > 1).any():
        raise ValueError("calibration_curve: levels must be a non-empty set of numbers in [0, 1]")
    h = h[np.isfinite(h)]
    if h.size == 0:
        raise ValueError("calibration_curve: no finite hpd value (the input is empty or all NaN)")
    if (h < 0).any() or (h > 1).any():
        raise ValueError("calibration_curve: hpd values are probabilities, found one outside [0, 1]")
    coverage = (h[None, :] <= levels[:, None]).mean(axis=1)
    return levels, coverage, float(np.abs(coverage - levels).mean())


# ------------------------------------------------------------------------------------------------
# Temperature scaling (utils/calibrate.py): the grid search over ops.map_likelihood_sweep's curves.  Pure host
# code: a grid, the best point of a measured curve, and the bracket of the next round.  Nothing is interpolated and nothing is assumed
# about convexity -- the result of a search is a temperature at which the NLL was measured.
# ------------------------------------------------------------------------------------------------
def temperature_grid(lo, hi, n, include=None):
    """-> ascending fp32 array: ``n`` log-spaced temperatures over [lo, hi], both ends included, computed in fp64 and rounded to fp32
    (what the kernel takes: every value is exactly the temperature that gets measured); ``include`` (a temperature, e.g. the one in
    use) is inserted in order unless its fp32 value is already a grid value.  Grid values that coincide after the rounding (a very
    narrow bracket) are kept once.  0 < lo < hi, finite, and still apart in fp32; n >= 2."""
    lo, hi, n = float(lo), float(hi), int(n)
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"temperature_grid: the bracket ({lo!r}, {hi!r}) must be finite with 0 < lo < hi")
    if n < 2:
        raise ValueError(f"temperature_grid: n = {n}: a grid holds both ends, so at least 2 points")
    grid = np.exp(np.linspace(np.log(lo), np.log(hi), n))
    grid[0], grid[-1] = lo, hi
    with np.errstate(over="ignore"):
        vals = list(grid.astype(np.float32))
        if include is not None:
            inc = np.float32(float(include))
            if not (np.isfinite(inc) and inc > 0):
                raise ValueError(f"temperature_grid: include = {include!r} must be positive and finite in fp32")
            vals.append(inc)
    out = np.unique(np.asarray(vals, dtype=np.float32))
    if not (np.isfinite(out).all() and out[0] > 0 and np.float32(lo) < np.float32(hi)):
        raise ValueError(f"temperature_grid: the bracket ({lo!r}, {hi!r}) does not survive the rounding to fp32")
    return out


def _curve(temps, curve, what):
    t = np.asarray(temps, dtype=np.float64).reshape(-1)
    c = np.asarray(curve, dtype=np.float64).reshape(-1)
    if t.size == 0 or t.size != c.size:
        raise ValueError(f"{what}: {t.size} temperatures and {c.size} curve values")
    if not np.isfinite(c).all() or not np.isfinite(t).all():
        raise ValueError(f"{what}: the curve holds a non-finite entry; leave the offending planes out of every temperature first")
    if np.unique(t).size != t.size:
        raise ValueError(f"{what}: a temperature appears twice")
    return t, c


def best_temperature(temps, curve):
    """-> (temperature, index into ``temps``) of the smallest curve value; a tie goes to the lower temperature.  ``temps`` need not be
    sorted.  A non-finite curve entry is refused: a NaN would otherwise win or lose by accident."""
    t, c = _curve(temps, curve, "best_temperature")
    ties = np.flatnonzero(c == c.min())
    i = int(ties[np.argmin(t[ties])])
    return float(t[i]), i


def next_bracket(temps, curve):
    """-> (lo, hi) of the next round: the two grid neighbours of the best point; at an end of the grid that end and its one neighbour.
    A grid of one point has no bracket and is refused."""
    t, c = _curve(temps, curve, "next_bracket")
    if t.size < 2:
        raise ValueError("next_bracket: a grid of one point has no neighbours")
    best, _ = best_temperature(t, c)
    s = np.sort(t)
    j = int(np.searchsorted(s, best))
    return float(s[max(j - 1, 0)]), float(s[min(j + 1, s.size - 1)])

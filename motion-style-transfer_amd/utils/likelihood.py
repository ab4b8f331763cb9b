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

"""Sharpness of the goal-map distribution: the host side of ops.map_credible.  The kernel gives, per plane and
level q, the threshold, area and mass of the q-credible region {x >= threshold}; here are the level handling of the drivers, the test
whether a ground-truth pixel lies inside a region, the mask for drawing one, and the table YNetTrainer.test prints: coverage (how often
the ground truth falls inside -- calibration, which should be q) beside the size of the regions (sharpness)."""
import numpy as np
import torch

DEFAULT_LEVELS = (0.5, 0.9)


def sharpness_levels(return_sharpness, what="evaluate(return_sharpness=...)"):
    """The drivers' flag -> None (off), or the levels as a tuple of floats: True means DEFAULT_LEVELS, anything else is a sequence of
    1 .. 8 strictly ascending levels inside (0, 1) (checked as ops.map_credible checks them)."""
    if return_sharpness is None or return_sharpness is False:
        return None
    if return_sharpness is True:
        return DEFAULT_LEVELS
    from .. import ops
    if np.ndim(return_sharpness) != 1:
        raise ValueError(f"{what}: False, True or a sequence of levels is expected, got {return_sharpness!r}")
    ops.credible_levels(return_sharpness, what)
    return tuple(float(q) for q in return_sharpness)


def level_name(q):
    """0.5 -> '50', 0.999 -> '99.9': the level as the per cent in a column name"""
    return format(round(float(q) * 100.0, 6), "g")


def inside_regions(goal_map, gt_xy, threshold):
    """Whether the ground truth lies inside each region: goal_map [N, C, H, W] logits, gt_xy [N, C, 2] (x, y) = (column, row), threshold
    [N, C, L] of ops.map_credible on the same map -> [N, C, L] float32: 1.0 where the logit at the rounded ground-truth pixel is >= the
    threshold, 0.0 where it is below, NaN where the ground truth rounds outside the map (or is NaN) or the plane has no region (NaN
    threshold).  The rounding (half-even) and the outside-the-map rule are ynet_map_likelihood's, whose hpd this is the binary form of."""
    N, C, H, W = goal_map.shape
    g = torch.round(gt_xy.to(goal_map.device).float())
    gx, gy = g[..., 0], g[..., 1]
    ok = (gx >= 0) & (gx < W) & (gy >= 0) & (gy < H)      # (false for a NaN coordinate)
    ix = (torch.where(ok, gy, torch.zeros_like(gy)) * W + torch.where(ok, gx, torch.zeros_like(gx))).long()
    xg = goal_map.reshape(N, C, H * W).gather(2, ix[..., None])      # [N, C, 1]
    valid = ok[..., None] & ~torch.isnan(threshold)
    return torch.where(valid, (xg >= threshold).float(), torch.full((), float("nan"), device=goal_map.device))


def region_mask(goal_map, threshold):
    """The boolean region for drawing: goal_map [..., H, W] >= threshold [...][..., None, None]; a NaN threshold gives an empty mask.
    With threshold [..., L] pass goal_map[..., None, :, :] for all levels at once."""
    return goal_map >= torch.as_tensor(threshold, device=goal_map.device)[..., None, None]


def sharpness_table(levels, inside, area, map_pixels, resize_factor):
    """Per level one dict: ``level`` (nominal), ``coverage`` (the mean of ``inside`` [N, L] over its finite rows: the share of ground
    truths inside the region; NaN when there is none), ``n`` (those rows), and the size of the regions ``area`` [N, L] (rows without a
    region -- area < 0 -- left out): ``area_mean`` / ``area_median`` in pixels of the resized map, ``share_mean`` / ``share_median`` as a
    share of the map's ``map_pixels`` (one number, or one per row where the scenes differ in size), ``area_orig_mean`` /
    ``area_orig_median`` in pixels of the original image (/ resize_factor^2).
    A sharp and calibrated forecast has coverage ~ level at a small area."""
    levels = [float(q) for q in levels]
    inside = np.asarray(inside, dtype=np.float64).reshape(-1, len(levels))
    area = np.asarray(area, dtype=np.float64).reshape(-1, len(levels))
    if inside.shape != area.shape:
        raise ValueError(f"sharpness_table: inside {inside.shape} and area {area.shape} differ")
    px = np.broadcast_to(np.asarray(map_pixels, dtype=np.float64).reshape(-1), (area.shape[0],)) if area.shape[0] else np.zeros(0)
    if not ((np.asarray(map_pixels) > 0).all() and resize_factor > 0):
        raise ValueError(f"sharpness_table: map_pixels {map_pixels!r} and resize_factor {resize_factor!r} must be positive")
    rows = []
    for l, q in enumerate(levels):
        hit = inside[:, l][np.isfinite(inside[:, l])]
        a, sh = area[:, l][area[:, l] >= 0], (area[:, l] / px)[area[:, l] >= 0]
        stat = lambda v: (float(v.mean()), float(np.median(v))) if v.size else (float("nan"), float("nan"))
        (mean, med), (smean, smed) = stat(a), stat(sh)
        rows.append({"level": q, "coverage": float(hit.mean()) if hit.size else float("nan"), "n": int(hit.size),
                     "area_mean": mean, "area_median": med, "share_mean": smean, "share_median": smed,
                     "area_orig_mean": mean / resize_factor ** 2, "area_orig_median": med / resize_factor ** 2})
    return rows


def sharpness_report(levels, inside, area, map_pixels, resize_factor):
    """The lines YNetTrainer.test(return_sharpness=...) prints per round, one per level"""
    lines = ["Sharpness (level: coverage of the ground-truth goal | mean / median area in map pixels | share of the map | original pixels)"]
    for r in sharpness_table(levels, inside, area, map_pixels, resize_factor):
        lines.append(f"  {level_name(r['level'])} %: {r['coverage']:.4f} (n = {r['n']}) | {r['area_mean']:.1f} / {r['area_median']:.1f} | "
                     f"{r['share_mean']:.5f} / {r['share_median']:.5f} | {r['area_orig_mean']:.1f} / {r['area_orig_median']:.1f}")
    return "\n".join(lines)

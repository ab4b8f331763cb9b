"""Temperature scaling of the goal-map distribution (not in the reference, which hand-sets T: 1.0 short-term, 1.8 long-term).

sigmoid(pred_goal_map / T), every plane normalised, is what evaluate(), predict(), TTST and CWS draw from (utils/evaluate.py:128-131,
utils/image_utils.py:110-135) and what predict_modes() reads its masses off.  An adapter fitted on a few tracks changes how peaked the
maps are, so the T that suited the pre-trained net no longer suits the adapted one.  ``calibrate_temperature`` chooses T by the
validation NLL: evaluate()'s loop over scenes and chunks up to the goal map and nothing after it, one ops.map_likelihood_sweep launch
per chunk (the NLL and the hpd at a whole grid of temperatures from one read of the maps), and a deterministic grid search
(utils/likelihood.py) over the curves.  DESIGN.md section 4.12."""
import warnings

import numpy as np
import torch

from .. import ops
from .evaluate import _goal_maps
from .image_utils import swap_pavement_terrain
from .likelihood import best_temperature, calibration_curve, next_bracket, temperature_grid

STEPS = ("waypoints", "goal", "all")


def check_arguments(waypoints, temperature, t_range, n_temps, rounds, steps):
    """The refusals of calibrate_temperature (and of YNetTrainer.calibrate_temperature, before it prepares any data): host code only."""
    if int(rounds) < 1:
        raise ValueError(f"calibrate_temperature: rounds = {rounds}: at least one pass over the loader")
    if not 2 <= int(n_temps) <= ops.SWEEP_MAX_TEMPS - 1:
        raise ValueError(f"calibrate_temperature: n_temps = {n_temps}, expected 2 .. {ops.SWEEP_MAX_TEMPS - 1} (the grid also holds the "
                         f"temperature in use, and one launch takes {ops.SWEEP_MAX_TEMPS})")
    try:
        lo, hi = (float(v) for v in t_range)
    except (TypeError, ValueError):
        raise ValueError(f"calibrate_temperature: t_range = {t_range!r}: a pair (lo, hi) is expected") from None
    if not (np.isfinite(lo) and np.isfinite(hi) and 0.0 < lo < hi):
        raise ValueError(f"calibrate_temperature: t_range = {t_range!r} must be finite with 0 < lo < hi")
    if steps not in STEPS:
        raise ValueError(f"calibrate_temperature: steps = {steps!r}, expected one of {STEPS}")
    if len(list(waypoints)) == 0:
        raise ValueError("calibrate_temperature: no way-points: there is no plane to score")
    ops.sweep_temperatures([temperature], "calibrate_temperature")
    temperature_grid(lo, hi, int(n_temps), include=temperature)


def _selected_planes(steps, waypoints, pred_len):
    if steps == "waypoints":
        return list(waypoints)
    if steps == "goal":
        return [waypoints[-1]]
    return list(range(pred_len))


def calibrate_temperature(model, val_loader, val_images, device, input_template, waypoints, obs_len, batch_size, resize_factor, temperature,
                          t_range=(0.25, 8.0), n_temps=16, rounds=2, steps="waypoints", network=None, swap_semantic=False):
    """The temperature that minimises the mean NLL of the ground truth under the goal-map distribution over ``val_loader`` (evaluate()'s
    loader: (trajectory, df_batch, scene_id) with the tracks in resized pixels, so ``resize_factor`` is not read).

    ``steps`` names the planes whose NLL is averaged: "waypoints" (those the samplers draw from), "goal" (the last way-point alone) or
    "all" (every future step).  The search is deterministic and assumes nothing about convexity: every round makes one pass over the
    loader and measures ``n_temps`` log-spaced temperatures over its bracket, ends included, plus ``temperature`` (the one in use);
    round 1's bracket is ``t_range``, the next round's the two grid neighbours of the best point.  No draw, no trajectory decoder, no
    generator read; evaluate()'s captured sweeps are neither used nor touched; the model is left in the mode it was found in.

    A plane with a non-finite NLL at any temperature of a round (a ground truth outside the map: one warning; a map without mass at
    a small T) is left out at every temperature of that round, so the curve compares the same planes.
    -> dict: ``temperature`` (float, the fp32 value: the best grid point of the last round, measured, not interpolated), ``nll`` /
    ``nll_before`` (mean NLL there / at the caller's temperature, last round), ``ece`` / ``ece_before`` (utils.likelihood.
    calibration_curve on the goal plane's hpd), ``curve`` [(temperatures, nll) per round], ``temperature_steps`` (per selected plane,
    the best grid temperature of the last round for that step alone; reported only), ``excluded``, ``n_planes``, ``at_boundary`` (the
    result is an end of ``t_range``: widen it)."""
    waypoints = list(waypoints)
    check_arguments(waypoints, temperature, t_range, n_temps, rounds, steps)
    n_temps, rounds = int(n_temps), int(rounds)
    t_in = float(np.float32(temperature))
    bracket = (float(t_range[0]), float(t_range[1]))
    was_training = [(m, m.training) for m in model.modules()]      # (per module: a frozen sub-module may differ from the root)
    model.eval()
    curves, warned = [], False
    try:
        with torch.no_grad():
            ops.refresh_filters(model)
            ops.check_likelihood_status()      # a report left pending by an earlier call of the caller's is raised, not swallowed below
            for _ in range(rounds):
                temps = temperature_grid(bracket[0], bracket[1], n_temps, include=t_in)
                nll_parts, hpd_parts = [], []
                for trajectory, _, scene_id in val_loader:
                    scene_image = model.segmentation(val_images[scene_id].to(device).unsqueeze(0))
                    scene_image = model.adapt_semantic(scene_image)
                    if swap_semantic:
                        scene_image = swap_pavement_terrain(scene_image)
                    if network == "embed":
                        scene_image = model.scene_embedding(scene_image)
                    planes = _selected_planes(steps, waypoints, trajectory.shape[1] - obs_len)
                    goal_col = planes.index(waypoints[-1])
                    for b in range(0, len(trajectory), batch_size):
                        batch = trajectory[b:b + batch_size]
                        gt_future = batch[:, obs_len:].to(device)
                        _, pred_goal_map, _ = _goal_maps(model, model.pred_features, scene_image, batch[:, :obs_len], input_template, waypoints,
                                                         obs_len, t_in, network)
                        if planes == list(range(planes[0], planes[0] + len(planes))):      # a channel range is read in place
                            maps, gt = pred_goal_map[:, planes[0]:planes[0] + len(planes)], gt_future[:, planes[0]:planes[0] + len(planes)]
                        else:
                            maps, gt = pred_goal_map[:, planes], gt_future[:, planes]
                        res = ops.map_likelihood_sweep(maps, gt, temps)      # every temperature of the round: one launch, one read
                        nll_parts.append(res["nll"])
                        hpd_parts.append(res["hpd"][:, :, goal_col])
                        if ops.check_likelihood_status(raise_error=False) and not warned:
                            warned = True
                            warnings.warn("calibrate_temperature: a ground-truth position lies outside the map; its plane is left out")
                        ops.check_patch_status()
                if not nll_parts:
                    raise RuntimeError("calibrate_temperature: the loader holds no track")
                nll = torch.cat(nll_parts, dim=1).double()                      # [n_T, N, c]
                hpd = torch.cat(hpd_parts, dim=1)                               # [n_T, N]: the goal plane
                finite = torch.isfinite(nll).all(dim=0)                         # [N, c]: the same planes at every temperature
                n_planes = int(finite.sum())
                if n_planes == 0:
                    raise RuntimeError("calibrate_temperature: no plane has a finite NLL at every temperature of the grid "
                                       "(every ground truth outside its map, or maps without mass)")
                kept = torch.where(finite, nll, torch.zeros((), dtype=torch.float64, device=nll.device))
                per_step = kept.sum(dim=1) / finite.sum(dim=0).clamp(min=1)       # [n_T, c]
                curve = (kept.sum(dim=(1, 2)) / n_planes).cpu().numpy()
                curves.append((temps.copy(), curve))
                bracket = next_bracket(temps, curve)
    finally:
        for m, flag in was_training:
            m.training = flag
    temps, curve = curves[-1]
    t_best, k_best = best_temperature(temps, curve)
    k_in = int(np.flatnonzero(temps == np.float32(t_in))[0])
    step_counts = finite.sum(dim=0).cpu().numpy()
    per_step = per_step.cpu().numpy()
    temperature_steps = [best_temperature(temps, per_step[:, c])[0] if step_counts[c] > 0 else float("nan") for c in range(per_step.shape[1])]
    goal_ok = finite[:, goal_col]

    def ece(k):
        h = hpd[k][goal_ok].cpu().numpy()
        return calibration_curve(h)[2] if np.isfinite(h).any() else float("nan")

    return {"temperature": t_best, "nll": float(curve[k_best]), "nll_before": float(curve[k_in]), "ece": ece(k_best), "ece_before": ece(k_in),
            "curve": curves, "temperature_steps": temperature_steps, "excluded": int((~finite).sum()), "n_planes": n_planes,
            "at_boundary": bool(np.float32(t_best) in (np.float32(t_range[0]), np.float32(t_range[1])))}

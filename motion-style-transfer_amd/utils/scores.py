"""The goal-map scores of evaluate(): one scorer object per ``return_*`` flag.  Every score reads the goal decoder's distribution itself --
sigmoid(pred_goal_map / T), every plane normalised, what `sampling` draws from -- with one launch per batch and no draw; with any of them
on the sweep takes the branch ``return_preds`` takes (same launches and draws otherwise; the captured sweep is neither used nor touched).

evaluate() drives the scorers it keeps (``on``) through the methods of Score: start() in front of the sweep, scene() per loader item, per
batch score() -- or empty() on a data-parallel rank without rows -- after_draw(), gather() and collect(), and after the sweep columns() and
steps().  A batch's scores are a dict of device tensors, one row per agent.  A subclass states only what is special to it."""
import warnings

import numpy as np
import torch

from .. import ops
from .compliance import MAX_CLASSES, class_rates, point_classes, scene_labels
from .marginals import central_intervals, inside_intervals, marginal_levels
from .radial import radial_options, radial_summary
from .sharpness import inside_regions, level_name, sharpness_levels


class Score:
    keys = ()              # the keys of a batch's scores: one host list each
    step_names = {}        # key -> its name in trajs_dict without the "_steps", where that is not the key
    status = None          # ops.check_<status>_status tells what a launch could not score
    warning = None         # ... as this warning, once per evaluate() call; None: it raises
    collect_rank = 0       # collect() runs in ascending rank (ties: the order of df_out's columns)

    def __init__(self, on):      # (a subclass validates its flag's value here, before anything runs)
        self.on = bool(on)
        self.lists = {k: [] for k in self.keys}
        self.warned = False
        self._arrays = None

    def _check(self, **kw):
        return self.status is not None and getattr(ops, f"check_{self.status}_status")(**kw)

    def start(self, val_images):      # a report left pending by an earlier ops.map_* call of the caller's is raised, not swallowed by collect()
        self._check()

    def scene(self, scene_id, image, device):      # the scene's planes as prepare_data left them, before adapt_semantic / swap_semantic
        pass

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        """pred_goal_map [n, pred_len, H, W] and gt_future [n, pred_len, 2] (resized pixels) of a batch -> its scores"""
        raise NotImplementedError

    def after_draw(self, scores, waypoint_samples, scene_id):      # the way-points as drawn [K, n, n_wp, 2], in the map's pixels
        pass

    def empty(self, steps, device, scene_id):
        """The scores of a batch of no rows and ``steps`` = pred_len steps: score()'s keys, dtypes and trailing shapes"""
        raise NotImplementedError

    def gather(self, scores, dp, sizes):
        return {k: dp.gather_rows(v, sizes) for k, v in scores.items()}

    def collect(self, scores):
        for k, v in scores.items():
            self.lists[k].append(v.cpu().numpy())
        # (synchronised by the copies above: a plane the launch could not score raises or warns here)
        if self._check(raise_error=self.warning is None) and not self.warned:
            self.warned = True
            warnings.warn(self.warning, stacklevel=2)      # (at evaluate()'s line)

    def arrays(self):
        """-> {key: [N, pred_len, ...]}: the sweep's batches, concatenated once"""
        if self._arrays is None:
            self._arrays = {k: np.concatenate(v, axis=0) for k, v in self.lists.items()}
        return self._arrays

    def columns(self, df_out):
        raise NotImplementedError

    def steps(self, trajs_dict):
        for k, v in self.arrays().items():
            trajs_dict[self.step_names.get(k, k) + "_steps"] = v


class LikelihoodScore(Score):
    """``return_likelihood``: the distribution against the ground truth (ops.map_likelihood).  df_out gains the
    columns ``nll`` (mean over the pred_len steps, nats), ``nll_goal``, ``entropy_goal`` and ``hpd_goal`` (last step), and with
    ``return_preds`` trajs_dict gains ``nll_steps``, ``entropy_steps`` and ``hpd_steps`` [N, pred_len].  A step whose ground truth lies
    outside the map has NaN nll / hpd (one warning per call)."""
    keys = ops.LIKELIHOOD_OUTPUTS
    status = "likelihood"
    warning = ("evaluate(return_likelihood=True): a ground-truth position lies outside the map; its nll and hpd "
               "are NaN (ADE / FDE are unaffected; utils.likelihood.calibration_curve leaves NaN entries out)")
    collect_rank = 1

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        return ops.map_likelihood(pred_goal_map, gt_future, temperature)

    def empty(self, steps, device, scene_id):
        return {k: torch.zeros((0, steps), device=device) for k in self.keys}

    def columns(self, df_out):
        a = self.arrays()
        df_out["nll"] = a["nll"].mean(axis=1)
        df_out["nll_goal"] = a["nll"][:, -1]
        df_out["entropy_goal"] = a["entropy"][:, -1]
        df_out["hpd_goal"] = a["hpd"][:, -1]


class ComplianceScore(Score):
    """``return_compliance``: the distribution against the scene (ops.map_class_mass).  The classes are
    utils.compliance.scene_labels(val_images[scene_id]) -- the world's classes, taken before ``swap_semantic`` and the scene embedding,
    K = the number of planes (a scene with more than 8 raises before the sweep starts).  df_out gains ``goal_mass_<k>`` (the share of the
    last step's distribution on class k), ``gt_goal_class`` (the class of the ground-truth goal pixel, -1 outside the map) and
    ``sample_goal_rate_<k>`` (the fraction of the sampled goals on class k); with ``return_preds`` trajs_dict gains ``class_mass_steps``
    [N, pred_len, K]."""
    keys = ("mass", "gt_class", "rate")

    def __init__(self, on):
        super().__init__(on)
        self.label_maps = {}      # scene id -> (labels [H, W] uint8 on the device, K)

    def start(self, val_images):      # (before the sweep starts, not at the first batch of the offending scene)
        for sid, im in val_images.items():
            if im.dim() == 3 and im.shape[0] > MAX_CLASSES:
                raise ValueError(f"evaluate(return_compliance=True): scene {sid} has {im.shape[0]} planes; the classes of at most "
                                 f"{MAX_CLASSES} planes are told apart")

    def scene(self, scene_id, image, device):      # once per scene
        if scene_id not in self.label_maps:
            self.label_maps[scene_id] = (scene_labels(image.to(device)), image.shape[0])

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        labels, n_cls = self.label_maps[scene_id]
        return {"mass": ops.map_class_mass(pred_goal_map, labels, n_cls, temperature), "gt_class": point_classes(gt_future[:, -1], labels)}

    def after_draw(self, scores, waypoint_samples, scene_id):      # the goals as drawn (before ETH's world coordinates)
        labels, n_cls = self.label_maps[scene_id]
        scores["rate"] = class_rates(point_classes(waypoint_samples[:, :, -1], labels), n_cls, dim=0).t().contiguous()

    def empty(self, steps, device, scene_id):
        n_cls = self.label_maps[scene_id][1]
        return {"mass": torch.zeros((0, steps, n_cls), device=device), "gt_class": torch.zeros(0, device=device, dtype=torch.int64),
                "rate": torch.zeros((0, n_cls), device=device, dtype=torch.float64)}

    def arrays(self):
        widths = {m.shape[-1] for m in self.lists["mass"]}
        if len(widths) != 1:
            raise ValueError(f"evaluate(return_compliance=True): the scenes differ in their number of planes ({sorted(widths)}); "
                             f"one table needs one set of classes")
        return super().arrays()

    def columns(self, df_out):
        a = self.arrays()
        for k in range(a["mass"].shape[-1]):
            df_out[f"goal_mass_{k}"] = a["mass"][:, -1, k]
        df_out["gt_goal_class"] = a["gt_class"]
        for k in range(a["rate"].shape[-1]):
            df_out[f"sample_goal_rate_{k}"] = a["rate"][:, k]

    def steps(self, trajs_dict):
        trajs_dict["class_mass_steps"] = self.arrays()["mass"]


class SharpnessScore(Score):
    """``return_sharpness`` (False, True = (0.5, 0.9), or a tuple of 1 .. 8 ascending levels in (0, 1)): how LARGE the credible regions of
    the distribution are, where ``hpd`` says how well calibrated (ops.map_credible): per level q the smallest set
    of whole logit plateaus that holds q of the mass.  df_out gains ``area<pct>_goal`` (pixels of the resized map, last step; -1 for a
    plane with a NaN) and ``inside<pct>_goal`` (1.0 / 0.0: the logit at the rounded ground-truth goal is >= the region's threshold; NaN
    where it rounds outside the map) per level, <pct> = 100 q; with ``return_preds`` trajs_dict gains ``area_steps`` (int32),
    ``threshold_steps`` and ``inside_steps``, each [N, pred_len, L].  A NaN logit in a goal map raises at its batch."""
    keys = ("area", "threshold", "inside")
    status = "credible"

    def __init__(self, return_sharpness):
        self.levels = sharpness_levels(return_sharpness)
        super().__init__(self.levels is not None)

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        sharp = ops.map_credible(pred_goal_map, self.levels, temperature)
        return {"area": sharp["area"], "threshold": sharp["threshold"], "inside": inside_regions(pred_goal_map, gt_future, sharp["threshold"])}

    def empty(self, steps, device, scene_id):
        shape = (0, steps, len(self.levels))
        return {"area": torch.zeros(shape, device=device, dtype=torch.int32), "threshold": torch.zeros(shape, device=device),
                "inside": torch.zeros(shape, device=device)}

    def columns(self, df_out):
        a = self.arrays()
        for l, q in enumerate(self.levels):
            df_out[f"area{level_name(q)}_goal"] = a["area"][:, -1, l]
            df_out[f"inside{level_name(q)}_goal"] = a["inside"][:, -1, l]


class RadialScore(Score):
    """``return_radial`` (False, True = {'radii': (4, 8, 16), 'k': (1, 5, 20)}, or such a dict): the goal error the distribution implies
    (ops.map_radial, utils/radial.py), from the mass profile of every step's plane around its ground truth
    (resized pixels; a ground truth outside the map is scored too).  df_out gains, for the last step, ``radial_mean_goal`` and
    ``radial_rms_goal`` (the expected error of ONE draw and its root mean square), ``best_of_<K>_lower_goal`` / ``best_of_<K>_upper_goal``
    per K (a bracket, one resized pixel wide, around the expectation of what best-of-K FDE samples) -- all four in the units of the sdd FDE,
    resized pixels / resize_factor -- and ``hit<r>_goal`` per radius (the mass closer than r RESIZED pixels to the goal); with
    ``return_preds`` trajs_dict gains ``radial_mean_steps``, ``radial_rms_steps`` [N, pred_len], ``radial_hit_steps`` [N, pred_len, n_radii],
    ``best_of_k_lower_steps`` and ``best_of_k_upper_steps`` [N, pred_len, n_k].  Only these reduced quantities are kept per batch, never
    the profile.  A plane that cannot be scored (a NaN logit; a ground truth that is NaN or more than 16384 pixels outside the map) is NaN
    (one warning per call for the latter)."""
    keys = ("mean", "rms", "hit", "best_of_k_lower", "best_of_k_upper")
    step_names = {"mean": "radial_mean", "rms": "radial_rms", "hit": "radial_hit"}
    status = "radial"
    warning = ("evaluate(return_radial=...): a ground-truth position is NaN or more than 16384 pixels outside the "
               "map; its radial scores are NaN (ADE / FDE are unaffected)")

    def __init__(self, return_radial):
        opts = radial_options(return_radial)
        super().__init__(opts is not None)
        self.radii, self.ks = (opts["radii"], opts["k"]) if self.on else ((), ())

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        n_rings = min(ops.RADIAL_MAX_RINGS, max(ops.radial_rings(H, W), max(self.radii)))
        rad = radial_summary(ops.map_radial(pred_goal_map, gt_future, n_rings, temperature), gt_future, H, W, self.radii, self.ks)
        for k in ("mean", "rms", "best_of_k_lower", "best_of_k_upper"):      # the units of evaluate()'s ADE / FDE
            rad[k] = rad[k] / resize_factor
        return rad

    def empty(self, steps, device, scene_id):
        tails = {"mean": (), "rms": (), "hit": (len(self.radii),), "best_of_k_lower": (len(self.ks),), "best_of_k_upper": (len(self.ks),)}
        return {k: torch.zeros((0, steps) + tails[k], device=device, dtype=torch.float64) for k in self.keys}

    def columns(self, df_out):
        a = self.arrays()
        df_out["radial_mean_goal"] = a["mean"][:, -1]
        df_out["radial_rms_goal"] = a["rms"][:, -1]
        for j, r in enumerate(self.radii):
            df_out[f"hit{r}_goal"] = a["hit"][:, -1, j]
        for j, k in enumerate(self.ks):
            df_out[f"best_of_{k}_lower_goal"] = a["best_of_k_lower"][:, -1, j]
            df_out[f"best_of_{k}_upper_goal"] = a["best_of_k_upper"][:, -1, j]


class MarginalScore(Score):
    """``return_marginals`` (False, True = (0.5, 0.9), or a tuple of 1 .. 8 ascending levels in (0, 1)): the distribution per axis
    (ops.map_marginals, utils/marginals.py), from the x- and the y-marginal of every step's plane (resized pixels;
    a ground truth outside the map is scored too).  df_out gains, for the last step, ``crps_x_goal``, ``crps_y_goal`` and ``crps_goal``
    (their sum) -- the continuous ranked probability score, a proper score in the units of the sdd FDE, resized pixels / resize_factor --
    ``pit_x_goal`` and ``pit_y_goal`` (the mid-point of the probability integral transform's two ends), and per level
    ``width<pct>_x_goal`` / ``width<pct>_y_goal`` (hi - lo of the central interval, in the units of the CRPS columns) and
    ``inside<pct>_x_goal`` / ``inside<pct>_y_goal`` (1.0 / 0.0: the rounded ground truth lies inside it; NaN where it cannot be scored);
    with ``return_preds`` trajs_dict gains ``crps_steps`` [N, pred_len, 2], ``pit_steps`` [N, pred_len, 2, 2] and ``interval_steps``
    [N, pred_len, 2, L, 2] (axis; level; lo, hi pixel indices of the resized map).  Only these reduced quantities are kept per batch,
    never the profiles.  A plane that cannot be scored (a NaN logit; a ground truth that is NaN or more than 16384 pixels outside the
    map) is NaN (one warning per call for the latter)."""
    keys = ("crps", "pit", "interval", "inside", "width")
    status = "marginals"
    warning = ("evaluate(return_marginals=...): a ground-truth position is NaN or more than 16384 pixels outside the "
               "map; its crps, pit and inside columns are NaN (ADE / FDE are unaffected)")

    def __init__(self, return_marginals):
        self.levels = marginal_levels(return_marginals)
        super().__init__(self.levels is not None)

    def score(self, pred_goal_map, gt_future, temperature, H, W, resize_factor, scene_id):
        m = ops.map_marginals(pred_goal_map, gt_future, temperature)
        interval = torch.stack([central_intervals(m["col"], self.levels), central_intervals(m["row"], self.levels)], dim=2)
        inside = inside_intervals(interval, gt_future.to(interval.device))      # [n, pred_len, 2 (x, y), L]
        nan = torch.full((), float("nan"), dtype=torch.float64, device=inside.device)
        inside = torch.where(~torch.isnan(m["crps"])[..., None], inside, nan)      # (a ground truth the launch could not score)
        width = torch.where(interval[..., 0] >= 0, (interval[..., 1] - interval[..., 0]).double() / resize_factor, nan)      # the units of evaluate()'s ADE / FDE
        return {"crps": m["crps"].double() / resize_factor, "pit": m["pit"], "interval": interval, "inside": inside, "width": width}

    def empty(self, steps, device, scene_id):
        L = len(self.levels)
        return {"crps": torch.zeros((0, steps, 2), device=device, dtype=torch.float64), "pit": torch.zeros((0, steps, 2, 2), device=device),
                "interval": torch.zeros((0, steps, 2, L, 2), device=device, dtype=torch.int64),
                "inside": torch.zeros((0, steps, 2, L), device=device, dtype=torch.float64),
                "width": torch.zeros((0, steps, 2, L), device=device, dtype=torch.float64)}

    def columns(self, df_out):
        a = self.arrays()
        df_out["crps_x_goal"] = a["crps"][:, -1, 0]
        df_out["crps_y_goal"] = a["crps"][:, -1, 1]
        df_out["crps_goal"] = a["crps"][:, -1, 0] + a["crps"][:, -1, 1]
        pit = a["pit"].astype(np.float64)
        df_out["pit_x_goal"] = 0.5 * (pit[:, -1, 0, 0] + pit[:, -1, 0, 1])
        df_out["pit_y_goal"] = 0.5 * (pit[:, -1, 1, 0] + pit[:, -1, 1, 1])
        for l, q in enumerate(self.levels):
            for j, axis in enumerate("xy"):
                df_out[f"width{level_name(q)}_{axis}_goal"] = a["width"][:, -1, j, l]
                df_out[f"inside{level_name(q)}_{axis}_goal"] = a["inside"][:, -1, j, l]

    def steps(self, trajs_dict):
        a = self.arrays()
        trajs_dict["crps_steps"] = a["crps"]
        trajs_dict["pit_steps"] = a["pit"]
        trajs_dict["interval_steps"] = a["interval"]

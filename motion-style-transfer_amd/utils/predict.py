"""Forecasts without ground truth: a scene and the observed steps alone -> the K = n_goal * n_traj sampled futures of every
agent, scored against the goal map and ranked.

The reference has no such call: its utils/evaluate.py:37-315 needs obs_len + pred_len steps per agent and keeps only the sample
closest to the ground truth; its plotting helpers re-run ``test`` for n_round rounds instead.  ``predict`` runs the same calls in
the same order as the non-plain branch of ``evaluate`` (utils/evaluate.py:109-266: encoder + goal decoder, sigmoid(x / T), goal /
way-point draws with optional TTST and CWS, the K folded trajectory-decoder passes) and then ONE launch of
``ynet_score_rank_samples``: score_k = sum over the way-points of log(sigmoid map at the sampled pixel + 1e-12), samples handed
back by descending score.  Every draw takes its seed from torch's CPU generator (NumPy's for the TTST centres) in evaluate()'s
order, so under torch.manual_seed(s) predict() on the first obs_len steps of a batch takes exactly the draws evaluate() takes on
that batch.  Nothing is captured into a hipGraph here; evaluate()'s captured-sweep cache is not touched.

``predict_styles`` is predict() for a scene whose agents wear different styles: one frozen model, the adapter sets of a
models.style_bank.StyleBank, one call.

``predict_modes`` is predict() with no draw at all: the goals are the modes of the goal map's logits under greedy non-maximum
suppression (ops.map_modes), each with the probability mass it claims.

``predict_with_entropy``, ``predict_with_compliance`` and ``predict_with_regions`` are predict() plus one read-out of the goal map
each: its entropy, the share of it on every semantic class of the scene (ops.map_class_mass, DESIGN.md
section 4.13), and its credible regions (ops.map_credible).  ``predict_with_intervals`` is predict() plus the median and
central intervals of the goal map's x- and y-marginal (ops.map_marginals).  ``predict_with_occupancy`` is predict() plus the
one read-out that is about the scene and not about an agent: the agents' goal maps summed per step, and the expected conflicts between
them (ops.map_occupancy).
"""
import functools
import inspect
import math

import numpy as np
import torch

from .. import ops
from .evaluate import _decoder_passes, _draw_waypoints, _goal_maps      # (evaluate()'s own steps, not copies)
from .image_utils import swap_pavement_terrain

MAX_SAMPLES = 64      # ynet_score_rank_samples ranks the samples of an agent on the lanes of one wavefront


def _validated(name, observed, scene_image, waypoints, n_goal, n_traj, obs_len, resize_factor, use_CWS, CWS_params, batch_size, forced_samples,
               bank=None, style=None):
    """Everything `name` (predict / predict_styles) refuses before the device is touched -> (observed as a float tensor [N, obs_len, 2],
    waypoints, n_goal, n_traj, obs_len, and with a ``bank`` the style index [N] of every agent)"""
    waypoints = list(waypoints)
    n_wp = len(waypoints)
    n_goal, n_traj, obs_len = int(n_goal), int(n_traj), int(obs_len)
    K = n_goal * n_traj
    if n_goal < 1 or n_traj < 1:
        raise ValueError(f"{name}: n_goal = {n_goal}, n_traj = {n_traj}: at least one sample per agent is needed")
    if K > MAX_SAMPLES:
        raise ValueError(f"{name}: n_goal * n_traj = {K} samples per agent; the ranking kernel takes up to {MAX_SAMPLES}")
    if n_wp < 1:
        raise ValueError(f"{name}: no way-points")
    if use_CWS and n_wp > 1 and CWS_params is None:
        raise ValueError(f"{name}: use_CWS needs CWS_params (sigma_factor, ratio, rot)")
    if not float(resize_factor) > 0:
        raise ValueError(f"{name}: resize_factor must be positive")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError(f"{name}: batch_size must be positive")
    obs = observed.detach() if torch.is_tensor(observed) else torch.from_numpy(np.ascontiguousarray(np.asarray(observed, dtype=np.float32)))
    if obs.dim() != 3 or obs.shape[2] != 2:
        raise ValueError(f"{name}: observed must be [N, obs_len, 2] (x, y) in resized pixel coordinates, got {tuple(obs.shape)}")
    if obs.shape[1] != obs_len:
        raise ValueError(f"{name}: observed holds {obs.shape[1]} steps per agent, obs_len is {obs_len}: pass exactly the observed steps "
                         f"(a longer track is never cut silently)")
    if not torch.is_tensor(scene_image) or scene_image.dim() != 3:
        raise ValueError(f"{name}: scene_image must be the tensor [C, H, W] of one scene")
    N = obs.shape[0]
    if N == 0:
        raise ValueError(f"{name}: no agents (observed is empty)")
    style_index = None
    if bank is not None:
        style_index = np.asarray(bank.indices(style), dtype=np.int64)      # (an unknown style is refused here)
        if style_index.shape != (N,):
            raise ValueError(f"{name}: {style_index.size} styles for {N} agents: one name or index per agent is needed")
    if torch.is_tensor(forced_samples) and tuple(forced_samples.shape) != (K, N, n_wp, 2):
        raise ValueError(f"{name}: forced_samples {tuple(forced_samples.shape)}, expected {(K, N, n_wp, 2)}"
                         + ("" if bank is None else " in the caller's order"))
    return obs.float(), waypoints, n_goal, n_traj, obs_len, style_index


def disk_area(radius):
    """A(r) = #{(dx, dy) : dx^2 + dy^2 <= r^2}: the pixels one mode suppresses at most"""
    r = int(radius)
    return sum(2 * math.isqrt(r * r - dx * dx) + 1 for dx in range(-r, r + 1))


def _check_modes_fit(name, n_modes, radius, H, W):
    """(n_modes - 1) * A(radius) < H * W: the first n_modes - 1 disks cannot cover the map, so finite logits always give n_modes modes"""
    area = disk_area(min(radius, H + W))      # (beyond H + W a disk holds the whole map anyway)
    if (n_modes - 1) * area >= H * W:
        raise ValueError(f"{name}: {n_modes} modes of radius {radius} ({area} pixels each) may not fit the {H}x{W} map: "
                         f"(n_modes - 1) * A(radius) = {(n_modes - 1) * area} >= {H * W}; ask for fewer modes or a smaller radius")


def _mode_waypoints(model, wp_sigmoid, pred_goal_map, batch, waypoints, n_modes, radius, obs_len, temperature, device, CWS_params):
    """The way-points of predict_modes for one chunk, with no draw -> ([n_modes, n, n_wp, 2], {"mass", "logit": [n, n_modes] in mode
    order, "short": [n] bool, an agent with fewer modes than asked for}).
    Goals: the modes of the RAW goal logits (a saturated fp32 sigmoid ties pixels whose logits differ).  Intermediate way-points: with
    CWS_params the expectation chain of cws_waypoints (n_traj = 1: no `sampling` call); without, the top pixel of each intermediate
    plane's logits, shared by the modes.  An entry no mode filled is (-1, -1): it is moved onto pixel (0, 0), so that the chunk's
    launches stay inside the map until its sync point, where _forecast raises."""
    last = waypoints[-1]
    goal = ops.map_modes(pred_goal_map[:, last:last + 1], n_modes, radius, temperature)
    found = {"mass": goal["mass"][:, 0], "logit": goal["logit"][:, 0], "short": goal["count"][:, 0] < n_modes}
    goals = goal["xy"][:, 0].clamp_min(0.0).permute(1, 0, 2).unsqueeze(2)      # [n_modes, n, 1, 2]
    if len(waypoints) == 1 or CWS_params is not None:
        return _draw_waypoints(model, wp_sigmoid, pred_goal_map, batch, waypoints, n_modes, 1, obs_len, device, use_CWS=CWS_params is not None,
                               CWS_params=CWS_params, forced_goals=goals), found
    tops = [ops.map_modes(pred_goal_map[:, w:w + 1], 1, 0, want_mass=False) for w in waypoints[:-1]]
    for t in tops:
        found["short"] = found["short"] | (t["count"][:, 0] < 1)
    inter = torch.stack([t["xy"][:, 0, 0] for t in tops], dim=1).clamp_min(0.0)      # [n, n_wp - 1, 2]
    return torch.cat([inter.unsqueeze(0).expand(n_modes, -1, -1, -1), goals], dim=2), found


def _forecast(name, model, refresh, chunk_plan, scene_image, obs, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature,
              use_TTST, use_CWS, rel_thresh, CWS_params, network, swap_semantic, batch_size, max_effective_batch, forced_samples, return_maps,
              return_entropy, modes=None, return_compliance=False, occupancy=None, intervals=None, regions=None):
    """The one body of predict(), predict_with_entropy(), predict_styles() and predict_modes(), on arguments that went through _validated.
    modes              None, or (n_modes, radius): the way-points are not drawn but read off the goal map (_mode_waypoints; then
                       n_goal = n_modes, n_traj = 1, and the results gain ``mode_mass`` and ``mode_logit``)
    return_compliance  the results gain ``goal_class_mass`` [N, pred_len, K]: one ops.map_class_mass launch per chunk against
                       utils.compliance.scene_labels(scene_image), the classes of the scene as given (before ``swap_semantic``)
    regions            None, or the credible levels (ops.credible_levels): the results gain ``region_area`` (int32), ``region_threshold``
                       and ``region_mass`` [N, pred_len, L]: one ops.map_credible launch per chunk
    intervals          None, or the levels of the central intervals (utils.marginals.marginal_levels): the results gain ``median_xy`` and
                       ``marginal_mean_xy`` [N, pred_len, 2] and ``interval_xy`` [N, pred_len, 2, L, 2] (axis; level; lo, hi) in pixels of
                       the resized map: one ops.map_marginals launch per chunk, without ground truth
    occupancy          None, or the cell edge (1, 2, 4, 8): the results gain ``occupancy`` and ``occupancy_any`` [pred_len, Hc, Wc],
                       ``conflict`` [pred_len] and ``risk`` [N, pred_len] from one ops.map_occupancy call; the scene must run as ONE
                       chunk (the pairs across two chunks would be lost), anything else is refused before the model is touched
    refresh()          packs the filters the chunks will read, on the caller's stream, before the decoder passes fan out over two (see
                       evaluate()): ops.refresh_filters(model), or a StyleBank's refresh() for its shadows and the shared layers
    chunk_plan(b, n)   for the n agents from b on -> (perm, pred_features): ``perm`` None, or the order the chunk runs in (row j of the
                       sweep is the chunk's agent perm[j]); ``pred_features`` the feature function of the chunk in that order
    When ``perm`` is the identity (or None) nothing is gathered and the ranking launch writes row b at row b; otherwise the observed
    steps and forced samples are gathered into the sweep's order, the ranking launch writes every agent's results at its row of the
    caller's order, and the maps, when asked for, are gathered back."""
    n_wp, K = len(waypoints), n_goal * n_traj
    N = obs.shape[0]
    step = N if batch_size is None else int(batch_size)
    if occupancy is not None and step < N:
        raise ValueError(f"{name}: the occupancy of a scene needs all its {N} agents in one chunk, batch_size = {step} would split them "
                         f"(the pairs across two chunks would be lost); pass batch_size=None or >= {N}")
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    out = {k: [] for k in ["trajectories", "waypoints", "scores", "order"] + (["goal_map", "goal_sigmoid_map"] if return_maps else [])
           + (["entropy"] if return_entropy else []) + (["mode_mass", "mode_logit"] if modes is not None else [])
           + (["goal_class_mass"] if return_compliance else [])
           + (["region_area", "region_threshold", "region_mass"] if regions is not None else [])
           + (["occupancy", "occupancy_any", "conflict", "risk"] if occupancy is not None else [])
           + (["median_xy", "interval_xy", "marginal_mean_xy"] if intervals is not None else [])}
    try:
        with torch.no_grad():
            refresh()
            scene = model.segmentation(scene_image.to(device).unsqueeze(0))
            if return_compliance:
                from .compliance import scene_labels
                labels = scene_labels(scene_image.to(device))      # (more than 8 planes: refused here, before any chunk runs)
            scene = model.adapt_semantic(scene)
            if swap_semantic:
                scene = swap_pavement_terrain(scene)
            if network == "embed":
                scene = model.scene_embedding(scene)
            _, _, H, W = scene.shape
            if modes is not None:
                _check_modes_fit(name, *modes, H, W)
            for b in range(0, N, step):
                batch = obs[b:b + step]
                n = len(batch)
                perm, pred_features = chunk_plan(b, n)
                mixed = perm is not None and not np.array_equal(perm, np.arange(n))
                if mixed:
                    perm_dev = torch.from_numpy(perm.astype(np.int32)).to(device)
                    batch = ops.gather_rows(batch.to(device).contiguous(), perm_dev)
                features, pred_goal_map, wp_sigmoid = _goal_maps(model, pred_features, scene, batch, input_template, waypoints, obs_len,
                                                                 temperature, network)

                if forced_samples is not None:
                    forced = forced_samples[:, b:b + n] if torch.is_tensor(forced_samples) else forced_samples[b]
                    waypoint_samples = forced.to(device)
                    if tuple(waypoint_samples.shape) != (K, n, n_wp, 2):
                        raise ValueError(f"{name}: forced samples {tuple(waypoint_samples.shape)} for the chunk at {b}, expected {(K, n, n_wp, 2)}")
                    if mixed:      # a row gather inside each of the K slabs
                        slab_rows = (torch.arange(K, device=device, dtype=torch.int32)[:, None] * n + perm_dev[None]).reshape(-1)
                        waypoint_samples = ops.gather_rows(waypoint_samples.float().contiguous().view(K * n, n_wp, 2), slab_rows).view(K, n, n_wp, 2)
                elif modes is not None:
                    waypoint_samples, found = _mode_waypoints(model, wp_sigmoid, pred_goal_map, batch, waypoints, *modes, obs_len, temperature,
                                                              device, CWS_params)
                else:      # (over the chunk as it runs: draw row j belongs to sweep row j)
                    waypoint_samples = _draw_waypoints(model, wp_sigmoid, pred_goal_map, batch, waypoints, n_goal, n_traj, obs_len, device,
                                                       use_TTST, use_CWS, rel_thresh, CWS_params)
                waypoint_samples = waypoint_samples.float().contiguous()

                if return_maps:
                    maps = {"goal_map": pred_goal_map, "goal_sigmoid_map": model.sigmoid(pred_goal_map / temperature)}
                    if mixed:
                        back = torch.from_numpy(np.argsort(perm).astype(np.int32)).to(device)      # caller row i <- sweep row back[i]
                        maps = {k: ops.gather_rows(v.contiguous(), back) for k, v in maps.items()}
                    for k, v in maps.items():
                        out[k].append(v)
                if return_entropy:
                    out["entropy"].append(ops.map_likelihood(pred_goal_map, None, temperature, want=("entropy",))["entropy"])
                if return_compliance:
                    out["goal_class_mass"].append(ops.map_class_mass(pred_goal_map, labels, scene_image.shape[0], temperature))
                if regions is not None:
                    for k, v in ops.map_credible(pred_goal_map, regions, temperature).items():
                        out["region_" + k].append(v)
                if intervals is not None:
                    from .marginals import central_intervals, profile_mean, quantiles
                    marg = ops.map_marginals(pred_goal_map, None, temperature, want=("col", "row"))
                    axes = (marg["col"], marg["row"])      # (x, y): the index along an axis is the pixel coordinate, as the way-points'
                    out["median_xy"].append(torch.stack([quantiles(p, (0.5,))[..., 0] for p in axes], dim=-1).float())
                    out["interval_xy"].append(torch.stack([central_intervals(p, intervals) for p in axes], dim=2).float())
                    out["marginal_mean_xy"].append(torch.stack([profile_mean(p) for p in axes], dim=-1).float())
                if occupancy is not None:      # (one group: the chunk is the scene)
                    occ = ops.map_occupancy(pred_goal_map, None, occupancy, temperature)
                    out["occupancy"].append(occ["occupancy"][0])
                    out["occupancy_any"].append(occ["any"][0])
                    out["conflict"].append(occ["conflict"][0])
                    out["risk"].append(occ["risk"])

                trajs_samples = _decoder_passes(model, features, waypoint_samples, input_template, n, n_wp, H, W, max_effective_batch, device)
                ranking = (wp_sigmoid, waypoint_samples, trajs_samples.contiguous(), resize_factor)
                ranked, ranked_goals, score, order = ops.score_rank_samples_rows(*ranking, perm) if mixed else ops.score_rank_samples(*ranking)
                out["trajectories"].append(ranked)
                out["waypoints"].append(ranked_goals)
                out["scores"].append(score)
                out["order"].append(order)
                ops.check_patch_status()      # (the ranking call waited for the chunk: a window that left the template raises here)
                if perm is not None:
                    ops.check_gather_status()
                if regions is not None:
                    ops.check_credible_status()      # (a NaN logit in a goal map of the chunk raises here)
                if occupancy is not None:
                    ops.check_occupancy_status()
                if modes is not None:
                    nan = ops.check_modes_status(raise_error=False)
                    short = torch.nonzero(found["short"]).flatten().tolist()
                    if short:
                        raise RuntimeError(f"{name}: agent {b + short[0]}" + (f" (and {len(short) - 1} more)" if len(short) > 1 else "")
                                           + f": fewer than the {modes[0]} modes asked for; its goal map holds "
                                           + ("a NaN" if nan else "too few logits above -inf"))
                    out["mode_mass"].append(found["mass"].gather(1, order.long()))      # (row r is mode order[:, r])
                    out["mode_logit"].append(found["logit"].gather(1, order.long()))
    finally:
        model.train(was_training)
    return {k: (v[0] if len(v) == 1 else torch.cat(v)) for k, v in out.items()}


def predict(model, scene_image, observed, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature,
            use_TTST=False, use_CWS=False, rel_thresh=0.002, CWS_params=None, network=None, swap_semantic=False, batch_size=None,
            max_effective_batch=256, forced_samples=None, return_maps=False):
    """K = n_goal * n_traj ranked forecasts per agent of ONE scene.

    scene_image      what ``val_images[scene_id]`` holds for evaluate(): the pre-processed planes [C, H, W] of the scene
    observed         [N, obs_len, 2] (x, y), already in resized pixel coordinates (the SceneDataset contract); host array / tensor
                     (window checks on the host) or device tensor
    forced_samples   (tests) as for evaluate(): {first agent of a chunk: [K, n, n_wp, 2]}, or one tensor [K, N, n_wp, 2]
    batch_size       agents per chunk (None: all at once)
    -> dict of device tensors: ``trajectories`` [N, K, pred_len, 2] best first, in original-image pixels (the convention of
       trajs_dict["prediction"]), ``waypoints`` [N, K, n_wp, 2] (resized pixels, as sampled), ``scores`` [N, K] descending,
       ``order`` [N, K] int32 (row r is sample order[:, r] of the sweep), and with ``return_maps`` ``goal_map`` [N, pred_len, H, W]
       and ``goal_sigmoid_map`` as evaluate(return_samples=True) stores them.
       predict_with_entropy() is this call plus ``entropy`` [N, pred_len]: how spread out every step's goal-map distribution is;
       predict_with_compliance() is this call plus ``goal_class_mass`` [N, pred_len, K]: the share of it on every class of the scene;
       predict_with_regions() is this call plus the credible regions of it, ``region_area`` / ``region_threshold`` / ``region_mass``;
       predict_with_occupancy() is this call plus the scene's ``occupancy`` / ``occupancy_any`` / ``conflict`` / ``risk``."""
    return _predict(False, **locals())


def predict_with_entropy(*args, **kwargs):
    """predict() with the same arguments, and one more result: ``entropy`` [N, pred_len] (device tensor), the entropy in nats of every
    future step's goal-map distribution -- sigmoid(pred_goal_map / T) normalised per plane, what `sampling` draws from.  It needs no
    ground truth and no draw: one ops.map_likelihood launch per chunk in its form without ground truth, the
    values evaluate(return_likelihood=True) reports as ``entropy_steps``.  Every other result is predict()'s, bit for bit.
    (A function of its own and not a keyword of predict(): predict()'s parameter list is pinned by tests/test_predict_host.py.)"""
    bound = _PREDICT_SIGNATURE.bind(*args, **kwargs)
    bound.apply_defaults()
    return _predict(True, **bound.arguments)


def predict_with_compliance(*args, return_entropy=False, **kwargs):
    """predict() with the same arguments, and one more result: ``goal_class_mass`` [N, pred_len, K] (device tensor, float32), the share
    of every future step's goal-map distribution -- sigmoid(pred_goal_map / T) normalised per plane, what `sampling` draws from -- that
    lies on each of the K classes of the scene (ops.map_class_mass, one launch per chunk).  The classes are
    utils.compliance.scene_labels(scene_image): K = the planes of ``scene_image`` (at most 8), taken as given, before
    ``swap_semantic``.  The values are the ones evaluate(return_compliance=True) reports as ``class_mass_steps``.
    ``return_entropy=True`` (keyword only) adds predict_with_entropy()'s ``entropy`` as well.  Every other result is predict()'s, bit
    for bit: no draw is added or moved.
    (A function of its own and not a keyword of predict(), as predict_with_entropy(): predict()'s parameter list is pinned by
    tests/test_predict_host.py, and predict_styles mirrors it.)"""
    bound = _PREDICT_SIGNATURE.bind(*args, **kwargs)
    bound.apply_defaults()
    return _predict(bool(return_entropy), **bound.arguments, return_compliance=True)


def predict_with_regions(*args, levels=(0.5, 0.9), **kwargs):
    """predict() with the same arguments, and three more results, each [N, pred_len, L] (device tensors): per future step and per level
    q of ``levels`` (keyword only; 1 .. 8 strictly ascending values inside (0, 1)) the q-credible region of the goal-map distribution --
    sigmoid(pred_goal_map / T) normalised per plane, what `sampling` draws from --, the smallest set of whole logit plateaus that holds
    q of the mass: ``region_threshold`` (float32; the region is {goal_map >= threshold}: utils.sharpness.region_mask draws it),
    ``region_area`` (int32, its pixels in the resized map) and ``region_mass`` (float32, the share it holds, >= q up to rounding).
    One ops.map_credible launch per chunk; the values are the ones evaluate(return_sharpness=levels) reports
    as ``area_steps`` and ``threshold_steps``.  It needs no ground truth and no draw; every other result is predict()'s, bit for bit.
    A goal map that holds a NaN raises RuntimeError at the chunk's sync point.
    (A function of its own and not a keyword of predict(), as predict_with_entropy(): predict()'s parameter list is pinned by
    tests/test_predict_host.py, and predict_styles mirrors it.)"""
    regions = tuple(float(q) for q in ops.credible_levels(levels, "predict_with_regions"))
    bound = _PREDICT_SIGNATURE.bind(*args, **kwargs)
    bound.apply_defaults()
    return _predict(False, **bound.arguments, regions=regions)


def predict_with_intervals(*args, levels=(0.5, 0.9), **kwargs):
    """predict() with the same arguments, and three more results (device tensors, float32): the forecast band per axis, as a pure function
    of (weights, scene, observed steps) -- per future step, from the x- and the y-marginal of the goal-map distribution (sigmoid(pred_goal_map
    / T) normalised per plane, what `sampling` draws from; its column and row sums):
      ``median_xy``         [N, pred_len, 2]         the median of each marginal
      ``interval_xy``       [N, pred_len, 2, L, 2]   (axis; level; lo, hi) the central interval per level q of ``levels`` (keyword only; 1 .. 8
                                                     strictly ascending values inside (0, 1)): its (1 - q) / 2 and (1 + q) / 2 quantiles, ends included
      ``marginal_mean_xy``  [N, pred_len, 2]         the mean of each marginal
    in pixels of the resized scene, the coordinates of ``waypoints`` (a quantile is the smallest pixel index whose CDF reaches it: utils.marginals).
    One ops.map_marginals launch per chunk without ground truth; the intervals are the ones
    evaluate(return_marginals=levels) reports as ``interval_steps``.  No draw; every other result is predict()'s, bit for bit.  A plane
    that holds a NaN has median and interval -1 and a NaN mean.
    (A function of its own and not a keyword of predict(), as predict_with_entropy(): predict()'s parameter list is pinned by
    tests/test_predict_host.py, and predict_styles mirrors it.)"""
    from .marginals import marginal_levels
    if isinstance(levels, bool) or levels is None:
        raise ValueError(f"predict_with_intervals: levels = {levels!r}: a sequence of 1 .. 8 ascending levels in (0, 1) is expected")
    intervals = marginal_levels(levels, "predict_with_intervals")
    bound = _PREDICT_SIGNATURE.bind(*args, **kwargs)
    bound.apply_defaults()
    return _predict(False, **bound.arguments, intervals=intervals)


def predict_with_occupancy(*args, cell=4, **kwargs):
    """predict() with the same arguments, and four more results (device tensors, float32) about the SCENE, not about one agent: the
    goal-map distributions of all N agents -- sigmoid(pred_goal_map / T) normalised per plane, what `sampling` draws from -- summed per
    future step over cells of ``cell`` x ``cell`` pixels of the resized map (keyword only; 1, 2, 4 or 8), the agents taken as
    independent:
      ``occupancy``      [pred_len, Hc, Wc]  the expected number of agents in the cell (every step sums to N)
      ``occupancy_any``  [pred_len, Hc, Wc]  the probability that the cell holds at least one agent
      ``conflict``       [pred_len]          the expected number of agent pairs that share a cell
      ``risk``           [N, pred_len]       the expected number of other agents in the agent's cell (sums to 2 * conflict per step)
    with Hc = ceil(H / cell), Wc = ceil(W / cell) (utils.occupancy: cell_grid, upsample_occupancy for overlays, conflict_report).
    One ops.map_occupancy call on the goal map.  It needs no ground truth and no draw; every other result is
    predict()'s, bit for bit.  The scene must run as ONE chunk: ``batch_size`` None or >= N.  Anything else raises ValueError, because
    the pairs of agents that fall into different chunks would be lost.  A goal map that holds a NaN raises RuntimeError at the chunk's
    sync point.
    Out of scope for now: evaluate(), a predict_styles or predict_modes form, scenes split over chunks, proximity within a radius
    instead of cell sharing, the trajectory decoder's maps, and capturing the call into a hipGraph.
    (A function of its own and not a keyword of predict(), as predict_with_entropy(): predict()'s parameter list is pinned by
    tests/test_predict_host.py, and predict_styles mirrors it.)"""
    if cell not in ops.OCCUPANCY_CELLS:
        raise ValueError(f"predict_with_occupancy: cell = {cell!r}, expected one of {ops.OCCUPANCY_CELLS}")
    bound = _PREDICT_SIGNATURE.bind(*args, **kwargs)
    bound.apply_defaults()
    return _predict(False, **bound.arguments, occupancy=int(cell))


def _predict(return_entropy, model, scene_image, observed, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature,
             use_TTST, use_CWS, rel_thresh, CWS_params, batch_size, forced_samples, **options):
    """predict() / predict_with_entropy(): no permutation, the model's own features and filters"""
    obs, waypoints, n_goal, n_traj, obs_len, _ = _validated("predict", observed, scene_image, waypoints, n_goal, n_traj, obs_len, resize_factor,
                                                            use_CWS, CWS_params, batch_size, forced_samples)
    return _forecast("predict", model, lambda: ops.refresh_filters(model), lambda b, n: (None, model.pred_features), scene_image, obs,
                     input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature, use_TTST=use_TTST, use_CWS=use_CWS,
                     rel_thresh=rel_thresh, CWS_params=CWS_params, batch_size=batch_size, forced_samples=forced_samples,
                     return_entropy=return_entropy, **options)


_PREDICT_SIGNATURE = inspect.signature(predict)


def predict_styles(bank, scene_image, observed, style, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature,
                   use_TTST=False, use_CWS=False, rel_thresh=0.002, CWS_params=None, network=None, swap_semantic=False, batch_size=None,
                   max_effective_batch=256, forced_samples=None, return_maps=False):
    """predict() over the agents of ONE scene that wear different styles of a StyleBank: the adapted encoder convolutions run once
    per style on that style's rows, every other layer and all K decoder passes once over the whole batch.

    bank             models.style_bank.StyleBank (holds the model)
    style            [N] style names or indices, one per agent (bank.names / bank.index; style_bank.BASE_STYLE = the model as loaded)
    forced_samples   as for predict(), in the CALLER's order: {first agent of a chunk: [K, n, n_wp, 2]} or one tensor [K, N, n_wp, 2]
    every other argument and every result as for predict(); the results are in the caller's order and carry ``style_index`` [N] (int64).
    The goal-map entropy of predict_with_entropy() is out of scope here for now: there is no predict_styles form of it.
    Neither is the scene compliance of predict_with_compliance(): out of scope here for now.
    Nor are the credible regions of predict_with_regions(), nor the scene occupancy of predict_with_occupancy().

    Each chunk (``batch_size`` agents of the caller's order; it may hold any subset of the styles) is stable-sorted by style index on
    the host -- the labels are host data.  ynet_gather_rows builds the sorted observed coordinates and forced samples, and
    ynet_score_rank_samples_rows writes every agent's ranked results at its row of the caller's order.  Without forced samples the
    draws are taken over the SORTED chunk: draw row j belongs to the j-th agent of the sorted order, so a mixed batch does not take
    the draws predict() would take for the caller's order.  When a chunk holds one style the sort is the identity, nothing is
    gathered and the launches are predict()'s on a model carrying that style.  With ``return_maps`` the maps are computed in sorted
    order and gathered back into the caller's order (one ynet_gather_rows pass over each map, paid only when the maps are asked for).
    evaluate()'s captured-sweep cache is neither used nor touched; the model's filter caches are not written (StyleBank)."""
    from ..models.style_bank import sort_by_style
    obs, waypoints, n_goal, n_traj, obs_len, style_index = _validated("predict_styles", observed, scene_image, waypoints, n_goal, n_traj, obs_len,
                                                                      resize_factor, use_CWS, CWS_params, batch_size, forced_samples, bank, style)

    def chunk_plan(b, n):      # the chunk stable-sorted by style, and the bank's features bound to the sorted chunk's row bounds
        perm, offsets = sort_by_style(style_index[b:b + n], len(bank))
        return perm, functools.partial(bank.pred_features, offsets=offsets)

    res = _forecast("predict_styles", bank.model, bank.refresh, chunk_plan, scene_image, obs, input_template, waypoints, n_goal, n_traj, obs_len,
                    resize_factor, temperature, use_TTST, use_CWS, rel_thresh, CWS_params, network, swap_semantic, batch_size,
                    max_effective_batch, forced_samples, return_maps, return_entropy=False)
    res["style_index"] = torch.from_numpy(style_index).to(res["scores"].device)
    return res


def predict_modes(model, scene_image, observed, input_template, waypoints, n_modes, radius, obs_len, resize_factor, temperature,
                  CWS_params=None, network=None, swap_semantic=False, batch_size=None, max_effective_batch=256, return_maps=False):
    """The n_modes most likely futures of every agent of ONE scene, with no draw: a pure function of (weights, scene, observed steps).
    No generator is read -- neither torch's nor NumPy's -- so two adapter sets can be compared forecast by forecast.

    n_modes, radius  the goals are the modes of the goal map under greedy non-maximum suppression (ops.map_modes on the raw logits of
                     the last way-point): the highest pixel, then the highest outside the disk of ``radius`` pixels around it, and
                     so on; 1 <= n_modes <= 64, radius >= 0, and (n_modes - 1) * A(radius) < H * W (disk_area), below which finite
                     logits always give n_modes modes
    CWS_params       with several way-points: given, the intermediate ones are the expectation chain of cws_waypoints from every
                     goal (deterministic); None, the top pixel of each intermediate plane's logits, shared by the modes
    every other argument as for predict().
    -> predict()'s results with K = n_modes (``trajectories``, ``waypoints``, ``scores``, ``order``, the maps with ``return_maps``;
       mode m is sample m of the sweep) and ``mode_mass``, ``mode_logit`` [N, n_modes] in the ranked order (row r is mode
       order[:, r]): the share of sigmoid(goal_map / T), normalised, that the mode claimed -- the masses of an agent are disjoint and
       sum to the covered share of its map -- and the raw logit of its peak.  With one way-point ``order`` is 0 .. n_modes - 1.
    An agent whose goal map gives fewer modes (non-finite logits) raises RuntimeError at the chunk's sync point.
    Out of scope for now: a predict_styles form, evaluate() over modes, sub-pixel refinement of the peak, capturing the call into
    a hipGraph, the scene compliance of predict_with_compliance() (the class mass of the goal map), and the scene occupancy of
    predict_with_occupancy()."""
    n_modes, radius = int(n_modes), int(radius)
    if not 1 <= n_modes <= MAX_SAMPLES:
        raise ValueError(f"predict_modes: n_modes = {n_modes}; the ranking kernel takes 1 .. {MAX_SAMPLES}")
    if radius < 0:
        raise ValueError(f"predict_modes: radius = {radius} is negative")
    use_CWS = CWS_params is not None
    obs, waypoints, _, _, obs_len, _ = _validated("predict_modes", observed, scene_image, waypoints, n_modes, 1, obs_len, resize_factor, use_CWS,
                                                  CWS_params, batch_size, None)
    return _forecast("predict_modes", model, lambda: ops.refresh_filters(model), lambda b, n: (None, model.pred_features), scene_image, obs,
                     input_template, waypoints, n_modes, 1, obs_len, resize_factor, temperature, use_TTST=False, use_CWS=use_CWS, rel_thresh=None,
                     CWS_params=CWS_params, network=network, swap_semantic=swap_semantic, batch_size=batch_size,
                     max_effective_batch=max_effective_batch, forced_samples=None, return_maps=return_maps, return_entropy=False,
                     modes=(n_modes, radius))

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
"""
import numpy as np
import torch

from .. import ops
from .evaluate import _decoder_passes, cws_waypoints, ttst_goals
from .image_utils import gather_patches, sampling, swap_pavement_terrain

MAX_SAMPLES = 64      # ynet_score_rank_samples ranks the samples of an agent on the lanes of one wavefront


def _observed_tensor(observed, obs_len):
    obs = observed.detach() if torch.is_tensor(observed) else torch.from_numpy(np.ascontiguousarray(np.asarray(observed, dtype=np.float32)))
    if obs.dim() != 3 or obs.shape[2] != 2:
        raise ValueError(f"predict: observed must be [N, obs_len, 2] (x, y) in resized pixel coordinates, got {tuple(obs.shape)}")
    if obs.shape[1] != obs_len:
        raise ValueError(f"predict: observed holds {obs.shape[1]} steps per agent, obs_len is {obs_len}: pass exactly the observed steps "
                         f"(a longer track is never cut silently)")
    return obs.float()


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
       and ``goal_sigmoid_map`` as evaluate(return_samples=True) stores them."""
    waypoints = list(waypoints)
    n_wp = len(waypoints)
    n_goal, n_traj, obs_len = int(n_goal), int(n_traj), int(obs_len)
    K = n_goal * n_traj
    if n_goal < 1 or n_traj < 1:
        raise ValueError(f"predict: n_goal = {n_goal}, n_traj = {n_traj}: at least one sample per agent is needed")
    if K > MAX_SAMPLES:
        raise ValueError(f"predict: n_goal * n_traj = {K} samples per agent; the ranking kernel takes up to {MAX_SAMPLES}")
    if n_wp < 1:
        raise ValueError("predict: no way-points")
    if use_CWS and n_wp > 1 and CWS_params is None:
        raise ValueError("predict: use_CWS needs CWS_params (sigma_factor, ratio, rot)")
    if not float(resize_factor) > 0:
        raise ValueError("predict: resize_factor must be positive")
    if batch_size is not None and int(batch_size) < 1:
        raise ValueError("predict: batch_size must be positive")
    obs = _observed_tensor(observed, obs_len)
    if not torch.is_tensor(scene_image) or scene_image.dim() != 3:
        raise ValueError("predict: scene_image must be the tensor [C, H, W] of one scene")
    N = obs.shape[0]
    if N == 0:
        raise ValueError("predict: no agents (observed is empty)")
    if torch.is_tensor(forced_samples) and tuple(forced_samples.shape) != (K, N, n_wp, 2):
        raise ValueError(f"predict: forced_samples {tuple(forced_samples.shape)}, expected {(K, N, n_wp, 2)}")
    step = N if batch_size is None else int(batch_size)
    device = next(model.parameters()).device
    was_training = model.training
    model.eval()
    out = {k: [] for k in ["trajectories", "waypoints", "scores", "order"] + (["goal_map", "goal_sigmoid_map"] if return_maps else [])}
    try:
        with torch.no_grad():
            ops.refresh_filters(model)      # on the caller's stream, before the decoder passes fan out over two (see evaluate())
            scene = model.segmentation(scene_image.to(device).unsqueeze(0))
            scene = model.adapt_semantic(scene)
            if swap_semantic:
                scene = swap_pavement_terrain(scene)
            if network == "embed":
                scene = model.scene_embedding(scene)
            _, _, H, W = scene.shape
            for b in range(0, N, step):
                batch = obs[b:b + step]
                n = len(batch)
                observed_map = gather_patches(input_template, batch.reshape(-1, 2), H, W).view(-1, obs_len, H, W)
                if network == "embed":
                    observed_map = model.motion_embedding(observed_map)
                features = model.pred_features(scene.expand(n, -1, -1, -1), observed_map)
                pred_goal_map = model.pred_goal(features)
                wp_sigmoid = ops.sigmoid_temp(pred_goal_map, waypoints, temperature)

                if forced_samples is not None:
                    forced = forced_samples[:, b:b + n] if torch.is_tensor(forced_samples) else forced_samples[b]
                    waypoint_samples = forced.to(device)
                    if tuple(waypoint_samples.shape) != (K, n, n_wp, 2):
                        raise ValueError(f"predict: forced samples {tuple(waypoint_samples.shape)} for the chunk at {b}, expected {(K, n, n_wp, 2)}")
                else:
                    if use_TTST:
                        goal_samples = ttst_goals(model, wp_sigmoid[:, -1:], pred_goal_map[:, waypoints[-1:]], n_goal, rel_thresh)
                    else:
                        goal_samples = sampling(wp_sigmoid[:, -1:], num_samples=n_goal).permute(2, 0, 1, 3)
                    if use_CWS and n_wp > 1:
                        last_observed = batch[:, obs_len - 1].to(device)
                        waypoint_samples = cws_waypoints(model, wp_sigmoid, goal_samples, last_observed, n_goal, n_traj,
                                                         CWS_params["sigma_factor"], CWS_params["ratio"], CWS_params["rot"])
                    elif n_wp > 1:
                        waypoint_samples = sampling(wp_sigmoid[:, :-1], num_samples=n_goal * n_traj).permute(2, 0, 1, 3)
                        waypoint_samples = torch.cat([waypoint_samples, goal_samples.repeat(n_traj, 1, 1, 1)], dim=2)
                    else:
                        waypoint_samples = goal_samples
                waypoint_samples = waypoint_samples.float().contiguous()

                if return_maps:
                    out["goal_map"].append(pred_goal_map)
                    out["goal_sigmoid_map"].append(model.sigmoid(pred_goal_map / temperature))

                trajs_samples = _decoder_passes(model, features, waypoint_samples, input_template, n, n_wp, H, W, max_effective_batch, device)
                ranked, ranked_goals, score, order = ops.score_rank_samples(wp_sigmoid, waypoint_samples, trajs_samples.contiguous(),
                                                                           resize_factor)
                out["trajectories"].append(ranked)
                out["waypoints"].append(ranked_goals)
                out["scores"].append(score)
                out["order"].append(order)
                ops.check_patch_status()      # (score_rank_samples waited for the chunk: a window that left the template raises here)
    finally:
        model.train(was_training)
    return {k: (v[0] if len(v) == 1 else torch.cat(v)) for k, v in out.items()}

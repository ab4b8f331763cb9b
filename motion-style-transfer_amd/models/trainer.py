"""YNetTrainer on MI355X (mirror of models/trainer.py: same public methods, freeze policy,
optimizer, log lines and checkpoint format).

Reference: __init__ 46-75, _train 80-293 (freeze table 116-195), _test 299-352, forward_test / _forward_test /
_forward_batch 354-516, prepare_data 518-584, load_params / save_params / load_separated_params 586-614,
mark_*_bias_trainable 20-42.  ``saliency`` (new) wraps forward_test(decision='loss') and one backward; ``predict`` (new) forecasts
from the observed steps alone: all K samples, scored and ranked (utils/predict.py); ``load_styles`` / ``predict_styles`` (new) do so for
agents of several styles at once (models/style_bank.py).
Differences, all outside the arithmetic: image files are not decoded here (cv2/smp are out of scope) —
``prepare_data`` takes a dict {scene_id: float tensor [C,H,W]} in place of an image directory; an
optional ``dp`` (dist.DataParallel) shards batches over the GPUs of a node.
"""
import os
import pathlib
import re
from collections import OrderedDict, deque
from copy import deepcopy

import numpy as np
import torch
import torch.nn as nn
from torch.utils.data import DataLoader
from tqdm import tqdm

from .. import ops
from ..utils.dataloader import SceneDataset, scene_collate
from ..utils.evaluate import evaluate
from ..utils.image_utils import (draw_seed, gather_patches, analytic_dist_template, analytic_gaussian_template, create_dist_mat,
                                 create_gaussian_heatmap_template)
from ..utils.train_epoch import train_epoch
from .ynet import YNet


class HipBCEWithLogitsLoss(nn.Module):
    """nn.BCEWithLogitsLoss() (mean) on the fused HIP kernels.  `expected_grad` is the factor the caller is about to
    multiply the loss by (train_epoch sets it to its loss_scale): the gradient of the logits is then produced in the
    same pass as the loss.  It is a hint only -- results do not depend on it."""

    fuses_with_predictor = True      # a YNetDecoder told about the target (models/ynet.py: announce_bce_target) computes the
                                     # loss in its predictor kernel; forward() then only hands that value out

    def __init__(self):
        super().__init__()
        self.expected_grad = 1.0

    def forward(self, input, target):
        fused = getattr(input, "_ynet_fused_bce", None)
        if fused is not None:
            # The fused predictor returned these logits as NON-differentiable (its kernel already produced the gradients for
            # the announced target and upstream gradient): any other use would silently drop the decoder's gradient.
            same_target = fused[0] is target or (torch.is_tensor(target) and target.data_ptr() == fused[0].data_ptr()
                                                 and target.shape == fused[0].shape and target.stride() == fused[0].stride())
            if same_target and fused[2] == float(self.expected_grad):
                return fused[1]
            raise RuntimeError(
                "HipBCEWithLogitsLoss: these maps come from a decoder that was told its BCE target (announce_bce_target) "
                + ("but are compared with a different target tensor" if not same_target else
                   f"for the upstream gradient {fused[2]} but expected_grad is now {float(self.expected_grad)}")
                + "; compute the maps outside announce_bce_target (or set YNET_PRED_BCE=0) for any other use")
        return ops.bce_with_logits(input, target, self.expected_grad)


def _hip_criterion(criterion, loss_scale):
    """The criterion _forward_batch builds (models/trainer.py:374: nn.BCEWithLogitsLoss()) on the HIP BCE kernels: mean over the
    elements, the gradient of the logits written in the loss's own pass for the upstream gradient loss_scale (ops.bce_with_logits).
    Any other configuration is refused -- there is no ATen path."""
    if isinstance(criterion, HipBCEWithLogitsLoss):
        criterion.expected_grad = float(loss_scale)
        return criterion
    if (type(criterion) is nn.BCEWithLogitsLoss and criterion.reduction == "mean" and criterion.weight is None
            and criterion.pos_weight is None):
        return lambda x, t: ops.bce_with_logits(x, t, float(loss_scale))
    raise NotImplementedError(f"_forward_batch: criterion {criterion!r} has no HIP kernel (nn.BCEWithLogitsLoss() with the defaults only)")


def _mark_bias(module):
    for name, p in module.named_parameters():
        if "bias" in name:
            p.requires_grad = True


def mark_encoder_bias_trainable(model):
    _mark_bias(model.encoder)
    return model


def mark_goal_bias_trainable(model):
    _mark_bias(model.goal_decoder)
    return model


def mark_traj_bias_trainable(model):
    _mark_bias(model.traj_decoder)
    return model


def mark_ynet_bias_trainable(model):
    return mark_traj_bias_trainable(mark_goal_bias_trainable(mark_encoder_bias_trainable(model)))


_FUSION_PARTS = {"scene": ("scene",), "motion": ("motion",), "fusion": ("fusion",),
                 "scene_fusion": ("scene", "fusion"), "motion_fusion": ("motion", "fusion"),
                 "scene_motion": ("scene", "motion"), "scene_motion_fusion": ("scene", "motion", "fusion")}


def apply_freeze_policy(model, train_net, position=(), network=None, ynet_bias=False):
    """Which tensors train, per ``train_net`` (models/trainer.py:113-195)."""
    for p in model.semantic_segmentation.parameters():
        p.requires_grad = False
    if train_net in ("all", "train"):
        return model
    for p in model.parameters():
        p.requires_grad = False
    position = [str(i) for i in position]
    enc = model.encoder
    if train_net == "encoder" and len(position) == 0:
        for p in enc.parameters():
            p.requires_grad = True
    elif train_net == "encoder":
        for name, p in enc.named_parameters():
            if name.split(".")[1] in position:
                p.requires_grad = True
    elif "serial" in train_net or "parallel" in train_net:
        key = "serial" if "serial" in train_net else "parallel"
        for name, p in enc.named_parameters():
            if key in name:
                p.requires_grad = True
    elif "mosa" in train_net:
        for name, p in enc.named_parameters():
            if "lora" in name:
                p.requires_grad = True
    elif "semantic" in train_net:
        for name, p in model.named_parameters():
            if "semantic_adapter" in name:
                p.requires_grad = True
    elif network == "fusion" and train_net in _FUSION_PARTS:
        for part in _FUSION_PARTS[train_net]:
            for p in getattr(enc, part + "_stages").parameters():
                p.requires_grad = True
    elif train_net == "biasEncoder":
        mark_encoder_bias_trainable(model)
    elif train_net == "biasGoal":
        mark_goal_bias_trainable(model)
    elif train_net == "biasTraj":
        mark_traj_bias_trainable(model)
    elif train_net == "bias":
        mark_ynet_bias_trainable(model)
    elif "segmentation" in train_net:
        layer = train_net.split("_")[1]
        for name, p in model.semantic_segmentation.named_parameters():
            if (layer in name) if layer in ("head", "bias", "bn") else re.search(rf"decoder.blocks.\d.{layer}", name):
                p.requires_grad = True
    else:
        raise NotImplementedError
    if ynet_bias:
        mark_ynet_bias_trainable(model)
    return model


def compliance_report(df_metrics, images):
    """The lines test(return_compliance=True) prints per round, one per semantic class: the mean goal mass, the mean sampled-goal rate
    and the share of ground-truth goals on the class (goals outside the map count in none), beside the share of the map the class
    covers (agents weighted: every agent brings the areas of its own scene)."""
    from ..utils.compliance import class_area, scene_labels
    n_cls = sum(1 for c in df_metrics.columns if c.startswith("goal_mass_"))
    area = {sid: class_area(scene_labels(images[sid]), n_cls).cpu().numpy() for sid in df_metrics["sceneId"].unique()}
    mean_area = np.stack([area[sid] for sid in df_metrics["sceneId"]]).mean(axis=0)
    gt = df_metrics["gt_goal_class"].to_numpy()
    lines = ["Scene compliance (class: goal mass | sampled-goal rate | ground-truth goals | map area)"]
    for k in range(n_cls):
        lines.append(f"  class {k}: {df_metrics[f'goal_mass_{k}'].mean():.4f} | {df_metrics[f'sample_goal_rate_{k}'].mean():.4f} | "
                     f"{float((gt == k).mean()):.4f} | {mean_area[k]:.4f}")
    return "\n".join(lines)


def sharpness_report_of(df_metrics, images, resize_factor):
    """The lines test(return_sharpness=...) prints per round, one per level (utils.sharpness.sharpness_report), from evaluate()'s
    area<pct>_goal / inside<pct>_goal columns; every agent brings the size of its own scene's map."""
    from ..utils.sharpness import sharpness_report
    names = [c[len("area"):-len("_goal")] for c in df_metrics.columns if c.startswith("area") and c.endswith("_goal")]
    pixels = {sid: int(images[sid].shape[-2]) * int(images[sid].shape[-1]) for sid in df_metrics["sceneId"].unique()}
    return sharpness_report([float(n) / 100.0 for n in names], df_metrics[[f"inside{n}_goal" for n in names]].to_numpy(),
                            df_metrics[[f"area{n}_goal" for n in names]].to_numpy(),
                            np.array([pixels[sid] for sid in df_metrics["sceneId"]], dtype=np.float64), resize_factor)


def radial_report_of(df_metrics, return_radial, fde=None):
    """The lines test(return_radial=...) prints per round (utils.radial.radial_report), from evaluate()'s radial_mean_goal, hit<r>_goal and
    best_of_<K>_lower_goal / _upper_goal columns, beside the round's sampled FDE."""
    from ..utils.radial import radial_options, radial_report
    opt = radial_options(return_radial, "test(return_radial=...)")
    return radial_report(opt["radii"], opt["k"], df_metrics["radial_mean_goal"].to_numpy(),
                         df_metrics[[f"hit{r}_goal" for r in opt["radii"]]].to_numpy(),
                         df_metrics[[f"best_of_{k}_lower_goal" for k in opt["k"]]].to_numpy(),
                         df_metrics[[f"best_of_{k}_upper_goal" for k in opt["k"]]].to_numpy(), fde)


def marginals_report_of(df_metrics, return_marginals, fde=None):
    """The lines test(return_marginals=...) prints per round (utils.marginals.marginals_report), from evaluate()'s crps_x_goal / crps_y_goal
    and width<pct>_<axis>_goal / inside<pct>_<axis>_goal columns, beside the round's sampled FDE."""
    from ..utils.marginals import marginal_levels, marginals_report
    from ..utils.sharpness import level_name
    levels = marginal_levels(return_marginals, "test(return_marginals=...)")
    per_axis = lambda stem: np.stack([df_metrics[[f"{stem}{level_name(q)}_{axis}_goal" for q in levels]].to_numpy() for axis in "xy"], axis=1)
    return marginals_report(levels, df_metrics[["crps_x_goal", "crps_y_goal"]].to_numpy(), per_axis("inside"), per_axis("width"), fde)


class YNetTrainer:
    def __init__(self, params, device=None):
        self.params = params
        self.device = device if device else torch.device("cuda" if torch.cuda.is_available() else "cpu")
        self.device = torch.device(self.device)
        if self.device.type == "cuda" and self.device.index is not None and torch.cuda.is_available():
            torch.cuda.set_device(self.device)      # the HIP kernels launch on the current device's streams
        print(f"Working on {self.device}")
        self.division_factor = 2 ** len(params["encoder_channels"])
        self.template_size = int(4200 * params["resize_factor"])
        self.model = YNet(
            obs_len=params["obs_len"], pred_len=params["pred_len"],
            segmentation_model_fp=params["segmentation_model_fp"], use_features_only=params["use_features_only"],
            n_semantic_classes=params["n_semantic_classes"], encoder_channels=params["encoder_channels"],
            decoder_channels=params["decoder_channels"], n_waypoints=len(params["waypoints"]),
            train_net=params["train_net"], position=params["position"], network=params["network"],
            n_fusion=params["n_fusion"])
        self.dp = None

    # ------------------------------------------------------------------------------------------
    def templates(self, kernlen=None, nsig=None):
        """models/trainer.py:60-62, 209-211.  On the GPU the templates are analytic (ops.AnalyticTemplate: the windows
        get_patch slices out of them are computed in the kernel, bit-identical, and the 4.4 / 7.7 MB arrays are never
        built); YNET_ANALYTIC_HEATMAPS=0 keeps the materialised tensors."""
        analytic = self.device.type == "cuda" and os.environ.get("YNET_ANALYTIC_HEATMAPS", "1") != "0"
        if analytic:
            input_template = analytic_dist_template(self.template_size, self.device)
        else:
            input_template = torch.Tensor(create_dist_mat(size=self.template_size)).to(self.device)
        if kernlen is None:
            return input_template
        if analytic:
            gt_template = analytic_gaussian_template(self.template_size, kernlen, nsig, False, self.device)
        else:
            gt_template = torch.Tensor(create_gaussian_heatmap_template(
                size=self.template_size, kernlen=kernlen, nsig=nsig, normalize=False)).to(self.device)
        return input_template, gt_template

    def train(self, df_train, df_val, train_image_path, val_image_path, experiment_name):
        return self._train(df_train, df_val, train_image_path, val_image_path, experiment_name, **self.params)

    def _train(self, df_train, df_val, train_image_path, val_image_path, experiment_name, ckpt_path,
               dataset_name, resize_factor, obs_len, pred_len, batch_size, lr, n_epoch,
               waypoints, n_goal, n_traj, kernlen, nsig, e_unfreeze, loss_scale, temperature,
               use_raw_data=False, save_every_n=10, train_net="all", position=[],
               fine_tune=False, augment=False, ynet_bias=False,
               use_CWS=False, resl_thresh=0.002, CWS_params=None, n_early_stop=5,
               steps=[20], lr_decay_ratio=0.1, network=None, swap_semantic=False, window_size=9,
               smooth_val=False, **kwargs):
        train_images, train_loader, self.homo_mat = self.prepare_data(
            df_train, train_image_path, dataset_name, "train", obs_len, pred_len, resize_factor, use_raw_data, augment)
        val_images, val_loader, _ = self.prepare_data(
            df_val, val_image_path, dataset_name, "val", obs_len, pred_len, resize_factor, use_raw_data, False)

        model = self.model.to(self.device)
        apply_freeze_policy(model, train_net, position, network, ynet_bias)
        optimizer = torch.optim.Adam(model.parameters(), lr=lr)
        if fine_tune:
            print("LR Schedular because finetuning")
            lr_scheduler = torch.optim.lr_scheduler.MultiStepLR(optimizer, milestones=steps, gamma=lr_decay_ratio)
        print("The number of trainable parameters: {:d}".format(
            sum(p.numel() for p in model.parameters() if p.requires_grad)))
        criterion = HipBCEWithLogitsLoss()
        input_template, gt_template = self.templates(kernlen, nsig)
        if self.dp is not None:
            self.dp.__init__(model.parameters(), self.dp.group)

        best_val_ADE, best_epoch = 99999999999999, 0
        self.val_ADE, self.val_FDE = [], []
        state_dicts = deque()
        half_window_size = (window_size // 2) + 1
        rank0 = self.dp is None or self.dp.rank == 0

        print("Start training")
        for e in tqdm(range(n_epoch), desc="Epoch"):
            train_ADE, train_FDE, train_loss = train_epoch(
                model, train_loader, train_images, optimizer, criterion, loss_scale, self.device,
                dataset_name, self.homo_mat, gt_template, input_template, waypoints,
                e, obs_len, pred_len, batch_size, e_unfreeze, resize_factor, network, swap_semantic, dp=self.dp)
            val_ADE, val_FDE, _, _ = evaluate(
                model, val_loader, val_images, self.device, dataset_name, self.homo_mat, input_template, waypoints,
                "val", n_goal, n_traj, obs_len, batch_size, resize_factor, temperature, False, use_CWS,
                resl_thresh, CWS_params, network=network, swap_semantic=swap_semantic, dp=self.dp)
            line = (f"Epoch {e}: \tTrain (Top-1) ADE: {train_ADE:.2f} FDE: {train_FDE:.2f} \t\t"
                    f"Val (Top-k) ADE: {val_ADE:.2f} FDE: {val_FDE:.2f}")
            print(line + (f"   lr={lr_scheduler.get_last_lr()[0]}" if fine_tune else ""))
            self.val_ADE.append(val_ADE)
            self.val_FDE.append(val_FDE)
            if fine_tune:
                lr_scheduler.step()

            if smooth_val:
                print("Length: ", len(state_dicts))
                if len(state_dicts) == half_window_size:
                    curr_model_dict = state_dicts.popleft()
                state_dicts.append(deepcopy(model.state_dict()))
                val_ADE = best_val_ADE + 1 if e < window_size else sum(self.val_ADE[-window_size:]) / window_size
            else:
                curr_model_dict = deepcopy(model.state_dict())

            if val_ADE < best_val_ADE:
                best_val_ADE = val_ADE
                best_epoch = e - half_window_size + 1 if smooth_val else e
                best_state_dict = curr_model_dict
                if not fine_tune and rank0:
                    print(f"Best Epoch {e}: \nVal ADE: {val_ADE} \nVal FDE: {val_FDE}")
                    pathlib.Path(ckpt_path).mkdir(parents=True, exist_ok=True)
                    torch.save(model.state_dict(), f"{ckpt_path}/{experiment_name}_weights.pt")
            if (e + 1) % save_every_n == 0 and rank0:
                pathlib.Path(ckpt_path).mkdir(parents=True, exist_ok=True)
                self.save_params(f"{ckpt_path}/{experiment_name}__epoch_{e}.pt", train_net)
            if fine_tune and (best_val_ADE < min(self.val_ADE[-n_early_stop:])):
                print(f"Early stop at epoch {e}")
                break

        print(f"Best epoch at {best_epoch}")
        if best_epoch != 0:
            model.load_state_dict(best_state_dict, strict=True)
        if rank0:
            pathlib.Path(ckpt_path).mkdir(parents=True, exist_ok=True)
            self.save_params(f"{ckpt_path}/{experiment_name}.pt", train_net)
        return self.val_ADE, self.val_FDE

    # ------------------------------------------------------------------------------------------
    def test(self, df_test, image_path, return_preds=False, return_samples=False, return_likelihood=False, return_compliance=False,
             return_marginals=False, return_radial=False, return_sharpness=False):
        """``return_likelihood`` (not in the reference): evaluate() also scores the goal-map distribution against the ground truth
        (df_metrics columns nll, nll_goal, entropy_goal, hpd_goal) and every round prints its mean NLL and calibration error.
        ``return_compliance`` (not in the reference): evaluate() also reports where in the scene the goals go (df_metrics columns
        goal_mass_<k>, gt_goal_class, sample_goal_rate_<k>) and every round prints one line per semantic class: the mean goal mass,
        the mean sampled-goal rate and the share of ground-truth goals on the class, beside the share of the map the class covers.
        ``return_sharpness`` (not in the reference; False, True = (0.5, 0.9), or a tuple of levels): evaluate() also reports the size of
        the goal map's credible regions (df_metrics columns area<pct>_goal, inside<pct>_goal) and every round prints one line per level:
        how often the ground-truth goal lies inside the region (calibration) beside the region's mean and median area (sharpness).
        ``return_radial`` (not in the reference; False, True = {'radii': (4, 8, 16), 'k': (1, 5, 20)}, or such a dict): evaluate() also
        reports the goal error the goal map implies with no draw (df_metrics columns radial_mean_goal, radial_rms_goal, hit<r>_goal,
        best_of_<K>_lower_goal / _upper_goal) and every round prints, for the last step, the expected error of one draw, the bracket
        around the expected best-of-K error beside the round's sampled FDE, and the mass within each radius.
        ``return_marginals`` (not in the reference; False, True = (0.5, 0.9), or a tuple of levels): evaluate() also scores the goal map
        per axis (df_metrics columns crps_x_goal, crps_y_goal, crps_goal, pit_x_goal, pit_y_goal, width<pct>_<axis>_goal,
        inside<pct>_<axis>_goal) and every round prints the mean CRPS beside the round's sampled FDE and, per axis and level, the coverage
        of the central interval beside its mean width."""
        return self._test(df_test, image_path, return_preds=return_preds, return_samples=return_samples,
                          return_likelihood=return_likelihood, return_compliance=return_compliance, return_sharpness=return_sharpness,
                          return_radial=return_radial, return_marginals=return_marginals, **self.params)

    def _test(self, df_test, image_path, dataset_name, resize_factor, batch_size, n_round, obs_len, pred_len,
              waypoints, n_goal, n_traj, temperature, rel_threshold, use_TTST, use_CWS, CWS_params,
              use_raw_data=False, return_preds=False, return_samples=False, network=None, swap_semantic=False,
              return_likelihood=False, return_compliance=False, return_sharpness=False, return_radial=False, return_marginals=False,
              **kwargs):
        test_images, test_loader, self.homo_mat = self.prepare_data(
            df_test, image_path, dataset_name, "test", obs_len, pred_len, resize_factor, use_raw_data)
        model = self.model.to(self.device)
        input_template = self.templates()
        self.eval_ADE, self.eval_FDE = [], []
        list_metrics, list_trajs = [], []
        print("TTST setting:", use_TTST)
        print("Start testing")
        for e in tqdm(range(n_round), desc="Round"):
            test_ADE, test_FDE, df_metrics, trajs_dict = evaluate(
                model, test_loader, test_images, self.device, dataset_name, self.homo_mat, input_template, waypoints,
                "test", n_goal, n_traj, obs_len, batch_size, resize_factor, temperature, use_TTST, use_CWS,
                rel_threshold, CWS_params, return_preds=return_preds, return_samples=return_samples,
                network=network, swap_semantic=swap_semantic, dp=self.dp, return_likelihood=return_likelihood,
                return_compliance=return_compliance, return_sharpness=return_sharpness, return_radial=return_radial,
                return_marginals=return_marginals)
            list_metrics.append(df_metrics)
            list_trajs.append(trajs_dict)
            print(f"Round {e}: \nTest ADE: {test_ADE} \nTest FDE: {test_FDE}")
            if return_likelihood:
                from ..utils.likelihood import calibration_curve
                hpd_goal = df_metrics["hpd_goal"].to_numpy()      # (all NaN when every goal lies outside its map: nothing to calibrate)
                ece = calibration_curve(hpd_goal)[2] if np.isfinite(hpd_goal).any() else "n/a"
                print(f"Test NLL: {df_metrics['nll'].mean()} \nTest goal ECE: {ece}")
            if return_compliance:
                print(compliance_report(df_metrics, test_images))
            if return_sharpness:
                print(sharpness_report_of(df_metrics, test_images, resize_factor))
            if return_radial:
                print(radial_report_of(df_metrics, return_radial, test_FDE))
            if return_marginals:
                print(marginals_report_of(df_metrics, return_marginals, test_FDE))
            self.eval_ADE.append(test_ADE)
            self.eval_FDE.append(test_FDE)
        avg_ade = sum(self.eval_ADE) / len(self.eval_ADE)
        avg_fde = sum(self.eval_FDE) / len(self.eval_FDE)
        print(f"\nAverage performance (by {n_round}): \nTest ADE: {avg_ade} \nTest FDE: {avg_fde}")
        return avg_ade, avg_fde, list_metrics, list_trajs

    # ------------------------------------------------------------------------------------------
    def calibrate_temperature(self, df_val, image_path, t_range=(0.25, 8.0), n_temps=16, rounds=2, steps="waypoints"):
        """Temperature scaling (not in the reference, whose T is hand-set): the temperature of the goal-map distribution that minimises
        the NLL of ``df_val``'s ground truth, found by a grid search over ``t_range`` (utils.calibrate.calibrate_temperature; data
        prepared as for test()).  Prints the temperature, the NLL and the goal ECE before -> after, and returns the function's dict.
        ``self.params["temperature"]`` is NOT changed: the caller decides."""
        return self._calibrate_temperature(df_val, image_path, t_range=t_range, n_temps=n_temps, rounds=rounds, steps=steps, **self.params)

    def _calibrate_temperature(self, df_val, image_path, dataset_name, resize_factor, batch_size, obs_len, pred_len, waypoints, temperature,
                               t_range, n_temps, rounds, steps, use_raw_data=False, network=None, swap_semantic=False, **kwargs):
        from ..utils.calibrate import calibrate_temperature, check_arguments
        check_arguments(waypoints, temperature, t_range, n_temps, rounds, steps)      # (before any data or model is touched)
        val_images, val_loader, _ = self.prepare_data(df_val, image_path, dataset_name, "test", obs_len, pred_len, resize_factor, use_raw_data)
        model = self.model.to(self.device)
        out = calibrate_temperature(model, val_loader, val_images, self.device, self.templates(), waypoints, obs_len, batch_size, resize_factor,
                                    temperature, t_range=t_range, n_temps=n_temps, rounds=rounds, steps=steps, network=network,
                                    swap_semantic=swap_semantic)
        print(f"Calibrated temperature: {out['temperature']} (was {temperature}" + (", at the boundary of t_range" if out["at_boundary"] else "")
              + f") \nVal NLL: {out['nll_before']} -> {out['nll']} \nVal goal ECE: {out['ece_before']} -> {out['ece']}")
        return out

    # ------------------------------------------------------------------------------------------
    def predict(self, df_obs, image_path_or_images, return_maps=False):
        """Forecasts WITHOUT ground truth (new; the reference's test() needs obs_len + pred_len rows per agent and its plotting
        helpers re-run it): the K = n_goal * n_traj sampled futures of every agent, scored against the goal map and ranked
        (utils/predict.py).  ``df_obs``: a DataFrame with EXACTLY obs_len rows per metaId (columns metaId, sceneId, x, y in
        original-image pixels, scaled by resize_factor as SceneDataset does), or a dict {scene_id: [N, obs_len, 2] array} of such
        tracks (metaIds are then numbered in order).  ``image_path_or_images``: as for test(), the dict {scene_id: tensor}.
        -> ({scene_id: dict of device tensors, see utils.predict.predict}, DataFrame [metaId, sceneId, rank, score])."""
        return self._predict(df_obs, image_path_or_images, return_maps=return_maps, **self.params)

    def _predict(self, df_obs, image_path, dataset_name, resize_factor, obs_len, waypoints, n_goal, n_traj, temperature,
                 batch_size=None, rel_threshold=0.002, use_TTST=False, use_CWS=False, CWS_params=None, use_raw_data=False,
                 network=None, swap_semantic=False, return_maps=False, bank=None, style_column=None, modes=None, occupancy=None,
                 intervals=None, **kwargs):
        import pandas as pd
        from ..utils.predict import MAX_SAMPLES, predict, predict_modes, predict_styles, predict_with_intervals, predict_with_occupancy
        if dataset_name.lower() == "eth":
            raise NotImplementedError("predict: ETH/UCY forecasts are in world coordinates (homographies read from data files): "
                                      "out of the MI355X hot path, as in prepare_data")
        if modes is None and n_goal * n_traj > MAX_SAMPLES:
            raise ValueError(f"predict: n_goal * n_traj = {n_goal * n_traj} samples per agent; the ranking kernel takes up to {MAX_SAMPLES}")
        if isinstance(df_obs, dict):
            rows, first = [], 0
            for scene_id, tracks in df_obs.items():
                xy = np.asarray(tracks.detach().cpu() if torch.is_tensor(tracks) else tracks, dtype=np.float64)
                if xy.ndim != 3 or xy.shape[2] != 2:
                    raise ValueError(f"predict: scene {scene_id}: expected [N, obs_len, 2] tracks, got {xy.shape}")
                if xy.shape[1] != obs_len:
                    raise ValueError(f"predict: scene {scene_id}: {xy.shape[1]} steps per agent, obs_len is {obs_len}: pass exactly the "
                                     f"observed steps (a longer track is never cut silently)")
                ids = np.repeat(np.arange(first, first + xy.shape[0]), obs_len)
                rows.append(pd.DataFrame({"metaId": ids, "sceneId": scene_id, "x": xy[..., 0].reshape(-1), "y": xy[..., 1].reshape(-1)}))
                first += xy.shape[0]
            if not rows:
                raise ValueError("predict: no data is provided")
            df_obs = pd.concat(rows, ignore_index=True)
        counts = df_obs.groupby("metaId", sort=False).size()
        if len(counts) == 0:
            raise ValueError("predict: no data is provided")
        if (counts != obs_len).any():
            bad = counts[counts != obs_len]
            raise ValueError(f"predict: every metaId needs exactly obs_len = {obs_len} rows (the observed steps alone); metaId {bad.index[0]} has "
                             f"{int(bad.iloc[0])}" + (f" and {len(bad) - 1} more differ" if len(bad) > 1 else ""))
        # scenes: the label-map / padding path of prepare_data; tracks: SceneDataset with no future steps (scaled by resize_factor)
        images, loader, _ = self.prepare_data(df_obs, image_path, dataset_name, "test", obs_len, 0, resize_factor, use_raw_data)
        model = self.model.to(self.device)
        input_template = self.templates()
        results, frames = {}, []
        for observed, meta, scene_id in loader:
            kw = dict(use_TTST=use_TTST, use_CWS=use_CWS, rel_thresh=rel_threshold, CWS_params=CWS_params, network=network,
                      swap_semantic=swap_semantic, batch_size=batch_size, return_maps=return_maps)
            if modes is not None:      # (n_modes, radius): no draw, so none of the sampling options
                res = predict_modes(model, images[scene_id], observed, input_template, waypoints, *modes, obs_len, resize_factor, temperature,
                                    CWS_params=CWS_params if use_CWS else None, network=network, swap_semantic=swap_semantic,
                                    batch_size=batch_size, return_maps=return_maps)
            elif occupancy is not None:      # the cell edge: predict() plus the scene's occupancy; every scene runs as one chunk
                res = predict_with_occupancy(model, images[scene_id], observed, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor,
                                             temperature, cell=occupancy, **{**kw, "batch_size": None})
            elif intervals is not None:      # the levels: predict() plus the per-axis median and central intervals
                res = predict_with_intervals(model, images[scene_id], observed, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor,
                                             temperature, levels=intervals, **kw)
            elif bank is None:
                res = predict(model, images[scene_id], observed, input_template, waypoints, n_goal, n_traj, obs_len, resize_factor, temperature, **kw)
            else:
                styles = meta[0][style_column].to_numpy().reshape(-1, obs_len)
                if (styles != styles[:, :1]).any():
                    raise ValueError(f"predict_styles: scene {scene_id}: column {style_column!r} changes inside a track (one style per metaId)")
                res = predict_styles(bank, images[scene_id], observed, styles[:, 0].tolist(), input_template, waypoints, n_goal, n_traj, obs_len,
                                     resize_factor, temperature, **kw)
            results[scene_id] = res
            scores = res["scores"].cpu().numpy()
            n, k = scores.shape
            frames.append(pd.DataFrame({"metaId": np.repeat(meta[0].metaId.unique(), k), "sceneId": [scene_id] * (n * k),
                                        "rank": np.tile(np.arange(k), n), "score": scores.reshape(-1)}))
            if modes is not None:
                frames[-1]["mass"] = res["mode_mass"].cpu().numpy().reshape(-1)
        return results, pd.concat(frames, ignore_index=True)

    def load_styles(self, pretrained_path, styles):
        """Load the base weights and keep one adapter set per style BESIDE the model (models/style_bank.py): ``styles`` maps a style
        name to the path of a file written by save_params (or to a tuned state dict).  -> the StyleBank, also kept as ``self.styles``.
        Unlike load_separated_params no tuned tensor is written into the model: style_bank.BASE_STYLE names the model as loaded."""
        from .style_bank import StyleBank
        self.load_params(pretrained_path)
        self.styles = StyleBank(self.model.to(self.device), styles)
        return self.styles

    def predict_styles(self, df_obs, image_path_or_images, style_column="style", return_maps=False):
        """predict() for scenes whose agents wear different styles of ``self.styles`` (load_styles): ``df_obs`` as for predict() (the
        DataFrame form) with one more column, ``style_column``, that holds the style name of every row's agent (constant per metaId).
        -> as predict(); every scene's dict carries ``style_index`` (utils.predict.predict_styles)."""
        bank = getattr(self, "styles", None)
        if bank is None:
            raise RuntimeError("predict_styles: no style bank; call load_styles(pretrained_path, {name: tuned_path}) first")
        if isinstance(df_obs, dict) or style_column not in df_obs.columns:
            raise ValueError(f"predict_styles: df_obs must be a DataFrame with a {style_column!r} column (the style of every agent)")
        for name in df_obs[style_column].unique():
            bank.index(name)      # (an unknown style is refused before any scene runs)
        return self._predict(df_obs, image_path_or_images, return_maps=return_maps, bank=bank, style_column=style_column, **self.params)

    def predict_modes(self, df_obs, image_path_or_images, n_modes, radius, return_maps=False):
        """predict() with no draw: the ``n_modes`` most likely futures of every agent, their goals read off the goal map by greedy
        non-maximum suppression with a disk of ``radius`` pixels (of the resized map), each with the probability mass it claims
        (utils.predict.predict_modes).  ``df_obs`` and ``image_path_or_images`` as for predict(); n_goal, n_traj and use_TTST of the
        parameters are not read, and with use_CWS the intermediate way-points are CWS expectations.
        -> as predict(); every scene's dict carries ``mode_mass`` and ``mode_logit``, and the DataFrame a ``mass`` column."""
        n_modes, radius = int(n_modes), int(radius)
        if not 1 <= n_modes <= 64 or radius < 0:      # (before any scene is prepared; utils.predict.predict_modes says why)
            raise ValueError(f"predict_modes: n_modes = {n_modes} (1 .. 64), radius = {radius} (>= 0)")
        return self._predict(df_obs, image_path_or_images, return_maps=return_maps, modes=(n_modes, radius), **self.params)

    def predict_occupancy(self, df_obs, image_path_or_images, cell=4):
        """predict() plus the question a forecast of a SCENE is asked first: where will anybody be at step t, and which agents are
        forecast into the same place (utils.predict.predict_with_occupancy).  ``df_obs`` and ``image_path_or_images`` as for
        predict(); ``cell``: the edge of a cell in pixels of the resized map (1, 2, 4 or 8).  Every scene runs as one chunk whatever
        ``batch_size`` the parameters hold: the pairs across two chunks would be lost.
        -> as predict(); every scene's dict carries ``occupancy`` and ``occupancy_any`` [pred_len, Hc, Wc], ``conflict`` [pred_len]
        and ``risk`` [N, pred_len] (utils.occupancy.conflict_report ranks the agents per step)."""
        if cell not in (1, 2, 4, 8):      # (before any scene is prepared)
            raise ValueError(f"predict_occupancy: cell = {cell!r}, expected one of (1, 2, 4, 8)")
        return self._predict(df_obs, image_path_or_images, occupancy=int(cell), **self.params)

    def predict_intervals(self, df_obs, image_path_or_images, levels=(0.5, 0.9)):
        """predict() plus the forecast band per axis, with no draw: where along x and along y every agent will be at step t -- the
        median and the central interval per level of the goal map's x- and y-marginal (utils.predict.predict_with_intervals).
        ``df_obs`` and ``image_path_or_images`` as for predict(); ``levels``: 1 .. 8 ascending levels in (0, 1).
        -> as predict(); every scene's dict carries ``median_xy`` and ``marginal_mean_xy`` [N, pred_len, 2] and ``interval_xy``
        [N, pred_len, 2, L, 2] (axis; level; lo, hi), in pixels of the resized scene."""
        from ..utils.marginals import marginal_levels
        if isinstance(levels, bool) or levels is None:      # (before any scene is prepared)
            raise ValueError(f"predict_intervals: levels = {levels!r}: a sequence of 1 .. 8 ascending levels in (0, 1) is expected")
        levels = marginal_levels(levels, "predict_intervals(levels=...)")
        return self._predict(df_obs, image_path_or_images, intervals=levels, **self.params)

    # ------------------------------------------------------------------------------------------
    def forward_test(self, df_test, image_path, set_input, noisy_std_frac):
        return self._forward_test(df_test, image_path, set_input, noisy_std_frac, **self.params)

    def _forward_test(self, df_test, image_path, set_input, noisy_std_frac, decision, dataset_name, obs_len, pred_len,
                      resize_factor, use_raw_data, waypoints, kernlen, nsig, loss_scale, **kwargs):
        """models/trainer.py:357-457 for the one scene of ``df_test`` (all its trajectories form one batch).

        decision 'map':  (pred_goal_map, pred_traj_map, scene_raw_img) -- with ``noisy_std_frac``
                         (pred_goal_map, pred_traj_map, scene_raw_img, noisy_scene_img, semantic_input_cat);
        decision 'loss': (goal_loss, traj_loss, scene_raw_img[, noisy_scene_img]).
        ``set_input`` names the inputs that receive a gradient: 'scene' (the scene image), 'semantic' (the semantic map after the
        segmentation / semantic adapter: a leaf of its own, the scene then gets none), 'traj' (the observed-trajectory heat-maps).
        They are autograd leaves, so ``(goal_loss + traj_loss).backward()`` fills their ``.grad``; ``self.forward_inputs`` holds
        them by name after the call ('traj' is not among the returned values).  The reference passes ``False`` as set_input on its
        'loss' branch (models/trainer.py:387, 400, 416) and raises TypeError there; this is what that branch evidently meant.
        With ``noisy_std_frac`` every input named in set_input is replaced by a noisy copy x + N(0, (frac * (max - min))^2)
        (ops.add_range_noise: drawn on the device from a seed of torch's default generator -- reproducible under torch.manual_seed,
        NOT the draws of the reference's normal_), and that copy is the leaf; noisy_scene_img is the scene input actually fed.
        The heat-maps are the analytic templates' (bit-identical to get_patch); the criterion the reference builds,
        nn.BCEWithLogitsLoss(), runs on the HIP BCE kernels (ops.bce_with_logits)."""
        if decision not in ("loss", "map"):
            raise ValueError(f"No support for decision={decision}")
        test_images, test_loader, self.homo_mat = self.prepare_data(
            df_test, image_path, dataset_name, "test", obs_len, pred_len, resize_factor, use_raw_data)
        if len(test_loader) == 0:
            raise ValueError("No data is provided")
        if len(test_loader) > 1:
            raise ValueError(f"Received more than 1 scene ({len(test_loader)})")
        input_template, gt_template = self.templates(kernlen, nsig)
        criterion = nn.BCEWithLogitsLoss()
        traj, _, scene_id = next(iter(test_loader))
        scene_raw_img = test_images[scene_id].to(self.device).unsqueeze(0)
        set_input = tuple(set_input) if set_input else ()
        scene_raw_img.requires_grad_("scene" in set_input and not (noisy_std_frac is not None))
        out = self._forward_batch(scene_raw_img, traj, input_template, gt_template, criterion, obs_len, pred_len, waypoints,
                                  loss_scale, self.device, set_input, noisy_std_frac, decision == "map")
        if decision == "loss":
            goal_loss, traj_loss, noisy_scene_img = out[0], out[1], out[2]
            if noisy_std_frac is not None:
                return goal_loss, traj_loss, scene_raw_img, noisy_scene_img
            return goal_loss, traj_loss, scene_raw_img
        pred_goal_map, pred_traj_map, noisy_scene_img, semantic_input_cat = out
        if noisy_std_frac is not None:
            return pred_goal_map, pred_traj_map, scene_raw_img, noisy_scene_img, semantic_input_cat
        return pred_goal_map, pred_traj_map, scene_raw_img

    def _forward_batch(self, scene_raw_img, traj, input_template, gt_template, criterion, obs_len, pred_len, waypoints,
                       loss_scale, device, set_input=None, noisy_std_frac=None, return_pred_map=False):
        """models/trainer.py:459-516.  Returns (goal_loss, traj_loss, scene input fed) or, with return_pred_map,
        (pred_goal_map, pred_traj_map, scene input fed, [semantic | observed] cat or None)."""
        set_input = tuple(set_input) if set_input else ()
        model = self.model.to(self.device)
        network = self.params.get("network") if hasattr(self.params, "get") else None
        if set_input and network == "embed":
            raise NotImplementedError("input gradients of network='embed' (its first convolutions are the embeddings') are not served")
        _, _, H, W = scene_raw_img.shape
        coords = traj
        ops.check_patch_windows(input_template.shape, coords, H, W)
        observed_map = gather_patches(input_template, coords[:, :obs_len].reshape(-1, 2), H, W).view(-1, obs_len, H, W)
        gt_future_map = gather_patches(gt_template, coords[:, obs_len:].reshape(-1, 2), H, W).view(-1, pred_len, H, W)
        B = observed_map.shape[0]
        scene_image = model.segmentation(scene_raw_img)
        semantic_image = model.adapt_semantic(scene_image)
        scene_leaf = "scene" in set_input or "semantic" in set_input
        noisy = noisy_std_frac is not None
        if noisy and scene_leaf:
            semantic_image = ops.add_range_noise(semantic_image, noisy_std_frac, draw_seed()).requires_grad_()
        elif "semantic" in set_input:
            semantic_image = semantic_image.detach().requires_grad_()
        if noisy and "traj" in set_input:
            observed_map = ops.add_range_noise(observed_map, noisy_std_frac, draw_seed()).requires_grad_()
        elif "traj" in set_input:
            observed_map.requires_grad_()
        self.forward_inputs = {"traj": observed_map}
        if "semantic" in set_input or (noisy and scene_leaf):
            self.forward_inputs["semantic"] = semantic_image
        if "scene" in set_input:
            self.forward_inputs["scene"] = semantic_image if noisy else scene_raw_img
        sem_fed, obs_fed = semantic_image, observed_map
        if network == "embed":      # utils/train_epoch.py:80-83 (the reference's _forward_batch skips it)
            semantic_image = model.scene_embedding(semantic_image)
            observed_map = model.motion_embedding(observed_map)
        # one scene for every trajectory: broadcast, its gradient summed over the batch inside the first layer's backward
        semantic_map = ops.BatchExpand(semantic_image, B) if B > 1 else semantic_image
        features = model.pred_features(semantic_map, observed_map)
        pred_goal_map = model.pred_goal(features)
        bce = _hip_criterion(criterion, loss_scale)
        goal_loss = bce(pred_goal_map, gt_future_map) * loss_scale
        pred_waypoint_map = pred_goal_map[:, list(waypoints)]
        pyramid = ops.avgpool_pyramid_grad(pred_waypoint_map, len(features))
        traj_input = [ops.lazy_cat([f, g]) for f, g in zip(features, pyramid)]
        pred_traj_map = model.pred_traj(traj_input)
        traj_loss = bce(pred_traj_map, gt_future_map) * loss_scale
        scene_fed = sem_fed if (noisy and scene_leaf) else scene_raw_img
        if return_pred_map:
            cat = None
            if noisy:
                with torch.no_grad():
                    cat = torch.cat([sem_fed.detach().expand(B, -1, -1, -1), obs_fed.detach()], dim=1)
            return pred_goal_map, pred_traj_map, scene_fed, cat
        return goal_loss, traj_loss, scene_fed

    def saliency(self, df_test, image_path, target="both", set_input=("scene", "traj")):
        """Input-gradient saliency (the inputs of evaluator/visualization.py:1565 plot_saliency_maps): d loss / d input for
        loss = goal_loss + traj_loss ('both'), goal_loss or traj_loss, from forward_test(decision='loss') and ONE backward.
        Returns {name: gradient} for the names of ``set_input`` -- 'scene' / 'semantic' [C_s, H, W] (summed over the batch),
        'traj' [B, obs_len, H, W] -- as device tensors.  The parameters' ``.grad`` fields are left as they were."""
        if target not in ("both", "goal", "traj"):
            raise ValueError(f"saliency: target must be 'both', 'goal' or 'traj', got {target!r}")
        if isinstance(set_input, str) or not set_input or any(n not in ("scene", "traj", "semantic") for n in set_input) \
                or len(set(set_input)) != len(tuple(set_input)):
            raise ValueError(f"saliency: set_input must be a non-empty sequence of distinct names among 'scene', 'traj', 'semantic', "
                             f"got {set_input!r}")
        if "scene" in set_input and "semantic" in set_input:
            raise ValueError("saliency: 'scene' and 'semantic' exclude each other (the semantic map is a leaf of its own)")
        params = {k: v for k, v in self.params.items() if k != "decision"}
        try:
            return self._saliency_grads(df_test, image_path, target, tuple(set_input), params)
        finally:
            self.forward_inputs = {}
            ops.release_stale_entries()      # (the graph of the call is gone by now)

    def _saliency_grads(self, df_test, image_path, target, set_input, params):
        goal_loss, traj_loss, _ = self._forward_test(df_test, image_path, set_input, None, "loss", **params)
        loss = goal_loss + traj_loss if target == "both" else (goal_loss if target == "goal" else traj_loss)
        leaves = [self.forward_inputs[n] for n in set_input]
        grads = torch.autograd.grad(loss, leaves, allow_unused=True)
        out = {}
        for n, t, g in zip(set_input, leaves, grads):
            g = torch.zeros_like(t) if g is None else g
            out[n] = g[0] if n in ("scene", "semantic") else g
        return out

    # ------------------------------------------------------------------------------------------
    def prepare_data(self, df, image_path, dataset_name, mode, obs_len, pred_len, resize_factor, use_raw_data,
                     augment=False):
        name = dataset_name.lower()
        if name not in ("sdd", "ind-dataset-v1.0", "eth"):
            raise ValueError(f"{name} dataset is not supported")
        if name == "eth":
            raise NotImplementedError("ETH/UCY homographies are read from data files: out of the MI355X hot path")
        if not isinstance(image_path, dict):
            raise ImportError("decoding scene images needs OpenCV + segmentation_models_pytorch (out of scope here): "
                              "pass a dict {scene_id: float tensor [C,H,W]} (pre-processed, padded to a multiple "
                              f"of {self.division_factor}) instead of an image directory")
        # pad (utils/image_utils.py:95-107) and, for raw label maps, the one-hot encoding of
        # preprocess_image_for_segmentation(seg_mask=True) (image_utils.py:74-81) run on the device; decoding image files,
        # cv2.resize and the RGB normalisation of the segmentation backbone stay outside (no OpenCV / smp in this image)
        images = dict(image_path)
        if augment:
            # models/trainer.py:566-571: augment_data BEFORE resize / pad / encode -- every scene rotated by 90 / 180 / 270 degrees, then everything
            # flipped (utils/data_utils.py:176-233; the index permutations and the coordinate transforms run on the device).  Raw label maps only:
            # pre-processed planes arrive padded, and the reference pads AFTER it rotates (the border stays at the bottom / right)
            if any((im.dim() if torch.is_tensor(im) else np.asarray(im).ndim) != 2 for im in images.values()):
                raise ValueError("augment=True needs the raw label maps [H, W] (the reference augments before it pads and encodes); "
                                 "pre-processed planes [C, H, W] cannot be rotated correctly here")
            from ..utils.data_utils import augment_data
            df, images = augment_data(df, images=images, seg_mask=True)
            print("Augmented data and images")
        else:
            print("No data and images augmentation")
        for k, im in images.items():
            t = im if torch.is_tensor(im) else torch.from_numpy(np.ascontiguousarray(im))
            if t.dim() == 2:            # a label map [H, W]: padded with label 0, then one-hot planes
                if self.device.type != "cuda":
                    raise RuntimeError("raw label maps are encoded by the HIP kernels: a HIP device is required")
                images[k] = ops.seg_onehot_pad(t.to(self.device), classes=self.params.get("n_semantic_classes", 6) if hasattr(self.params, "get") else 6,
                                               division_factor=self.division_factor)
            elif t.shape[-1] % self.division_factor or t.shape[-2] % self.division_factor:
                # PRE-PROCESSED planes cannot be padded correctly here: the reference pads the raw image / label map first and
                # encodes afterwards (models/trainer.py:581-582), so its border is class 0 (plane 0 == 1) for a label map and
                # (0 - mean) / std for RGB -- a zero border in every plane would be neither.  Raw label maps [H, W]
                # take the branch above (ynet_seg_onehot_pad pads before it encodes, like the reference).
                raise ValueError(f"scene {k}: pre-processed planes {tuple(t.shape)} are not padded to a multiple of "
                                 f"{self.division_factor}; pass the raw label map [H, W] (padded and encoded on the device) "
                                 f"or pad before pre-processing (utils.image_utils.pad)")
            else:
                images[k] = t
        image_path = images
        dataset = SceneDataset(df, resize=resize_factor, total_len=obs_len + pred_len)
        generator = None
        if mode == "train" and self.dp is not None:
            # data-parallel ranks must walk the scenes in the SAME order (train_epoch shards the batches of one scene
            # over the ranks): the shuffle draws from a generator seeded identically everywhere (seed from rank 0)
            generator = torch.Generator()
            generator.manual_seed(self.dp.shared_seed())
        loader = DataLoader(dataset, batch_size=1, collate_fn=scene_collate, shuffle=(mode == "train"), generator=generator)
        return image_path, loader, None

    def load_params(self, path):
        on_gpu = self.device.type == "cuda"
        self.model.load_state_dict(torch.load(path, map_location=None if on_gpu else "cpu", weights_only=False), strict=False)
        print("Loaded ynet model to GPU" if on_gpu else "Loaded ynet model to CPU")

    def save_params(self, path, train_net):
        if train_net in ("all", "train"):
            state_dict = {k: v for k, v in self.model.state_dict().items() if "segmentation" not in k}
        else:
            state_dict = OrderedDict((n, p) for n, p in self.model.named_parameters() if p.requires_grad)
        torch.save(state_dict, path)

    def load_separated_params(self, pretrained_path, tuned_path):
        on_gpu = self.device.type == "cuda"
        for path in (pretrained_path, tuned_path):
            self.model.load_state_dict(torch.load(path, map_location=None if on_gpu else "cpu", weights_only=False), strict=False)
        print("Loaded ynet model to GPU" if on_gpu else "Loaded ynet model to CPU")

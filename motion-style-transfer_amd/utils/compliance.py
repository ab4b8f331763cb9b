"""Scene compliance: where in the scene a forecaster puts its goals, by semantic class.

ops.map_class_mass gives the share of the goal-map distribution on every class; the helpers here are the host and torch glue around
it -- the label map of a scene, the class under a point, and per-class rates and areas.  No kernel of their own: the inputs are one
label map per scene and a few points per agent.  The reference shows the goal decoder's output per style as pictures only
(evaluator/visualization.py: plot_goal_output)."""
import numpy as np
import torch

MAX_CLASSES = 8      # YNET_MAP_MAX_CLASSES of include/ynet_hip.h


def scene_labels(planes):
    """The planes [K, H, W] that prepare_data leaves per scene -> the label map [H, W] (uint8, on the planes' device): argmax over the
    planes (ties: the lowest class).  Exact for the one-hot planes of a raw label map.  For soft planes -- a segmentation network's
    scores -- it is the HARD decision per pixel: the mass on a class then means the mass on the pixels the class wins.
    More than 8 planes, or an input that is not 3-D, is refused."""
    if not torch.is_tensor(planes):
        planes = torch.from_numpy(np.ascontiguousarray(planes))
    if planes.dim() != 3:
        raise ValueError(f"scene_labels: expected the planes [K, H, W] of one scene, got {tuple(planes.shape)}")
    if not 1 <= planes.shape[0] <= MAX_CLASSES:
        raise ValueError(f"scene_labels: {planes.shape[0]} planes; ops.map_class_mass takes 1 .. {MAX_CLASSES} classes")
    return planes.argmax(dim=0).to(torch.uint8).contiguous()


def point_classes(xy, labels):
    """The class under every point: ``xy`` [..., 2] (x, y) = (column, row) in the label map's pixels, rounded half-even as the
    likelihood kernel rounds its ground truth; ``labels`` [H, W] integer tensor.  -> int64 [...] on the labels' device; -1 for a point
    that rounds outside the map or is NaN."""
    if not torch.is_tensor(labels) or labels.dim() != 2:
        raise ValueError("point_classes: labels must be the [H, W] label map of one scene")
    xy = torch.as_tensor(xy)
    if xy.dim() < 1 or xy.shape[-1] != 2:
        raise ValueError(f"point_classes: expected points [..., 2] (x, y), got {tuple(xy.shape)}")
    H, W = labels.shape
    g = torch.round(xy.to(labels.device).double())      # half to even; NaN stays NaN and fails every comparison below
    inside = (g[..., 0] >= 0) & (g[..., 0] < W) & (g[..., 1] >= 0) & (g[..., 1] < H)
    zero = torch.zeros_like(g[..., 0])
    gx, gy = torch.where(inside, g[..., 0], zero).long(), torch.where(inside, g[..., 1], zero).long()
    return torch.where(inside, labels[gy, gx].long(), torch.full_like(gx, -1))


def class_rates(classes, n_classes, dim=-1):
    """``classes``: integer tensor of classes as point_classes returns them -> float64 tensor with ``dim`` replaced by n_classes:
    entry k = the fraction of the points along ``dim`` that lie on class k.  A -1 (or any value outside 0 .. n_classes - 1) counts
    in no class but in the denominator, so the rates sum to the share of the points that hit a class."""
    classes = torch.as_tensor(classes)
    K = int(n_classes)
    if K < 1:
        raise ValueError(f"class_rates: n_classes = {K}")
    if classes.dim() < 1 or classes.is_floating_point():
        raise ValueError("class_rates: expected an integer tensor of classes with at least one dimension")
    c = classes.movedim(dim, -1)
    if c.shape[-1] == 0:
        raise ValueError("class_rates: no points along the chosen dimension")
    ks = torch.arange(K, device=c.device).view(*([1] * (c.dim() - 1)), K, 1)
    # an integer count over the number of points, one correctly rounded division: the same bits on any device.  (The divisor is a
    # tensor: by a Python number torch multiplies with the reciprocal on the device, and 3 / 20 comes out one ulp high.)
    n = torch.tensor(float(c.shape[-1]), dtype=torch.float64, device=c.device)
    return ((c.unsqueeze(-2) == ks).sum(dim=-1).double() / n).movedim(-1, dim)


def class_area(labels, n_classes):
    """The share of the map every class covers -> float64 [n_classes] (what the mass of a uniform goal map would be; labels
    >= n_classes count in the denominator only, as in ops.map_class_mass)."""
    if not torch.is_tensor(labels) or labels.dim() != 2 or labels.numel() == 0:
        raise ValueError("class_area: labels must be the non-empty [H, W] label map of one scene")
    K = int(n_classes)
    if K < 1:
        raise ValueError(f"class_area: n_classes = {K}")
    return torch.bincount(labels.reshape(-1).long(), minlength=K)[:K].double() / labels.numel()

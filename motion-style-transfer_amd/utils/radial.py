"""Radial scores of the goal-map distribution: the host side of ops.map_radial.  The kernel gives, per plane, the
mass of sigmoid(pred_goal_map / T) in every one-pixel ring around the ground truth; evaluate() draws its goals i.i.d. with replacement
from that distribution (utils/evaluate.py:128-131, utils/image_utils.py:110-135), so everything a draw-based goal error estimates follows
from the profile with no draw: with F(r) the mass closer than r,
    P(a draw lands within r) = F(r),        E[the smallest of K draws' distances] = integral over r of (1 - F(r))^K.
Pure torch on the small tensors ([..., R] per plane, a thousand times smaller than the map), on whatever device they live, in fp64."""
import torch

DEFAULT_RADII = (4, 8, 16)      # map pixels
DEFAULT_KS = (1, 5, 20)
MAX_RINGS = 1024                # ops.RADIAL_MAX_RINGS


def radial_options(return_radial, what="evaluate(return_radial=...)"):
    """The drivers' flag -> None (off), or {'radii': tuple of ints, 'k': tuple of ints}: True means DEFAULT_RADII and DEFAULT_KS, a dict
    may give either or both -- ``radii``: 1 or more whole numbers of map pixels in 0 .. 1024 (F is known at whole radii only), ``k``:
    1 or more whole numbers of draws >= 1.  Anything else is refused."""
    if return_radial is None or return_radial is False:
        return None
    if return_radial is True:
        return {"radii": DEFAULT_RADII, "k": DEFAULT_KS}
    if not isinstance(return_radial, dict) or not set(return_radial) <= {"radii", "k"}:
        raise ValueError(f"{what}: False, True or a dict with 'radii' and / or 'k' is expected, got {return_radial!r}")

    def whole(key, default, lo, hi):
        seq = return_radial.get(key, default)
        try:
            seq = tuple(seq)
        except TypeError:
            seq = ()
        ok = len(seq) > 0 and all(isinstance(v, (int, float)) and not isinstance(v, bool) and float(v) == int(v) and lo <= v <= hi for v in seq)
        if not ok:
            raise ValueError(f"{what}: {key!r} must be a non-empty sequence of whole numbers in {lo} .. {hi}, got {return_radial.get(key)!r}")
        return tuple(int(v) for v in seq)

    return {"radii": whole("radii", DEFAULT_RADII, 0, MAX_RINGS), "k": whole("k", DEFAULT_KS, 1, 1 << 30)}


def radial_cdf(ring):
    """ring [..., R] -> F [..., R + 1] in fp64: F[j] = the mass closer than j pixels = ring[0] + .. + ring[j - 1]; F[0] = 0."""
    ring = torch.as_tensor(ring).double()
    return torch.cat([torch.zeros_like(ring[..., :1]), ring.cumsum(dim=-1)], dim=-1)


def hit_rate(ring, radii):
    """The probability that one draw lands closer than r map pixels to the ground truth, per radius -> [..., n_radii] in fp64.  The
    profile knows F at whole radii up to R only: a radius that is negative, not whole or above R is refused."""
    ring = torch.as_tensor(ring)
    R = ring.shape[-1]
    radii = list(radii)
    for r in radii:
        if isinstance(r, bool) or float(r) != int(r) or not 0 <= int(r) <= R:
            raise ValueError(f"hit_rate: radius {r!r}: a whole number of map pixels in 0 .. {R} (the rings of the profile) is expected")
    return radial_cdf(ring)[..., [int(r) for r in radii]]


def farthest_corner(gt_xy, H: int, W: int):
    """gt_xy [..., 2] (x, y) -> the ceiling of the distance from the rounded ground truth to the farthest pixel of an H x W map (a
    corner), fp64: no draw lies farther."""
    g = torch.round(torch.as_tensor(gt_xy).double())
    dx = torch.maximum(g[..., 0].abs(), (W - 1 - g[..., 0]).abs())
    dy = torch.maximum(g[..., 1].abs(), (H - 1 - g[..., 1]).abs())
    return torch.ceil(torch.sqrt(dx * dx + dy * dy))


def expected_best_of_k(ring, tail, ks, far=None):
    """Bounds on E[the smallest of K i.i.d. draws' distances to the ground truth], in map pixels -> (lower, upper), each [..., n_k] fp64.
    With S(j) = the mass at j pixels or more (S(0) = 1, S(R) = tail) the survival function of the distance lies between S(j + 1) and
    S(j) on [j, j + 1), so
        lower = sum_{j < R} S(j + 1)^K,        upper = sum_{j < R} S(j)^K + tail^K * max(0, far - R).
    ``far`` (a number, or a tensor like tail): the ceiling of the largest possible distance (farthest_corner); needed only where
    tail > 0.  With an empty tail the bracket is exactly one pixel wide (the width of a ring)."""
    ring, tail = torch.as_tensor(ring).double(), torch.as_tensor(tail).double()
    if ring.shape[:-1] != tail.shape:
        raise ValueError(f"expected_best_of_k: ring {tuple(ring.shape)} and tail {tuple(tail.shape)} do not belong together")
    ks = list(ks)
    if not ks or any(isinstance(k, bool) or float(k) != int(k) or int(k) < 1 for k in ks):
        raise ValueError(f"expected_best_of_k: ks {ks!r}: whole numbers of draws >= 1 are expected")
    R = ring.shape[-1]
    has_tail = bool((tail > 0).any())
    if far is None:
        if has_tail:
            raise ValueError("expected_best_of_k: a plane has mass beyond the rings (tail > 0): the upper bound needs `far`, the largest "
                             "possible distance (utils.radial.farthest_corner)")
        beyond = torch.zeros_like(tail)
    else:
        beyond = (torch.as_tensor(far, device=tail.device).double() - R).clamp(min=0).expand_as(tail)
    # S[..., j], j = 0 .. R: summed from the far end, so that S(R) is the tail itself; S(0) = 1 by definition
    S = torch.cat([ring, tail[..., None]], dim=-1).flip(-1).cumsum(dim=-1).flip(-1)
    S = torch.cat([torch.ones_like(S[..., :1]) + 0.0 * S[..., :1], S[..., 1:]], dim=-1).clamp(max=1.0)      # (0 * NaN keeps a NaN plane NaN)
    lower, upper = [], []
    for k in ks:
        Sk = S ** int(k)
        lower.append(Sk[..., 1:].sum(dim=-1))
        upper.append(Sk[..., :-1].sum(dim=-1) + torch.where(tail > 0, Sk[..., -1] * beyond, torch.zeros_like(tail) + 0.0 * tail))
    return torch.stack(lower, dim=-1), torch.stack(upper, dim=-1)


def radial_summary(profile, gt_xy, H: int, W: int, radii, ks):
    """What evaluate() keeps of a batch's profile (the dict of ops.map_radial with all four outputs; gt_xy [N, C, 2] in map pixels) ->
    {"mean", "rms" [N, C], "hit" [N, C, n_radii], "best_of_k_lower", "best_of_k_upper" [N, C, n_k]}, fp64, in MAP pixels."""
    lower, upper = expected_best_of_k(profile["ring"], profile["tail"], ks, farthest_corner(gt_xy.to(profile["tail"].device), H, W))
    return {"mean": profile["mean"].double(), "rms": profile["mean_sq"].double().sqrt(), "hit": hit_rate(profile["ring"], radii),
            "best_of_k_lower": lower, "best_of_k_upper": upper}


def radial_report(radii, ks, mean, hit, lower, upper, fde=None):
    """The lines YNetTrainer.test(return_radial=...) prints per round for the last step: mean [N], lower / upper [N, n_k] in the units
    of FDE, hit [N, n_radii]; rows with a NaN (a plane that could not be scored) are left out of each average."""
    import numpy as np
    mean, hit = np.asarray(mean, dtype=np.float64), np.asarray(hit, dtype=np.float64).reshape(-1, len(radii))
    lower, upper = np.asarray(lower, dtype=np.float64).reshape(-1, len(ks)), np.asarray(upper, dtype=np.float64).reshape(-1, len(ks))
    avg = lambda v: float(v[np.isfinite(v)].mean()) if np.isfinite(v).any() else float("nan")
    lines = [f"Radial goal scores (no draw; n = {int(np.isfinite(mean).sum())})", f"  expected goal error of one draw: {avg(mean):.4f}"]
    for j, k in enumerate(ks):
        lines.append(f"  expected best-of-{k} goal error: {avg(lower[:, j]):.4f} .. {avg(upper[:, j]):.4f}"
                     + (f"   (sampled FDE of this round: {float(fde):.4f})" if fde is not None else ""))
    lines.append("  mass within r map pixels of the goal: " + ", ".join(f"r = {r}: {avg(hit[:, j]):.4f}" for j, r in enumerate(radii)))
    return "\n".join(lines)

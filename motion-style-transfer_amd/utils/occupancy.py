"""Scene occupancy of the goal maps: the host side of ops.map_occupancy.  The kernel gives, per scene and future
step, the expected number of agents in every cell of the map, the probability that a cell holds anybody, the expected number of agent
pairs that share a cell and every agent's share of them; here are the cell grid, the map for drawing an occupancy over the scene, and
the table of conflicts per step."""
import numpy as np
import torch

CELLS = (1, 2, 4, 8)


def cell_grid(H, W, cell):
    """-> (Hc, Wc) = (ceil(H / cell), ceil(W / cell)): the cells of an H x W map; the last row and column of cells are partial where
    cell does not divide H or W"""
    H, W, cell = int(H), int(W), int(cell)
    if cell not in CELLS:
        raise ValueError(f"cell_grid: cell = {cell}, expected one of {CELLS}")
    if H < 1 or W < 1:
        raise ValueError(f"cell_grid: a map of {H}x{W} has no cells")
    return -(-H // cell), -(-W // cell)


def cell_pixels(H, W, cell):
    """-> [Hc, Wc] int64: the pixels of the map inside every cell (cell * cell, less in a partial edge cell)"""
    Hc, Wc = cell_grid(H, W, cell)
    rows = torch.clamp(H - torch.arange(Hc) * cell, max=cell)
    cols = torch.clamp(W - torch.arange(Wc) * cell, max=cell)
    return rows.view(Hc, 1) * cols.view(1, Wc)


def upsample_occupancy(occ, H, W, cell):
    """A per-cell map [..., Hc, Wc] (``occupancy``: an expected count per cell) as a per-pixel map [..., H, W] for overlays: every pixel
    gets its cell's value over the pixels in the cell, so the result is a density per pixel of the resized map and sums to what
    ``occ`` sums to.  (For ``any``, a probability and not a count, index instead: any[..., rows // cell, cols // cell].)"""
    Hc, Wc = cell_grid(H, W, cell)
    occ = torch.as_tensor(occ)
    if occ.dim() < 2 or tuple(occ.shape[-2:]) != (Hc, Wc):
        raise ValueError(f"upsample_occupancy: {tuple(occ.shape)} does not end in the {(Hc, Wc)} cells of a {H}x{W} map at cell {cell}")
    per_pixel = occ / cell_pixels(H, W, cell).to(device=occ.device, dtype=occ.dtype)
    rows = torch.arange(H, device=occ.device) // cell
    cols = torch.arange(W, device=occ.device) // cell
    return per_pixel[..., rows[:, None], cols[None, :]]


def conflict_report(conflict, risk, resize_factor, cell):
    """Per future step one dict, from ``conflict`` [C] (one scene's row of ops.map_occupancy's result) and ``risk`` [N, C]:
    ``step``, ``pairs`` (the expected number of agent pairs that share a cell at that step), ``agents`` (the agents' rows ranked by
    descending risk; a NaN risk goes last), ``risk`` (their risks in that order: the expected number of other agents in the agent's
    cell) and ``cell_edge`` (the edge of a cell in pixels of the original image: cell / resize_factor)."""
    conflict = np.asarray(torch.as_tensor(conflict).detach().cpu(), dtype=np.float64).reshape(-1)
    risk = np.asarray(torch.as_tensor(risk).detach().cpu(), dtype=np.float64)
    if int(cell) not in CELLS or not float(resize_factor) > 0:
        raise ValueError(f"conflict_report: cell {cell!r} must be one of {CELLS} and resize_factor {resize_factor!r} positive")
    if risk.ndim != 2 or risk.shape[1] != conflict.size:
        raise ValueError(f"conflict_report: risk {risk.shape} does not go with the {conflict.size} steps of conflict (expected [N, {conflict.size}])")
    edge = int(cell) / float(resize_factor)
    rows = []
    for c in range(conflict.size):
        r = risk[:, c]
        order = np.argsort(np.where(np.isnan(r), np.inf, -r), kind="stable")      # (ties keep the row order)
        rows.append({"step": c, "pairs": float(conflict[c]), "agents": order.tolist(), "risk": r[order].tolist(), "cell_edge": edge})
    return rows

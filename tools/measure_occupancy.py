"""Event times of one ynet_map_occupancy call (three launches) against ynet_map_likelihood on the same logits (the clock of ONE read of
the map) and the stock-torch composition on the device (sigmoid, normalise, pool, sums and products over the agents), at the evaluation
sweep's own shape: 128 agents x 12 steps of 256 x 256, one group.  Cell 1 and 4, with and without ``risk``.
Per candidate: 3 warm calls, then 9 windows of 20 back-to-back calls between two events, the candidates taking turns window by window;
median, least and largest window / 20.  ``reads`` is the median over map_likelihood's median.
usage: python tools/measure_occupancy.py [rows.json]   (needs the MI355X; one JSON line per cell edge on stdout)"""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
ops = importlib.import_module("motion-style-transfer_amd.ops")
dev = torch.device("cuda:0")
B, C, H, W, T = 128, 12, 256, 256, 1.8
WINDOWS, PER_WINDOW = 9, 20

def torch_comp(x, cell, risk):
    w = torch.sigmoid(x / T)
    p = w / w.sum(dim=(2, 3), keepdim=True)
    m = torch.nn.functional.avg_pool2d(p, cell, divisor_override=1) if cell > 1 else p      # (H and W are multiples of the cell here)
    D = m.sum(0)
    out = {"occupancy": D[None], "any": (1.0 - (1.0 - m).prod(0))[None], "conflict": (0.5 * (D * D - (m * m).sum(0)).sum(dim=(1, 2)))[None]}
    if risk:
        out["risk"] = (m * (D - m)).sum(dim=(2, 3))
    return out

gen = torch.Generator(device=dev).manual_seed(3)
x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
nbytes = x.numel() * 4
NO_RISK = ("occupancy", "any", "conflict")
out = []
for cell in (1, 4):
    cands = (("map_occupancy", lambda: ops.map_occupancy(x, None, cell, T, want=NO_RISK)),
             ("map_occupancy_risk", lambda: ops.map_occupancy(x, None, cell, T)),
             ("map_likelihood", lambda: ops.map_likelihood(x, gt, T)),
             ("torch_composition", lambda: torch_comp(x, cell, False)),
             ("torch_composition_risk", lambda: torch_comp(x, cell, True)))
    for _, fn in cands:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ts = {name: [] for name, _ in cands}
    for _ in range(WINDOWS):
        for name, fn in cands:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(PER_WINDOW):
                fn()
            b.record()
            torch.cuda.synchronize()
            ts[name].append(a.elapsed_time(b) * 1e3 / PER_WINDOW)
    one_read = statistics.median(ts["map_likelihood"])
    row = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "H": H, "W": W, "groups": 1, "cell": cell, "T": T, "bytes_one_read": nbytes}
    for name, v in ts.items():
        med = statistics.median(v)
        row[name] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "reads": round(med / one_read, 2)}
    got, ref = ops.map_occupancy(x, None, cell, T), torch_comp(x, cell, True)
    row["max_abs_diff_vs_torch_fp32"] = {k: float((got[k] - ref[k]).abs().max()) for k in got}
    ops.check_likelihood_status()
    ops.check_occupancy_status()
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:          # optional: keep the rows in a JSON file
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

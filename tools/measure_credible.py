"""Event times of one ynet_map_credible launch against ynet_map_likelihood on the same tensor (one read of the logits) and the stock-torch
composition on the device -- sigmoid, sort descending, cumsum, searchsorted, and the plateau fix-up -- (DESIGN.md section 4.14): ten
warm replays each, median, at B 32 x 12 and B 128 x 30 planes of 256 x 256, 2 and 8 levels, T = 1 and 1.8.
usage: python tools/measure_credible.py [rows.json]   (needs the MI355X; one JSON line per case on stdout)"""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
ops = importlib.import_module("motion-style-transfer_amd.ops")
dev = torch.device("cuda:0")
LEVELS = {2: (0.5, 0.9), 8: (0.1, 0.25, 0.5, 0.75, 0.9, 0.99, 0.999, 0.999999)}

def torch_comp(x, q, T):
    B, C, H, W = x.shape
    xs = torch.sort(x.flatten(2), dim=2, descending=True).values
    cum = torch.sigmoid(xs / T).cumsum(dim=2)
    Z = cum[..., -1:]
    pos = torch.searchsorted(cum, (q * Z).contiguous()).clamp_(max=H * W - 1)      # the first sorted pixel at which the mass reaches q Z
    thr = xs.gather(2, pos)
    area = torch.searchsorted(-xs, (-thr).contiguous(), right=True)               # the plateau fix-up: every pixel that ties with it
    mass = cum.gather(2, area - 1) / Z
    return area, thr, mass

def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)

out = []
for B, C in ((32, 12), (128, 30)):
    H = W = 256
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
    gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
    nbytes = x.numel() * 4
    for L in (2, 8):
        q = torch.tensor(LEVELS[L], device=dev)
        for T in (1.0, 1.8):
            row = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "H": H, "W": W, "L": L, "T": T, "bytes_one_read": nbytes}
            for name, fn in (("map_credible", lambda: ops.map_credible(x, LEVELS[L], T)),
                             ("map_likelihood", lambda: ops.map_likelihood(x, gt, T)),
                             ("torch_composition", lambda: torch_comp(x, q, T))):
                med, lo, hi = timed(fn)
                row[name] = {"median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
            row["reads_worth_vs_map_likelihood"] = round(row["map_credible"]["median_us"] / row["map_likelihood"]["median_us"], 2)
            row["speedup_vs_torch"] = round(row["torch_composition"]["median_us"] / row["map_credible"]["median_us"], 2)
            a, b = ops.map_credible(x, LEVELS[L], T), torch_comp(x, q, T)
            row["areas_equal_to_torch_fp32"] = float((a["area"] == b[0]).float().mean())
            row["max_abs_mass_diff_vs_torch_fp32"] = float((a["mass"] - b[2]).abs().max())
            ops.check_credible_status()
            ops.check_likelihood_status()
            print(json.dumps(row), flush=True)
            out.append(row)
            del a, b
            torch.cuda.empty_cache()
    del x
if len(sys.argv) > 1:          # optional: keep the rows in a JSON file
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

"""Event times of one ynet_map_likelihood launch against ynet_softargmax2d on the same tensor and the stock-torch composition on the
device: ten warm replays each, median, at B 32 x 12 and B 128 x 30 planes of 256 x 256, T = 1 and 1.8.
usage: python tools/measure_likelihood.py [rows.json]   (needs the MI355X; one JSON line per case on stdout)"""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
ops = importlib.import_module("motion-style-transfer_amd.ops")
dev = torch.device("cuda:0")

def torch_comp(x, gt, T):
    z = x / T
    w = torch.sigmoid(z)
    ls = torch.nn.functional.logsigmoid(z)
    Z = w.sum(dim=(2, 3))
    logZ = torch.log(Z)
    ent = logZ - (w * ls).sum(dim=(2, 3)) / Z
    B, C, H, W = x.shape
    g = torch.round(gt).long()
    xg = x.flatten(2).gather(2, (g[..., 1] * W + g[..., 0]).unsqueeze(-1))
    nll = logZ - torch.nn.functional.logsigmoid(xg[..., 0] / T)
    hpd = torch.where(x >= xg.unsqueeze(-1), w, torch.zeros((), device=x.device)).sum(dim=(2, 3)) / Z
    return nll, ent, hpd

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
for B, C, T in ((32, 12, 1.0), (32, 12, 1.8), (128, 30, 1.0), (128, 30, 1.8)):
    H = W = 256
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
    gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
    nbytes = x.numel() * 4
    row = {"B": B, "C": C, "H": H, "W": W, "T": T, "bytes": nbytes}
    for name, fn in (("map_likelihood", lambda: ops.map_likelihood(x, gt, T)),
                     ("map_likelihood_entropy_only", lambda: ops.map_likelihood(x, None, T, want=("entropy",))),
                     ("softargmax2d", lambda: ops.softargmax2d(x)),
                     ("torch_composition", lambda: torch_comp(x, gt, T))):
        med, lo, hi = timed(fn)
        row[name] = {"median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
    a = ops.map_likelihood(x, gt, T); b = torch_comp(x, gt, T)
    row["max_abs_diff_vs_torch_fp32"] = {k: float((a[k] - v).abs().max()) for k, v in zip(("nll", "entropy", "hpd"), b)}
    ops.check_likelihood_status()
    print(json.dumps(row), flush=True)
    out.append(row)
    del x
if len(sys.argv) > 1:          # optional: keep the rows in a JSON file
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

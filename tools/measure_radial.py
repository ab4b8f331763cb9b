"""Event times of one ynet_map_radial launch against ynet_map_likelihood on the same tensor (one read of the logits: the project's clock
for a map read) and the stock-torch composition on the device -- sigmoid, normalise, integer ring index, scatter_add -- (DESIGN.md
section 4.16): thirty warm replays each, median, at 128 x 12 planes of 256 x 256, the default ring count, T = 1 and 1.8.
usage: python tools/measure_radial.py [rows.json]   (needs the MI355X; one JSON line per case on stdout)
YNET_HIP_LIB=<another build> runs the same cases against it; MEASURE_RADIAL_TORCH=0 leaves the torch composition out (A/B runs)."""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)


def torch_comp(x, gt, R, T):
    B, C, H, W = x.shape
    w = torch.sigmoid(x / T)
    Z = w.sum(dim=(2, 3))
    g = torch.round(gt).long()
    dy = torch.arange(H, device=x.device).view(1, 1, H, 1) - g[..., 1, None, None]
    dx = torch.arange(W, device=x.device).view(1, 1, 1, W) - g[..., 0, None, None]
    d2 = dx * dx + dy * dy
    k = torch.sqrt(d2.double()).long()                                   # (exact below 2^52: a correctly rounded fp64 root never reaches the next integer)
    hist = torch.zeros(B, C, R + 1, device=x.device).scatter_add_(2, k.clamp(max=R).flatten(2), w.flatten(2))
    return hist[..., :R] / Z[..., None], hist[..., R] / Z, (w * torch.sqrt(d2.float())).sum(dim=(2, 3)) / Z, (w * d2.float()).sum(dim=(2, 3)) / Z


def timed(fn, reps=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts), min(ts), max(ts)


def main():
    ops = importlib.import_module("motion-style-transfer_amd.ops")
    lib_path = importlib.import_module("motion-style-transfer_amd._lib").LIB_PATH
    dev = torch.device("cuda:0")
    out = []
    B, C, H, W = 128, 12, 256, 256
    R = ops.radial_rings(H, W)
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
    gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
    nbytes = x.numel() * 4
    for T in (1.0, 1.8):
        row = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(lib_path), "B": B, "C": C, "H": H, "W": W, "n_rings": R, "T": T,
               "bytes_one_read": nbytes}
        cases = [("map_radial", lambda: ops.map_radial(x, gt, None, T)), ("map_likelihood", lambda: ops.map_likelihood(x, gt, T))]
        if os.environ.get("MEASURE_RADIAL_TORCH", "1") != "0":
            cases.append(("torch_composition", lambda: torch_comp(x, gt, R, T)))
        for name, fn in cases:
            med, lo, hi = timed(fn, reps=30 if name != "torch_composition" else 10, warm=5 if name != "torch_composition" else 2)
            row[name] = {"median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
        row["reads_worth_vs_map_likelihood"] = round(row["map_radial"]["median_us"] / row["map_likelihood"]["median_us"], 2)
        if "torch_composition" in row:
            row["speedup_vs_torch"] = round(row["torch_composition"]["median_us"] / row["map_radial"]["median_us"], 2)
            a, b = ops.map_radial(x, gt, None, T), torch_comp(x, gt, R, T)
            row["max_abs_ring_diff_vs_torch_fp32"] = float((a["ring"] - b[0]).abs().max())
            row["max_rel_mean_diff_vs_torch_fp32"] = float(((a["mean"] - b[2]).abs() / b[2]).max())
            del a, b
        ops.check_radial_status()
        ops.check_likelihood_status()
        print(json.dumps(row), flush=True)
        out.append(row)
        torch.cuda.empty_cache()
    if len(sys.argv) > 1:          # optional: keep the rows in a JSON file
        with open(sys.argv[1], "w") as f:
            json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

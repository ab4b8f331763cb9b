"""Event times of one ynet_map_marginals launch against ynet_map_likelihood on the same tensor (one read of the logits: the project's clock
for a map read) and the stock-torch composition on the device -- sigmoid, normalise, two sums, two cumsums, CRPS, PIT -- (DESIGN.md
section 4.17): thirty warm replays each, median, at 128 x 12 planes of 256 x 256 and of 512 x 512, T = 1 and 1.8; the launch is also timed
in its form without ground truth (col and row alone).  (The A/B of the register path that the kernel once had -- against the path it
kept, forced on the same 256 x 256 planes in the same process -- is recorded in profiles/marginals_register_ab.json.)
usage: python tools/measure_marginals.py [rows.json]   (needs the MI355X; one JSON line per case on stdout; default
profiles/marginals_measure.json)
YNET_HIP_LIB=<another build> runs the same cases against it; MEASURE_MARGINALS_TORCH=0 leaves the torch composition out."""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)


def torch_comp(x, gt, T):
    B, C, H, W = x.shape
    w = torch.sigmoid(x / T)
    Z = w.sum(dim=(2, 3))
    g = torch.round(gt).long()
    out = {}
    for name, sums, side, ga in (("col", w.sum(dim=2), W, g[..., 0]), ("row", w.sum(dim=3), H, g[..., 1])):
        out[name] = sums / Z[..., None]
        F = (sums.cumsum(dim=-1) / Z[..., None]).clamp(max=1.0)
        t = torch.arange(side, device=x.device).view(1, 1, side)
        out["crps_" + name] = torch.where(t < ga[..., None], F * F, (1 - F) * (1 - F)).sum(dim=-1) + (ga - side).clamp(min=0) + (-ga).clamp(min=0)
        at = lambda k: torch.where(k < 0, torch.zeros_like(Z), torch.where(k >= side - 1, torch.ones_like(Z), F.gather(2, k.clamp(0, side - 1)[..., None])[..., 0]))
        out["pit_" + name] = torch.stack([at(ga - 1), at(ga)], dim=-1)
    return out


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
    B, C = 128, 12
    for H, W in ((256, 256), (512, 512)):
        gen = torch.Generator(device=dev).manual_seed(3)
        x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
        gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
        nbytes = x.numel() * 4
        for T in (1.0, 1.8):
            row = {"device": torch.cuda.get_device_name(0), "lib": os.path.basename(lib_path), "B": B, "C": C, "H": H, "W": W, "T": T,
                   "bytes_one_read": nbytes}

            cases = [("map_marginals", lambda: ops.map_marginals(x, gt, T)), ("map_likelihood", lambda: ops.map_likelihood(x, gt, T)),
                     ("map_marginals_profiles_only", lambda: ops.map_marginals(x, None, T, want=("col", "row")))]
            if os.environ.get("MEASURE_MARGINALS_TORCH", "1") != "0":
                cases.append(("torch_composition", lambda: torch_comp(x, gt, T)))
            for name, fn in cases:
                med, lo, hi = timed(fn, reps=30 if name != "torch_composition" else 10, warm=5 if name != "torch_composition" else 2)
                row[name] = {"median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
            row["reads_worth_vs_map_likelihood"] = round(row["map_marginals"]["median_us"] / row["map_likelihood"]["median_us"], 2)
            if "torch_composition" in row:
                row["speedup_vs_torch"] = round(row["torch_composition"]["median_us"] / row["map_marginals"]["median_us"], 2)
                a, b = ops.map_marginals(x, gt, T), torch_comp(x, gt, T)
                row["max_abs_col_diff_vs_torch_fp32"] = float((a["col"] - b["col"]).abs().max())
                row["max_rel_crps_diff_vs_torch_fp32"] = float(((a["crps"][..., 0] - b["crps_col"]).abs() / b["crps_col"]).max())
                del a, b
            ops.check_marginals_status()
            ops.check_likelihood_status()
            print(json.dumps(row), flush=True)
            out.append(row)
            torch.cuda.empty_cache()
        del x, gt
        torch.cuda.empty_cache()
    path = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "marginals_measure.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)


if __name__ == "__main__":
    main()

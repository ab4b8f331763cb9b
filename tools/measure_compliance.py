"""Event times of one ynet_map_class_mass launch against ynet_map_likelihood on the same logits (read once: the natural floor) and the
stock-torch composition on the device (sigmoid, normalise, einsum with the one-hot planes), at the evaluation sweep's own shape:
128 x 12 planes of 256 x 256, 6 classes.  Per candidate and temperature: 3 warm launches, then 9 windows of
50 back-to-back launches between two events, the candidates taking turns window by window; median, least and largest window / 50.
(Each launch is enqueued through ops: ~20 us of host work, hidden behind the previous launch as long as a launch runs longer.)
usage: python tools/measure_compliance.py [rows.json]   (needs the MI355X; one JSON line per temperature on stdout)"""
import importlib, json, os, sys, statistics
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
ops = importlib.import_module("motion-style-transfer_amd.ops")
dev = torch.device("cuda:0")
B, C, H, W, K = 128, 12, 256, 256, 6
WINDOWS, PER_WINDOW = 9, 50

def torch_comp(x, onehot, T):
    w = torch.sigmoid(x / T)
    p = w / w.sum(dim=(2, 3), keepdim=True)
    return torch.einsum("bchw,khw->bck", p, onehot)

gen = torch.Generator(device=dev).manual_seed(3)
x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
labels = torch.randint(0, K, (H, W), device=dev, generator=gen).to(torch.uint8)
onehot = torch.nn.functional.one_hot(labels.long(), K).permute(2, 0, 1).float().contiguous()
gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
nbytes = x.numel() * 4 + labels.numel()
out = []
for T in (1.0, 1.8):
    cands = (("map_class_mass", lambda: ops.map_class_mass(x, labels, K, T)),
             ("map_likelihood", lambda: ops.map_likelihood(x, gt, T)),
             ("torch_composition", lambda: torch_comp(x, onehot, T)))
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
    row = {"device": torch.cuda.get_device_name(0), "B": B, "C": C, "H": H, "W": W, "K": K, "T": T, "bytes_one_read": nbytes}
    for name, v in ts.items():
        med = statistics.median(v)
        row[name] = {"median_us": round(med, 1), "min_us": round(min(v), 1), "max_us": round(max(v), 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
    row["max_abs_diff_vs_torch_fp32"] = float((ops.map_class_mass(x, labels, K, T) - torch_comp(x, onehot, T)).abs().max())
    ops.check_likelihood_status()
    print(json.dumps(row), flush=True)
    out.append(row)
if len(sys.argv) > 1:          # optional: keep the rows in a JSON file
    with open(sys.argv[1], "w") as f:
        json.dump(out, f, indent=1)

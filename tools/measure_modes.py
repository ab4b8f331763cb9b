"""Event times of one ynet_map_modes launch against the stock-torch composition on the device (M rounds of argmax + disk masked_fill
+ the masked sums) and one ynet_softargmax2d launch over the same tensor (the cost of reading the map once), DESIGN.md section 4.11:
ten warm replays each, median, at B 32 x 1 plane of 256 x 256 and B 128 x 1 plane of 512 x 512, M 20, r 8.  With --predict also the
wall time of predict_modes beside predict() at K 20, B 32, 256 x 256 from this process.
usage: python tools/measure_modes.py [--predict] [rows.json]   (needs the MI355X; one JSON line per case on stdout)"""
import importlib, json, os, sys, statistics, time
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
PKG = "motion-style-transfer_amd"
ops = importlib.import_module(PKG + ".ops")
dev = torch.device("cuda:0")

def torch_comp(x, M, r, T):
    """greedy NMS in stock torch on the device: per round an argmax, a disk masked_fill and a masked sum, each over the whole [B, H, W]"""
    B, _, H, W = x.shape
    v = x[:, 0]
    w = torch.sigmoid(v / T)
    Z = w.sum(dim=(1, 2))
    live = v.clone()
    sup = torch.zeros_like(v, dtype=torch.bool)
    rows, cols = torch.arange(H, device=x.device).view(1, H, 1), torch.arange(W, device=x.device).view(1, 1, W)
    xy, mass = [], []
    for _ in range(M):
        idx = live.flatten(1).argmax(dim=1)
        row, col = (idx // W).view(B, 1, 1), (idx % W).view(B, 1, 1)
        disk = (rows - row) ** 2 + (cols - col) ** 2 <= r * r
        mass.append((w * (disk & ~sup)).sum(dim=(1, 2)) / Z)
        sup |= disk
        live.masked_fill_(disk, float("-inf"))
        xy.append(torch.stack([col.view(B), row.view(B)], dim=1))
    return torch.stack(xy, dim=1).float(), torch.stack(mass, dim=1)

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

args = [a for a in sys.argv[1:] if a != "--predict"]
out = []
M, r, T = 20, 8, 1.0
for B, H in ((32, 256), (128, 512)):
    W = H
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, 1, H, W, device=dev, generator=gen) * 3.0 - 6.0
    nbytes = x.numel() * 4
    row = {"B": B, "H": H, "W": W, "M": M, "radius": r, "T": T, "bytes": nbytes}
    for name, fn in (("map_modes", lambda: ops.map_modes(x, M, r, T)),
                     ("map_modes_no_mass", lambda: ops.map_modes(x, M, r, want_mass=False)),
                     ("map_modes_one_mode", lambda: ops.map_modes(x, 1, r, T)),
                     ("softargmax2d", lambda: ops.softargmax2d(x)),
                     ("torch_composition", lambda: torch_comp(x, M, r, T))):
        med, lo, hi = timed(fn)
        row[name] = {"median_us": round(med, 1), "min_us": round(lo, 1), "max_us": round(hi, 1), "TB_per_s_one_read": round(nbytes / med / 1e6, 3)}
    a, (bxy, bmass) = ops.map_modes(x, M, r, T), torch_comp(x, M, r, T)
    row["picks_equal_torch"] = bool(torch.equal(a["xy"][:, 0], bxy))
    row["max_abs_mass_diff_vs_torch_fp32"] = float((a["mass"][:, 0] - bmass).abs().max())
    ops.check_modes_status()
    print(json.dumps(row), flush=True)
    out.append(row)
    del x

if "--predict" in sys.argv[1:]:      # wall time of the two drivers at section 4.8's C5 shape, from one process, synchronised
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from conftest import Golden, build_model
    from oracle import ynet_oracle as O
    P = importlib.import_module(PKG + ".utils.predict")
    g = Golden("trained_short_full")
    cfg = g.cfg()
    model = build_model(cfg, g.state_dict(), dev)
    in_t = O.dist_template(cfg.template_size).to(dev)
    observed = g.t("traj")[:, :cfg.obs_len].repeat(32 // g.t("traj").shape[0], 1, 1)
    common = (model, g.t("scene")[0], observed, in_t, list(cfg.waypoints))
    tail = (cfg.obs_len, cfg.resize_factor, cfg.temperature)

    def wall(fn, reps=10, warm=3):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    row = {"shape": "B 32, 256 x 256, K = M = 20", "predict": wall(lambda: P.predict(*common, 20, 1, *tail, network=cfg.network)),
           "predict_modes_r8": wall(lambda: P.predict_modes(*common, 20, 8, *tail, network=cfg.network))}
    print(json.dumps(row), flush=True)
    out.append(row)
if args:          # optional: keep the rows in a JSON file
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)

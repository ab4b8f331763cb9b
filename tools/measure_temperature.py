"""Event times of one ynet_map_likelihood_sweep launch against n_T back-to-back launches of ynet_map_likelihood (nll and hpd wanted) on
the same tensors in the same process: ten warm replays each, median, at B 32 x 12 and B 128 x 30 planes of
256 x 256, n_T = 4, 16 and 32 log-spaced temperatures over [0.25, 8].  Both sides go through the C entry points with their outputs
allocated beforehand, so the columns hold launches and nothing else.  With --calibrate also the wall time of a two-round
calibrate_temperature beside two evaluate(return_likelihood=True) calls (one per candidate temperature: what the search would cost
without the sweep, per pair of candidates) at B 32, 256 x 256, K 20 from this process.
usage: python tools/measure_temperature.py [--calibrate] [rows.json]   (needs the MI355X; one JSON line per case on stdout)"""
import ctypes, importlib, json, os, sys, statistics, time
import numpy as np
import torch
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # (tools/ -> the repository)
sys.path.insert(0, ROOT)
ops = importlib.import_module("motion-style-transfer_amd.ops")
lk = importlib.import_module("motion-style-transfer_amd.utils.likelihood")
L = importlib.import_module("motion-style-transfer_amd._lib")
lib = L.load()
dev = torch.device("cuda:0")

def timed(fn, reps=10, warm=3):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); torch.cuda.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return {"median_us": round(statistics.median(ts), 1), "min_us": round(min(ts), 1), "max_us": round(max(ts), 1)}

out = []
for B, C in ((32, 12), (128, 30)):
    H = W = 256
    gen = torch.Generator(device=dev).manual_seed(3)
    x = torch.randn(B, C, H, W, device=dev, generator=gen) * 3.0 - 6.0
    gt = torch.stack([torch.randint(0, W, (B, C), device=dev, generator=gen), torch.randint(0, H, (B, C), device=dev, generator=gen)], -1).float()
    status = torch.zeros(1, device=dev, dtype=torch.int32)
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    for n_T in (4, 16, 32):
        temps = lk.temperature_grid(0.25, 8.0, n_T)
        sweep = {k: torch.empty(n_T, B, C, device=dev) for k in ("nll", "hpd")}
        loop = {k: torch.empty(n_T, B, C, device=dev) for k in ("nll", "hpd")}
        tp = temps.ctypes.data_as(ctypes.POINTER(ctypes.c_float))

        def one_sweep():
            L.check(lib.ynet_map_likelihood_sweep(x.data_ptr(), x.stride(0), gt.data_ptr(), B, C, H, W, tp, n_T, sweep["nll"].data_ptr(),
                                                  sweep["hpd"].data_ptr(), status.data_ptr(), stream), lib)

        def n_launches():
            for k in range(n_T):
                L.check(lib.ynet_map_likelihood(x.data_ptr(), x.stride(0), gt.data_ptr(), B, C, H, W, float(temps[k]), loop["nll"][k].data_ptr(),
                                                None, loop["hpd"][k].data_ptr(), status.data_ptr(), stream), lib)

        row = {"B": B, "C": C, "H": H, "W": W, "n_T": n_T, "bytes": x.numel() * 4, "sweep": timed(one_sweep), "n_T_launches": timed(n_launches)}
        row["sweep_over_launches"] = round(row["sweep"]["median_us"] / row["n_T_launches"]["median_us"], 3)
        row["max_abs_diff"] = {k: float((sweep[k] - loop[k]).abs().max()) for k in sweep}
        assert int(status.item()) == 0
        print(json.dumps(row), flush=True)
        out.append(row)
    del x

if "--calibrate" in sys.argv[1:]:      # wall time of the drivers at section 4.8's C5 shape, from one process, synchronised
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import pandas as pd
    from conftest import Golden, build_model
    from oracle import ynet_oracle as O
    ev = importlib.import_module("motion-style-transfer_amd.utils.evaluate")
    cal = importlib.import_module("motion-style-transfer_amd.utils.calibrate")
    g = Golden("trained_short_full")
    cfg = g.cfg()
    model = build_model(cfg, g.state_dict(), dev)
    in_t = O.dist_template(cfg.template_size).to(dev)
    traj = g.t("traj").repeat(32 // g.t("traj").shape[0], 1, 1)
    loader = [(traj, [pd.DataFrame({"metaId": np.arange(traj.shape[0])})], "scene0")]
    images = {"scene0": g.t("scene")[0]}

    def wall(fn, reps=10, warm=3):
        for _ in range(warm):
            fn()
        ts = []
        for _ in range(reps):
            torch.cuda.synchronize(); t0 = time.perf_counter(); fn(); torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        return {"median_ms": round(statistics.median(ts), 3), "min_ms": round(min(ts), 3), "max_ms": round(max(ts), 3)}

    def two_evaluates():
        for T in (cfg.temperature, 2.0 * cfg.temperature):
            ev.evaluate(model, loader, images, dev, "sdd", None, in_t, list(cfg.waypoints), "test", 20, 1, cfg.obs_len, 32, cfg.resize_factor, T,
                        network=cfg.network, return_likelihood=True)

    def calibrate():
        return cal.calibrate_temperature(model, loader, images, dev, in_t, list(cfg.waypoints), cfg.obs_len, 32, cfg.resize_factor, cfg.temperature,
                                         network=cfg.network)

    import warnings
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        res = calibrate()
        row = {"shape": "B 32, 256 x 256, K 20", "calibrate_temperature_2_rounds_of_17": wall(calibrate), "two_evaluate_return_likelihood": wall(two_evaluates),
               "temperature": res["temperature"], "nll_before": res["nll_before"], "nll": res["nll"]}
    print(json.dumps(row), flush=True)
    out.append(row)
args = [a for a in sys.argv[1:] if a != "--calibrate"]
if args:          # optional: keep the rows in a JSON file
    with open(args[0], "w") as f:
        json.dump(out, f, indent=1)

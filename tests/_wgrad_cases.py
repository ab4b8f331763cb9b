"""The filter-gradient kernels at every plan edge: the case tables, the seeded inputs and the fp64 references (tests/test_wgrad_cases_host.py checks this
module and the plans on the CPU, tests/test_gpu_wgrad_edges.py runs ynet_conv2d_wgrad against it).

ynet_conv2d_wgrad dispatches among four kernel families (csrc/wgrad_mfma.hip), each with a plan of its own: the register-staged 4-row tiles (kernel 1: K 1, 3, 5,
any alignment), the LDS-DMA two-row tiles (2: their tile cursor), the rolling rows (3: strips cut into segments of 16 / 8 / 4 two-row steps) and the 1x1 streaming
kernel (4: a chunk walk across images); reduce_partials_kernel sums the `nsplit` partial slices of all of them.  ynet_conv2d_wgrad_plan tells what a call will
launch.  Every row below names the kernel it must plan and the plan values that make it the edge it is; EDGES maps every edge the sweep is about to a predicate
over (case, plan), and the host test asserts that each edge is hit by the rows that claim it and by nothing weaker -- removing a row fails there.

Inputs, two seeded families per case:
  "a": standard-normal x and dy (as _align_cases.ConvRef draws them); the mask is relu of a normal tensor with MASK_VALUES planted at fixed positions;
  "b": exact integers -- x and dy uniform in {-3 .. 3}, the mask drawn from MASK_VALUES: every product and partial sum is an integer below 2^24
       (9 B H W < 2^24, asserted), so fp32 arithmetic in ANY order is exact and the device must match the reference bit for bit.
The mask is an INPUT of ynet_conv2d_wgrad (the layer's post-ReLU activation), never computed by the device: no element needs excluding.

References: stock torch on .double() inputs on the CPU (dW and db of F.conv2d; x wants no gradient), dy replaced by where(mask > 0, dy, 0) -- never the code under test."""
import ctypes
import functools

import torch
import torch.nn.functional as F

import _align_cases as A

FLT_MIN = float(torch.finfo(torch.float32).tiny)           # 1.17549435e-38, the smallest normal: > 0, and not a denormal a flush could take
MASK_VALUES = [-1.0, -0.0, 0.0, FLT_MIN, 1.0, 2.0]         # (-0.0 and +0.0 both close the gate: the rule is mask > 0)
PLACEMENT = (0, 8)                                         # every operand: 16-byte aligned, 8 floats of NaN between images
OFF_4_BYTES = (1, 8)

# name: (B, H, W, sources, cout, K, masked, bias), the kernel ynet_conv2d_wgrad_plan must report, the plan values the row is there for, its edges (EDGES), options:
#   shared = i: source i is one image expanded along the batch with stride 0 (the scene map);  slice = i: source i is a channel slice of a wider tensor;
#   misplace = operand ("src0", "dy", "mask"): that operand lies 4 bytes off, so the call is not `aligned`
CASES = {
    # ---- rolling rows (kernel 3)
    "roll_two_steps": ((12, 4, 64, [130], 130, 3, True, True), 3, dict(tiles_y=2, seg=4, nseg_y=1, nsplit=20, nsegs=24), ["roll_tiles_y_2", "roll_fallback", "nw_above_grid_cap"], {}),
    "roll_nsegs_eq_nsplit": ((5, 10, 64, [130], 130, 3, True, False), 3, dict(seg=4, nseg_y=2, nsplit=20, nsegs=20), ["roll_nsegs_eq_nsplit", "roll_last_segment_one_step", "roll_fallback"], {}),
    "roll_one_column": ((12, 10, 32, [130], 130, 3, True, True), 3, dict(tiles_x=1, seg=4, nsplit=20, nsegs=24), ["roll_one_column"], {}),
    "roll_unmasked_85": ((16, 10, 96, [65], 65, 3, False, True), 3, dict(tiles_x=3, seg=4, nsplit=85, nsegs=96, co_blks=3, ci_blks=3),
                         ["roll_unmasked", "roll_interior_column", "roll_two_segments_some", "one_channel_block_tail", "nsplit_above_32_odd", "workspace_exact"], {}),
    "roll_seg_8": ((16, 18, 96, [130], 130, 3, False, True), 3, dict(seg=8, nseg_y=2, nsplit=30, nsegs=96), ["roll_seg_8", "roll_last_segment_one_step", "roll_unmasked", "workspace_exact", "nsplit_25_32"], {}),
    "roll_seg_16": ((16, 34, 96, [130], 130, 3, False, False), 3, dict(seg=16, nseg_y=2, nsplit=30, nsegs=96), ["roll_seg_16", "roll_last_segment_one_step"], {}),
    "roll_five_segments": ((12, 34, 96, [65], 65, 3, True, True), 3, dict(seg=4, nseg_y=5, nsplit=56, nsegs=180), ["roll_seg_4_by_three", "roll_last_segment_one_step"], {}),
    "roll_one_block_512": ((16, 128, 64, [6, 8], 32, 3, True, True), 3, dict(seg=4, nsplit=512, nsegs=512, co_blks=1, ci_blks=1), ["roll_nsplit_512", "shared_source", "sliced_source"], dict(shared=0, slice=1)),
    "roll_block_plus_one": ((16, 64, 64, [33], 17, 3, True, True), 3, dict(seg=4, nsplit=256, co_blks=1, ci_blks=2), ["one_channel_block_tail", "partial_channel_blocks"], {}),
    "roll_four_sources": ((4, 128, 64, [16, 16, 8, 2], 48, 3, True, False), 3, dict(seg=4, nsplit=128), ["four_sources", "sliced_source"], dict(slice=2)),
    "roll_unmasked_cat": ((6, 64, 64, [64, 33], 64, 3, False, True), 3, dict(seg=4, nsplit=96, nsegs=96), ["roll_unmasked", "roll_nsegs_eq_nsplit", "workspace_exact", "sliced_source"], dict(slice=1)),
    # (one channel block, unmasked: the 768 workgroups of the three-per-CU rule, each with one two-step segment -- the most partial slices any launch writes)
    "roll_unmasked_768": ((768, 4, 32, [5], 3, 3, False, True), 3, dict(seg=4, nseg_y=1, nsplit=768, nsegs=768), ["roll_nsplit_768", "roll_tiles_y_2", "workspace_exact"], {}),
    # ---- near misses of the rolling-row gates: each must plan the two-row tiles
    "miss_odd_h": ((12, 5, 64, [130], 130, 3, True, True), 2, dict(), ["miss_odd_h", "dma_odd_h"], {}),
    "miss_w_36": ((12, 4, 36, [130], 130, 3, True, True), 2, dict(), ["miss_w"], {}),
    "miss_too_few_segments": ((4, 64, 64, [64, 33], 64, 3, False, True), 2, dict(nsplit=64), ["miss_segments", "sliced_source"], dict(slice=1)),
    "miss_h_2": ((30, 2, 64, [130], 130, 3, True, True), 2, dict(tiles_y=1), ["miss_tiles_y"], {}),
    # ---- LDS-DMA two-row tiles (kernel 2); cursor = (step_x, step_y, step_b)
    "dma_cursor_y": ((7, 6, 36, [130], 130, 3, True, True), 2, dict(nsplit=20, ntiles=42, cursor=(0, 1, 3)), ["cursor_carry_y", "dma_ragged_right", "nsplit_9_24"], {}),
    "dma_odd_h_100": ((9, 5, 100, [130], 130, 3, False, True), 2, dict(nsplit=20, ntiles=108, cursor=(0, 2, 1)), ["dma_odd_h", "cursor_carry_y"], {}),
    "dma_both_carries": ((5, 7, 68, [65], 65, 3, True, False), 2, dict(nsplit=56, ntiles=60, cursor=(2, 2, 4)), ["cursor_carry_x", "dma_odd_h"], {}),
    "dma_images_only": ((30, 2, 32, [130], 130, 3, True, True), 2, dict(tiles_x=1, tiles_y=1, nsplit=20, cursor=(0, 0, 20)), ["cursor_images_only"], {}),
    "dma_w_4": ((25, 4, 4, [130], 130, 3, False, True), 2, dict(tiles_x=1, nsplit=20, cursor=(0, 0, 10)), ["dma_w_4"], {}),
    "dma_one_tile": ((1, 1, 4, [3], 5, 3, False, True), 2, dict(ntiles=1, nsplit=1), ["nsplit_1", "nw_not_multiple_of_32", "workspace_exact"], {}),
    "dma_nsplit_eq_tiles": ((3, 17, 36, [33], 17, 3, True, True), 2, dict(ntiles=54, nsplit=54), ["dma_nsplit_eq_tiles", "dma_odd_h", "partial_channel_blocks", "nsplit_above_32_odd"], {}),
    # ---- register-staged 4-row tiles (kernel 1)
    "staged_w_35": ((7, 9, 35, [130], 130, 3, True, True), 1, dict(nsplit=20, ntiles=42, rows=4), ["staged_w_not_4", "staged_row_tail", "staged_nsplit_below_tiles"], {}),
    "staged_smallest": ((1, 1, 1, [1], 1, 3, False, True), 1, dict(ntiles=1, nsplit=1), ["nsplit_1"], {}),
    "staged_33_65": ((2, 9, 7, [33], 65, 3, True, True), 1, dict(nsplit=6), ["partial_channel_blocks", "nsplit_2_7"], {}),
    "staged_65_33": ((5, 13, 66, [65], 33, 3, False, False), 1, dict(nsplit=60), ["staged_w_not_4"], {}),
    "staged_k5_13": ((4, 9, 13, [13], 33, 5, True, True), 1, dict(ci_blks=3, nsplit=12), ["k5_block_tail", "nsplit_9_24"], {}),
    "staged_k5_whole": ((6, 12, 34, [12], 6, 5, False, True), 1, dict(ci_blks=2, nsplit=36), ["k5_whole_blocks"], {}),
    "staged_k5_7_9": ((1, 7, 9, [7], 9, 5, True, False), 1, dict(ci_blks=2, nsplit=2), ["k5_block_tail", "nsplit_2_7"], {}),
    "staged_k1_hw_15": ((2, 3, 5, [32], 12, 1, False, True), 1, dict(), ["stream_refused_hw"], {}),
    "staged_k1_cout_33": ((2, 8, 8, [32], 33, 1, False, True), 1, dict(), ["stream_refused_cout"], {}),
    "staged_k1_masked": ((2, 8, 8, [31], 12, 1, True, True), 1, dict(), ["k1_masked"], {}),
    "staged_k1_two_sources": ((3, 8, 8, [16, 16], 12, 1, False, False), 1, dict(), ["stream_refused_sources", "sliced_source"], dict(slice=0)),
    "staged_k1_65": ((5, 9, 33, [65], 65, 1, True, True), 1, dict(nsplit=30), ["k1_masked", "nsplit_25_32"], {}),
    "staged_off_4_bytes": ((3, 8, 36, [33], 17, 3, True, True), 1, dict(rows=4), ["misaligned_takes_staged"], dict(misplace="dy")),
    # ---- 1x1 streaming (kernel 4); nsplit = its grid
    "stream_grid_1": ((2, 4, 4, [32], 16, 1, False, True), 4, dict(nsplit=1, ct=1), ["stream_ct_1_upper", "nsplit_1"], {}),
    "stream_one_chunk": ((1, 4, 4, [32], 17, 1, False, True), 4, dict(nsplit=1, ct=2), ["stream_ct_2_lower", "stream_idle_waves"], {}),
    "stream_grid_3": ((3, 4, 12, [32], 32, 1, False, False), 4, dict(nsplit=3, ct=2), ["stream_grid_shrink", "nsplit_2_7"], {}),
    "stream_cout_1": ((5, 12, 20, [32], 1, 1, False, True), 4, dict(nsplit=19, ct=1), ["stream_cout_1", "stream_grid_shrink", "nsplit_9_24"], {}),
    "stream_full_grid": ((12, 100, 36, [32], 30, 1, False, True), 4, dict(nsplit=512, ct=2), ["stream_full_grid_crossing"], {}),
}


def cursor(p):
    """(step_x, step_y, step_b) of wgrad_dma_kernel's tile cursor for a plan."""
    q = p["nsplit"] // p["tiles_x"]
    return p["nsplit"] % p["tiles_x"], q % p["tiles_y"], q // p["tiles_y"]


def cursor_carries(p):
    """Walk the cursor of every workgroup as the kernel does (mixed-radix adds with carries) -> (x carries, y carries, every tile visited exactly once)."""
    tx, ty, ns, nt = p["tiles_x"], p["tiles_y"], p["nsplit"], p["ntiles"]
    sx, sy, sb = cursor(p)
    ncx = ncy = 0
    seen = []
    for split in range(ns):
        x, y, b = split % tx, (split // tx) % ty, split // (tx * ty)
        for tile in range(split, nt, ns):
            seen.append((b * ty + y) * tx + x)
            if tile + ns < nt:
                x += sx
                cx = int(x >= tx)
                x -= cx * tx
                y += sy + cx
                cy = int(y >= ty)
                y -= cy * ty
                b += sb + cy
                ncx += cx
                ncy += cy
    return ncx, ncy, sorted(seen) == list(range(nt))


def _tail(tiles_y, seg):
    return tiles_y % seg == 1


# edge -> predicate over (shape, plan): True where the row reaches the edge
EDGES = {
    "roll_tiles_y_2": lambda s, p: p["kernel"] == 3 and p["tiles_y"] == 2,
    "roll_fallback": lambda s, p: p["kernel"] == 3 and p["seg"] == 4 and p["nsegs"] < 3 * p["nsplit"],
    "roll_nsegs_eq_nsplit": lambda s, p: p["kernel"] == 3 and p["nsegs"] == p["nsplit"],
    "roll_last_segment_one_step": lambda s, p: p["kernel"] == 3 and _tail(p["tiles_y"], p["seg"]),
    "roll_one_column": lambda s, p: p["kernel"] == 3 and p["tiles_x"] == 1,
    "roll_interior_column": lambda s, p: p["kernel"] == 3 and p["tiles_x"] >= 3,
    "roll_unmasked": lambda s, p: p["kernel"] == 3 and not s[6],
    "roll_two_segments_some": lambda s, p: p["kernel"] == 3 and p["nsplit"] < p["nsegs"] < 2 * p["nsplit"],
    "roll_seg_8": lambda s, p: p["kernel"] == 3 and p["seg"] == 8,
    "roll_seg_16": lambda s, p: p["kernel"] == 3 and p["seg"] == 16,
    "roll_seg_4_by_three": lambda s, p: p["kernel"] == 3 and p["seg"] == 4 and p["nsegs"] >= 3 * p["nsplit"] and p["nseg_y"] >= 5,
    "roll_nsplit_512": lambda s, p: p["kernel"] == 3 and p["nsplit"] == 512,
    "roll_nsplit_768": lambda s, p: p["kernel"] == 3 and p["nsplit"] == 768,
    "miss_odd_h": lambda s, p: p["kernel"] == 2 and s[1] % 2 == 1 and s[2] % 32 == 0 and s[1] >= 4,
    "miss_w": lambda s, p: p["kernel"] == 2 and s[2] % 32 != 0 and s[1] % 2 == 0 and s[1] >= 4 and s[2] > 32,
    "miss_segments": lambda s, p: p["kernel"] == 2 and s[2] % 32 == 0 and s[1] % 2 == 0 and s[1] >= 4,
    "miss_tiles_y": lambda s, p: p["kernel"] == 2 and s[2] % 32 == 0 and s[1] == 2 and s[0] * (s[2] // 32) >= p["nsplit"],
    "cursor_carry_x": lambda s, p: p["kernel"] == 2 and cursor(p)[0] > 0 and cursor_carries(p)[0] > 0,
    "cursor_carry_y": lambda s, p: p["kernel"] == 2 and cursor(p)[1] > 0 and cursor_carries(p)[1] > 0,
    "cursor_images_only": lambda s, p: p["kernel"] == 2 and p["tiles_x"] == p["tiles_y"] == 1 and p["nsplit"] < p["ntiles"],
    "dma_ragged_right": lambda s, p: p["kernel"] == 2 and s[2] % 32 != 0 and s[2] > 32,
    "dma_odd_h": lambda s, p: p["kernel"] == 2 and s[1] % 2 == 1 and s[1] > 1,
    "dma_w_4": lambda s, p: p["kernel"] == 2 and s[2] == 4,
    "dma_nsplit_eq_tiles": lambda s, p: p["kernel"] == 2 and p["nsplit"] == p["ntiles"] > 1,
    "staged_w_not_4": lambda s, p: p["kernel"] == 1 and s[5] == 3 and s[2] % 4 != 0,
    "staged_row_tail": lambda s, p: p["kernel"] == 1 and s[1] % 4 == 1 and s[1] > 4,
    "staged_nsplit_below_tiles": lambda s, p: p["kernel"] == 1 and p["nsplit"] < p["ntiles"],
    "k5_block_tail": lambda s, p: p["kernel"] == 1 and s[5] == 5 and sum(s[3]) % 6 == 1,
    "k5_whole_blocks": lambda s, p: p["kernel"] == 1 and s[5] == 5 and sum(s[3]) % 6 == 0,
    "k1_masked": lambda s, p: p["kernel"] == 1 and s[5] == 1 and s[6],
    "stream_refused_hw": lambda s, p: p["kernel"] == 1 and s[5] == 1 and s[3] == [32] and s[4] <= 32 and not s[6] and (s[1] * s[2]) % 16 != 0,
    "stream_refused_cout": lambda s, p: p["kernel"] == 1 and s[5] == 1 and s[3] == [32] and s[4] == 33 and not s[6] and (s[1] * s[2]) % 16 == 0,
    "stream_refused_sources": lambda s, p: p["kernel"] == 1 and s[5] == 1 and sum(s[3]) == 32 and len(s[3]) == 2 and s[4] <= 32 and not s[6] and (s[1] * s[2]) % 16 == 0,
    "misaligned_takes_staged": lambda s, p: p["kernel"] == 1 and s[5] == 3 and s[2] % 4 == 0,
    "stream_ct_1_upper": lambda s, p: p["kernel"] == 4 and p["ct"] == 1 and s[4] == 16,
    "stream_ct_2_lower": lambda s, p: p["kernel"] == 4 and p["ct"] == 2 and s[4] == 17,
    "stream_idle_waves": lambda s, p: p["kernel"] == 4 and s[0] * (s[1] * s[2] // 16) == 1,
    "stream_grid_shrink": lambda s, p: p["kernel"] == 4 and 1 < p["nsplit"] < 512,
    "stream_cout_1": lambda s, p: p["kernel"] == 4 and s[4] == 1,
    # (full grid: the stride of 2048 chunks is no multiple of the hw16 chunks of an image, and every workgroup takes more than one chunk)
    "stream_full_grid_crossing": lambda s, p: p["kernel"] == 4 and p["nsplit"] == 512 and 2048 % (s[1] * s[2] // 16) != 0 and s[0] * (s[1] * s[2] // 16) > 2048,
    "one_channel_block_tail": lambda s, p: p["kernel"] in (2, 3) and (sum(s[3]) % 32 == 1 or s[4] % 32 == 1),
    "partial_channel_blocks": lambda s, p: sum(s[3]) % 32 != 0 and s[4] % 32 != 0 and sum(s[3]) > 32,
    "four_sources": lambda s, p: len(s[3]) == 4 and sum(1 for i in range(1, 4) if sum(s[3][:i]) % 32 != 0) >= 2,
    "shared_source": lambda s, p: len(s[3]) > 1,
    "sliced_source": lambda s, p: len(s[3]) > 1,
    # reduce_partials_kernel: its split loop runs unrolled by 32 while s + 24 < nsplit, then by 8
    "nsplit_1": lambda s, p: p["nsplit"] == 1,
    "nsplit_2_7": lambda s, p: 2 <= p["nsplit"] <= 7,
    "nsplit_9_24": lambda s, p: 9 <= p["nsplit"] <= 24,
    "nsplit_25_32": lambda s, p: 25 <= p["nsplit"] <= 32,
    "nsplit_above_32_odd": lambda s, p: p["nsplit"] > 32 and p["nsplit"] % 32 != 0,
    "nw_above_grid_cap": lambda s, p: s[4] * sum(s[3]) * s[5] ** 2 > 131072,
    "nw_not_multiple_of_32": lambda s, p: (s[4] * sum(s[3]) * s[5] ** 2) % 32 != 0 and p["nsplit"] == 1,
    "workspace_exact": lambda s, p: p["partial_floats"] == p["workspace_floats"],
}
# edges that are an option of the row (how the GPU test builds its buffers) on top of the predicate
OPTION_EDGES = {"shared_source": "shared", "sliced_source": "slice", "misaligned_takes_staged": "misplace"}
# rows per kernel: removing a row fails the host test even where another row reaches the same edges
ROWS_PER_KERNEL = {1: 13, 2: 11, 3: 12, 4: 5}


def shape_of(name):
    return CASES[name][0]


def aligned_of(name):
    return 0 if CASES[name][4].get("misplace") else 1


def plan(lib, L, B, H, W, cs, cout, K, masked, aligned=1, want_bias=1):
    """ynet_conv2d_wgrad_plan as a dict (+ cin's workspace_floats): host code, no device."""
    p = L.WgradPlan()
    arr = (ctypes.c_int * len(cs))(*cs)
    rc = lib.ynet_conv2d_wgrad_plan(B, H, W, cout, arr, len(cs), K, int(bool(masked)), int(aligned), int(bool(want_bias)), ctypes.byref(p))
    assert rc == 0, lib.ynet_last_error()
    d = {n: getattr(p, n) for n, _ in L.WgradPlan._fields_}
    d["workspace_floats"] = lib.ynet_conv2d_wgrad_workspace_floats(B, H, W, cout, sum(cs), K)
    return d


def case_plan(lib, L, name, want_bias=None):
    B, H, W, cs, cout, K, masked, bias = shape_of(name)
    return plan(lib, L, B, H, W, cs, cout, K, masked, aligned_of(name), bias if want_bias is None else want_bias)


# ------------------------------------------------------------------------------------------------ inputs
def _ints(*shape, key):
    return torch.randint(-3, 4, shape, generator=A._gen(key, *shape)).float()


def _planted_positions(B, C, H, W):
    """Fixed mask positions (b, c, y, x): the first and last pixel of the first and last image, and the corners of the 32-column / 2- and 4-row tiles."""
    pos = []
    for b in sorted({0, B - 1}):
        for c in sorted({0, C - 1}):
            ys = sorted({y for y in (0, 1, 2, 3, 4, H - 2, H - 1) if 0 <= y < H})
            xs = sorted({x for x in (0, 3, 4, 31, 32, W - 33, W - 32, W - 1) if 0 <= x < W})
            pos += [(b, c, y, x) for y in ys for x in xs]
    return pos


def make_mask(B, C, H, W, family):
    if family == "b":
        idx = torch.randint(0, len(MASK_VALUES), (B, C, H, W), generator=A._gen(31, B, C, H, W))
        return torch.tensor(MASK_VALUES, dtype=torch.float32)[idx]
    m = torch.relu(A.randn(B, C, H, W, key=30))
    for i, (b, c, y, x) in enumerate(_planted_positions(B, C, H, W)):
        m[b, c, y, x] = MASK_VALUES[i % len(MASK_VALUES)]
    return m


class WgradInputs:
    """xs (source i of a `shared` row: one image, [1, c, H, W]), dy, mask (or None) of a case and family, fp32 on the CPU."""

    def __init__(self, name, family):
        (B, H, W, cs, cout, K, masked, bias), _, _, _, opts = CASES[name]
        draw = (lambda *s, key: A.randn(*s, key=key)) if family == "a" else _ints
        shared = opts.get("shared")
        self.xs = [draw(1 if i == shared else B, c, H, W, key=(20, i)) for i, c in enumerate(cs)]
        self.dy = draw(B, cout, H, W, key=(21,))
        self.mask = make_mask(B, cout, H, W, family) if masked else None
        self.shared = shared


@functools.lru_cache(maxsize=None)
def inputs(name, family):
    return WgradInputs(name, family)


def reference(inp, K, dtype=torch.float64):
    """(dW, db) of conv(cat(xs), w) for the output gradient where(mask > 0, dy, 0): stock autograd in `dtype` on the CPU."""
    B = inp.dy.shape[0]
    x = torch.cat([(t.expand(B, -1, -1, -1) if t.shape[0] != B else t) for t in inp.xs], 1).to(dtype)
    g = inp.dy if inp.mask is None else torch.where(inp.mask > 0, inp.dy, torch.zeros(()))
    cout, cin = g.shape[1], x.shape[1]
    w = torch.zeros(cout, cin, K, K, dtype=dtype, requires_grad=True)      # (linear in w and b: their values do not enter dW, db)
    b = torch.zeros(cout, dtype=dtype, requires_grad=True)
    F.conv2d(x, w, b, padding=K // 2).backward(g.to(dtype))
    return w.grad, b.grad


@functools.lru_cache(maxsize=None)
def ref64(name, family):
    return reference(inputs(name, family), shape_of(name)[5])

"""The Winograd convolution kernels at every plan edge: the case table, the seeded inputs and the fp64 references (tests/test_wino_cases_host.py checks this module
and the plans on the CPU, tests/test_gpu_wino_edges.py runs the kernels against it).

csrc/conv_wino.hip has five convolution kernels -- conv_wino_kernel (one source, all filters resident), conv_wino_cat_kernel (up to three concatenated sources, chunks
of four channels), conv_wino16_kernel (the slice form: 16 output channels per workgroup), conv_wino_up_kernel / conv_wino16_up_kernel (bilinear x2 inside) -- and
wino_filter_kernel, which transforms the filters of all of them; make_plan (csrc/conv_auto.cpp) dispatches to them.  YNET_WINOGRAD_MIN / YNET_WINOGRAD16_MIN are read
once per process, so no row lowers a size gate: every row sits AT its gate (B H W >= 131072, the slice forms 40960), the smallest launch the product can make.

Every row names the (family, variant, launches) ynet_conv2d_auto must take and the edges it is there for; EDGES recomputes every edge from the kernels' own formulas
(the em of every row pair, the chunk counts, the slices, the XCD walk with the 256 CUs of the MI355X) and the host test asserts that every claim is reached, that every
edge of EDGES is claimed and that the three row stagers each meet every em value a tile can have.

Inputs, two seeded families per row:
  "a": normal data scaled as _align_cases.ConvRef scales it (filter 1 / sqrt(9 cin), bias 0.1); post-ReLU where the operand is an activation (relu_of, an up-convolution's input);
  "b": exact integers -- x in [-3, 3], filter in [-2, 2], bias, addend and dy in [-4, 4], activations in {0 .. 3}.  F(2x2, 3x3) on them is exact in fp32: the filter
       transform halves and quarters, the bilinear weights are quarters in both directions, so every value the kernels hold is a multiple of 1 / 64 and every partial sum stays
       below 2^24 such units (asserted per row).  The device must match the reference bit for bit, zeros, ties of the pool code and ReLU gates included.

References: stock torch on .double() inputs on the CPU, cached per (row, family) -- never the code under test."""
import ctypes
import functools
import zlib

import torch
import torch.nn.functional as F

import _align_cases as A

NO_W16, FOR_16 = 2, 4                 # YNET_AUTO_NO_WINOGRAD16, YNET_AUTO_WINOGRAD16_FOR_16 (include/ynet_hip.h)
GATE, GATE16 = 128 * 128 * 8, 64 * 64 * 10
CUS = 256                             # the compute units of the MI355X: what the launches size their grids by
PAD = 8                               # floats of NaN between the images of every operand (keeps the 16-byte gates)
LEAD, TRAIL = 4, 1                    # NaN planes around a sliced source (4 planes of a map with H W % 4 == 0 keep the slice on a 16-byte boundary)
UNWANTED = 16                         # channels of a destination nobody wants (a way-point map's gradient)

# name: (entry, B, H, W, source channels, destination channels (None: unwanted), relu, bias, packing mode, operands, expected (family, variant, launches), edges)
#   entry     "auto": ynet_conv2d_auto with a fresh cache and tag;  "cat": ynet_winograd_filter_cat + ynet_conv2d_winograd_cat called directly
#   mode      0 a forward convolution, 1 a data gradient (the sources are dy, the destinations dx of the concatenated inputs)
#   operands  relu_of / pooled / pool_code / words (wbits_out, then a 32 -> 32 data gradient gated by relu_wbits) / addend: modulus / s2d: flags per destination /
#             up (upsample2x: H, W are the up-sampled size) / flags / shared: i (source i is one image, batch stride 0) / slice: i (source i is a channel slice of a wider
#             NaN tensor) / dst_in: (first channel, channels) of the wider NaN tensor the destination is a slice of
R, NR = True, False
CASES = {
    # ---- conv_wino_kernel: tile geometry
    "wino_single_tiles_256": ("auto", 256, 16, 32, [32], [32], R, True, 0, {}, (1, 21, 1), ["wino_single_tile_image", "wino_one_tile_per_workgroup"]),
    "wino_257_tiles": ("auto", 257, 16, 32, [32], [32], R, True, 0, {}, (1, 21, 1), ["wino_tiles_not_multiple_of_8", "wino_short_xcd", "wino_idle_workgroups", "wino_two_tiles_in_a_workgroup"]),
    "wino_one_column": ("auto", 16, 256, 32, [16], [16], R, True, 0, {}, (1, 21, 1), ["wino_one_tile_wide"]),
    "wino_one_tile_row": ("auto", 8, 16, 1024, [32], [16], R, False, 0, {}, (1, 21, 1), ["wino_one_tile_high"]),
    "wino_3x3_tiles": ("auto", 29, 48, 96, [32], [32], NR, True, 0, {}, (1, 21, 1), ["wino_interior_tile_3x3", "wino_tiles_not_multiple_of_8"]),
    "wino_mode1_16_32": ("auto", 8, 128, 128, [16], [32], NR, False, 1, {}, (1, 21, 1), ["wino_mode_1"]),
    "wino_dst_slice": ("auto", 8, 128, 128, [32], [16], R, True, 0, {"dst_in": (8, 24)}, (1, 21, 1), ["dst_slice"]),
    # ---- data gradients
    "dgrad_split48": ("auto", 256, 16, 32, [32], [16, 32], NR, False, 1, {}, (1, 23, 1), ["split48", "wino_single_tile_image"]),
    "dgrad_split48_s2d": ("auto", 256, 16, 32, [32], [16, 32], NR, False, 1, {"s2d": [1, 0]}, (1, 23, 1), ["split48_s2d"]),
    "dgrad_pieces_unwanted": ("auto", 8, 128, 128, [32], [32, 16, None], NR, False, 1, {}, (1, 21, 2), ["unwanted_destination", "two_pieces"]),
    "dgrad_s2d_16": ("auto", 8, 128, 128, [32], [16, None], NR, False, 1, {"s2d": [1, 0]}, (1, 21, 1), ["s2d_16", "unwanted_destination"]),
    "dgrad_relu_of": ("auto", 256, 16, 32, [32], [32], NR, False, 1, {"relu_of": True}, (1, 21, 1), ["wino_relu_of", "wino_single_tile_image"]),
    "fwd_words": ("auto", 256, 16, 32, [32], [32], R, True, 0, {"words": True}, (1, 21, 1), ["wino_words", "wino_single_tile_image"]),
    "dgrad_16_64_slice_form": ("auto", 8, 128, 128, [16], [64], NR, False, 1, {}, (3, 22, 1), ["w16_at_128"]),
    "dgrad_16_64_two_launches": ("auto", 8, 128, 128, [16], [64], NR, False, 1, {"flags": NO_W16}, (1, 21, 2), ["wide_as_two_launches"]),
    # ---- conv_wino_cat_kernel
    "cat_1_1": ("auto", 8, 128, 128, [1, 1], [32], R, True, 0, {}, (2, 41, 1), ["cat_nch_2", "cat_one_valid_plane"]),
    "cat_1_1_1": ("auto", 8, 128, 128, [1, 1, 1], [32], R, True, 0, {"slice": 1}, (2, 41, 1), ["cat_nch_3", "cat_one_valid_plane", "sliced_source"]),
    "cat_20_20_16": ("auto", 8, 128, 128, [20, 20, 16], [32], R, True, 0, {}, (2, 41, 1), ["cat_nch_14"]),
    "cat_21_27_2": ("auto", 8, 128, 128, [21, 27, 2], [32], NR, True, 0, {"slice": 0}, (2, 41, 1), ["cat_nch_14", "cat_every_source_ragged", "sliced_source"]),
    "cat_single_5": ("auto", 8, 128, 128, [5], [32], R, True, 0, {"flags": NO_W16}, (2, 41, 1), ["cat_single_source", "cat_nch_2"]),
    "cat_single_56": ("auto", 8, 128, 128, [56], [32], R, False, 0, {"flags": NO_W16}, (2, 41, 1), ["cat_single_source", "cat_nch_14"]),
    "cat_direct_single_8": ("cat", 8, 128, 128, [8], [32], R, True, 0, {}, None, ["cat_direct_entry", "cat_nch_2"]),
    "cat40_32_28": ("auto", 8, 128, 128, [32, 28], [32], R, True, 0, {}, (2, 40, 2), ["variant_40_low_end"]),
    "cat40_56_1": ("auto", 8, 128, 128, [56, 1], [32], R, True, 0, {"slice": 1}, (2, 40, 2), ["variant_40_two_rest_sources", "sliced_source"]),
    "cat40_88": ("auto", 8, 128, 128, [88], [32], NR, True, 0, {}, (2, 40, 2), ["variant_40_high_end"]),
    # (the second launch of variants 40 / 43 adds onto the first one's output IN PLACE: a tile visited twice would be added twice -- with a tile count the walk does not fill)
    "cat40_257_tiles": ("auto", 257, 16, 32, [56, 1], [32], R, True, 0, {}, (2, 40, 2), ["in_place_addend_short_xcd", "cat_tiles_not_multiple_of_8"]),
    "cat_single_tiles": ("auto", 256, 16, 32, [32, 16, 1], [32], R, True, 0, {}, (2, 41, 1), ["cat_single_tile_image"]),
    "cat_3x3_tiles": ("auto", 29, 48, 96, [32, 16, 1], [32], R, True, 0, {"slice": 1}, (2, 41, 1), ["cat_interior_tile_3x3", "cat_tiles_not_multiple_of_8", "cat_short_xcd", "cat_idle_workgroups", "sliced_source"]),
    "cat_pool_code": ("auto", 16, 256, 32, [6, 8], [32], R, True, 0, {"pooled": True, "pool_code": True, "shared": 0}, (2, 10, 1),
                      ["pool_code", "cat_pooled", "cat_one_tile_wide", "shared_source_slot_0"]),
    "cat_addend_mod3": ("auto", 256, 16, 32, [1, 1], [32], R, True, 0, {"addend": 3}, (2, 30, 1), ["cat_addend", "addend_modulus_not_dividing_B", "cat_single_tile_image"]),
    "cat_shared_slot1": ("auto", 8, 128, 128, [16, 6, 8], [32], R, True, 0, {"shared": 1}, (2, 41, 1), ["shared_source_slot_1"]),
    "cat_shared_slot2": ("auto", 8, 16, 1024, [32, 16, 1], [32], R, True, 0, {"shared": 2}, (2, 41, 1), ["shared_source_slot_2", "cat_one_tile_high"]),
    "cat_words_41": ("auto", 8, 128, 128, [32, 16, 1], [32], R, True, 0, {"words": True}, (2, 41, 1), ["cat_words_41"]),
    "cat_words_40": ("auto", 8, 128, 128, [56, 1], [32], R, True, 0, {"words": True}, (2, 40, 2), ["cat_words_40"]),
    # ---- conv_wino16_kernel (the slice form)
    "w16_64_128": ("auto", 10, 64, 64, [64], [128], R, True, 0, {}, (3, 22, 1), ["w16_eight_slices"]),
    "w16_84_64": ("auto", 10, 64, 64, [84], [64], R, True, 0, {}, (3, 22, 1), ["w16_nch_21"]),
    "w16_5_16": ("auto", 10, 64, 64, [5], [16], R, True, 0, {}, (3, 22, 1), ["w16_nch_2", "w16_one_slice"]),
    "w16_41_tiles": ("auto", 41, 32, 32, [64], [64], R, True, 0, {}, (3, 22, 1), ["w16_tiles_not_multiple_of_8", "w16_short_xcd", "w16_empty_xcd", "w16_idle_workgroups", "w16_single_tile_image"]),
    "w16_43_41_tiles": ("auto", 41, 32, 32, [32, 64, 1], [64], R, True, 0, {}, (3, 43, 2), ["in_place_addend_short_xcd", "w16_empty_xcd"]),
    "w16_cat_single_tiles": ("auto", 40, 32, 32, [32, 64, 1], [64], R, True, 0, {"slice": 2}, (3, 43, 2), ["w16_single_tile_image", "variant_43_cut_1", "sliced_source"]),
    "w16_one_column": ("auto", 5, 256, 32, [64], [64], R, True, 0, {}, (3, 22, 1), ["w16_one_tile_wide"]),
    "w16_one_tile_row": ("auto", 2, 32, 640, [64], [32], NR, True, 0, {}, (3, 22, 1), ["w16_one_tile_high"]),
    "w16_3x3_tiles": ("auto", 5, 96, 96, [64], [64], R, True, 0, {}, (3, 22, 1), ["w16_interior_tile_3x3", "w16_tiles_not_multiple_of_8"]),
    "w16_43_row0_30": ("auto", 10, 64, 64, [30, 63, 1], [64], R, True, 0, {"slice": 1}, (3, 43, 2), ["variant_43_cut_1", "variant_43_ragged_row0", "sliced_source"]),
    "w16_43_cut_2": ("auto", 10, 64, 64, [4, 80, 84], [64], R, True, 0, {}, (3, 43, 2), ["variant_43_cut_2"]),
    "w16_43_at_128": ("auto", 8, 128, 128, [33, 3, 52], [32], R, True, 0, {}, (3, 43, 2), ["variant_43_ragged_row0", "w16_at_128"]),
    "w16_43_128_outputs": ("auto", 10, 64, 64, [64, 64, 1], [128], R, True, 0, {}, (3, 43, 2), ["variant_43_128_outputs", "w16_eight_slices"]),
    "w16_dgrad_32_64": ("auto", 10, 64, 64, [64], [32, 64], NR, False, 1, {}, (3, 22, 2), ["w16_two_destinations"]),
    "w16_relu_of_128": ("auto", 10, 64, 64, [64], [128], NR, False, 1, {"relu_of": True}, (3, 22, 1), ["w16_relu_of", "w16_eight_slices"]),
    "w16_addend_mod4": ("auto", 10, 64, 64, [64, 1], [128], R, True, 0, {"addend": 4}, (3, 31, 1), ["w16_addend", "addend_modulus_not_dividing_B", "w16_eight_slices"]),
    "w16_pooled": ("auto", 10, 64, 64, [5], [16], R, True, 0, {"pooled": True}, (3, 11, 1), ["w16_pooled", "w16_nch_2"]),
    "w16_for_16": ("auto", 10, 64, 64, [32], [16], R, True, 0, {"flags": FOR_16}, (3, 20, 1), ["w16_for_16", "w16_one_slice"]),
    # ---- the up-convolutions (H, W: the up-sampled size)
    "up_single_tiles": ("auto", 256, 16, 32, [32], [16], NR, True, 0, {"up": True}, (4, 0, 1), ["up_single_tile_image"]),
    "up_one_column": ("auto", 16, 256, 32, [32], [16], R, True, 0, {"up": True}, (4, 0, 1), ["up_one_tile_wide"]),
    "up_3x3_tiles": ("auto", 29, 48, 96, [32], [16], NR, True, 0, {"up": True}, (4, 0, 1), ["up_interior_tile_3x3"]),
    "up_shared_input": ("auto", 8, 128, 128, [32], [16], NR, False, 0, {"up": True, "shared": 0}, (4, 0, 1), ["up_shared_input"]),
    "up16_8_64": ("auto", 40, 32, 32, [8], [64], NR, True, 0, {"up": True}, (5, 0, 1), ["up16_cin_8", "up16_single_tile_image"]),
    "up16_84_16": ("auto", 5, 96, 96, [84], [16], R, True, 0, {"up": True}, (5, 0, 1), ["up16_cin_84", "up16_interior_tile_3x3"]),
    "up16_one_column": ("auto", 5, 256, 32, [64], [32], NR, True, 0, {"up": True}, (5, 0, 1), ["up16_one_tile_wide"]),
}
# rows that are NOT at their gate (one image fewer is still served): the tile counts the XCD walk does not fill, and the slice form at the 128^2 shapes the issue
# gives it (at the gate of conv_wino_kernel, which the same descriptors take under YNET_AUTO_NO_WINOGRAD16)
ABOVE_GATE = {"wino_257_tiles", "w16_41_tiles", "cat40_257_tiles", "w16_43_41_tiles", "dgrad_16_64_slice_form", "w16_43_at_128"}
# host only: what the dispatcher must refuse to the Winograd families.  name: (B, H, W, sources, destinations, up) -> family 0, or the word its error names
REFUSALS = {
    "cat_89": ((8, 128, 128, [89], [32], False), 0),
    "w16_85": ((10, 64, 64, [85], [64], False), 0),
    "up_88_64": ((10, 64, 64, [88], [64], True), b"upsample2x"),
}


def case(name):
    entry, B, H, W, cs, couts, relu, bias, mode, opts, plan, edges = CASES[name]
    return dict(entry=entry, B=B, H=H, W=W, cs=cs, couts=couts, relu=relu, bias=bias, mode=mode, opts=opts, plan=plan, edges=edges,
                sizes=[c if c is not None else UNWANTED for c in couts], up=bool(opts.get("up")))


# ------------------------------------------------------------------------------------------------ the launches of a row, from the kernels' own formulas
def padded(cs):
    return sum((c + 3) & ~3 for c in cs)


def launches(name):
    """[(kernel, source channels, output channels)] of the row's plan: kernel in "wino", "cat", "w16", "up", "up16" (run_plan of csrc/conv_auto.cpp)."""
    c = case(name)
    cs, sizes = c["cs"], c["sizes"]
    wanted = [n for n, w in zip(sizes, c["couts"]) if w is not None]
    if c["entry"] == "cat":
        return [("cat", cs, 32)]
    fam, var, n = c["plan"]
    if fam in (4, 5):
        return [("up" if fam == 4 else "up16", cs, sizes[0])]
    if fam == 1:
        if var == 23:
            return [("wino", cs, 48)]
        pieces = [p for w in wanted for p in ([32] * (w // 32) + [16] * (w % 32 // 16))]
        return [("wino", cs, p) for p in pieces]
    if fam == 2:
        if var == 40:
            rest = ([cs[0] - 32] if cs[0] > 32 else []) + cs[1:]
            return [("wino", [32], 32), ("cat", rest, 32)]
        return [("cat", cs, 32)]
    if var == 43:
        cut = cut_of(cs, sum(sizes))
        return [("w16", cs[:cut], sum(sizes)), ("w16", cs[cut:], sum(sizes))]
    if var in (20, 22):
        return [("w16", cs, w) for w in wanted]
    return [("w16", cs, sum(sizes))]


def w16_serves(cs, cout):
    return 1 <= len(cs) <= 3 and cout in (16, 32, 64, 128) and 2 <= padded(cs) // 4 <= 21


def cut_of(cs, cout):
    """Variant 43's cut: the first split of the sources into two slice-form launches (make_plan's loop)."""
    for cut in range(1, len(cs)):
        if w16_serves(cs[:cut], cout) and w16_serves(cs[cut:], cout):
            return cut
    return None


def em_values(kernel, H, W):
    """The edge masks the row pairs of a launch take: 1 top | 2 bottom | 4 left | 8 right, per unit (2 output rows; 4 for the slice form; one low-resolution row
    for conv_wino_up_kernel, two for conv_wino16_up_kernel)."""
    if kernel in ("up", "up16"):
        Hl, Wl, r = H // 2, W // 2, (1 if kernel == "up" else 2)
        ys = {(1 if i == 0 else 0) | (2 if i + r == Hl else 0) for i in range(0, Hl, r)}
        xs = {(4 if j == 0 else 0) | (8 if j + 16 == Wl else 0) for j in range(0, Wl, 16)}
    else:
        r = 4 if kernel == "w16" else 2
        ys = {(1 if y == 0 else 0) | (2 if y + r == H else 0) for y in range(0, H, r)}
        xs = {(4 if x == 0 else 0) | (8 if x + 32 == W else 0) for x in range(0, W, 32)}
    return {y | x for y in ys for x in xs}


def walk(kernel, B, H, W, cout):
    """The XCD walk of a launch on CUS compute units -> dict(ntiles, grid, per_xcd, short (an XCD with fewer tiles than per_xcd), empty (an XCD with none), idle (workgroups with
    tile_first >= tile_end), most / least (tiles of a working workgroup), once (every tile visited exactly once per slice))."""
    th = 32 if kernel in ("w16", "up16") else 16
    ntiles = B * (H // th) * (W // 32)
    per_xcd = (ntiles + 7) // 8
    seen, counts, idle = [], [], 0
    if kernel in ("w16", "up16"):
        ns = cout // 16
        team = max(1, min((CUS // 8) // ns, per_xcd))
        grid, g8 = 8 * ns * team, ns * team
        for blk in range(grid):
            xcd, idx = blk & 7, blk >> 3
            first, end = xcd * per_xcd + idx // ns, min(ntiles, (xcd + 1) * per_xcd)
            mine = list(range(first, end, g8 // ns))
            idle += not mine
            if mine:
                counts.append(len(mine))
            if idx % ns == 0:
                seen += mine
    else:
        grid = min(ntiles, CUS)
        if grid >= 8:
            grid &= ~7
        xw = grid % 8 == 0 and ntiles >= grid
        for blk in range(grid):
            xcd = blk & 7
            first, end, stride = (xcd * per_xcd + (blk >> 3), min(ntiles, (xcd + 1) * per_xcd), grid >> 3) if xw else (blk, ntiles, grid)
            mine = list(range(first, end, stride))
            idle += not mine
            if mine:
                counts.append(len(mine))
            seen += mine
    sizes = [max(0, min(ntiles, (x + 1) * per_xcd) - x * per_xcd) for x in range(8)]
    return dict(ntiles=ntiles, grid=grid, per_xcd=per_xcd, short=any(0 < s < per_xcd for s in sizes), empty=any(s == 0 for s in sizes), idle=idle,
                most=max(counts), least=min(counts), once=sorted(seen) == list(range(ntiles)))


def _geometry(prefix, kernel, th):
    """The edges every stager shares, for one kernel."""
    def of(name):
        c = case(name)
        return [(k, cs, co) for k, cs, co in launches(name) if k == kernel], c
    def any_launch(pred):
        def f(name):
            ls, c = of(name)
            return any(pred(c, walk(k, c["B"], c["H"], c["W"], co), cs, co) for k, cs, co in ls)
        return f
    return {
        prefix + "_one_tile_wide": any_launch(lambda c, w, cs, co: c["W"] == 32 and c["H"] > th),
        prefix + "_single_tile_image": any_launch(lambda c, w, cs, co: c["W"] == 32 and c["H"] == th),
        prefix + "_one_tile_high": any_launch(lambda c, w, cs, co: c["H"] == th and c["W"] > 32),
        prefix + "_interior_tile_3x3": any_launch(lambda c, w, cs, co: c["H"] == 3 * th and c["W"] == 96 and 0 in em_values(kernel, c["H"], c["W"])),
        prefix + "_tiles_not_multiple_of_8": any_launch(lambda c, w, cs, co: w["ntiles"] % 8 != 0),
        prefix + "_short_xcd": any_launch(lambda c, w, cs, co: w["short"]),
        prefix + "_idle_workgroups": any_launch(lambda c, w, cs, co: w["idle"] > 0),
    }


def _opt(key, fam=None, value=None):
    def f(name):
        c = case(name)
        ok = key in c["opts"] and (value is None or c["opts"][key] == value)
        return ok and (fam is None or (c["plan"] is not None and c["plan"][0] == fam))
    return f


def _nch(kernel, n):
    return lambda name: any(k == kernel and padded(cs) // 4 == n for k, cs, co in launches(name))


def _variant(v, pred=lambda c: True):
    return lambda name: case(name)["plan"] is not None and case(name)["plan"][1] == v and pred(case(name))


# edge -> predicate over the row's name: True where the row's shape reaches it
EDGES = {
    **_geometry("wino", "wino", 16), **_geometry("cat", "cat", 16), **_geometry("w16", "w16", 32),
    "wino_one_tile_per_workgroup": lambda n: any(k == "wino" and walk(k, case(n)["B"], case(n)["H"], case(n)["W"], co)["ntiles"] == CUS for k, cs, co in launches(n)),
    "wino_two_tiles_in_a_workgroup": lambda n: any(k == "wino" and (lambda w: w["most"] == 2 and w["least"] == 1 and w["idle"] > 0)(walk(k, case(n)["B"], case(n)["H"], case(n)["W"], co))
                                                   for k, cs, co in launches(n)),
    "w16_empty_xcd": lambda n: any(k == "w16" and walk(k, case(n)["B"], case(n)["H"], case(n)["W"], co)["empty"] for k, cs, co in launches(n)),
    "w16_eight_slices": lambda n: any(k == "w16" and co == 128 for k, cs, co in launches(n)),
    "w16_one_slice": lambda n: any(k == "w16" and co == 16 for k, cs, co in launches(n)),
    "w16_at_128": lambda n: any(k == "w16" for k, cs, co in launches(n)) and case(n)["H"] == 128,
    "w16_two_destinations": lambda n: [k for k, cs, co in launches(n)] == ["w16", "w16"] and case(n)["plan"][1] == 22,
    "wino_mode_1": lambda n: case(n)["mode"] == 1 and case(n)["plan"] == (1, 21, 1) and not case(n)["opts"],
    "cat_nch_2": _nch("cat", 2), "cat_nch_3": _nch("cat", 3), "cat_nch_14": _nch("cat", 14), "w16_nch_2": _nch("w16", 2), "w16_nch_21": _nch("w16", 21),
    "cat_one_valid_plane": lambda n: any(k == "cat" and all(c == 1 for c in cs) for k, cs, co in launches(n)),
    "cat_every_source_ragged": lambda n: any(k == "cat" and len(cs) == 3 and all(c % 4 for c in cs) for k, cs, co in launches(n)),
    "cat_single_source": lambda n: case(n)["entry"] == "auto" and [(k, len(cs)) for k, cs, co in launches(n)] == [("cat", 1)],
    "cat_direct_entry": lambda n: case(n)["entry"] == "cat" and len(case(n)["cs"]) == 1,
    "variant_40_low_end": _variant(40, lambda c: padded(c["cs"]) == 60),
    "variant_40_high_end": _variant(40, lambda c: padded(c["cs"]) == 88),
    "variant_40_two_rest_sources": _variant(40, lambda c: c["cs"][0] > 32 and len(c["cs"]) == 2),
    "variant_43_cut_1": _variant(43, lambda c: cut_of(c["cs"], sum(c["sizes"])) == 1),
    "variant_43_cut_2": _variant(43, lambda c: cut_of(c["cs"], sum(c["sizes"])) == 2),
    "variant_43_ragged_row0": _variant(43, lambda c: sum(c["cs"][:cut_of(c["cs"], sum(c["sizes"]))]) % 4 != 0),
    "variant_43_128_outputs": _variant(43, lambda c: sum(c["sizes"]) == 128),
    "in_place_addend_short_xcd": lambda n: case(n)["plan"][1] in (40, 43) and (lambda k, cs, co: walk(k, case(n)["B"], case(n)["H"], case(n)["W"], co)["short"])(*launches(n)[1]),
    "split48": _variant(23, lambda c: "s2d" not in c["opts"]), "split48_s2d": _variant(23, lambda c: c["opts"].get("s2d") == [1, 0]),
    "s2d_16": _variant(21, lambda c: c["opts"].get("s2d") == [1, 0] and c["couts"][0] == 16),
    "two_pieces": _variant(21, lambda c: c["plan"][2] == 2 and not c["opts"]),
    "wide_as_two_launches": _variant(21, lambda c: c["plan"][2] == 2 and c["opts"].get("flags") == NO_W16 and c["couts"] == [64]),
    "unwanted_destination": lambda n: None in case(n)["couts"],
    "dst_slice": _opt("dst_in"), "sliced_source": _opt("slice"),
    "wino_relu_of": _opt("relu_of", 1), "w16_relu_of": _opt("relu_of", 3), "wino_words": _opt("words", 1),
    "cat_words_41": lambda n: _opt("words", 2)(n) and case(n)["plan"][1] == 41, "cat_words_40": lambda n: _opt("words", 2)(n) and case(n)["plan"][1] == 40,
    "cat_addend": _opt("addend", 2), "w16_addend": _opt("addend", 3),
    "addend_modulus_not_dividing_B": lambda n: "addend" in case(n)["opts"] and case(n)["B"] % case(n)["opts"]["addend"] != 0,
    "cat_pooled": _opt("pooled", 2), "w16_pooled": _opt("pooled", 3), "pool_code": _opt("pool_code", 2),
    "w16_for_16": lambda n: case(n)["plan"] == (3, 20, 1),
    "shared_source_slot_0": _opt("shared", 2, 0), "shared_source_slot_1": _opt("shared", 2, 1), "shared_source_slot_2": _opt("shared", 2, 2), "up_shared_input": _opt("shared", 4, 0),
    "up_single_tile_image": lambda n: case(n)["plan"][0] == 4 and (case(n)["H"], case(n)["W"]) == (16, 32),
    "up_one_tile_wide": lambda n: case(n)["plan"][0] == 4 and case(n)["W"] == 32 and case(n)["H"] > 16,
    "up_interior_tile_3x3": lambda n: case(n)["plan"][0] == 4 and (case(n)["H"], case(n)["W"]) == (48, 96),
    "up16_single_tile_image": lambda n: case(n)["plan"][0] == 5 and (case(n)["H"], case(n)["W"]) == (32, 32),
    "up16_one_tile_wide": lambda n: case(n)["plan"][0] == 5 and case(n)["W"] == 32 and case(n)["H"] > 32,
    "up16_interior_tile_3x3": lambda n: case(n)["plan"][0] == 5 and (case(n)["H"], case(n)["W"]) == (96, 96),
    "up16_cin_8": lambda n: case(n)["plan"][0] == 5 and case(n)["cs"] == [8], "up16_cin_84": lambda n: case(n)["plan"][0] == 5 and case(n)["cs"] == [84],
}
EM_ALL = {0, 1, 2, 4, 8, 5, 6, 9, 10, 12, 13, 14}      # (3, 7, 11, 15 need a row pair that is the image's first AND last: H >= 16 rules them out)
# rows per stager: removing a row fails the host test even where another row reaches the same edges
ROWS_PER_FAMILY = {None: 1, 1: 14, 2: 18, 3: 19, 4: 4, 5: 3}


# ------------------------------------------------------------------------------------------------ descriptors
def standin(name, base=1 << 20):
    """16-byte aligned stand-in addresses and the strides of the GPU test's buffers (ynet_conv2d_auto_plan looks at pointers for alignment and NULL only)."""
    c = case(name)
    H, W, o = c["H"], c["W"], c["opts"]
    hw_src = (H // 2) * (W // 2) if c["up"] else H * W
    hw = H * W
    ctot = sum(c["sizes"])
    P = dict(src=[(base * (1 + i), 0 if o.get("shared") == i else n * hw_src + PAD) for i, n in enumerate(c["cs"])],
             dst=[(base * (8 + i) if w is not None else None, (n * hw + PAD) if w is not None else 0) for i, (n, w) in enumerate(zip(c["sizes"], c["couts"]))],
             wp=base * 16, bias=base * 17 if c["bias"] else None)
    if "dst_in" in o:
        P["dst"] = [(base * 8 + 4 * o["dst_in"][0] * hw, o["dst_in"][1] * hw + PAD)]
    if o.get("relu_of"):
        P["relu_of"] = (base * 18, ctot * hw + PAD)
    if o.get("pooled"):
        P["pooled"] = (base * 19, ctot * (hw // 4) + PAD)
    if o.get("pool_code"):
        P["pool_code"] = base * 20
    if "addend" in o:
        P["addend"] = (base * 21, ctot * hw + PAD)
    if o.get("words"):
        P["wbits_out"] = base * 22
    return P


def make_desc(L, name, P):
    """The YnetConvAuto of a row on the addresses P (standin's layout): the host test plans it, the GPU test runs it."""
    c = case(name)
    o = c["opts"]
    d = L.ConvAuto()
    d.nsrc, d.ndst = len(c["cs"]), len(c["sizes"])
    for i, (n, (p, bs)) in enumerate(zip(c["cs"], P["src"])):
        d.src[i], d.src_c[i], d.src_bs[i] = p, n, bs
    for i, (n, (p, bs)) in enumerate(zip(c["sizes"], P["dst"])):
        d.dst[i], d.dst_c[i], d.dst_bs[i] = p, n, bs
        d.dst_s2d[i] = int(bool(o.get("s2d") and o["s2d"][i]))
    d.wp, d.bias = P["wp"], P.get("bias")
    d.B, d.H, d.W, d.K, d.relu, d.upsample2x = c["B"], c["H"], c["W"], 3, int(c["relu"]), int(c["up"])
    if "relu_of" in P:
        d.relu_of, d.relu_of_bs = P["relu_of"]
    if "relu_wbits" in P:
        d.relu_wbits = P["relu_wbits"]
    if "pooled" in P:
        d.pooled, d.pooled_bs = P["pooled"]
    if "pool_code" in P:
        d.pool_code = P["pool_code"]
    if "addend" in P:
        d.addend, d.addend_bs = P["addend"]
        d.addend_bmod = o["addend"]
    if "wbits_out" in P:
        d.wbits_out = P["wbits_out"]
    d.flags = o.get("flags", 0)
    return d


def gate_desc(L, B, H, W, c_dy=32, c_dx=32, P=None):
    """The descriptor of the 32 -> 32 data gradient that consumes a row's 1-bit words (relu_of + relu_wbits)."""
    P = P or dict(src=(4096, c_dy * H * W + PAD), dst=(8192, c_dx * H * W + PAD), wp=12288, relu_of=(16384, c_dx * H * W + PAD), relu_wbits=20480)
    d = L.ConvAuto()
    d.nsrc = d.ndst = 1
    d.src[0], d.src_c[0], d.src_bs[0] = P["src"][0], c_dy, P["src"][1]
    d.dst[0], d.dst_c[0], d.dst_bs[0] = P["dst"][0], c_dx, P["dst"][1]
    d.wp, d.B, d.H, d.W, d.K = P["wp"], B, H, W, 3
    d.relu_of, d.relu_of_bs = P["relu_of"]
    d.relu_wbits = P["relu_wbits"]
    return d


def plan_of(lib, L, d):
    """(family, variant, launches) ynet_conv2d_auto_plan reports, or the error."""
    t = L.ConvTaken()
    if lib.ynet_conv2d_auto_plan(ctypes.byref(d), ctypes.byref(t)) != 0:
        return lib.ynet_last_error()
    return t.family, t.variant, t.nlaunch


def supported(lib, kernel, B, H, W, cs, cout):
    """The *_supported query of one launch."""
    arr = (ctypes.c_int * len(cs))(*cs)
    if kernel == "wino":
        return lib.ynet_conv2d_winograd_supported(B, H, W, cs[0], cout, 3)
    if kernel == "cat":
        return lib.ynet_conv2d_winograd_cat_supported(B, H, W, arr, len(cs), cout, 3)
    if kernel == "w16":
        return lib.ynet_conv2d_winograd16_supported(B, H, W, arr, len(cs), cout, 3)
    return int(lib.ynet_upsample2x_conv2d_winograd_supported(B, H, W, cs[0], cout, 3) == (1 if kernel == "up" else 2))


# ------------------------------------------------------------------------------------------------ inputs
def _key(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def _draw(family, lo, hi, scale, *shape, key):
    if family == "b":
        return torch.randint(lo, hi + 1, shape, generator=A._gen(key, *shape)).float()
    return A.randn(*shape, key=key, scale=scale)


class WinoInputs:
    """xs (a `shared` source: one image), w ([cout][cin][3][3]; mode 1: the forward layout of the layer whose gradient it is, [dy channels][dx channels][3][3]), bias, act
    (relu_of), addend ([modulus][cout][H][W]), and for a `words` row dy2 / w2: the 32 -> 32 data gradient gated by the row's ReLU.  fp32 on the CPU."""

    def __init__(self, name, family):
        c = case(name)
        B, H, W, o, k = c["B"], c["H"], c["W"], c["opts"], _key(name)
        hs, ws_ = (H // 2, W // 2) if c["up"] else (H, W)
        cin, ctot = sum(c["cs"]), sum(c["sizes"])
        self.xs = []
        for i, n in enumerate(c["cs"]):
            x = _draw(family, 0 if c["up"] else -3, 3, 1.0, 1 if o.get("shared") == i else B, n, hs, ws_, key=(k, 1 + i))
            self.xs.append(torch.relu(x) if c["up"] else x)      # (an up-convolution's input is a post-ReLU map)
        shape = (cin, ctot, 3, 3) if c["mode"] == 1 else (ctot, cin, 3, 3)
        self.w = _draw(family, -2, 2, 1.0 / (9 * cin) ** 0.5, *shape, key=(k, 10))
        self.bias = _draw(family, -4, 4, 0.1, ctot, key=(k, 11)) if c["bias"] else None
        self.act = torch.relu(_draw(family, -3, 3, 1.0, B, ctot, H, W, key=(k, 12))) if o.get("relu_of") else None      # (family b: {0 .. 3}, half of it zeros)
        self.addend = _draw(family, -4, 4, 1.0, o["addend"], ctot, H, W, key=(k, 13)) if "addend" in o else None
        self.dy2 = self.w2 = None
        if o.get("words"):
            self.dy2 = _draw(family, -4, 4, 1.0, B, 32, H, W, key=(k, 14))
            self.w2 = _draw(family, -2, 2, 1.0 / (9 * 32) ** 0.5, 32, 32, 3, 3, key=(k, 15))


@functools.lru_cache(maxsize=2)
def inputs(name, family):
    return WinoInputs(name, family)


def pool_code(y):
    """The code byte of every 2 x 2 block of the post-ReLU map y [B][C][H][W] by the layout in include/ynet_hip.h: bits 0..1 the FIRST maximum in scan order, bits 2..5
    "element is positive" in scan order."""
    B, C, H, W = y.shape
    blk = y.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    best, idx = blk[..., 0], torch.zeros(blk.shape[:-1], dtype=torch.int32)
    code = (blk[..., 0] > 0).int() << 2
    for k in range(1, 4):
        gt = blk[..., k] > best
        idx = torch.where(gt, torch.full_like(idx, k), idx)
        best = torch.where(gt, blk[..., k], best)
        code |= (blk[..., k] > 0).int() << (2 + k)
    return (code | idx).to(torch.uint8)


def blocks(t):
    B, C, H, W = t.shape
    return t.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)


def reference(name, inp, dtype=torch.float64):
    """Stock torch in `dtype` on the CPU -> dict: pre (the pre-activation / the ungated gradient, all destination channels), y (the same behind ReLU / the relu_of gate),
    pooled, code, and for a `words` row gated: y > 0 ? conv_transpose(dy2, w2) : 0."""
    c = case(name)
    B, o = c["B"], c["opts"]
    x = torch.cat([t.expand(B, -1, -1, -1) if t.shape[0] != B else t for t in inp.xs], 1).to(dtype)
    w = inp.w.to(dtype)
    out = {}
    if c["mode"] == 1:
        pre = F.conv_transpose2d(x, w, padding=1)
        y = torch.where(inp.act > 0, pre, torch.zeros((), dtype=dtype)) if inp.act is not None else pre      # (relu_of > 0 ? dx : 0 -- a gated element is +0.0, not -0.0)
    else:
        if c["up"]:
            x = F.interpolate(x, scale_factor=2, mode="bilinear", align_corners=False)
        pre = F.conv2d(x, w, inp.bias.to(dtype) if inp.bias is not None else None, padding=1)
        if inp.addend is not None:
            pre = pre + inp.addend.to(dtype)[torch.arange(B) % o["addend"]]
        y = F.relu(pre) if c["relu"] else pre
    out["pre"], out["y"] = pre, y
    if o.get("pooled"):
        out["pooled"] = F.max_pool2d(y, 2, 2)
    if o.get("pool_code"):
        out["code"] = pool_code(y)
    if o.get("words"):
        out["gated"] = torch.where(y > 0, F.conv_transpose2d(inp.dy2.to(dtype), inp.w2.to(dtype), padding=1), torch.zeros((), dtype=dtype))
    return out


@functools.lru_cache(maxsize=2)
def ref64(name, family):
    return reference(name, inputs(name, family))


def ambiguous(name, ref):
    """Where the fp32 kernels and the fp64 reference may disagree on a gate -> (elements [B][C][H][W] with |pre-activation| < AMBIGUOUS, or None; blocks [B][C][H/2][W/2]
    whose arg-max may differ, or None).  A block's arg-max is open when its two largest outputs lie closer than AMBIGUOUS -- unless all four pre-activations are below
    -AMBIGUOUS: then the device holds four zeros as the reference does and the first of them wins in both."""
    c = case(name)
    o = c["opts"]
    el = blk = None
    if c["relu"] and (o.get("words") or o.get("pool_code")):
        el = ref["pre"].abs() < A.AMBIGUOUS
    if o.get("pool_code"):
        top = blocks(ref["y"]).topk(2, dim=-1).values
        all_off = (blocks(ref["pre"]) <= -A.AMBIGUOUS).all(-1)
        blk = ((top[..., 0] - top[..., 1]) < A.AMBIGUOUS) & ~all_off
    return el, blk


def s2d(t):
    """Row-major [B][C][H][W] -> space-to-depth [B][4 C][H / 2][W / 2]: element (2 i + r, 2 j + c) of channel ch at plane (2 r + c) C + ch, position (i, j)."""
    B, C, H, W = t.shape
    return t.view(B, C, H // 2, 2, W // 2, 2).permute(0, 3, 5, 1, 2, 4).reshape(B, 4 * C, H // 2, W // 2)

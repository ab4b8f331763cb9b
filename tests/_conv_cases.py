"""The direct convolution kernels at every plan edge: the case table, the seeded inputs, the fp64 references and the dispatcher's formulas in plain Python
(tests/test_conv_cases_host.py checks this module and the plans on the CPU, tests/test_gpu_conv_edges.py runs the kernels against it).

csrc/conv_mfma.hip has conv_dma_kernel (the LDS-DMA generation: unfolded tiles of 1 .. 4 16-channel tiles x 2 / 4 rows per wave, folded tiles for maps no wider than
16 / 8 pixels; six epilogue forms EPI 0 .. 5), conv_mfma_kernel (the register-staged generation: any alignment, any K), conv1x1_stream_kernel, conv_split_reduce_kernel,
conv_emask_kernel and pack_weight_kernel; conv_dispatch_kernels picks the template arguments.  Every row names the launch ynet_conv2d_last_launch(0) must report -- the
claim is written down by hand, `launch_plan` recomputes it from the dispatcher's formulas (copied here as plain Python) and the host test holds the two and ynet_conv2d_plan
against each other -- and the edges it is there for; EDGES recomputes every edge from those formulas.

The gates are read from the environment once per process: SWITCHES lists them, the host test asserts that none is set.
One gate has no far side at all: the 1x1 streaming kernel wants H W % 4 == 0 next to 16-byte loads, which need W % 4 == 0 -- no shape passes one and fails the other.
ynet_conv2d_plan does not know the streaming kernel (it names the tile kernel an unaligned 1x1 call takes), so the streaming rows are held to the launch note alone.

Inputs, two seeded families per row:
  "a": normal data scaled as _align_cases.ConvRef scales it (filter 1 / sqrt(K K cin), bias 0.1); post-ReLU where the operand is an activation (relu_of, a mask); the output
       gradient of a bit-mask row is zero in the 3 x 3 neighbourhood of every element whose fp64 pre-activation is within A.AMBIGUOUS of 0, so the device's own gate
       decides nothing the comparison sees;
  "b": exact integers -- x in [-3, 3], filter in [-2, 2], bias, addend and dy in [-4, 4], activations in {0 .. 3}.  Every partial sum is an integer below 2^24 (asserted per
       row), so any summation order, a split channel loop included, gives the same fp32 value: the device must match the reference bit for bit.

References: stock torch on .double() inputs on the CPU, cached per (row, family) -- never the code under test."""
import functools
import zlib

import torch
import torch.nn.functional as F

import _align_cases as A

PAD = 8                               # floats of NaN between the images of every operand (keeps the 16-byte gates where W % 4 == 0)
LEAD, TRAIL = 2, 1                    # NaN planes around a sliced source
UNWANTED = 16                         # channels of a destination nobody wants
CIN_PAD, COUT_PAD = 16, 64            # YNET_CIN_PAD, YNET_COUT_PAD (csrc/conv_mfma.hip)
SLOTS_MAX = 8 * 256                   # resident workgroups: at most 8 per CU x 256 CUs
SWITCHES = ["YNET_CONV_R", "YNET_CONV_R4_MIN", "YNET_CONV_R2_MIN", "YNET_CONV_FOLD", "YNET_CONV_NARROW", "YNET_CONV_DMA", "YNET_CONV_1X1_STREAM", "YNET_CONV_NO_KSPLIT",
            "YNET_KSPLIT_ITEMS", "YNET_KSPLIT_TARGET", "YNET_RELU_BITS", "YNET_CONV_DEBUG"]
REG, DMA, FOLDED, STREAM = 1, 2, 3, 4      # the kind ynet_conv2d_last_launch(0) reports in bits 0..3


def cdiv(a, b):
    return -(-a // b)


# ------------------------------------------------------------------------------------------------ the dispatcher's formulas (csrc/conv_mfma.hip), default gates
def m16_tiles(K, cout):
    if K != 3:
        return 0
    if cout <= 16:
        return 1
    if 32 < cout <= 48:
        return 3
    return 2 if cout <= 32 else 4


def conv_fold(H, W):
    if W <= 8 and H % 4 == 0:
        return 4
    if W <= 16 and H % 2 == 0:
        return 2
    return 1


def units(B, H, W):
    """narrow_tiles' work items: the one-row-per-wave tiles of the map (folded where conv_fold folds)."""
    f = conv_fold(H, W)
    return B * cdiv(W, 32 // f) * cdiv(H, 4 * f)


def narrow_tiles(B, H, W, nt16, target=2048):
    if nt16 <= 1:
        return nt16
    u, n = units(B, H, W), nt16
    while n > 1 and u * cdiv(nt16, n) < target:
        n = 2 if n > 2 else 1
    return n


def pick_rows(B, H, W, cout, cb, r4_min=1024, r2_min=64):
    for r in (4, 2):
        if cdiv(W, 32) * cdiv(H, 4 * r) * cdiv(cout, cb) * B >= (r4_min if r == 4 else r2_min):
            return r
    return 1


def dma_rows(B, H, W, cout, nt16):
    rows = pick_rows(B, H, W, cout, 16 * nt16)
    return 2 if nt16 >= 3 and rows == 4 else rows


def conv_ksplit(items, nchunks, min_items=256, target=512):
    if items >= min_items or nchunks < 4:
        return 1
    return max(1, min(cdiv(target, items), nchunks // 2, 8))


def workspace_floats(B, H, W, cout):
    """ynet_conv2d_workspace_floats."""
    return 0 if W % 4 or B * H * W > 64 * 1024 else 8 * B * cout * H * W


def rows_tiles_ok(B, H, W, cout, K):
    """make_direct_plan gives GEN_DMA: the unfolded LDS-DMA tiles with two or more rows per wave serve an aligned call of this shape (the epilogue forms live there)."""
    nt16 = narrow_tiles(B, H, W, m16_tiles(K, cout))
    return K == 3 and W % 4 == 0 and nt16 > 0 and conv_fold(H, W) == 1 and dma_rows(B, H, W, cout, nt16) >= 2


def pool_supported(B, H, W, cout, K):
    return (H | W) & 1 == 0 and rows_tiles_ok(B, H, W, cout, K)


def add_supported(B, H, W, cout, K):
    nt16 = m16_tiles(K, cout)
    return K == 3 and W % 4 == 0 and nt16 in (2, 4) and conv_fold(H, W) == 1 and dma_rows(B, H, W, cout, nt16) >= 2


def bits_words(B, H, W, cout, K):
    """ynet_conv2d_relu_bits_words: [tile][256 lanes][WPL]."""
    if not rows_tiles_ok(B, H, W, cout, K):
        return 0
    nt16 = narrow_tiles(B, H, W, m16_tiles(K, cout))
    rows = dma_rows(B, H, W, cout, nt16)
    return cdiv(W, 32) * cdiv(H, 4 * rows) * cdiv(cout, 16 * nt16) * B * 256 * cdiv(nt16 * rows * 8, 32)


def dispatch(B, H, W, cs, cout, K, vl=1, vs=1, ws=0, addend=False, mask=False, epi=False, stream_ok=True):
    """conv_dispatch_kernels + launch_*_m -> dict(kind, rows, tiles, cb (output channels per workgroup), cc, fold, ksplit, cps, nchunks, items (tiles before the split),
    ntiles, tw, th, cgroups).  cout: the channels left after the unwanted trailing destinations are dropped; vl / vs: 16-byte loads / stores are legal; ws: the floats of
    the caller's workspace (0: none); epi: a pooled or bit-mask launch (never split); stream_ok: the 1x1 streaming kernel's gates on the operands hold."""
    full = m16_tiles(K, cout)
    nt16 = full if addend else narrow_tiles(B, H, W, full)
    kind = None
    if addend:
        assert add_supported(B, H, W, cout, K) and vl and vs and not mask
        kind, rows, tiles, cc, fold, cb = DMA, dma_rows(B, H, W, cout, nt16), nt16, 4, 1, 16 * nt16
    elif nt16 and vl and vs:
        fold = conv_fold(H, W)
        if fold > 1:
            kind, rows, tiles, cc, cb = FOLDED, 1, nt16, (8 if nt16 <= 2 else 4), 16 * nt16
        else:
            rows = dma_rows(B, H, W, cout, nt16)
            if rows >= 2:
                kind, tiles, cb, cc = DMA, nt16, 16 * nt16, (8 if rows == 2 and nt16 == 1 else 4)      # (the small tiles take CC 8: the two-row one-tile kernel)
    if kind is None:
        fold = 1
        if K == 1 and stream_ok and len(cs) == 1 and not mask and cout <= 32 and vl and vs and H * W % 4 == 0:
            return dict(kind=STREAM, rows=0, tiles=1 if cout <= 16 else 2, cb=cout, cc=0, fold=1, ksplit=1, cps=0, nchunks=0, items=0, ntiles=0, tw=0, th=0, cgroups=1)
        kind = REG
        if nt16:
            tiles, cb, cc = nt16, 16 * nt16, 8
            rows = pick_rows(B, H, W, cout, cb)
            rows = 2 if nt16 >= 3 and rows == 4 else rows
        elif K == 1:
            tiles, cc = (2 if cout > 32 else 1), 16
            cb = 32 * tiles
            rows = pick_rows(B, H, W, cout, cb)
        else:
            assert K == 5
            tiles, cc, rows = (2 if cout > 32 else 1), 4, 4
            cb = 32 * tiles
    tw, th = 32 // fold, 4 * rows * fold
    cgroups = cdiv(cout, cb)
    items = cdiv(W, tw) * cdiv(H, th) * cgroups * B
    nchunks = sum(cdiv(c, cc) for c in cs)
    k = 1
    if ws > 0 and W % 4 == 0 and not addend and not epi:
        k = conv_ksplit(items, nchunks)
    while k > 1 and k * B * cout * H * W > ws:
        k -= 1
    cps = cdiv(nchunks, k)
    k = cdiv(nchunks, cps)      # no empty split
    return dict(kind=kind, rows=rows, tiles=tiles, cb=cb, cc=cc, fold=fold, ksplit=k, cps=cps, nchunks=nchunks, items=items, ntiles=items * k, tw=tw, th=th, cgroups=cgroups,
                wanted_k=conv_ksplit(items, nchunks) if ws > 0 and W % 4 == 0 and not addend and not epi else 1)


def plan_word(B, H, W, cout, K):
    """ynet_conv2d_plan from the formulas: rows | tiles << 8 | m16 << 16 | dma << 17 | x4 << 18 | log2(fold) << 19 | CC << 21 (the plain call on aligned operands where
    W % 4 == 0; the plan knows nothing of the 1x1 streaming kernel and names the tile kernel an unaligned 1x1 call takes)."""
    al = int(W % 4 == 0)
    p = dispatch(B, H, W, [1 << 20], cout, K, vl=al, vs=al, stream_ok=False)
    dma = int(p["kind"] in (DMA, FOLDED))
    return p["rows"] | p["tiles"] << 8 | int(K == 3) << 16 | dma << 17 | dma << 18 | {1: 0, 2: 1, 4: 2}[p["fold"]] << 19 | p["cc"] << 21


def note(kind, rows, ksplit, vl, vs):
    """The word ynet_conv2d_last_launch(0) reports."""
    return kind | rows << 4 | ksplit << 8 | vl << 12 | vs << 13


def walk(ntiles, grid):
    """The persistent walk of `grid` workgroups over `ntiles` tiles as the kernels make it -> [tiles of workgroup 0, of workgroup 1, ...]."""
    xw = grid % 8 == 0 and ntiles >= grid
    per_xcd = cdiv(ntiles, 8)
    out = []
    for blk in range(grid):
        if xw:
            out.append(list(range((blk & 7) * per_xcd + (blk >> 3), min(ntiles, ((blk & 7) + 1) * per_xcd), grid >> 3)))
        else:
            out.append(list(range(blk, ntiles, grid)))
    return out


def decode(t, p, B, H, W):
    """Tile index -> (split, channel group, tile column, tile row, image): conv_dma_body's decode."""
    tx, ty = cdiv(W, p["tw"]), cdiv(H, p["th"])
    ks, t = t % p["ksplit"], t // p["ksplit"]
    cg, t = t % p["cgroups"], t // p["cgroups"]
    x, t = t % tx, t // tx
    return ks, cg, x, t % ty, t // ty


def advance(coord, step, radix):
    """advance_tile: the mixed-radix step with one carry per digit that the persistent workgroups take instead of dividing."""
    out, carry = [], 0
    for c, s, r in zip(coord[:-1], step[:-1], radix):
        c += s + carry
        carry = int(c >= r)
        out.append(c - carry * r)
    return tuple(out) + (coord[-1] + step[-1] + carry,)


# ------------------------------------------------------------------------------------------------ the rows
# name: (entry, B, H, W, source channels, destination channels (None: unwanted, UNWANTED channels), K, relu, bias, mode, operands, claim, edges)
#   entry     "conv" ynet_conv2d / "dgrad_relu" ynet_conv2d_dgrad_relu / "bits" ynet_conv2d_relu_bits, then ynet_conv2d_dgrad_relu_bits of a `dy` channels -> cout data
#             gradient on the same output shape / "pool" ynet_conv2d_pool / "add" ynet_conv2d_add
#   mode      0 a forward convolution, 1 a data gradient (the sources are dy, the filter is the forward layer's [dy channels][dx channels][K][K])
#   operands  mask (input side, one source: x is kept where mask > 0) / relu_of / addend: modulus (0: one image per image of the batch) / shared: {i: m} (source i has batch
#             stride 0 (m 0) or repeats with the batch modulus m) / slice: i (source i is a channel slice of a wider NaN tensor) / dst_in: (first, total) (destination 0 is a
#             channel slice of a wider NaN tensor) / place: (operand, (off, pad)) (one of _align_cases.PLACEMENTS; operand "src0" .. "dst0" .. "mask") / workspace: floats
#             (default: ynet_conv2d_workspace_floats, what ops.conv2d passes; 0: none) / dy: channels and dmask (the bit-mask pair's data gradient, masked on its input side)
#   claim     (kind, rows, ksplit, 16-byte loads, 16-byte stores, channel tiles, chunk depth): what ynet_conv2d_last_launch(0) must report after the call and, for the last
#             two, what `dispatch` derives (ynet_conv2d_plan's tile count and chunk depth for an aligned plain call)
R, NR = True, False
T, S = (410, 17, 20), (8, 32, 64)      # 2050 one-row units of a ragged map (narrow_tiles keeps every tile count, rows 2) / 64 two-row units of one 16-channel tile
CASES = {
    # ---- 1. rows per wave at their gates (B - 1 plans differently: GATED)
    "r4_t1": ("conv", 16, 256, 128, [4], [16], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["rows4_one_tile"]),
    "r4_t2": ("conv", 16, 256, 128, [3], [32], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 2, 4), ["rows4_two_tiles", "narrow_32_keeps_2"]),
    "r2_t2": ("conv", 8, 256, 128, [5, 3], [32], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 2, 4), ["rows2_two_tiles", "narrow_32_keeps_2", "ragged_chunk_in_every_source"]),
    "r2_t1": ("conv", 64, 8, 32, [8], [16], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 1, 8), ["rows2_one_tile"]),
    "r2_t1_narrowed": ("conv", 2, 64, 64, [8], [32], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 1, 8), ["rows2_one_tile_narrowed_from_two", "narrow_32_to_1","one_chunk_small_tile_two_groups"]),
    "below_r2_gate": ("conv", 63, 8, 32, [8], [16], 3, R, True, 0, {}, (REG, 1, 1, 1, 1, 1, 8), ["below_rows2_gate"]),
    "t3_forced_r2": ("conv", 512, 17, 20, [3], [33], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 3, 4), ["three_tiles_forced_to_rows2"]),
    "t4": ("conv", *T, [3], [49], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 4, 4), ["four_tiles"]),
    "cg2_cout65": ("conv", *T, [3], [65], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 4, 4), ["two_groups_last_partial", "one_chunk_large_tile_two_groups"]),
    "cg3_cout130": ("conv", 1024, 5, 20, [3], [130], 3, NR, True, 0, {}, (DMA, 2, 1, 1, 1, 4, 4), ["three_groups_last_partial", "three_tiles_forced_to_rows2"]),
    # ---- 2. narrow_tiles
    "n48_keep": ("conv", *T, [3], [48], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 3, 4), ["narrow_48_keeps_3"]),
    "n48_to_2": ("conv", 205, 17, 20, [3], [48], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 2, 4), ["narrow_48_to_2"]),
    "n48_to_1": ("conv", 204, 17, 20, [3], [48], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["narrow_48_to_1"]),
    "n64_keep": ("conv", *T, [3], [64], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 4, 4), ["narrow_64_keeps_4"]),
    "n64_to_2": ("conv", 409, 17, 20, [3], [64], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 2, 4), ["narrow_64_to_2"]),
    "n64_to_1": ("conv", 204, 17, 20, [3], [64], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["narrow_64_to_1"]),
    "n32_to_1": ("conv", 409, 17, 20, [3], [32], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["narrow_32_to_1"]),
    # ---- 3. folded tiles
    "fold4_w8": ("conv", 4, 8, 8, [65], [130], 3, R, True, 0, {}, (FOLDED, 1, 3, 1, 1, 1, 8), ["fold4_w8", "ksplit_cap_half_the_chunks", "cin_above_cin_pad", "ragged_chunk_in_every_source"]),
    "fold4_w4": ("conv", 4, 8, 4, [8], [16], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 1, 8), ["fold4_w4", "walk_fewer_than_8_tiles"]),
    "fold2_w16": ("conv", 4, 16, 16, [64, 2], [64], 3, R, True, 0, {}, (FOLDED, 1, 3, 1, 1, 1, 8), ["fold2_w16"]),
    "fold2_w12": ("conv", 3, 6, 12, [21, 27, 2], [16], 3, R, True, 0, {}, (FOLDED, 1, 4, 1, 1, 1, 8), ["fold2_w12", "ragged_chunk_in_every_source"]),
    "fold_off_odd_h": ("conv", 64, 7, 16, [8], [16], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 1, 8), ["fold_off_odd_h"]),
    "fold2_w8_h6": ("conv", 4, 6, 8, [8], [16], 3, NR, True, 0, {}, (FOLDED, 1, 1, 1, 1, 1, 8), ["fold2_w8_h_mod4_is_2"]),
    "fold4_two_tiles": ("conv", 2048, 16, 8, [3], [17], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 2, 8), ["folded_two_tiles"]),
    "fold4_three_tiles": ("conv", 2048, 16, 8, [3], [33], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 3, 4), ["folded_three_tiles"]),
    "fold2_four_tiles": ("conv", 2048, 8, 16, [3], [49], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 4, 4), ["folded_four_tiles"]),
    # ---- 4. channel chunks
    "src4_one_channel_slots": ("conv", *S, [3, 1, 5, 1], [32], 3, R, True, 0, {}, (DMA, 2, 2, 1, 1, 1, 8), ["four_sources", "one_channel_source_slot_1", "one_channel_source_slot_3"]),
    # ---- 5. split-K
    "ks_cap8": ("conv", 4, 8, 8, [128], [16], 3, R, True, 0, {}, (FOLDED, 1, 8, 1, 1, 1, 8), ["ksplit_cap_8", "cin_above_cin_pad", "split_with_relu_and_bias"]),
    "ks_cap_items": ("conv", 8, 32, 32, [96], [64], 3, R, True, 0, {}, (DMA, 2, 4, 1, 1, 1, 8), ["ksplit_cap_items", "split_with_relu_and_bias"]),
    "ks_uneven": ("conv", 4, 8, 8, [56], [16], 3, NR, True, 0, {}, (FOLDED, 1, 3, 1, 1, 1, 8), ["ksplit_last_split_shorter"]),
    "ks_items_255": ("conv", 255, 16, 8, [32], [16], 3, R, True, 0, {}, (FOLDED, 1, 2, 1, 1, 1, 8), ["ksplit_items_255", "ksplit_nchunks_4"]),
    "ks_items_256": ("conv", 256, 16, 8, [32], [16], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 1, 8), ["ksplit_items_256"]),
    "ks_nchunks_3": ("conv", 4, 8, 8, [24], [16], 3, R, True, 0, {}, (FOLDED, 1, 1, 1, 1, 1, 8), ["ksplit_nchunks_3"]),
    "ks_ws_to_3": ("conv", 8, 32, 32, [96], [64], 3, R, True, 0, {"workspace": 3 * 8 * 64 * 1024}, (DMA, 2, 3, 1, 1, 1, 8), ["workspace_lowers_ksplit_to_3"]),
    "ks_ws_to_1": ("conv", 8, 32, 32, [96], [64], 3, R, True, 0, {"workspace": 2 * 8 * 64 * 1024 - 1}, (DMA, 2, 1, 1, 1, 1, 8), ["workspace_lowers_ksplit_to_1"]),
    "ks_ws_0": ("conv", 8, 32, 32, [96], [64], 3, R, True, 0, {"workspace": 0}, (DMA, 2, 1, 1, 1, 1, 8), ["workspace_0"]),
    "ks_two_dst": ("conv", 4, 16, 16, [64], [16, 48], 3, R, True, 0, {}, (FOLDED, 1, 4, 1, 1, 1, 8), ["split_two_destinations"]),
    "ks_unwanted_middle": ("conv", 4, 16, 16, [64], [5, None, 7], 3, NR, False, 1, {}, (FOLDED, 1, 4, 1, 1, 1, 8), ["split_unwanted_middle_destination"]),
    "ks_relu_of_reduce": ("dgrad_relu", 4, 16, 16, [64], [64], 3, NR, False, 1, {"relu_of": True}, (FOLDED, 1, 4, 1, 1, 1, 8), ["split_relu_of_in_the_reduction"]),
    "ks_relu_of_two_row": ("dgrad_relu", 8, 32, 32, [64], [64], 3, NR, False, 1, {"relu_of": True}, (DMA, 2, 4, 1, 1, 1, 8), ["split_relu_of_two_row_tile"]),
    "ks_reg_relu_of": ("dgrad_relu", 2, 32, 32, [64], [64], 3, NR, False, 1, {"relu_of": True}, (REG, 1, 4, 1, 1, 1, 8), ["split_register_staged_then_mask_pass"]),
    "k5_ws_65536": ("conv", 1, 256, 256, [16], [8], 5, R, True, 0, {}, (REG, 4, 2, 1, 1, 1, 4), ["workspace_at_65536_pixels"]),
    "k5_ws_above": ("conv", 1, 256, 260, [16], [8], 5, R, True, 0, {}, (REG, 4, 1, 1, 1, 1, 4), ["workspace_above_65536_pixels"]),
    # ---- 6. destinations
    "dst_5_20_7": ("conv", *T, [3], [5, 20, 7], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 2, 4), ["destinations_inside_a_tile"]),
    "dst_trailing_unwanted": ("conv", *T, [3], [60, None], 3, NR, False, 1, {}, (DMA, 2, 1, 1, 1, 4, 4), ["trailing_unwanted_destination"]),
    "dst_middle_unwanted": ("conv", *T, [3], [5, None, 7], 3, NR, False, 1, {}, (DMA, 2, 1, 1, 1, 2, 4), ["middle_unwanted_destination"]),
    "dst_four": ("conv", *S, [8], [3, 5, 7, 1], 3, NR, True, 0, {}, (DMA, 2, 1, 1, 1, 1, 8), ["four_destinations"]),
    "dst_slice": ("conv", *S, [8], [16], 3, R, True, 0, {"dst_in": (3, 24)}, (DMA, 2, 1, 1, 1, 1, 8), ["destination_slice"]),
    "reg_dst_5_20_7": ("conv", 3, 9, 13, [5], [5, 20, 7], 3, R, True, 0, {}, (REG, 1, 1, 0, 0, 1, 8), ["reg_destinations_inside_a_tile", "w_mod_4_scalar_stores"]),
    "reg_dst_trailing_unwanted": ("conv", 3, 9, 13, [5], [60, None], 3, NR, False, 1, {}, (REG, 1, 1, 0, 0, 1, 8), ["reg_trailing_unwanted_destination"]),
    "reg_dst_middle_unwanted": ("conv", 3, 9, 13, [5], [5, None, 7], 3, NR, False, 1, {}, (REG, 1, 1, 0, 0, 1, 8), ["reg_middle_unwanted_destination"]),
    # ---- 7. sources
    "src_stride0": ("conv", *S, [8, 8], [16], 3, R, True, 0, {"shared": {1: 0}}, (DMA, 2, 1, 1, 1, 1, 8), ["source_batch_stride_0"]),
    "src_bmod3": ("conv", *S, [8, 8], [16], 3, R, True, 0, {"shared": {0: 3}, "slice": 1}, (DMA, 2, 1, 1, 1, 1, 8), ["source_modulus_not_dividing_B", "sliced_source"]),
    "mask_large": ("conv", *T, [8], [32], 3, NR, False, 1, {"mask": True}, (DMA, 2, 1, 1, 1, 2, 4), ["mask_quads_per_channel"]),
    "mask_small": ("conv", 64, 8, 32, [16], [16], 3, NR, False, 1, {"mask": True}, (DMA, 2, 1, 1, 1, 1, 8), ["mask_flat_items"]),
    "mask_fold": ("conv", 4, 8, 8, [16], [16], 3, NR, False, 1, {"mask": True, "slice": 0}, (FOLDED, 1, 1, 1, 1, 1, 8), ["mask_folded", "sliced_source"]),
    "mask_reg": ("conv", 3, 9, 13, [5], [7], 3, NR, False, 1, {"mask": True}, (REG, 1, 1, 0, 0, 1, 8), ["mask_register_staged"]),
    # ---- 8. ragged maps
    "ragged_h_rows2": ("conv", 11, 18, 36, [4], [16], 3, R, True, 0, {}, (DMA, 2, 1, 1, 1, 1, 8), ["ragged_h_rows2", "w_mod_32_is_4", "walk_odd_tiles_below_the_grid"]),
    "ragged_h_rows4": ("conv", 256, 17, 36, [4], [16], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["ragged_h_rows4", "w_mod_32_is_4"]),
    "w28": ("conv", 512, 17, 28, [4], [16], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["w_mod_32_is_28"]),
    "reg_rows2": ("conv", 16, 32, 30, [5], [16], 3, R, True, 0, {}, (REG, 2, 1, 0, 0, 1, 8), ["reg_rows2", "w_mod_4_scalar_stores"]),
    "reg_rows4": ("conv", 512, 17, 30, [3], [16], 3, R, True, 0, {}, (REG, 4, 1, 0, 0, 1, 8), ["reg_rows4"]),
    "h1": ("conv", 5, 1, 64, [4], [16], 3, R, True, 0, {}, (REG, 1, 1, 1, 1, 1, 8), ["h_1"]),
    "w1": ("conv", 5, 64, 1, [4], [16], 3, R, True, 0, {}, (REG, 1, 1, 0, 0, 1, 8), ["w_1"]),
    "one_pixel": ("conv", 3, 1, 1, [4], [16], 3, R, True, 0, {}, (REG, 1, 1, 0, 0, 1, 8), ["one_pixel_map"]),
    # ---- 9. the epilogue forms: at their own two-row gate, and at a ragged H, W with W % 4 == 0
    "add_t2": ("add", *S, [8], [32], 3, R, True, 0, {"addend": 0}, (DMA, 2, 1, 1, 1, 2, 4), ["add_two_tiles_not_narrowed"]),
    "add_t4": ("add", *S, [8], [64], 3, R, True, 0, {"addend": 2}, (DMA, 2, 1, 1, 1, 4, 4), ["add_four_tiles", "addend_modulus_dividing_B"]),
    "add_t2_ragged_mod3": ("add", 11, 18, 36, [5, 3], [32], 3, R, True, 0, {"addend": 3}, (DMA, 2, 1, 1, 1, 2, 4), ["add_ragged", "addend_modulus_not_dividing_B", "add_odd_tiles_below_the_grid"]),
    "add_t4_ragged": ("add", 11, 18, 36, [8], [64], 3, NR, False, 0, {"addend": 0}, (DMA, 2, 1, 1, 1, 4, 4), ["add_ragged", "add_four_tiles"]),
    "relu_of_t1": ("dgrad_relu", 64, 8, 32, [8], [16], 3, NR, False, 1, {"relu_of": True}, (DMA, 2, 1, 1, 1, 1, 8), ["relu_of_in_the_kernel_one_tile"]),
    "relu_of_t2_masked_ragged": ("dgrad_relu", *T, [8], [32], 3, NR, False, 1, {"relu_of": True, "mask": True}, (DMA, 2, 1, 1, 1, 2, 4), ["relu_of_in_the_kernel_masked", "relu_of_ragged"]),
    "relu_of_t4_ragged": ("dgrad_relu", *T, [4], [64], 3, NR, False, 1, {"relu_of": True}, (DMA, 2, 1, 1, 1, 4, 4), ["relu_of_in_the_kernel_four_tiles", "relu_of_ragged"]),
    "relu_of_rows4": ("dgrad_relu", 256, 17, 36, [4], [16], 3, NR, False, 1, {"relu_of": True}, (DMA, 4, 1, 1, 1, 1, 4), ["relu_of_in_the_kernel_rows4", "relu_of_ragged"]),
    "relu_of_1x1": ("dgrad_relu", 2, 32, 32, [12], [32], 1, NR, False, 1, {"relu_of": True}, (STREAM, 0, 1, 1, 1, 2, 0), ["relu_of_pass_after_1x1"]),
    "relu_of_5x5": ("dgrad_relu", 1, 16, 16, [9], [7], 5, NR, False, 1, {"relu_of": True}, (REG, 4, 1, 1, 1, 1, 4), ["relu_of_pass_after_5x5"]),
    "relu_of_reg": ("dgrad_relu", 3, 24, 40, [5], [7], 3, NR, False, 1, {"relu_of": True, "mask": True}, (REG, 1, 1, 1, 1, 1, 8), ["relu_of_pass_after_register_staged"]),
    "relu_of_fold": ("dgrad_relu", 4, 8, 8, [8], [16], 3, NR, False, 1, {"relu_of": True}, (FOLDED, 1, 1, 1, 1, 1, 8), ["relu_of_pass_after_folded"]),
    "pool_rows2_gate": ("pool", 64, 8, 32, [8], [16], 3, R, True, 0, {"pooled": True}, (DMA, 2, 1, 1, 1, 1, 8), ["pool_rows2", "pool_whole_tiles_at_the_gate"]),
    "pool_rows2_ragged": ("pool", 11, 18, 36, [4], [16], 3, R, True, 0, {"pooled": True}, (DMA, 2, 1, 1, 1, 1, 8), ["pool_rows2", "pool_ragged_h"]),
    "pool_rows4_ragged": ("pool", 256, 18, 36, [4], [16], 3, R, True, 0, {"pooled": True}, (DMA, 4, 1, 1, 1, 1, 4), ["pool_rows4", "pool_ragged_h"]),
    "pool_t2": ("pool", 410, 18, 20, [3], [32], 3, R, True, 0, {"pooled": True}, (DMA, 2, 1, 1, 1, 2, 4), ["pool_two_tiles", "pool_ragged_h"]),
    "pool_t4_no_relu": ("pool", 410, 18, 20, [3], [64], 3, NR, True, 0, {"pooled": True}, (DMA, 2, 1, 1, 1, 4, 4), ["pool_four_tiles"]),
    "bits_t1": ("bits", 64, 8, 32, [8], [16], 3, R, True, 0, {"dy": 8}, (DMA, 2, 1, 1, 1, 1, 8), ["bits_one_tile", "bits_one_word"]),
    "bits_t2_masked": ("bits", *T, [3], [32], 3, R, True, 0, {"dy": 8, "dmask": True}, (DMA, 2, 1, 1, 1, 2, 4), ["bits_two_tiles", "bits_one_word", "bits_masked_gradient", "bits_ragged"]),
    "bits_t4": ("bits", *T, [3], [64], 3, R, True, 0, {"dy": 4}, (DMA, 2, 1, 1, 1, 4, 4), ["bits_four_tiles", "bits_two_words", "bits_ragged"]),
    "bits_rows4_t2": ("bits", 512, 17, 20, [3], [32], 3, R, False, 0, {"dy": 4}, (DMA, 4, 1, 1, 1, 2, 4), ["bits_rows4", "bits_two_words"]),
    # ---- 10. the other kernels
    "s1_cout16": ("conv", 2, 32, 32, [32], [16], 1, NR, True, 0, {}, (STREAM, 0, 1, 1, 1, 1, 0), ["stream_cout_16"]),
    "s1_cout17": ("conv", 2, 32, 32, [32], [17], 1, NR, True, 0, {}, (STREAM, 0, 1, 1, 1, 2, 0), ["stream_cout_17"]),
    "s1_cout32_relu": ("conv", 3, 5, 12, [7], [32], 1, R, True, 0, {}, (STREAM, 0, 1, 1, 1, 2, 0), ["stream_cout_32", "stream_relu"]),
    "s1_cout33": ("conv", 2, 32, 32, [32], [33], 1, NR, True, 0, {}, (REG, 1, 1, 1, 1, 2, 16), ["stream_gate_cout_33"]),
    "k1_two_sources_shared": ("conv", 5, 32, 32, [20, 12], [33], 1, R, True, 0, {"shared": {1: 2}}, (REG, 1, 1, 1, 1, 2, 16), ["tile_1x1_two_sources", "tile_1x1_cout_33", "tile_1x1_shared_source"]),
    "k1_two_sources_narrow": ("conv", 2, 32, 32, [20, 12], [16], 1, R, True, 0, {}, (REG, 1, 1, 1, 1, 1, 16), ["tile_1x1_two_sources"]),
    "k5_cout32": ("conv", 2, 12, 20, [5], [32], 5, R, True, 0, {}, (REG, 4, 1, 1, 1, 1, 4), ["k5_cout_32"]),
    "k5_cout33": ("conv", 2, 12, 20, [5], [33], 5, R, True, 0, {}, (REG, 4, 1, 1, 1, 2, 4), ["k5_cout_33"]),
    "k5_map_2x3": ("conv", 3, 2, 3, [5], [7], 5, R, True, 0, {}, (REG, 4, 1, 0, 0, 1, 4), ["k5_map_smaller_than_the_filter"]),
    "reg_t2_dst_off16": ("conv", *T, [8], [32], 3, R, True, 0, {"place": ("dst0", (0, 2))}, (REG, 2, 1, 1, 0, 2, 8), ["reg_two_tiles"]),
    "reg_t3_src_off16": ("conv", *T, [8], [48], 3, R, True, 0, {"place": ("src0", (1, 0))}, (REG, 2, 1, 0, 1, 3, 8), ["reg_three_tiles"]),
    "reg_t4_src_off16": ("conv", *T, [8], [64], 3, R, True, 0, {"place": ("src0", (1, 0))}, (REG, 2, 1, 0, 1, 4, 8), ["reg_four_tiles"]),
    # ---- 11. the persistent walk
    "walk_2049": ("conv", 2049, 5, 20, [3], [16], 3, R, True, 0, {}, (DMA, 4, 1, 1, 1, 1, 4), ["walk_more_tiles_than_any_grid", "walk_tiles_mod_8_is_1"]),
    "walk_add_2055": ("add", 2055, 5, 20, [3], [32], 3, R, True, 0, {"addend": 4}, (DMA, 4, 1, 1, 1, 2, 4), ["add_more_tiles_than_any_grid", "walk_tiles_mod_8_is_7", "add_rows4", "addend_modulus_not_dividing_B"]),
}
# rows that sit AT a gate: one image fewer plans differently (or is refused by the entry's *_supported)
GATED = ["r4_t1", "r4_t2", "r2_t2", "r2_t1", "r2_t1_narrowed", "t3_forced_r2", "t4", "cg2_cout65", "cg3_cout130", "n48_keep", "n48_to_2", "n64_keep",
         "fold_off_odd_h", "fold4_three_tiles", "fold2_four_tiles", "add_t2", "add_t4", "relu_of_t1", "pool_rows2_gate", "pool_rows4_ragged", "pool_t2", "bits_t1", "bits_t2_masked",
         "bits_t4", "bits_rows4_t2", "ks_items_256"]
# one NaN and one +inf planted in one source pixel (tests/test_gpu_conv_edges.py): a two-row row, a folded row, a split-K row; and a NaN under a closed mask
PLANTED = {"dst_four": (3, 2, 17, 33), "fold2_w8_h6": (1, 5, 0, 7), "ks_uneven": (2, 41, 7, 0), "add_t4_ragged": (10, 7, 17, 35),
           # (the pooled copy, rows 2 and rows 4 on a ragged map: the 3 x 3 neighbourhood straddles four 2 x 2 blocks and the corner of four tiles)
           "pool_rows2_ragged": (10, 3, 8, 32), "pool_rows4_ragged": (255, 1, 16, 32)}      # (image, channel, row, column) of source 0
MASKED_NAN = ["mask_small", "mask_large", "mask_fold", "mask_reg"]
# what the entries must refuse before any launch: name: (entry, B, H, W, sources, cout, K, the word the error names)
REFUSALS = {
    "pool_k1": ("pool", 8, 32, 64, [8], 16, 1, b"conv2d_pool:"),
    "pool_k5": ("pool", 8, 32, 64, [8], 16, 5, b"conv2d_pool:"),
    "pool_folded_map": ("pool", 64, 8, 16, [8], 16, 3, b"conv2d_pool:"),
    "pool_one_row_map": ("pool", 63, 8, 32, [8], 16, 3, b"conv2d_pool:"),
    "pool_w_mod_4": ("pool", 64, 8, 30, [8], 16, 3, b"conv2d_pool:"),
    "add_cout_16": ("add", 8, 32, 64, [8], 16, 3, b"conv2d_add:"),
    "add_cout_48": ("add", 8, 32, 64, [8], 48, 3, b"conv2d_add:"),
    "add_one_row_map": ("add", 7, 32, 64, [8], 32, 3, b"conv2d_add:"),
    "bits_out_no_words": ("bits_out", 63, 8, 32, [8], 16, 3, b"conv2d_relu_bits:"),
    "bits_in_no_words": ("bits_in", 63, 8, 32, [8], 16, 3, b"conv2d_dgrad_relu_bits:"),
    "mask_two_sources": ("mask", 8, 32, 64, [8, 8], 16, 3, b"conv2d:"),
    "five_sources": ("conv", 8, 32, 64, [4, 4, 4, 4, 4], 16, 3, b"conv2d:"),
}


def case(name):
    entry, B, H, W, cs, couts, K, relu, bias, mode, opts, claim, edges = CASES[name]
    sizes = [c if c is not None else UNWANTED for c in couts]
    wanted = list(couts)
    while len(wanted) > 1 and wanted[-1] is None:
        wanted.pop()
    return dict(entry=entry, B=B, H=H, W=W, cs=cs, couts=couts, K=K, relu=relu, bias=bias, mode=mode, opts=opts, claim=claim, edges=edges, sizes=sizes,
                ctot=sum(sizes), cout=sum(sizes[:len(wanted)]), ndst=len(wanted), cin=sum(cs))


def aligned(c, ignore_place=False):
    """(16-byte loads legal, 16-byte stores legal) for the row's operands."""
    vl = vs = int(c["W"] % 4 == 0)
    if "place" in c["opts"] and not ignore_place:
        op, (off, pad) = c["opts"]["place"]
        if off % 4 or pad % 4:
            if op.startswith("dst"):
                vs = 0
            else:
                vl = 0
    return vl, vs


def ws_of(c):
    return c["opts"].get("workspace", workspace_floats(c["B"], c["H"], c["W"], c["ctot"])) if c["entry"] in ("conv", "dgrad_relu") else 0


def launch_plan(name, B=None, ignore_place=False):
    """`dispatch` for a row (B: another batch size, for the gates)."""
    c = case(name)
    o = c["opts"]
    vl, vs = aligned(c, ignore_place)
    B = c["B"] if B is None else B
    ws = ws_of(c) if B == c["B"] else (o.get("workspace", workspace_floats(B, c["H"], c["W"], c["ctot"])) if c["entry"] in ("conv", "dgrad_relu") else 0)
    shared = o.get("shared", {})
    return dispatch(B, c["H"], c["W"], c["cs"], c["cout"], c["K"], vl, vs, ws, addend=c["entry"] == "add", mask="mask" in o, epi=c["entry"] in ("pool", "bits"),
                    stream_ok=c["ndst"] == 1 and c["couts"][0] is not None and not shared.get(0))


def claim_of(p, vl, vs):
    return (p["kind"], p["rows"], p["ksplit"], vl, vs, p["tiles"], p["cc"])


# ------------------------------------------------------------------------------------------------ the edges, recomputed from the formulas
def _p(n):
    return launch_plan(n)


def _is(n, entry=None, kind=None, **kw):
    c, p = case(n), _p(n)
    return (entry is None or c["entry"] == entry) and (kind is None or p["kind"] == kind) and all(p[k] == v for k, v in kw.items())


def _narrow(cout, to):
    def f(n):
        c = case(n)
        u = units(c["B"], c["H"], c["W"])
        full = m16_tiles(3, cout)
        band = u >= 2048 if to == full else (1024 <= u < 2048 if to == 2 else u < (1024 if full > 2 else 2048))
        return c["entry"] == "conv" and c["K"] == 3 and c["cout"] == cout and band and _p(n)["tiles"] == to and aligned(c) == (1, 1)
    return f


def _fold(w, f, pred=lambda c: True):
    return lambda n: case(n)["W"] == w and conv_fold(case(n)["H"], w) == f and _is(n, kind=FOLDED if f > 1 else None, fold=f) and pred(case(n))


def _split(n):
    return _p(n)["ksplit"] > 1


def _last_partial(groups):
    return lambda n: _is(n, kind=DMA, tiles=4, cgroups=groups) and case(n)["cout"] % 64 != 0 and case(n)["bias"]


def _raw_rows(n, B=None):
    c, p = case(n), _p(n)
    return pick_rows(c["B"] if B is None else B, c["H"], c["W"], c["cout"], p["cb"])


def _dsts_inside_tiles(c):
    """Some wanted destination begins and some wanted destination ends inside a 16-channel tile."""
    edges, c0 = [], 0
    for n, w in zip(c["sizes"], c["couts"]):
        if w is not None:
            edges += [c0 % 16 != 0, (c0 + n) % 16 != 0]
        c0 += n
    return len(c["couts"]) == 3 and all(edges[1:-1]) and None not in c["couts"]


def _gate_epi(entry, **kw):
    return lambda n: _is(n, entry=entry, kind=DMA, **kw)


def _ragged_epi(entry):
    return lambda n: _is(n, entry=entry, kind=DMA) and case(n)["W"] % 4 == 0 and case(n)["W"] % 32 != 0 and case(n)["H"] % _p(n)["th"] != 0


def _bits_wpl(n):
    p = _p(n)
    return cdiv(p["tiles"] * p["rows"] * 8, 32)


def _dst_case(kind, couts_pred):
    return lambda n: _is(n, entry="conv", kind=kind) and couts_pred(case(n)) and not _split(n)


EDGES = {
    # 1. rows per wave
    "rows4_one_tile": lambda n: _is(n, entry="conv", kind=DMA, rows=4, tiles=1) and case(n)["cout"] == 16,
    "rows4_two_tiles": lambda n: _is(n, entry="conv", kind=DMA, rows=4, tiles=2) and case(n)["cout"] == 32,
    "rows2_two_tiles": lambda n: _is(n, entry="conv", kind=DMA, rows=2, tiles=2, cc=4),
    "rows2_one_tile": lambda n: _is(n, entry="conv", kind=DMA, rows=2, tiles=1, cc=8) and case(n)["cout"] == 16,      # (a small tile: CC 8)
    "rows2_one_tile_narrowed_from_two": lambda n: _is(n, entry="conv", kind=DMA, rows=2, tiles=1, cc=8, cgroups=2) and case(n)["cout"] == 32,
    "below_rows2_gate": lambda n: _is(n, entry="conv", kind=REG, rows=1) and aligned(case(n)) == (1, 1) and dispatch(case(n)["B"] + 1, case(n)["H"], case(n)["W"], case(n)["cs"], case(n)["cout"], 3)["kind"] == DMA,
    "three_tiles_forced_to_rows2": lambda n: _is(n, kind=DMA, rows=2) and _p(n)["tiles"] >= 3 and _raw_rows(n) == 4 and units(case(n)["B"], case(n)["H"], case(n)["W"]) >= 2048,
    "four_tiles": lambda n: _is(n, entry="conv", kind=DMA, tiles=4) and 49 <= case(n)["cout"] <= 64 and case(n)["cout"] % 16 != 0,
    "two_groups_last_partial": _last_partial(2), "three_groups_last_partial": _last_partial(3),
    # 2. narrow_tiles
    "narrow_48_keeps_3": _narrow(48, 3), "narrow_48_to_2": _narrow(48, 2), "narrow_48_to_1": _narrow(48, 1),
    "narrow_64_keeps_4": _narrow(64, 4), "narrow_64_to_2": _narrow(64, 2), "narrow_64_to_1": _narrow(64, 1),
    "narrow_32_keeps_2": _narrow(32, 2), "narrow_32_to_1": _narrow(32, 1),
    # 3. folded tiles
    "fold4_w8": _fold(8, 4), "fold4_w4": _fold(4, 4), "fold2_w16": _fold(16, 2), "fold2_w12": _fold(12, 2),
    "fold_off_odd_h": _fold(16, 1, lambda c: c["H"] % 2 == 1), "fold2_w8_h_mod4_is_2": _fold(8, 2, lambda c: c["H"] % 4 == 2),
    "folded_two_tiles": lambda n: _is(n, kind=FOLDED, tiles=2, cc=8), "folded_three_tiles": lambda n: _is(n, kind=FOLDED, tiles=3, fold=4, cc=4),
    "folded_four_tiles": lambda n: _is(n, kind=FOLDED, tiles=4, fold=2, cc=4),
    # 4. channel chunks
    "one_chunk_large_tile_two_groups": lambda n: _is(n, kind=DMA, cc=4, nchunks=1) and _p(n)["cgroups"] >= 2 and case(n)["bias"] and case(n)["cin"] <= 4,
    "one_chunk_small_tile_two_groups": lambda n: _is(n, kind=DMA, cc=8, nchunks=1) and _p(n)["cgroups"] >= 2 and case(n)["bias"] and case(n)["cin"] <= 8,
    "ragged_chunk_in_every_source": lambda n: _p(n)["kind"] in (DMA, FOLDED) and all(s % _p(n)["cc"] for s in case(n)["cs"]),
    "four_sources": lambda n: len(case(n)["cs"]) == 4 and _p(n)["kind"] == DMA,
    "one_channel_source_slot_1": lambda n: len(case(n)["cs"]) > 1 and case(n)["cs"][1] == 1, "one_channel_source_slot_3": lambda n: len(case(n)["cs"]) > 3 and case(n)["cs"][3] == 1,
    "cin_above_cin_pad": lambda n: case(n)["cin"] > CIN_PAD and case(n)["cin"] % CIN_PAD != 0 or case(n)["cin"] >= 8 * CIN_PAD,
    # 5. split-K
    "ksplit_cap_half_the_chunks": lambda n: (lambda p: p["wanted_k"] == p["nchunks"] // 2 < min(8, cdiv(512, p["items"])))(_p(n)),
    "ksplit_cap_8": lambda n: (lambda p: p["ksplit"] == 8 and p["nchunks"] // 2 >= 8 and cdiv(512, p["items"]) > 8)(_p(n)),
    "ksplit_cap_items": lambda n: (lambda p: p["ksplit"] == cdiv(512, p["items"]) < min(8, p["nchunks"] // 2))(_p(n)),
    "ksplit_last_split_shorter": lambda n: (lambda p: p["ksplit"] > 1 and p["nchunks"] % p["cps"] != 0)(_p(n)),
    "ksplit_items_255": lambda n: _p(n)["items"] == 255 and _split(n), "ksplit_items_256": lambda n: (lambda p: p["items"] == 256 and p["nchunks"] >= 4 and p["ksplit"] == 1)(_p(n)) and ws_of(case(n)) > 0,
    "ksplit_nchunks_3": lambda n: (lambda p: p["nchunks"] == 3 and p["items"] < 256 and p["ksplit"] == 1)(_p(n)) and ws_of(case(n)) > 0, "ksplit_nchunks_4": lambda n: _p(n)["nchunks"] == 4 and _split(n),
    "workspace_lowers_ksplit_to_3": lambda n: (lambda p: p["wanted_k"] > 3 and p["ksplit"] == 3)(_p(n)) and "workspace" in case(n)["opts"],
    "workspace_lowers_ksplit_to_1": lambda n: (lambda p: p["wanted_k"] > 1 and p["ksplit"] == 1)(_p(n)) and case(n)["opts"].get("workspace", 0) > 0,
    "workspace_0": lambda n: case(n)["opts"].get("workspace") == 0 and dispatch(case(n)["B"], case(n)["H"], case(n)["W"], case(n)["cs"], case(n)["cout"], 3, ws=1 << 40)["ksplit"] > 1,
    "split_with_relu_and_bias": lambda n: _split(n) and case(n)["relu"] and case(n)["bias"],
    "split_two_destinations": lambda n: _split(n) and case(n)["couts"] == [16, 48],
    "split_unwanted_middle_destination": lambda n: _split(n) and len(case(n)["couts"]) == 3 and case(n)["couts"][1] is None,
    "split_relu_of_in_the_reduction": lambda n: _split(n) and _is(n, entry="dgrad_relu", kind=FOLDED),
    "split_relu_of_two_row_tile": lambda n: _split(n) and _is(n, entry="dgrad_relu", kind=DMA),
    "split_register_staged_then_mask_pass": lambda n: _split(n) and _is(n, entry="dgrad_relu", kind=REG),
    "workspace_at_65536_pixels": lambda n: case(n)["B"] * case(n)["H"] * case(n)["W"] == 65536 and _split(n),
    "workspace_above_65536_pixels": lambda n: 65536 < case(n)["B"] * case(n)["H"] * case(n)["W"] <= 65536 + 1024 and case(n)["W"] % 4 == 0 and ws_of(case(n)) == 0,
    # 6. destinations
    "destinations_inside_a_tile": _dst_case(DMA, _dsts_inside_tiles), "reg_destinations_inside_a_tile": _dst_case(REG, _dsts_inside_tiles),
    "trailing_unwanted_destination": _dst_case(DMA, lambda c: c["couts"][-1] is None and cdiv(c["cout"], COUT_PAD) < cdiv(c["ctot"], COUT_PAD)),
    "reg_trailing_unwanted_destination": _dst_case(REG, lambda c: c["couts"][-1] is None and cdiv(c["cout"], COUT_PAD) < cdiv(c["ctot"], COUT_PAD)),
    "middle_unwanted_destination": _dst_case(DMA, lambda c: len(c["couts"]) == 3 and c["couts"][1] is None),
    "reg_middle_unwanted_destination": _dst_case(REG, lambda c: len(c["couts"]) == 3 and c["couts"][1] is None),
    "four_destinations": lambda n: len(case(n)["couts"]) == 4 and None not in case(n)["couts"],
    "destination_slice": lambda n: "dst_in" in case(n)["opts"],
    # 7. sources
    "source_batch_stride_0": lambda n: 0 in case(n)["opts"].get("shared", {}).values() and _p(n)["kind"] == DMA,
    "source_modulus_not_dividing_B": lambda n: any(m and case(n)["B"] % m for m in case(n)["opts"].get("shared", {}).values()) and _p(n)["kind"] == DMA,
    "sliced_source": lambda n: "slice" in case(n)["opts"],
    "mask_quads_per_channel": lambda n: _is(n, entry="conv", kind=DMA, cc=4) and "mask" in case(n)["opts"],
    "mask_flat_items": lambda n: _is(n, entry="conv", kind=DMA, cc=8) and "mask" in case(n)["opts"],
    "mask_folded": lambda n: _is(n, entry="conv", kind=FOLDED, cc=8) and "mask" in case(n)["opts"],
    "mask_register_staged": lambda n: _is(n, entry="conv", kind=REG) and "mask" in case(n)["opts"],
    # 8. ragged maps
    "ragged_h_rows2": lambda n: _is(n, entry="conv", kind=DMA, rows=2) and case(n)["H"] % 8 != 0, "ragged_h_rows4": lambda n: _is(n, entry="conv", kind=DMA, rows=4) and case(n)["H"] % 16 != 0,
    "w_mod_32_is_4": lambda n: case(n)["W"] % 32 == 4 and _p(n)["kind"] == DMA, "w_mod_32_is_28": lambda n: case(n)["W"] % 32 == 28 and _p(n)["kind"] == DMA,
    "w_mod_4_scalar_stores": lambda n: case(n)["W"] % 4 != 0 and case(n)["W"] > 4 and _is(n, kind=REG, ksplit=1) and aligned(case(n)) == (0, 0),
    "reg_rows2": lambda n: _is(n, entry="conv", kind=REG, rows=2, tiles=1), "reg_rows4": lambda n: _is(n, entry="conv", kind=REG, rows=4, tiles=1) and case(n)["K"] == 3,
    "h_1": lambda n: case(n)["H"] == 1 and case(n)["W"] > 32, "w_1": lambda n: case(n)["W"] == 1 and case(n)["H"] > 32, "one_pixel_map": lambda n: case(n)["H"] == case(n)["W"] == 1,
    # 9. the epilogue forms
    "add_two_tiles_not_narrowed": lambda n: _is(n, entry="add", kind=DMA, tiles=2, rows=2) and narrow_tiles(case(n)["B"], case(n)["H"], case(n)["W"], 2) == 1,
    "add_four_tiles": _gate_epi("add", tiles=4), "add_ragged": _ragged_epi("add"), "add_rows4": _gate_epi("add", rows=4),
    "addend_modulus_not_dividing_B": lambda n: case(n)["opts"].get("addend", 0) > 0 and case(n)["B"] % case(n)["opts"]["addend"] != 0,
    "addend_modulus_dividing_B": lambda n: 1 < case(n)["opts"].get("addend", 0) < case(n)["B"] and case(n)["B"] % case(n)["opts"]["addend"] == 0,
    "add_odd_tiles_below_the_grid": lambda n: _is(n, entry="add") and 8 <= _p(n)["ntiles"] < 256 and _p(n)["ntiles"] % 8 != 0,
    "add_more_tiles_than_any_grid": lambda n: _is(n, entry="add") and _p(n)["ntiles"] > SLOTS_MAX and _p(n)["ntiles"] % 8 in (1, 7),
    "relu_of_in_the_kernel_one_tile": _gate_epi("dgrad_relu", tiles=1, rows=2, ksplit=1),
    "relu_of_in_the_kernel_masked": lambda n: _is(n, entry="dgrad_relu", kind=DMA, ksplit=1) and "mask" in case(n)["opts"],
    "relu_of_in_the_kernel_four_tiles": _gate_epi("dgrad_relu", tiles=4, ksplit=1), "relu_of_in_the_kernel_rows4": _gate_epi("dgrad_relu", rows=4, ksplit=1),
    "relu_of_ragged": _ragged_epi("dgrad_relu"),
    "relu_of_pass_after_1x1": lambda n: _is(n, entry="dgrad_relu", kind=STREAM), "relu_of_pass_after_5x5": lambda n: _is(n, entry="dgrad_relu", kind=REG) and case(n)["K"] == 5,
    "relu_of_pass_after_register_staged": lambda n: _is(n, entry="dgrad_relu", kind=REG, ksplit=1) and case(n)["K"] == 3,
    "relu_of_pass_after_folded": lambda n: _is(n, entry="dgrad_relu", kind=FOLDED, ksplit=1),
    "pool_rows2": _gate_epi("pool", rows=2), "pool_rows4": _gate_epi("pool", rows=4), "pool_two_tiles": _gate_epi("pool", tiles=2), "pool_four_tiles": _gate_epi("pool", tiles=4),
    "pool_whole_tiles_at_the_gate": lambda n: _is(n, entry="pool") and case(n)["H"] % _p(n)["th"] == 0 and case(n)["W"] % 32 == 0 and not pool_supported(case(n)["B"] - 1, case(n)["H"], case(n)["W"], case(n)["cout"], 3),
    "pool_ragged_h": lambda n: _is(n, entry="pool") and case(n)["H"] % _p(n)["th"] != 0 and case(n)["W"] % 32 != 0,
    "bits_one_tile": _gate_epi("bits", tiles=1), "bits_two_tiles": _gate_epi("bits", tiles=2), "bits_four_tiles": _gate_epi("bits", tiles=4), "bits_rows4": _gate_epi("bits", rows=4),
    "bits_one_word": lambda n: _is(n, entry="bits") and _bits_wpl(n) == 1, "bits_two_words": lambda n: _is(n, entry="bits") and _bits_wpl(n) == 2,
    "bits_masked_gradient": lambda n: _is(n, entry="bits") and bool(case(n)["opts"].get("dmask")), "bits_ragged": _ragged_epi("bits"),
    # 10. the other kernels
    "stream_cout_16": lambda n: _is(n, kind=STREAM) and case(n)["cout"] == 16, "stream_cout_17": lambda n: _is(n, kind=STREAM) and case(n)["cout"] == 17,
    "stream_cout_32": lambda n: _is(n, kind=STREAM) and case(n)["cout"] == 32, "stream_relu": lambda n: _is(n, entry="conv", kind=STREAM) and case(n)["relu"] and case(n)["H"] * case(n)["W"] % 32 != 0,
    "stream_gate_cout_33": lambda n: _is(n, kind=REG, tiles=2, cc=16) and case(n)["cout"] == 33 and len(case(n)["cs"]) == 1 and not case(n)["opts"],
    "tile_1x1_cout_33": lambda n: _is(n, kind=REG, tiles=2, cc=16) and case(n)["cout"] == 33, "tile_1x1_two_sources": lambda n: _is(n, kind=REG, cc=16) and len(case(n)["cs"]) == 2,
    "tile_1x1_shared_source": lambda n: _is(n, kind=REG, cc=16) and bool(case(n)["opts"].get("shared")),
    "k5_cout_32": lambda n: case(n)["K"] == 5 and case(n)["cout"] == 32 and _p(n)["tiles"] == 1, "k5_cout_33": lambda n: case(n)["K"] == 5 and case(n)["cout"] == 33 and _p(n)["tiles"] == 2,
    "k5_map_smaller_than_the_filter": lambda n: case(n)["K"] == 5 and case(n)["H"] < 5 and case(n)["W"] < 5,
    # (the register-staged 16-wide tiles with 2 .. 4 channel tiles: an operand off a 16-byte boundary on a shape whose aligned plan is LDS-DMA)
    "reg_two_tiles": lambda n: _is(n, kind=REG, tiles=2, cc=8) and launch_plan(n, ignore_place=True)["kind"] == DMA,
    "reg_three_tiles": lambda n: _is(n, kind=REG, tiles=3, cc=8) and launch_plan(n, ignore_place=True)["kind"] == DMA,
    "reg_four_tiles": lambda n: _is(n, kind=REG, tiles=4, cc=8) and launch_plan(n, ignore_place=True)["kind"] == DMA,
    # 11. the persistent walk
    "walk_more_tiles_than_any_grid": lambda n: _is(n, entry="conv") and _p(n)["ntiles"] > SLOTS_MAX and _p(n)["ntiles"] % 8 in (1, 7),
    "walk_tiles_mod_8_is_1": lambda n: _p(n)["ntiles"] > SLOTS_MAX and _p(n)["ntiles"] % 8 == 1, "walk_tiles_mod_8_is_7": lambda n: _p(n)["ntiles"] > SLOTS_MAX and _p(n)["ntiles"] % 8 == 7,
    "walk_fewer_than_8_tiles": lambda n: _p(n)["kind"] != STREAM and _p(n)["ntiles"] < 8,
    "walk_odd_tiles_below_the_grid": lambda n: _is(n, entry="conv") and 8 <= _p(n)["ntiles"] < 256 and _p(n)["ntiles"] % 8 != 0,
}


def gate_key(name, B):
    """What must change one image below a GATED row: the launch, the raw pick_rows, or whether the entry serves the shape at all."""
    c = case(name)
    args = (B, c["H"], c["W"], c["cout"], c["K"])
    ok = {"pool": pool_supported, "add": add_supported, "bits": lambda *a: bits_words(*a) > 0}.get(c["entry"], lambda *a: True)(*args)
    if not ok:
        return None
    p = launch_plan(name, B)
    return claim_of(p, *aligned(c)), pick_rows(B, c["H"], c["W"], c["cout"], p["cb"])


# ------------------------------------------------------------------------------------------------ inputs
def _key(name):
    return zlib.crc32(name.encode()) & 0x7fffffff


def _draw(family, lo, hi, scale, *shape, key):
    if family == "b":
        return torch.randint(lo, hi + 1, shape, generator=A._gen(key, *shape)).float()
    return A.randn(*shape, key=key, scale=scale)


def images(c, i):
    """Images of source i: B, or the batch modulus of a shared one (1 for batch stride 0)."""
    m = c["opts"].get("shared", {}).get(i)
    return c["B"] if m is None else max(m, 1)


class ConvInputs:
    """xs (a shared source: its own images only), w (mode 0 [cout][cin][K][K]; mode 1 the forward layout of the layer whose gradient it is, [dy channels][dx channels][K][K]),
    bias, mask (input side, the shape of source 0), act (relu_of), addend ([modulus or B][cout][H][W]) and, for a bit-mask row, dy2 / w2 / dmask: the dy -> cout data gradient
    gated by the row's ReLU.  fp32 on the CPU."""

    def __init__(self, name, family):
        c = case(name)
        B, H, W, K, o, k = c["B"], c["H"], c["W"], c["K"], c["opts"], _key(name)
        cin, ctot = c["cin"], c["ctot"]
        self.xs = [_draw(family, -3, 3, 1.0, images(c, i), n, H, W, key=(k, 1 + i)) for i, n in enumerate(c["cs"])]
        shape = (cin, ctot, K, K) if c["mode"] == 1 else (ctot, cin, K, K)
        self.w = _draw(family, -2, 2, 1.0 / (K * K * cin) ** 0.5, *shape, key=(k, 10))
        self.bias = _draw(family, -4, 4, 0.1, ctot, key=(k, 11)) if c["bias"] else None
        self.mask = torch.relu(_draw(family, -3, 3, 1.0, B, c["cs"][0], H, W, key=(k, 16))) if o.get("mask") else None
        self.act = torch.relu(_draw(family, -3, 3, 1.0, B, ctot, H, W, key=(k, 12))) if o.get("relu_of") else None      # (family b: {0 .. 3}, half of it zeros)
        self.addend = _draw(family, -4, 4, 1.0, o["addend"] or B, ctot, H, W, key=(k, 13)) if "addend" in o else None
        self.dy2 = self.w2 = self.dmask = None
        if c["entry"] == "bits":
            self.dy2 = _draw(family, -4, 4, 1.0, B, o["dy"], H, W, key=(k, 14))
            self.w2 = _draw(family, -2, 2, 1.0 / (9 * o["dy"]) ** 0.5, o["dy"], ctot, 3, 3, key=(k, 15))
            self.dmask = torch.relu(_draw(family, -3, 3, 1.0, B, o["dy"], H, W, key=(k, 17))) if o.get("dmask") else None
            if family == "a":      # no gradient reaches an element whose gate is ambiguous
                near = (_forward(c, self, torch.float64).abs() < A.AMBIGUOUS).any(1, keepdim=True).double()
                self.dy2 = self.dy2 * ~(F.max_pool2d(near, 3, 1, 1) > 0)


@functools.lru_cache(maxsize=2)
def inputs(name, family):
    return ConvInputs(name, family)


def _forward(c, inp, dtype):
    """The pre-activation (mode 1: the ungated gradient) of all destination channels."""
    B, K = c["B"], c["K"]
    x = torch.cat([t[torch.arange(B) % t.shape[0]] for t in inp.xs], 1).to(dtype)
    if inp.mask is not None:
        x = torch.where(inp.mask > 0, x, torch.zeros((), dtype=dtype))
    w = inp.w.to(dtype)
    if c["mode"] == 1:
        pre = F.conv_transpose2d(x, w, padding=K // 2)
    else:
        pre = F.conv2d(x, w, inp.bias.to(dtype) if inp.bias is not None else None, padding=K // 2)
    if inp.addend is not None:
        pre = pre + inp.addend.to(dtype)[torch.arange(B) % inp.addend.shape[0]]
    return pre


def pool_rule(y):
    """The 2 x 2 max-pooled copy by the rule include/ynet_hip.h states for it: the maximum of the block, NaN where any of its four elements is."""
    B, C, H, W = y.shape
    blk = y.view(B, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(B, C, H // 2, W // 2, 4)
    top = torch.where(torch.isnan(blk), torch.full_like(blk, float("-inf")), blk).max(-1).values
    return torch.where(torch.isnan(blk).any(-1), torch.full_like(top, float("nan")), top)


def reference(name, inp, dtype=torch.float64):
    """Stock torch in `dtype` on the CPU -> dict: pre, y (behind the ReLU / the relu_of gate), pooled, and for a bit-mask row gated: y > 0 ? conv^T(dy2 [masked], w2) : 0."""
    c = case(name)
    zero = torch.zeros((), dtype=dtype)
    pre = _forward(c, inp, dtype)
    y = F.relu(pre) if c["relu"] else pre
    if inp.act is not None:
        y = torch.where(inp.act > 0, y, zero)      # (a gated element is +0.0)
    out = dict(pre=pre, y=y)
    if c["entry"] == "pool":
        out["pooled"] = pool_rule(y)
    if c["entry"] == "bits":
        dy = inp.dy2.to(dtype)
        if inp.dmask is not None:
            dy = torch.where(inp.dmask > 0, dy, zero)
        out["gated"] = torch.where(y > 0, F.conv_transpose2d(dy, inp.w2.to(dtype), padding=1), zero)
    return out


@functools.lru_cache(maxsize=2)
def ref64(name, family):
    return reference(name, inputs(name, family))


def ambiguous(name, ref):
    """Elements [B][C][H][W] of a bit-mask row whose gate the fp32 kernel and the fp64 reference may see differently (None for every other row)."""
    return ref["pre"].abs() < A.AMBIGUOUS if case(name)["entry"] == "bits" else None


def restate(x, w, bias, K):
    """conv(x, w) + bias as plain loops over the taps in fp64: out[b, o, y, x] = sum_i sum_ky sum_kx x[b, i, y + ky - K / 2, x + kx - K / 2] w[o, i, ky, kx]."""
    B, cin, H, W = x.shape
    xp = F.pad(x.double(), (K // 2,) * 4)
    out = torch.zeros(B, w.shape[0], H, W, dtype=torch.float64)
    for ky in range(K):
        for kx in range(K):
            out += torch.einsum("bihw,oi->bohw", xp[:, :, ky:ky + H, kx:kx + W], w[:, :, ky, kx].double())
    return out + (bias.double().view(1, -1, 1, 1) if bias is not None else 0)


def packed(w, mode):
    """ynet_pack_weight in plain Python: [rows_pad + one chunk of slack][K K][cols_pad], zero padded; mode 0 wp[ci][t][co] = w[co][ci][t], mode 1 wp[co][t][ci] = w[co][ci][K K - 1 - t]."""
    cout, cin, K, _ = w.shape
    rows, cols = (cin, cout) if mode == 0 else (cout, cin)
    wp = torch.zeros(cdiv(rows, CIN_PAD) * CIN_PAD + CIN_PAD, K * K, cdiv(cols, COUT_PAD) * COUT_PAD)
    flat = w.reshape(cout, cin, K * K)
    for t in range(K * K):
        wp[:rows, t, :cols] = flat[:, :, t].t() if mode == 0 else flat[:, :, K * K - 1 - t]
    return wp

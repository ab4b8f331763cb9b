"""One layer, one direction, two plans: the smallest shapes at which ynet_conv2d_auto lays the transformed filters of a layer out differently at two
batch sizes IN THE SAME NUMBER OF FLOATS (128^2 maps, B 4 against B 8) -- the premise of tests/test_gpu_auto_cache.py, which
tests/test_cabi_symbols.py checks on every machine: ynet_conv2d_auto_plan and ynet_conv2d_auto_cache_layout are host code."""
import ctypes

H = W = 128
BATCHES = (4, 8)
# name: ([source channels], [destination channels, None = not wanted], data gradient?, {B: (family, variant, launches)}, cache floats at both sizes)
LAYERS = {
    "fwd_32_32": ([32], [32], False, {4: (3, 22, 1), 8: (1, 21, 1)}, 16384),
    "fwd_cat_32_32_1_32": ([32, 32, 1], [32], False, {4: (3, 42, 1), 8: (2, 40, 2)}, 34816),
    "dgrad_32_to_16_32_unwanted": ([32], [16, 32, None], True, {4: (3, 22, 2), 8: (1, 23, 1)}, 24576),
}
# the up-convolution's backward (YNET_AUTO_UPCONV_BWD) of a 32 -> 16 layer at 64^2: B 12 and B 32 share a layout, B 8 has another
UP_COUT, UP_CIN, UP_HW, UP_BATCHES = 16, 32, 64, (12, 32, 8, 12)


def sizes(couts):
    """Channels per destination (an unwanted one still spans 16 columns of the filter)."""
    return [16 if c is None else c for c in couts]


def descriptor(L, B, cs, couts, dgrad, flags=0):
    """The YnetConvAuto of one LAYERS row at batch size B with stand-in addresses (the plan looks at their alignment only): a forward convolution with bias and
    ReLU, or a plain data gradient."""
    d = L.ConvAuto()
    d.nsrc, d.ndst = len(cs), len(couts)
    for i, c in enumerate(cs):
        d.src[i], d.src_c[i], d.src_bs[i] = 256, c, c * H * W
    for i, (c, n) in enumerate(zip(couts, sizes(couts))):
        d.dst[i], d.dst_c[i], d.dst_bs[i] = (None if c is None else 256), n, (0 if c is None else n * H * W)
    d.wp, d.B, d.H, d.W, d.K, d.flags = 256, B, H, W, 3, flags
    if not dgrad:
        d.bias, d.relu = 256, 1
    return d


def up_descriptor(L, B, masked, flags=0):
    """The YnetConvAuto of the up-convolution's backward at batch size B (stand-in addresses), through the ReLU backward of the layer below when `masked`."""
    hw = UP_HW * UP_HW
    d = L.ConvAuto()
    d.nsrc = d.ndst = 1
    d.src[0], d.src_c[0], d.src_bs[0] = 256, 4 * UP_COUT, 4 * UP_COUT * hw
    d.dst[0], d.dst_c[0], d.dst_bs[0] = 256, UP_CIN, UP_CIN * hw
    if masked:
        d.relu_of, d.relu_of_bs = 256, UP_CIN * hw
    d.wp, d.B, d.H, d.W, d.K, d.flags = 256, B, UP_HW, UP_HW, 3, flags | L.AUTO_UPCONV_BWD
    return d


def layout(L, lib, d):
    """(ynet_conv2d_auto_cache_layout's value, the floats it reports) of a descriptor."""
    floats = ctypes.c_longlong(-2)
    value = lib.ynet_conv2d_auto_cache_layout(ctypes.byref(d), ctypes.byref(floats))
    assert floats.value >= 0, lib.ynet_last_error()
    return int(value), int(floats.value)

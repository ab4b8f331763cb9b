"""ynet_conv2d_auto's filter cache inside the package: one entry of the layer's cache per ynet_conv2d_auto_cache_layout value (ops._auto_call).  A layer
visited at two batch sizes whose plans lay the transformed filter out differently -- in the same number of floats: tests/_auto_cache_cases.py -- keeps
two buffers, neither is touched by the other plan's calls, a captured launch goes on reading its own, and the batch sizes of the up-convolution's backward
that share a layout share a buffer.  Outputs are compared bit for bit with the same call on a fresh cache: the same kernels, the same filter."""
import pytest
import torch

import _auto_cache_cases as A
from conftest import pkg

pytestmark = pytest.mark.gpu
H, W = A.H, A.W


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


def same_bits(a, b):
    return torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


class Layer:
    """One A.LAYERS row on the device: operands for the largest batch, of which a call at batch size B uses the first B images."""

    def __init__(self, dev, name):
        self.ops = pkg("ops")
        self.cs, self.couts, self.dgrad, self.plans, self.floats = A.LAYERS[name]
        self.what = "dgrad" if self.dgrad else "fwd"
        Bmax, cin, self.sizes = max(A.BATCHES), sum(self.cs), A.sizes(self.couts)
        ctot = sum(self.sizes)
        self.xs = [rnd(Bmax, c, H, W, seed=20 + i).to(dev) for i, c in enumerate(self.cs)]
        w = rnd(cin, ctot, 3, 3, seed=2, scale=0.2) if self.dgrad else rnd(ctot, cin, 3, 3, seed=2, scale=0.2)
        self.wp = self.ops.pack_weight(w.to(dev), 1 if self.dgrad else 0)
        self.bias = None if self.dgrad else rnd(ctot, seed=3).to(dev)
        self.dev = dev

    def __call__(self, B, cache, outs=None):
        """conv2d_auto_raw at batch size B on `cache` -> (YnetConvTaken, the wanted outputs)."""
        if outs is None:
            outs = [torch.full((B, n, H, W), float("nan"), device=self.dev) for n in self.sizes]
        srcs = [(x.data_ptr(), c, c * H * W) for x, c in zip(self.xs, self.cs)]
        dsts = [(None, n, 0) if c is None else (t.data_ptr(), n, n * H * W) for t, c, n in zip(outs, self.couts, self.sizes)]
        _, tk = self.ops.conv2d_auto_raw(srcs, None, self.wp, self.bias, dsts, B, H, W, 3, not self.dgrad, wino=(cache, self.what))
        return tk, [t for t, c in zip(outs, self.couts) if c is not None]

    def layout(self, B):
        L = pkg("_lib")
        return A.layout(L, self.ops._lib(), A.descriptor(L, B, self.cs, self.couts, self.dgrad, flags=self.ops._auto_flags(({}, self.what))))


def auto_entries(cache, head="auto"):
    return {k: v for k, v in cache.items() if isinstance(k, tuple) and k[0] == head}


@pytest.mark.parametrize("name", list(A.LAYERS))
def test_two_layouts_of_one_layer_coexist(dev, name):
    """B 4, B 8, B 4, B 8 on ONE cache: each plan transforms once, into a buffer of its own of exactly its floats, keyed by its layout; the other plan's calls
    leave that buffer at its address with its bits, and every output equals the same call on a fresh cache bit for bit."""
    layer = Layer(dev, name)
    cache, held = {}, {}      # held: B -> (entry, address, a clone of the buffer behind its transform)
    for step, B in enumerate((4, 8, 4, 8)):
        tk, outs = layer(B, cache)
        assert (tk.family, tk.variant, tk.nlaunch) == layer.plans[B], (name, step, B)
        assert tk.transformed == (1 if step < 2 else 0), (name, step, B)
        ents = auto_entries(cache)
        if step < 2:
            (key,) = set(ents) - {h[0] for h in held.values()}
            layout, floats = layer.layout(B)
            assert key == ("auto", layer.what, layout) and floats == layer.floats == ents[key].u.numel(), (name, B, key)
            held[B] = (key, ents[key].u.data_ptr(), ents[key].u.clone())
        assert len(ents) == min(step + 1, 2) and set(ents) == {h[0] for h in held.values()}, (name, step, list(ents))
        for b, (key, addr, kept) in held.items():      # (this plan's buffer and the other plan's: where they were, as they were)
            assert cache[key].u.data_ptr() == addr and same_bits(cache[key].u, kept), (name, step, b)
        tk_fresh, want = layer(B, {})
        assert tk_fresh.transformed == 1
        for got, ref in zip(outs, want):
            assert not bool(torch.isnan(ref).any()) and same_bits(got, ref), (name, step, B)


def test_a_captured_launch_survives_another_plan(dev):
    """[32] -> [32] at 128^2: an eager call at B 4, ONE more B 4 call captured (single stream; it transforms nothing -- a transform inside the graph would repair
    the buffer at every replay and hide the fault this test is for), an eager call at B 8 on the same cache, then the replay: the eager B 4 output, bit for bit."""
    layer = Layer(dev, "fwd_32_32")
    cache = {}
    tk, (eager,) = layer(4, cache)
    assert tk.transformed == 1 and tk.family == 3
    static = [torch.full((4, 32, H, W), float("nan"), device=dev)]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        tk_cap, _ = layer(4, cache, outs=static)
    assert tk_cap.transformed == 0 and tk_cap.family == 3
    tk8, (out8,) = layer(8, cache)
    assert tk8.transformed == 1 and tk8.family == 1 and len(auto_entries(cache)) == 2
    static[0].fill_(float("nan"))
    graph.replay()
    torch.cuda.synchronize()
    assert same_bits(static[0], eager)
    _, (want8,) = layer(8, {})
    assert same_bits(out8, want8)


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "relu_of"])
def test_the_up_convolution_form_shares_a_layout(dev, masked):
    """upconv_dgrad_raw (32 -> 16 at 64^2 -> 128^2) at B 12, 32, 8, 12 on ONE cache: as many entries as ynet_conv2d_auto_cache_layout has values for those
    batch sizes -- two, B 12 and B 32 share one --, the tables made once per entry, every dx bit-equal to the same call on a fresh cache."""
    ops, L = pkg("ops"), pkg("_lib")
    cout, cin, hw = A.UP_COUT, A.UP_CIN, A.UP_HW
    Bmax = max(A.UP_BATCHES)
    K = rnd(cout, cin, 3, 3, seed=11, scale=0.1).to(dev)
    D = rnd(Bmax, 4 * cout, hw, hw, seed=12).to(dev)
    gate = torch.relu(rnd(Bmax, cin, hw, hw, seed=13)).to(dev)

    def call(B, cache):
        dx = torch.full((B, cin, hw, hw), float("nan"), device=dev)
        return ops.upconv_dgrad_raw(D.data_ptr(), K, dx.data_ptr(), gate.data_ptr() if masked else None, B, cout, cin, hw, hw, cache), dx

    flags = ops._auto_flags(({}, "dgrad"))
    layouts = {B: A.layout(L, ops._lib(), A.up_descriptor(L, B, masked, flags=flags)) for B in set(A.UP_BATCHES)}
    assert layouts[12] == layouts[32] != layouts[8]
    cache, seen, transformed = {}, set(), []
    for B in A.UP_BATCHES:
        tk, dx = call(B, cache)
        transformed.append(tk.transformed)
        seen.add(layouts[B])
        ents = auto_entries(cache, "upconv_bwd")
        assert set(ents) == {("upconv_bwd", l_[0]) for l_ in seen} and all(ents[("upconv_bwd", l_[0])].u.numel() == l_[1] for l_ in seen), (B, list(ents))
        tk_fresh, want = call(B, {})
        assert tk_fresh.transformed == 1 and (tk_fresh.family, tk_fresh.variant, tk_fresh.nlaunch) == (tk.family, tk.variant, tk.nlaunch)
        assert not bool(torch.isnan(want).any()) and same_bits(dx, want), B
    assert transformed == [1, 0, 1, 0]
    assert len(auto_entries(cache, "upconv_bwd")) == len(set(layouts.values())) == 2

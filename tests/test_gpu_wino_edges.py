"""The Winograd convolution kernels at every plan edge (tests/_wino_cases.py has the rows, the inputs and the fp64 references; tests/test_wino_cases_host.py shows on
the CPU that every row plans what it claims, sits at its size gate and reaches the edge it names).

The library is called directly, so the test owns every buffer: sources, relu_of and addend lie in NaN-poisoned buffers with 8 floats of slack between images (a read past
an image that reaches arithmetic poisons the result), one source of a `slice` row is a channel slice of a wider NaN tensor (4 planes in front, 1 behind: a descriptor that
spans too many planes reads NaN), a `shared` source is one image with batch stride 0; every destination, the pooled copy, the code bytes (poison 255), the word tensor
(poison -1) and the filter cache -- exactly ynet_conv2d_auto_cache_floats floats and a guard -- are poisoned with slack around them.  Per row and input family: `taken`
equals the plan; family (a) (normal inputs) meets the project's tolerance against fp64 (forward: rtol 1e-5, atol max(2e-5, 2e-6 of the largest reference); data gradients:
TOL_DX), family (b) (exact integers) matches the reference bit for bit with nothing excluded -- outputs, pooled copy, pool codes, the word-gated gradient; a second call
with the same cache transforms nothing and repeats every bit; no slack, guard, unwanted destination or input changes.  The 1-bit words are private to the tiling: they are
checked through their consumer, a 32 -> 32 data gradient gated by them whose relu_of points at NaN.

Measured on the MI355X: the 118 cases take 15 s (tests/test_gpu_kernels.py: 61 s for 313), most of it the fp64 references on the CPU; no row failed on the unedited
kernels.  Largest family (a) error per kernel family, each against a bound of 2e-5 + rtol |want| (the 2e-6-of-the-largest-output term never exceeds 2e-5 here):
  conv_wino_kernel        forward 1.84e-6 (fwd_words), data gradient 1.72e-6 (dgrad_split48_s2d), word-gated gradient 1.67e-6 (cat_words_40)
  conv_wino_cat_kernel    forward 2.01e-6 (cat_words_41)
  conv_wino16_kernel      forward 2.10e-6 (w16_43_128_outputs), data gradient 2.05e-6 (w16_dgrad_32_64)
  conv_wino_up_kernel     7.61e-7 (up_single_tiles)        conv_wino16_up_kernel   1.14e-6 (up16_84_16)

What a broken kernel looks like here (each an edit of csrc/conv_wino.hip or csrc/conv_auto.cpp on a scratch copy that changes values only and keeps every address inside its
buffer, built alone and run once against this file -- the first seven against the 57 rows it had before the last edit added two; both input families of every row named
failed, every other row passed):
  * the right-edge bit of em dropped in conv_wino_kernel's stager      -> all 14 rows of family 1, and the 5 rows of family 2 with a conv_wino_kernel launch (variant 40's
                                                                           first launch: cat40_32_28, cat40_56_1, cat40_88, cat_words_40; the word consumer of cat_words_41)
  * the same in conv_wino_cat_kernel's stager                          -> all 18 rows with a conv_wino_cat_kernel launch (cat_direct_single_8 included), nothing else
  * the same in conv_wino16_kernel's stager                            -> all 18 rows with a slice-form launch (dgrad_16_64_slice_form included), nothing else
  * conv_wino16_kernel: bias[slice * 16 + ...] -> bias[...]            -> the 12 slice-form rows with a bias and more than one slice (w16_5_16, w16_pooled, w16_for_16 have one
                                                                           slice, the data gradients no bias)
  * conv_wino16_kernel: the addend's image b % aux_bmod -> b where b < aux_bmod, else 0 (b itself would leave the addend's buffer)   -> w16_addend_mod4
  * make_plan: row0 of variant 43's second launch -> 0                 -> the 5 variant-43 rows (w16_cat_single_tiles, w16_43_row0_30, w16_43_cut_2, w16_43_at_128, w16_43_128_outputs)
  * the pool code's arg-max: row1[0] > mx -> >=                         -> cat_pool_code (family (a) too: a block of four zeros behind the ReLU then names element 2)
  * conv_wino16_kernel: tile_end without the min(a.ntiles, ...), the tile index clamped to the last tile instead (an XCD's spare steps recompute tile ntiles - 1)
                                                                        -> w16_43_41_tiles alone: recomputing a tile writes the same values again EXCEPT where the launch adds onto
                                                                           its own destination (variants 40 / 43).  The issue's rows could not see this edit; w16_43_41_tiles and
                                                                           cat40_257_tiles were added for it."""
import ctypes

import pytest
import torch

import _align_cases as A
import _wino_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096            # floats behind the filter cache, words / bytes around the word and code tensors
TOL_FWD = dict(rtol=1e-5, atol=2e-5, scale_rel=2e-6)      # test_winograd_convolution_matches_the_direct_form's bound


def _poisoned(n, dev):
    return torch.full((n,), NAN, device=dev, dtype=torch.float32)


def _all_poison(t):
    want = A.bits(torch.full((1,), NAN, dtype=torch.float32, device=t.device))
    return bool((A.bits(t) == want).all())


class _Guarded:
    """n elements of an integer type between two guards, all holding `poison`."""

    def __init__(self, n, dtype, poison, dev):
        self.n, self.poison = n, poison
        self.buf = torch.full((n + 2 * GUARD,), poison, dtype=dtype, device=dev)
        self.body = self.buf[GUARD:GUARD + n]
        assert self.body.data_ptr() % 16 == 0

    def refill(self):
        self.buf.fill_(self.poison)

    def intact(self):
        return bool((self.buf[:GUARD] == self.poison).all()) and bool((self.buf[GUARD + self.n:] == self.poison).all())


class _Row:
    """The device buffers of one row and family, and its calls."""

    def __init__(self, ops, L, name, family, dev):
        self.ops, self.L, self.lib, self.name, self.dev = ops, L, ops._lib(), name, dev
        self.c = c = C.case(name)
        self.inp = inp = C.inputs(name, family)
        B, H, W, o = c["B"], c["H"], c["W"], c["opts"]
        self.inputs, src = [], []
        for i, (x, n) in enumerate(zip(inp.xs, c["cs"])):
            if o.get("slice") == i:
                wide = torch.full((x.shape[0], C.LEAD + n + C.TRAIL, *x.shape[2:]), NAN)
                wide[:, C.LEAD:C.LEAD + n] = x
                v, buf = A.offset_view(wide.to(dev), 0, C.PAD)
                v = v[:, C.LEAD:C.LEAD + n]
            else:
                v, buf = A.offset_view(x.to(dev), 0, C.PAD)
            assert torch.equal(v.cpu(), x) and (x.shape[0] == B) != (o.get("shared") == i)
            self.inputs.append(buf)
            src.append((v.data_ptr(), 0 if o.get("shared") == i else v.stride(0)))      # (stride 0: one image for the whole batch)
        self.wp = ops.pack_weight(inp.w.to(dev), c["mode"])
        self.bias = inp.bias.to(dev) if inp.bias is not None else None
        self.inputs += [self.wp] + ([self.bias] if self.bias is not None else [])
        self.P = P = dict(src=src, wp=self.wp.data_ptr(), bias=self.bias.data_ptr() if self.bias is not None else None)
        # destinations: (view, buffer, shape of the buffer's tensor) or None for an unwanted one, which keeps a poisoned tensor nobody may touch
        self.dsts, P["dst"] = [], []
        for n, w in zip(c["sizes"], c["couts"]):
            first, total = o.get("dst_in", (0, n))
            v, buf = A.offset_view(torch.full((B, total, H, W), NAN, device=dev), 0, C.PAD)
            self.dsts.append((v[:, first:first + n], v, buf, (B, total, H, W), w is not None))
            P["dst"].append((v[:, first:first + n].data_ptr(), v.stride(0)) if w is not None else (None, 0))
        ctot = sum(c["sizes"])
        self.act = self.addend = self.pooled = self.code = self.words = None
        if inp.act is not None:
            self.act, buf = A.offset_view(inp.act.to(dev), 0, C.PAD)
            self.inputs.append(buf)
            P["relu_of"] = (self.act.data_ptr(), self.act.stride(0))
        if inp.addend is not None:
            self.addend, buf = A.offset_view(inp.addend.to(dev), 0, C.PAD)
            self.inputs.append(buf)
            P["addend"] = (self.addend.data_ptr(), self.addend.stride(0))
        if o.get("pooled"):
            v, buf = A.offset_view(torch.full((B, ctot, H // 2, W // 2), NAN, device=dev), 0, C.PAD)
            self.pooled = (v, buf)
            P["pooled"] = (v.data_ptr(), v.stride(0))
        if o.get("pool_code"):
            self.code = _Guarded(B * ctot * (H // 2) * (W // 2), torch.uint8, 255, dev)
            P["pool_code"] = self.code.body.data_ptr()
        if o.get("words"):
            n_words = self.lib.ynet_winograd_relu_bits_words(B, H, W)
            assert n_words > 0
            self.words = _Guarded(n_words, torch.int32, -1, dev)
            P["wbits_out"] = self.words.body.data_ptr()
        self.snaps = [b.clone() for b in self.inputs]
        if c["entry"] == "auto":
            self.d = C.make_desc(L, name, P)
            self.need = self.lib.ynet_conv2d_auto_cache_floats(ctypes.byref(self.d))
            assert self.need > 0, self.lib.ynet_last_error()
            self.tag = (ctypes.c_ulonglong * 2)(0, 0)
            self.cache = _poisoned(self.need + GUARD, dev)
            self.d.cache, self.d.cache_floats, self.d.cache_tag, self.d.wp_version = self.cache.data_ptr(), self.need, self.tag, 1
        else:
            self.arr = (ctypes.c_int * len(c["cs"]))(*c["cs"])
            self.need = self.lib.ynet_winograd_filter_cat_floats(self.arr, len(c["cs"]), 32)
            self.cache = _poisoned(self.need + GUARD, dev)

    def repoison(self):
        for _, _, buf, _, _ in self.dsts:
            buf.fill_(NAN)
        if self.pooled is not None:
            self.pooled[1].fill_(NAN)
        for g in (self.code, self.words):
            if g is not None:
                g.refill()

    def call(self, first):
        """One call -> YnetConvTaken (None for a direct entry)."""
        ops, lib, c = self.ops, self.lib, self.c
        if c["entry"] == "auto":
            tk = self.L.ConvTaken()
            rc = lib.ynet_conv2d_auto(ctypes.byref(self.d), ctypes.byref(tk), ops._stream())
            assert rc == 0, lib.ynet_last_error()
            torch.cuda.synchronize()
            return tk
        if first:
            assert lib.ynet_winograd_filter_cat(self.wp.data_ptr(), self.cache.data_ptr(), self.arr, len(c["cs"]), 32, 0, 32, ops._stream()) == 0, lib.ynet_last_error()
        sp, sc, sb = ops._arrays([(p, n, bs) for (p, bs), n in zip(self.P["src"], c["cs"])])
        (p, bs), = self.P["dst"]
        rc = lib.ynet_conv2d_winograd_cat(sp, sc, sb, len(c["cs"]), self.cache.data_ptr(), self.P["bias"], p, bs, 32, c["B"], c["H"], c["W"], int(c["relu"]), ops._stream())
        assert rc == 0, lib.ynet_last_error()
        torch.cuda.synchronize()
        return None

    def outputs(self):
        """Clones of everything the call writes."""
        out = [v.clone() for v, _, _, _, _ in self.dsts]
        if self.pooled is not None:
            out.append(self.pooled[0].clone())
        for g in (self.code, self.words):
            if g is not None:
                out.append(g.body.clone())
        return out

    def nothing_else_changed(self):
        name = self.name
        for (v, full, buf, shape, wanted), n in zip(self.dsts, self.c["sizes"]):
            assert A.slack_intact(buf, shape, 0, C.PAD), f"{name}: written around a destination"
            if not wanted:
                assert _all_poison(buf), f"{name}: the unwanted destination was written"
            elif shape[1] != n:      # a slice of a wider tensor: the other channels
                first = self.c["opts"]["dst_in"][0]
                assert _all_poison(full[:, :first]) and _all_poison(full[:, first + n:]), f"{name}: written outside the destination's channels"
        if self.pooled is not None:
            assert A.slack_intact(self.pooled[1], tuple(self.pooled[0].shape), 0, C.PAD), f"{name}: written around the pooled copy"
        for g, what in ((self.code, "code bytes"), (self.words, "words")):
            assert g is None or g.intact(), f"{name}: written around the {what}"
        assert _all_poison(self.cache[self.need:]), f"{name}: written behind the filter cache's {self.need} floats"
        assert all(A.same_bits(b, s) if b.dtype == torch.float32 else torch.equal(b, s) for b, s in zip(self.inputs, self.snaps)), f"{name}: an input buffer changed"

    def gated_gradient(self):
        """The consumer of the words: dx = conv^T(dy2, w2) gated by them (conv_wino_kernel, EM 2).  relu_of -- which the dispatcher wants beside the words -- is all NaN:
        a launch that read the float activation instead would write zeros everywhere."""
        ops, lib, L, c, dev = self.ops, self.lib, self.L, self.c, self.dev
        B, H, W = c["B"], c["H"], c["W"]
        dy, dybuf = A.offset_view(self.inp.dy2.to(dev), 0, C.PAD)
        wp2 = ops.pack_weight(self.inp.w2.to(dev), 1)
        act, _ = A.offset_view(torch.full((B, 32, H, W), NAN, device=dev), 0, C.PAD)
        dx, dxbuf = A.offset_view(torch.full((B, 32, H, W), NAN, device=dev), 0, C.PAD)
        d = C.gate_desc(L, B, H, W, P=dict(src=(dy.data_ptr(), dy.stride(0)), dst=(dx.data_ptr(), dx.stride(0)), wp=wp2.data_ptr(), relu_of=(act.data_ptr(), act.stride(0)),
                                           relu_wbits=self.words.body.data_ptr()))
        need = lib.ynet_conv2d_auto_cache_floats(ctypes.byref(d))
        cache, tag, tk = _poisoned(need + GUARD, dev), (ctypes.c_ulonglong * 2)(0, 0), L.ConvTaken()
        d.cache, d.cache_floats, d.cache_tag, d.wp_version = cache.data_ptr(), need, tag, 1
        words = self.words.body.clone()
        assert lib.ynet_conv2d_auto(ctypes.byref(d), ctypes.byref(tk), ops._stream()) == 0, lib.ynet_last_error()
        torch.cuda.synchronize()
        assert (tk.family, tk.variant, tk.nlaunch, tk.tmpl[0][2]) == (1, 21, 1, 2), (self.name, tk.family, tk.variant, tk.nlaunch, tk.tmpl[0][2])
        assert A.slack_intact(dxbuf, (B, 32, H, W), 0, C.PAD) and _all_poison(cache[need:]) and torch.equal(words, self.words.body) and self.words.intact()
        assert A.same_bits(dy, self.inp.dy2.to(dev))
        return dx


def _compare(name, family, what, got, want, tol, keep=None):
    """Family (b): every bit.  Family (a): the tolerance, outside `keep`'s complement where a gate is ambiguous."""
    assert bool(torch.isfinite(got).all()), f"{name} {what}: not finite"
    if family == "b":
        w32 = want.float()
        assert A.same_bits(got, w32), f"{name} {what}: exact-integer inputs, {int((got != w32).sum())} elements differ, largest {float((got - w32).abs().max())}"
        return
    if keep is not None:
        got, want = got[keep], want[keep]
    bad, err, atol = A.mismatch(got, want, **tol)
    print(f"{name} {what}: largest error {err:.3g} (bound {atol:.3g} + {tol['rtol']:g} |want|)")
    assert bad == 0, f"{name} {what}: {bad} elements beyond the tolerance, largest error {err:.3g}"


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_winograd_convolution_at_a_plan_edge(dev, name, family):
    ops, L = pkg("ops"), pkg("_lib")
    c = C.case(name)
    o, B, H, W = c["opts"], c["B"], c["H"], c["W"]
    r = _Row(ops, L, name, family, dev)
    if c["entry"] == "auto":
        assert C.plan_of(r.lib, L, r.d) == c["plan"], name
    ref = C.ref64(name, family)
    tol = A.TOL_DX if c["mode"] == 1 else TOL_FWD

    tk = r.call(True)
    if tk is not None:
        assert (tk.family, tk.variant, tk.nlaunch) == c["plan"], (name, tk.family, tk.variant, tk.nlaunch)
        assert tk.transformed == 1 and tk.wrote_s2d == (1 if o.get("s2d") else 0) and tk.wrote_wbits == int(bool(o.get("words"))) and tk.wrote_pool_code == int(bool(o.get("pool_code")))
    want_y = ref["y"].to(dev)
    c0 = 0
    for i, ((v, _, _, _, wanted), n) in enumerate(zip(r.dsts, c["sizes"])):
        if wanted:
            want = want_y[:, c0:c0 + n]
            got = v
            if o.get("s2d") and o["s2d"][i]:      # written space-to-depth: the same numbers, rearranged
                want, got = C.s2d(want.contiguous()), v.view(B, 4 * n, H // 2, W // 2)
            _compare(name, family, f"destination {i}", got, want, tol)
        c0 += n
    el, blk = C.ambiguous(name, ref)
    if family == "a":      # the exclusion cap, on the row's own numbers
        assert el is None or float(el.float().mean()) <= 1e-3, name
        assert blk is None or float(blk.float().mean()) <= 1e-3, name
    else:
        el = blk = None      # nothing is excluded
    if r.pooled is not None:
        _compare(name, family, "pooled copy", r.pooled[0], ref["pooled"].to(dev), TOL_FWD)
    if r.code is not None:
        got, want = r.code.body.view(B, 32, H // 2, W // 2).cpu(), ref["code"]
        if family == "b":
            assert torch.equal(got, want), f"{name} pool code: {int((got != want).sum())} codes differ"
        else:
            sure = ~blk
            assert torch.equal((got & 3)[sure], (want & 3)[sure]), f"{name} pool code: arg-max differs outside the ambiguous blocks"
            pos_g = torch.stack([(got >> (2 + k)) & 1 for k in range(4)], -1)
            pos_w = torch.stack([(want >> (2 + k)) & 1 for k in range(4)], -1)
            keep = ~C.blocks(el)
            assert torch.equal(pos_g[keep], pos_w[keep]) and bool((got < 64).all()), f"{name} pool code: positive bits differ outside the ambiguous elements"
    dx = None
    if r.words is not None:
        dx = r.gated_gradient()
        _compare(name, family, "word-gated gradient", dx, ref["gated"].to(dev), A.TOL_DX, keep=None if el is None else ~el.to(dev))

    # a second call with the same cache: no transform, every bit again (into re-poisoned outputs)
    first = r.outputs()
    r.repoison()
    tk2 = r.call(False)
    assert tk2 is None or (tk2.transformed == 0 and (tk2.family, tk2.variant, tk2.nlaunch) == c["plan"]), name
    for a_, b_ in zip(first, r.outputs()):
        assert torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(b_, nan=12345.0)) if a_.dtype == torch.float32 else torch.equal(a_, b_), f"{name}: the second call differs"
    r.nothing_else_changed()

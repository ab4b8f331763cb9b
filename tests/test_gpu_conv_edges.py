"""The direct convolution kernels (csrc/conv_mfma.hip) at every plan edge (tests/_conv_cases.py has the rows, the inputs and the fp64 references; tests/test_conv_cases_host.py
shows on the CPU that every row launches what it claims, sits at its gate and reaches the edges it names).

The library is called through its C ABI, so the test owns every buffer: sources, mask, relu_of and addend lie in NaN-poisoned buffers with 8 floats of slack between images,
a `slice` source is a channel slice of a wider NaN tensor (a kernel that relied on zero filter rows instead of the range check for the channels past a source's end would
bring 0 x NaN into the output), a shared source has batch stride 0 or a batch modulus; every destination, the pooled copy, the workspace (exactly the floats the call is told
of, and a guard) and the 1-bit words (poison -1) are poisoned with slack around them.  Per row and input family: the call succeeds; ynet_conv2d_last_launch(0) is the claim,
and for an aligned plain row ynet_conv2d_plan names the same rows, tile count, generation, fold and chunk depth; family (a) (normal inputs) meets the project's tolerances
against fp64 (A.TOL_Y forward, A.TOL_DX for data gradients), family (b) (exact integers) matches the reference bit for bit -- outputs, pooled copy, the gradient gated by the
1-bit words, which must also equal the float relu_of form of the same data --; no slack, guard, unwanted destination or input changes.

Measured on the MI355X: the 238 cases take 10 s (the slowest, r4_t1, 1.0 s), most of it the fp64 references on the CPU; no row failed on the unedited kernels.

What a broken library looks like here (edits of csrc/conv_mfma.hip on a scratch copy that change values only and keep every address inside its buffer, built once and run once
against the 234 cases this file had before the planted pool rows; 116 failed, every other case passed):
  * set_goff's quad form (the per-channel DMA items): gx < W -> gx + 4 < W, the last quad of every image row reads as zero
        -> both families of all 37 rows with a chunk depth of 4 on the LDS-DMA tiles (folded three / four tiles included), mask_large under its planted NaNs and the
           planted add_t4_ragged; no row of the flat-item small tiles, the register-staged tiles or the streaming kernel
  * conv_split_reduce_kernel: bias[co] -> bias[0]    -> both families of the 11 rows that split the channel loop and have a bias, and the planted ks_uneven
  * conv_emask_kernel: emask > 0 -> emask >= 0       -> relu_of_1x1, relu_of_5x5, relu_of_reg, relu_of_fold, ks_reg_relu_of (the five rows whose mask is a pass of its own)
  * ynet_conv2d_pool without its shape check         -> the five pool_* refusals: the plain kernel had written the destination and noted its launch before the call failed"""
import copy
import ctypes

import pytest
import torch

import _align_cases as A
import _conv_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096            # floats behind the workspace, words around the word tensor


def _all_poison(t):
    want = A.bits(torch.full((1,), NAN, dtype=torch.float32, device=t.device))
    return bool((A.bits(t) == want).all())


class _Op:
    """One operand in a poisoned buffer: .v the view, .buf the flat buffer, .at its (off, pad), .shape the shape of the tensor the buffer holds."""

    def __init__(self, t, dev, at=(0, C.PAD)):
        self.at, self.shape = at, tuple(t.shape)
        self.v, self.buf = A.offset_view(t.to(dev), *at)
        self.full = self.v

    def intact(self):
        return A.slack_intact(self.buf, self.shape, *self.at)


class _Row:
    """The device buffers of one row and its calls."""

    def __init__(self, name, inp, dev):
        self.ops, self.L = pkg("ops"), pkg("_lib")
        self.lib, self.name, self.dev, self.inp = self.ops._lib(), name, dev, inp
        self.c = c = C.case(name)
        B, H, W, o = c["B"], c["H"], c["W"], c["opts"]
        place = dict([o["place"]]) if "place" in o else {}
        self.inputs, self.src = [], []
        for i, (x, n) in enumerate(zip(inp.xs, c["cs"])):
            at = place.get(f"src{i}", (0, C.PAD))
            if o.get("slice") == i:
                wide = torch.full((x.shape[0], C.LEAD + n + C.TRAIL, H, W), NAN)
                wide[:, C.LEAD:C.LEAD + n] = x
                op = _Op(wide, dev, at)
                op.v = op.v[:, C.LEAD:C.LEAD + n]
            else:
                op = _Op(x, dev, at)
            m = o.get("shared", {}).get(i)
            assert x.shape[0] == C.images(c, i) and torch.equal(torch.nan_to_num(op.v.cpu(), nan=7.0), torch.nan_to_num(x, nan=7.0))
            self.inputs.append(op.buf)
            self.src.append((op.v.data_ptr(), n, 0 if m == 0 else op.v.stride(0), m or 0))
        self.wp = self.ops.pack_weight(inp.w.to(dev), c["mode"])
        self.bias = inp.bias.to(dev) if inp.bias is not None else None
        self.inputs += [self.wp] + ([self.bias] if self.bias is not None else [])
        self.dsts = []
        for i, (n, w) in enumerate(zip(c["sizes"], c["couts"])):
            first, total = o.get("dst_in", (0, n)) if i == 0 else (0, n)
            op = _Op(torch.full((B, total, H, W), NAN), dev, place.get(f"dst{i}", (0, C.PAD)))
            op.v, op.first, op.wanted = op.full[:, first:first + n], first, w is not None
            self.dsts.append(op)
        self.mask = self.act = self.addend = self.pooled = self.words = self.ws = None
        if inp.mask is not None:
            self.mask = _Op(inp.mask, dev, place.get("mask", (0, C.PAD)))
            self.inputs.append(self.mask.buf)
        if inp.act is not None:
            self.act = _Op(inp.act, dev)
            self.inputs.append(self.act.buf)
        if inp.addend is not None:
            self.addend = _Op(inp.addend, dev)
            self.inputs.append(self.addend.buf)
        if c["entry"] == "pool":
            self.pooled = _Op(torch.full((B, c["ctot"], H // 2, W // 2), NAN), dev)
        if c["entry"] == "bits":
            self.n_words = self.lib.ynet_conv2d_relu_bits_words(B, H, W, c["ctot"], c["K"])
            assert self.n_words > 0
            self.words = torch.full((self.n_words + 2 * GUARD,), -1, dtype=torch.int32, device=dev)
        self.ws_floats = C.ws_of(c)
        if self.ws_floats > 0:
            self.ws = torch.full((self.ws_floats + GUARD,), NAN, device=dev)
            assert self.ws.data_ptr() % 16 == 0
        self.snaps = [b.clone() for b in self.inputs]

    def _src_arrays(self):
        sp, sc, sb = self.ops._arrays([s[:3] for s in self.src])
        bm = (ctypes.c_int * len(self.src))(*[s[3] for s in self.src]) if any(s[3] for s in self.src) else None
        return sp, sc, sb, bm

    def call(self):
        """The row's call -> (status, what ynet_conv2d_last_launch(0) reports after it)."""
        lib, c, st = self.lib, self.c, self.ops._stream()
        B, H, W, K, relu = c["B"], c["H"], c["W"], c["K"], int(c["relu"])
        sp, sc, sb, bm = self._src_arrays()
        bias = self.bias.data_ptr() if self.bias is not None else None
        mask = (self.mask.v.data_ptr(), self.mask.v.stride(0)) if self.mask is not None else (None, 0)
        ws = (self.ws.data_ptr(), self.ws_floats) if self.ws is not None else (None, 0)
        d0 = self.dsts[0].v
        lib.ynet_conv2d_last_launch(0)
        if c["entry"] == "conv":
            dp, dc, db = self.ops._arrays([(d.v.data_ptr() if d.wanted else None, n, d.v.stride(0)) for d, n in zip(self.dsts, c["sizes"])])
            rc = lib.ynet_conv2d(sp, sc, sb, bm, len(self.src), *mask, self.wp.data_ptr(), bias, dp, dc, db, len(self.dsts), B, H, W, K, relu, *ws, st)
        elif c["entry"] == "dgrad_relu":
            p, n, bs, _ = self.src[0]
            rc = lib.ynet_conv2d_dgrad_relu(p, n, bs, *mask, self.wp.data_ptr(), d0.data_ptr(), c["ctot"], d0.stride(0), self.act.v.data_ptr(), self.act.v.stride(0), B, H, W, K, *ws, st)
        elif c["entry"] == "pool":
            rc = lib.ynet_conv2d_pool(sp, sc, sb, len(self.src), self.wp.data_ptr(), bias, d0.data_ptr(), c["ctot"], d0.stride(0), self.pooled.v.data_ptr(), self.pooled.v.stride(0),
                                      B, H, W, K, relu, st)
        elif c["entry"] == "add":
            rc = lib.ynet_conv2d_add(sp, sc, sb, bm, len(self.src), self.wp.data_ptr(), bias, d0.data_ptr(), c["ctot"], d0.stride(0), B, H, W, K, relu,
                                     self.addend.v.data_ptr(), self.addend.v.stride(0), c["opts"]["addend"], st)
        else:
            rc = lib.ynet_conv2d_relu_bits(sp, sc, sb, len(self.src), self.wp.data_ptr(), bias, d0.data_ptr(), c["ctot"], d0.stride(0), self.words[GUARD:].data_ptr(), B, H, W, K, st)
        msg = lib.ynet_last_error()
        torch.cuda.synchronize()
        assert rc == 0, (self.name, msg)
        return lib.ynet_conv2d_last_launch(0)

    def gated_gradients(self):
        """The consumer of the words, dx = bit ? conv^T(dy2 [masked], w2) : 0, and the float relu_of form of the same data (relu_of: the row's own output on the device)
        -> (dx by the words, dx by relu_of, the two launch notes)."""
        lib, c, dev, inp, st = self.lib, self.c, self.dev, self.inp, self.ops._stream()
        B, H, W, K, n = c["B"], c["H"], c["W"], c["K"], c["opts"]["dy"]
        dy, wp2 = _Op(inp.dy2, dev), self.ops.pack_weight(inp.w2.to(dev), 1)
        dm = _Op(inp.dmask, dev) if inp.dmask is not None else None
        mask = (dm.v.data_ptr(), dm.v.stride(0)) if dm is not None else (None, 0)
        words, y = self.words.clone(), self.dsts[0].v
        out, notes = [], []
        for form in ("bits", "relu_of"):
            dx = _Op(torch.full((B, c["ctot"], H, W), NAN), dev)
            lib.ynet_conv2d_last_launch(0)
            if form == "bits":
                rc = lib.ynet_conv2d_dgrad_relu_bits(dy.v.data_ptr(), n, dy.v.stride(0), *mask, wp2.data_ptr(), dx.v.data_ptr(), c["ctot"], dx.v.stride(0), self.words[GUARD:].data_ptr(),
                                                     B, H, W, K, st)
            else:
                rc = lib.ynet_conv2d_dgrad_relu(dy.v.data_ptr(), n, dy.v.stride(0), *mask, wp2.data_ptr(), dx.v.data_ptr(), c["ctot"], dx.v.stride(0), y.data_ptr(), y.stride(0),
                                                B, H, W, K, None, 0, st)
            msg = lib.ynet_last_error()
            torch.cuda.synchronize()
            assert rc == 0, (self.name, form, msg)
            notes.append(lib.ynet_conv2d_last_launch(0))
            assert dx.intact() and torch.equal(words, self.words), (self.name, form)
            out.append(dx.v)
        assert A.same_bits(dy.v, inp.dy2.to(dev)) and dy.intact() and (dm is None or (A.same_bits(dm.v, inp.dmask.to(dev)) and dm.intact()))
        return out[0], out[1], notes

    def nothing_else_changed(self):
        name = self.name
        for d, n in zip(self.dsts, self.c["sizes"]):
            assert d.intact(), f"{name}: written around a destination"
            if not d.wanted:
                assert _all_poison(d.buf), f"{name}: the unwanted destination's stand-in was written"
            elif d.shape[1] != n:      # a slice of a wider tensor: the other channels
                assert _all_poison(d.full[:, :d.first]) and _all_poison(d.full[:, d.first + n:]), f"{name}: written outside the destination's channels"
        assert self.pooled is None or self.pooled.intact(), f"{name}: written around the pooled copy"
        if self.words is not None:
            assert bool((self.words[:GUARD] == -1).all()) and bool((self.words[GUARD + self.n_words:] == -1).all()), f"{name}: written around the words"
        assert self.ws is None or _all_poison(self.ws[self.ws_floats:]), f"{name}: written behind the workspace's {self.ws_floats} floats"
        assert all(A.same_bits(b, s) for b, s in zip(self.inputs, self.snaps)), f"{name}: an input buffer changed"


def _compare(name, family, what, got, want, tol):
    """Family (b): every bit.  Family (a): the tolerance."""
    assert bool(torch.isfinite(got).all()), f"{name} {what}: not finite"
    if family == "b":
        w32 = want.float()
        assert A.same_bits(got, w32), f"{name} {what}: exact-integer inputs, {int((got != w32).sum())} elements differ, largest {float((got - w32).abs().max())}"
        return
    bad, err, atol = A.mismatch(got, want, **tol)
    print(f"{name} {what}: largest error {err:.3g} (bound {atol:.3g} + {tol['rtol']:g} |want|)")
    assert bad == 0, f"{name} {what}: {bad} elements beyond the tolerance, largest error {err:.3g}"


def _check_outputs(r, family, ref, tol):
    c, dev = r.c, r.dev
    want_y, c0 = ref["y"].to(dev), 0
    for i, (d, n) in enumerate(zip(r.dsts, c["sizes"])):
        if d.wanted:
            _compare(r.name, family, f"destination {i}", d.v, want_y[:, c0:c0 + n], tol)
        c0 += n
    if r.pooled is not None:
        _compare(r.name, family, "pooled copy", r.pooled.v, ref["pooled"].to(dev), tol)


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_convolution_at_a_plan_edge(dev, name, family):
    c = C.case(name)
    kind, rows, ksplit, vl, vs, tiles, cc = c["claim"]
    r = _Row(name, C.inputs(name, family), dev)
    ref = C.ref64(name, family)
    tol = A.TOL_DX if c["mode"] == 1 else A.TOL_Y

    got = r.call()
    assert got == C.note(kind, rows, ksplit, vl, vs), (name, hex(got), hex(C.note(kind, rows, ksplit, vl, vs)))
    if c["entry"] == "conv" and "mask" not in c["opts"] and "place" not in c["opts"] and kind != C.STREAM:      # the plan mirror: what bench.py names the kernel by
        word = r.lib.ynet_conv2d_plan(c["B"], c["H"], c["W"], c["cout"], c["K"])
        assert (word & 255, word >> 17 & 1, word >> 19 & 3 != 0) == (got >> 4 & 15, int(got & 15 in (C.DMA, C.FOLDED)), got & 15 == C.FOLDED), (name, hex(word), hex(got))
        assert (word >> 8 & 255, word >> 21) == (tiles, cc), (name, hex(word))
    _check_outputs(r, family, ref, tol)
    if c["entry"] == "bits":
        by_words, by_floats, notes = r.gated_gradients()
        assert notes == [C.note(kind, rows, 1, 1, 1)] * 2, (name, [hex(n) for n in notes])
        _compare(name, family, "gradient gated by the words", by_words, ref["gated"].to(dev), A.TOL_DX)
        _compare(name, family, "gradient gated by relu_of", by_floats, ref["gated"].to(dev), A.TOL_DX)
        if family == "b":
            assert A.same_bits(by_words, by_floats), name
    r.nothing_else_changed()


def _non_finite_as(name, got, want, tol):
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(torch.isposinf(got), torch.isposinf(want)) and torch.equal(torch.isneginf(got), torch.isneginf(want)), \
        f"{name}: NaN / inf in other places than the reference's"
    fin = torch.isfinite(want)
    bad, err, _ = A.mismatch(got[fin], want[fin], **tol)
    assert bad == 0, f"{name}: {bad} finite elements beyond the tolerance, largest error {err:.3g}"


@pytest.mark.parametrize("value", [NAN, float("inf")])
@pytest.mark.parametrize("name", list(C.PLANTED))
def test_a_planted_nan_or_inf_reaches_its_neighbourhood_only(dev, name, value):
    """One NaN / +inf in one source pixel: the reference works on the same data; the value reaches exactly the K x K neighbourhood's outputs, in every wanted channel.
    A pool row (rows 2 and rows 4 on a ragged map, the pixel on the corner of four tiles and of four 2 x 2 blocks): the pooled copy is NaN in exactly the four blocks the
    neighbourhood touches -- the rule the header states, the block's maximum, NaN where any of its four elements is -- and within tolerance elsewhere.  The same call plants
    a TIE: the source is zero around one other block, so its four outputs are all the bias and the pooled element must be relu(bias), bit for bit."""
    c = C.case(name)
    b, ch, y, x = C.PLANTED[name]
    pool = c["entry"] == "pool"
    inp = copy.copy(C.inputs(name, "a"))
    inp.xs = [t.clone() for t in inp.xs]
    inp.xs[0][b, ch, y, x] = value
    if pool:
        assert len(inp.xs) == 1 and inp.bias is not None and min(y, x) >= 8
        inp.xs[0][b, :, 1:5, 1:5] = 0.0      # the block of rows 2 .. 3, columns 2 .. 3 sees zeros only
    ref = C.reference(name, inp)
    k = c["K"] // 2
    hood = torch.zeros(c["B"], 1, c["H"], c["W"], dtype=torch.bool)
    hood[b, :, max(0, y - k):y + k + 1, max(0, x - k):x + k + 1] = True
    if value != value or not c["relu"]:
        assert torch.equal(~torch.isfinite(ref["y"]), hood.expand_as(ref["y"])), name      # (without a ReLU -inf stays)
    else:      # behind a ReLU -inf is 0: every output of the neighbourhood is +inf or 0, both occur, nothing else is touched
        bad = ~torch.isfinite(ref["y"])
        assert bool((bad <= hood).all()) and bool(torch.isposinf(ref["y"][bad]).all()) and bool((ref["y"][hood.expand_as(bad) & ~bad] == 0).all()) and 0 < int(bad.sum()) < 9 * c["ctot"], name
    if pool:
        blocks = torch.nn.functional.max_pool2d(hood.float(), 2, 2) > 0
        assert int(blocks.sum()) == 4 and torch.equal(torch.isnan(ref["pooled"]), blocks.expand_as(ref["pooled"]) & (value != value)), name
        tie = torch.relu(inp.bias).double()
        assert torch.equal(ref["y"][b, :, 2:4, 2:4], tie.view(-1, 1, 1).expand(-1, 2, 2)) and torch.equal(ref["pooled"][b, :, 1, 1], tie), name
    r = _Row(name, inp, dev)
    kind, rows, ksplit, vl, vs, _, _ = c["claim"]
    assert r.call() == C.note(kind, rows, ksplit, vl, vs)
    c0 = 0
    for d, n in zip(r.dsts, c["sizes"]):
        if d.wanted:
            _non_finite_as(name, d.v, ref["y"][:, c0:c0 + n].to(dev), A.TOL_Y)
        c0 += n
    if pool:
        _non_finite_as(name + " pooled copy", r.pooled.v, ref["pooled"].to(dev), A.TOL_Y)
        assert A.same_bits(r.pooled.v[b, :, 1, 1], torch.relu(inp.bias).to(dev)) and A.same_bits(r.dsts[0].v[b, :, 2:4, 2:4], torch.relu(inp.bias).to(dev).view(-1, 1, 1).expand(-1, 2, 2)), \
            f"{name}: the block of four equal elements"
    r.nothing_else_changed()


@pytest.mark.parametrize("name", C.MASKED_NAN)
def test_a_nan_under_a_closed_mask_does_not_reach_the_output(dev, name):
    c = C.case(name)
    inp = copy.copy(C.inputs(name, "a"))
    inp.xs = [t.clone() for t in inp.xs]
    shut = (inp.mask == 0).nonzero()
    for at in (shut[0], shut[len(shut) // 2], shut[-1]):
        inp.xs[0][tuple(at)] = NAN
    ref = C.ref64(name, "a")      # (the reference of the unplanted data: the mask keeps the NaNs out)
    r = _Row(name, inp, dev)
    kind, rows, ksplit, vl, vs, _, _ = c["claim"]
    assert r.call() == C.note(kind, rows, ksplit, vl, vs)
    _check_outputs(r, "a", ref, A.TOL_DX if c["mode"] == 1 else A.TOL_Y)
    r.nothing_else_changed()


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("shape", [(2, 3, 3), (17, 33, 3), (64, 16, 1), (7, 5, 5), (130, 65, 3)])
def test_pack_weight_against_its_restatement(dev, shape, mode):
    """ynet_pack_weight on its own: every float of the packed filter, the zero padding and the slack rows included (the buffer starts as NaN)."""
    ops = pkg("ops")
    lib = ops._lib()
    cout, cin, K = shape
    w = A.randn(cout, cin, K, K, key=(31, mode))
    want = C.packed(w, mode)
    n = lib.ynet_packed_weight_floats(cout, cin, K, mode)
    assert n == want.numel()
    buf = torch.full((n + GUARD,), NAN, device=dev)
    wd = w.to(dev)
    assert lib.ynet_pack_weight(wd.data_ptr(), buf.data_ptr(), cout, cin, K, mode, ops._stream()) == 0, lib.ynet_last_error()
    torch.cuda.synchronize()
    assert A.same_bits(buf[:n].cpu(), want.flatten()) and _all_poison(buf[n:])
    rows = cin if mode == 0 else cout
    assert float(buf[:n].view(want.shape)[rows:].abs().sum()) == 0      # the zero rows behind the last channel, the slack chunk included


@pytest.mark.parametrize("name", list(C.REFUSALS))
def test_shape_refusals_come_before_any_launch(dev, name):
    """Non-zero status, the entry named, every destination (the pooled copy, the words) still bit-identical to its fill, no launch noted."""
    ops = pkg("ops")
    lib, st = ops._lib(), ops._stream()
    entry, B, H, W, cs, cout, K, word = C.REFUSALS[name]
    cin = sum(cs)
    xs = [_Op(A.randn(B, n, H, W, key=(32, i)), dev) for i, n in enumerate(cs)]
    # (bits_in: a cs[0] -> cout data gradient, its filter in the forward layout [dy channels][dx channels])
    wp = ops.pack_weight(A.randn(cin, cout, K, K, key=(32, 9)).to(dev), 1) if entry == "bits_in" else ops.pack_weight(A.randn(cout, cin, K, K, key=(32, 9)).to(dev), 0)
    y = _Op(torch.full((B, cout, H, W), NAN), dev)
    extra = _Op(torch.full((B, cout, H // 2, W // 2) if entry == "pool" else (B, cout, H, W), NAN if entry == "pool" else 0.5), dev)
    words = torch.full((GUARD,), -1, dtype=torch.int32, device=dev)
    sp, sc, sb = ops._arrays([(x.v.data_ptr(), n, x.v.stride(0)) for x, n in zip(xs, cs)])
    yp, ybs, x0 = y.v.data_ptr(), y.v.stride(0), xs[0].v
    lib.ynet_conv2d_last_launch(0)
    if entry == "pool":
        assert not lib.ynet_conv2d_pool_supported(B, H, W, cout, K)
        rc = lib.ynet_conv2d_pool(sp, sc, sb, len(cs), wp.data_ptr(), None, yp, cout, ybs, extra.v.data_ptr(), extra.v.stride(0), B, H, W, K, 1, st)
    elif entry == "add":
        assert not lib.ynet_conv2d_add_supported(B, H, W, cout, K)
        rc = lib.ynet_conv2d_add(sp, sc, sb, None, len(cs), wp.data_ptr(), None, yp, cout, ybs, B, H, W, K, 1, extra.v.data_ptr(), extra.v.stride(0), 0, st)
    elif entry == "bits_out":
        assert lib.ynet_conv2d_relu_bits_words(B, H, W, cout, K) == 0
        rc = lib.ynet_conv2d_relu_bits(sp, sc, sb, len(cs), wp.data_ptr(), None, yp, cout, ybs, words.data_ptr(), B, H, W, K, st)
    elif entry == "bits_in":
        assert lib.ynet_conv2d_relu_bits_words(B, H, W, cout, K) == 0 and len(cs) == 1
        rc = lib.ynet_conv2d_dgrad_relu_bits(x0.data_ptr(), cs[0], x0.stride(0), None, 0, wp.data_ptr(), yp, cout, ybs, words.data_ptr(), B, H, W, K, st)
    else:
        dp, dcs, db = ops._arrays([(yp, cout, ybs)])
        mask = (extra.v.data_ptr(), extra.v.stride(0)) if entry == "mask" else (None, 0)
        rc = lib.ynet_conv2d(sp, sc, sb, None, len(cs), *mask, wp.data_ptr(), None, dp, dcs, db, 1, B, H, W, K, 1, None, 0, st)
    msg = lib.ynet_last_error()
    torch.cuda.synchronize()
    assert rc != 0 and word in msg and b"launch failed" not in msg, (name, msg)
    assert lib.ynet_conv2d_last_launch(0) == 0, name
    assert _all_poison(y.buf) and (entry != "pool" or _all_poison(extra.buf)) and bool((words == -1).all()), name
    assert all(x.intact() for x in xs)

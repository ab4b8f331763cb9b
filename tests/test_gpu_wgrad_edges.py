"""ynet_conv2d_wgrad at every plan edge of its four kernel families (tests/_wgrad_cases.py has the rows, the inputs and the fp64 references; tests/test_wgrad_cases_host.py
shows on the CPU that every row plans what it claims and that every edge is reached).

The library is called directly, so the test owns every buffer: sources, dy and mask lie in NaN-poisoned buffers with 8 floats of slack between images (a read past an
image that reaches arithmetic poisons the result), one source of a multi-source row is a channel slice of a wider NaN tensor, one row shares a stride-0 scene map; dW, db and
the workspace -- exactly ynet_conv2d_wgrad_workspace_floats floats and a guard -- are NaN-poisoned too.  Per row and input family: the launch note equals the plan;
family (a) (normal inputs) meets the project's tolerance against fp64, family (b) (exact integers) matches the reference bit for bit; a second call repeats the bits;
nothing is written behind the plan's partial_floats, around dW / db or into an input; db = NULL gives the same dW and writes no bias partial.

What a broken kernel looks like here (each a one-line edit of csrc/wgrad_mfma.hip on a scratch copy, run against this file on the MI355X; both input families of
every row named failed, every other row passed):
  * wgrad_roll_kernel: j1 = j0 + seg without the min                  -> the 8 rows whose last segment is short: roll_two_steps, roll_nsegs_eq_nsplit, roll_one_column,
                                                                         roll_unmasked_85, roll_seg_8, roll_seg_16, roll_five_segments, roll_unmasked_768
  * wgrad1x1_stream_kernel: if (pn > a.hw16)                           -> stream_full_grid (the one row whose chunk walk lands on an image's last chunk + 1)
  * wgrad_dma_kernel: the cursor's carry into the image index dropped  -> dma_cursor_y, dma_odd_h_100, miss_odd_h
  * the mask compared >= 0, in the staged kernel                       -> all 7 masked staged rows; in wgrad_dma_kernel (one of its four compares) -> all 7 masked two-row rows;
                                                                         in wgrad_roll_kernel (one of two) -> all 7 masked rolling rows
  * wgrad_plan: resident 768 -> 769                                    -> roll_unmasked_768.  The edit touches the size formula alone (no launch plans one-row tiles) and makes the
                                                                         workspace LARGER, so no guard can see it: the row fails at "agree to the last float"
The 82 cases take 5 s (tests/test_gpu_kernels.py: 61 s for 313).  Family (a) comes closest to its bound at roll_seg_16: dW off by 1.4e-3
where 1.05e-2 + 1e-4 |dW| is allowed (52224 pixels per filter tap)."""
import pytest
import torch

import _align_cases as A
import _wgrad_cases as C
from conftest import pkg

pytestmark = pytest.mark.gpu

NAN = float("nan")
GUARD = 4096            # floats behind the workspace
LEAD, TRAIL = 4, 1      # NaN channels around a sliced source (4 planes: a slice of an aligned tensor stays on a 16-byte boundary)


def _poisoned(n, dev):
    return torch.full((n,), NAN, device=dev, dtype=torch.float32)


def _all_poison(t):
    want = A.bits(torch.full((1,), NAN, dtype=torch.float32, device=t.device))
    return bool((A.bits(t) == want).all())


class _Operands:
    """The device buffers of one row and family: desc (pointer, channels, batch stride) per source, dy, mask; every buffer with a snapshot."""

    def __init__(self, name, family, dev):
        (B, H, W, cs, cout, K, masked, bias), _, _, _, opts = C.CASES[name]
        inp = C.inputs(name, family)
        where = {k: C.PLACEMENT for k in [f"src{i}" for i in range(len(cs))] + ["dy", "mask"]}
        if "misplace" in opts:
            where[opts["misplace"]] = C.OFF_4_BYTES
        self.bufs, self.descs = [], []
        for i, (x, c) in enumerate(zip(inp.xs, cs)):
            if i == opts.get("slice"):
                wide = torch.full((x.shape[0], LEAD + c + TRAIL, H, W), NAN)
                wide[:, LEAD:LEAD + c] = x
                v, buf = A.offset_view(wide.to(dev), *where[f"src{i}"])
                v = v[:, LEAD:LEAD + c]
            else:
                v, buf = A.offset_view(x.to(dev), *where[f"src{i}"])
            assert torch.equal(v.cpu(), x)
            self.bufs.append(buf)
            self.descs.append((v.data_ptr(), c, 0 if i == opts.get("shared") else v.stride(0)))      # (stride 0: one scene map for the whole batch)
        self.dy, buf = A.offset_view(inp.dy.to(dev), *where["dy"])
        self.bufs.append(buf)
        self.mask = None
        if masked:
            self.mask, buf = A.offset_view(inp.mask.to(dev), *where["mask"])
            self.bufs.append(buf)
        self.snaps = [b.clone() for b in self.bufs]
        planes = [(p, bs) for p, _, bs in self.descs] + [(self.dy.data_ptr(), self.dy.stride(0))] + ([(self.mask.data_ptr(), self.mask.stride(0))] if masked else [])
        self.aligned = int(all(p % 16 == 0 and bs % 4 == 0 for p, bs in planes))

    def unchanged(self):
        return all(A.same_bits(b, s) for b, s in zip(self.bufs, self.snaps))


def _call(ops, lib, name, o, want_bias):
    """One ynet_conv2d_wgrad call into fresh poisoned outputs -> (dW view, its buffer, db view or None, its buffer, workspace, launch note)."""
    B, H, W, cs, cout, K, masked, _ = C.shape_of(name)
    dev = o.dy.device
    cin = sum(cs)
    dw, dwbuf = A.offset_view(torch.full((1, 1, 1, cout * cin * K * K), NAN, device=dev), 4, 0)
    db, dbbuf = A.offset_view(torch.full((1, 1, 1, cout), NAN, device=dev), 4, 0)
    need = lib.ynet_conv2d_wgrad_workspace_floats(B, H, W, cout, cin, K)
    ws = _poisoned(need + GUARD, dev)
    sp, sc, sb = ops._arrays(o.descs)
    lib.ynet_conv2d_last_launch(1)
    rc = lib.ynet_conv2d_wgrad(sp, sc, sb, len(cs), o.dy.data_ptr(), o.dy.stride(0), o.mask.data_ptr() if masked else None, o.mask.stride(0) if masked else 0,
                               dw.data_ptr(), db.data_ptr() if want_bias else None, ws.data_ptr(), B, H, W, cout, K, ops._stream())
    assert rc == 0, lib.ynet_last_error()
    torch.cuda.synchronize()
    note = lib.ynet_conv2d_last_launch(1)
    return dw[0, 0, 0].view(cout, cin, K, K), dwbuf, db[0, 0, 0], dbbuf, ws, need, note


@pytest.mark.parametrize("family", ["a", "b"])
@pytest.mark.parametrize("name", list(C.CASES))
def test_conv2d_wgrad_at_a_plan_edge(dev, name, family):
    ops, L = pkg("ops"), pkg("_lib")
    lib = ops._lib()
    (B, H, W, cs, cout, K, masked, bias), kernel, _, edges, _ = C.CASES[name]
    cin = sum(cs)
    o = _Operands(name, family, dev)
    assert o.aligned == 1 or kernel == 1, name      # (planes of a map with H W % 4 != 0 cannot all lie on 16 bytes: such rows take the staged tiles on any count)
    assert o.aligned == 0 or C.aligned_of(name) == 1, name
    p = C.plan(lib, L, B, H, W, cs, cout, K, masked, o.aligned, bias)
    assert p["kernel"] == kernel, (name, p)
    want_w, want_b = (t.to(dev) for t in C.ref64(name, family))

    dw, dwbuf, db, dbbuf, ws, need, note = _call(ops, lib, name, o, bias)
    assert note == kernel, (name, note)
    assert 0 < p["partial_floats"] <= need
    if "workspace_exact" in edges:
        assert p["partial_floats"] == need, (name, p["partial_floats"], need)      # the size formula and the launch agree to the last float
    assert _all_poison(ws[p["partial_floats"]:]), f"{name}: written behind the plan's {p['partial_floats']} floats (workspace {need}, then the guard)"
    assert bool(torch.isfinite(ws[:p["partial_floats"]]).all()), f"{name}: a partial the plan counts was not written (or holds a read past an image)"
    assert A.slack_intact(dwbuf, (1, 1, 1, dw.numel()), 4, 0) and A.slack_intact(dbbuf, (1, 1, 1, cout), 4, 0), name
    assert bool(torch.isfinite(dw).all()), f"{name}: dW is not finite"
    if bias:
        assert bool(torch.isfinite(db).all()), f"{name}: db is not finite"
    else:
        assert _all_poison(db), f"{name}: db written without being asked for"
    checks = [("dW", dw, want_w)] + ([("db", db, want_b)] if bias else [])
    for what, got, want in checks:
        if family == "b":
            assert A.same_bits(got, want.float()), f"{name} {what}: exact-integer inputs, {int((got != want.float()).sum())} elements differ, largest {float((got - want.float()).abs().max())}"
        else:
            bad, err, atol = A.mismatch(got, want, **A.TOL_DW)
            print(f"{name} {what}: largest error {err:.3g} (bound {atol:.3g} + 1e-4 |want|)")
            assert bad == 0, f"{name} {what}: {bad} elements beyond the tolerance, largest error {err:.3g}"

    # a second call: the same bits (fixed-order reductions)
    dw2, _, db2, _, _, _, note2 = _call(ops, lib, name, o, bias)
    assert note2 == kernel and A.same_bits(dw, dw2) and (not bias or A.same_bits(db, db2)), name
    # db = NULL: the same dW, and no bias partial where the filter partials end
    p0 = C.plan(lib, L, B, H, W, cs, cout, K, masked, o.aligned, 0)
    assert p0["partial_floats"] == p0["nsplit"] * cout * cin * K * K and p0["nsplit"] == p["nsplit"]
    dw3, dwbuf3, db3, _, ws3, _, note3 = _call(ops, lib, name, o, False)
    assert note3 == kernel and A.same_bits(dw, dw3), name
    assert _all_poison(ws3[p0["partial_floats"]:]) and _all_poison(db3), f"{name}: db = NULL, yet something was written behind the filter partials"
    assert A.slack_intact(dwbuf3, (1, 1, 1, dw.numel()), 4, 0)
    assert o.unchanged(), f"{name}: an input buffer changed"

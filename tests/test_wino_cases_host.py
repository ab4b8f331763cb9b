"""tests/_wino_cases.py on the CPU: every row plans what it claims (ynet_conv2d_auto_plan and the *_supported queries are host code), sits at its size gate, reaches the edges
it names -- recomputed from the kernels' own formulas, with the 256 compute units of the MI355X for the XCD walk --, and the references are what the GPU test may hold the
kernels to: family (b) exact in fp32 by a bound on the generated tensors and by a plain fp32 restatement of F(2x2, 3x3), family (a) within the project's tolerances of
stock fp32 torch, with at most 0.1 % of its gates ambiguous."""
import pytest
import torch
import torch.nn.functional as F

import _align_cases as A
import _wino_cases as C
from conftest import pkg


@pytest.fixture(scope="module")
def libs():
    L = pkg("_lib")
    return L.load(), L


@pytest.mark.parametrize("name", list(C.CASES))
def test_row_plans_what_it_claims_at_its_gate(libs, name):
    lib, L = libs
    c = C.case(name)
    if c["entry"] == "auto":
        assert C.plan_of(lib, L, C.make_desc(L, name, C.standin(name))) == c["plan"], name
    else:
        assert c["entry"] == "cat" and c["plan"] is None and c["sizes"] == [32]
    ls = C.launches(name)
    assert c["plan"] is None or len(ls) == c["plan"][2], (name, ls)
    gate = C.GATE16 if ls[0][0] in ("w16", "up16") else C.GATE
    for kernel, cs, cout in ls:
        # (variant 40's first launch is conv_wino_kernel at the slice form's sizes: both gates hold at every row that has it)
        assert C.supported(lib, kernel, c["B"], c["H"], c["W"], cs, cout) == 1, (name, kernel, cs, cout)
        w = C.walk(kernel, c["B"], c["H"], c["W"], cout)
        assert w["once"], (name, w)      # (the walk as the kernel makes it visits every tile once)
    at_gate = (c["B"] - 1) * c["H"] * c["W"] < gate
    assert at_gate != (name in C.ABOVE_GATE), name
    if at_gate:      # one image fewer is refused by the matching *_supported
        assert any(C.supported(lib, kernel, c["B"] - 1, c["H"], c["W"], cs, cout) == 0 for kernel, cs, cout in ls), name
        k0, cs0, co0 = ls[-1]
        assert C.supported(lib, k0, c["B"] - 1, c["H"], c["W"], cs0, co0) == 0, name
    if c["opts"].get("words"):      # the consumer of the words: a 32 -> 32 data gradient gated by them
        assert sum(c["sizes"]) == 32 and C.plan_of(lib, L, C.gate_desc(L, c["B"], c["H"], c["W"])) == (1, 21, 1)
    if c["plan"] is not None and c["plan"][1] == 43:
        cut = C.cut_of(c["cs"], sum(c["sizes"]))
        assert cut is not None and [len(cs) for _, cs, _ in ls] == [cut, len(c["cs"]) - cut]


@pytest.mark.parametrize("name", list(C.REFUSALS))
def test_refusals(libs, name):
    lib, L = libs
    (B, H, W, cs, couts, up), want = C.REFUSALS[name]
    d = L.ConvAuto()
    d.nsrc = d.ndst = 1
    hw_src = (H // 2) * (W // 2) if up else H * W
    d.src[0], d.src_c[0], d.src_bs[0] = 4096, cs[0], cs[0] * hw_src
    d.dst[0], d.dst_c[0], d.dst_bs[0] = 8192, couts[0], couts[0] * H * W
    d.wp, d.B, d.H, d.W, d.K, d.relu, d.upsample2x = 12288, B, H, W, 3, 1, int(up)
    got = C.plan_of(lib, L, d)
    if want == 0:
        assert got[0] == 0 and got[2] == 1, (name, got)
        # ... and one channel fewer is served: the refusal is the channel limit's
        d.src_c[0], d.src_bs[0] = cs[0] - 1, (cs[0] - 1) * hw_src
        assert C.plan_of(lib, L, d)[0] != 0, name
    else:
        assert isinstance(got, bytes) and want in got, (name, got)
        d.src_c[0], d.src_bs[0] = 84, 84 * hw_src
        assert C.plan_of(lib, L, d) == (5, 0, 1), name


def test_every_edge_is_reached_and_no_row_is_spare():
    claimed = {e for n in C.CASES for e in C.case(n)["edges"]}
    assert claimed == set(C.EDGES), claimed ^ set(C.EDGES)
    for n in C.CASES:
        for e in C.case(n)["edges"]:
            assert C.EDGES[e](n), (n, e)      # no row claims an edge its shape cannot reach
    per_family = {}
    for n in C.CASES:
        f = C.case(n)["plan"][0] if C.case(n)["plan"] else None
        per_family[f] = per_family.get(f, 0) + 1
    assert per_family == C.ROWS_PER_FAMILY, per_family
    # every em value a row pair can have, for each of the three stagers
    em = {"wino": set(), "cat": set(), "w16": set(), "up": set(), "up16": set()}
    for n in C.CASES:
        for kernel, cs, co in C.launches(n):
            em[kernel] |= C.em_values(kernel, C.case(n)["H"], C.case(n)["W"])
    for kernel in ("wino", "cat", "w16"):
        assert em[kernel] == C.EM_ALL, (kernel, em[kernel] ^ C.EM_ALL)
    assert em["up"] == C.EM_ALL and em["up16"] >= {0, 1, 2, 4, 8, 12, 13, 14}
    # a map one tile wide sets the left and the right bit on the same row pair
    assert C.em_values("wino", 16, 32) == {12, 13, 14} and C.em_values("w16", 32, 32) == {12, 13, 14}
    # the walks the issue names: 257 tiles of conv_wino_kernel, 41 tiles of the slice form
    w = C.walk("wino", 257, 16, 32, 32)
    assert (w["ntiles"], w["grid"], w["per_xcd"], w["short"], w["idle"], w["most"], w["least"]) == (257, 256, 33, True, 6, 2, 1)
    w = C.walk("w16", 41, 32, 32, 64)
    assert (w["ntiles"], w["grid"], w["per_xcd"], w["short"], w["empty"], w["idle"]) == (41, 192, 6, True, True, 4 * 6 + 4)
    # the slice form's team: 32 / ns workgroups per XCD -- 4 for eight slices, which nothing else produces
    w = C.walk("w16", 10, 64, 64, 128)
    assert (w["ntiles"], w["per_xcd"], w["grid"], w["most"], w["least"], w["idle"]) == (40, 5, 8 * 8 * 4, 2, 1, 0)
    # the options: a stride-0 source in every slot, a sliced source in every stager that concatenates
    shared = {(C.case(n)["plan"][0], C.case(n)["opts"]["shared"]) for n in C.CASES if "shared" in C.case(n)["opts"]}
    assert shared == {(2, 0), (2, 1), (2, 2), (4, 0)}
    assert {C.case(n)["plan"][0] for n in C.CASES if "slice" in C.case(n)["opts"]} == {2, 3}
    assert {C.cut_of(C.case(n)["cs"], sum(C.case(n)["sizes"])) for n in C.CASES if C.case(n)["plan"] and C.case(n)["plan"][1] == 43} == {1, 2}


def _restate(x, w, bias):
    """relu(conv3x3(x, w) + bias) as F(2x2, 3x3) in fp32 torch, with the transforms as csrc/conv_wino.hip states them: U = G g G^T (wino_filter_kernel), V = B^T d B
    (wn_v01 / wn_v23: t0 - t2, t1 + t2, t2 - t1, t1 - t3), Y = A^T [sum over cin U (.) V] A."""
    G = torch.tensor([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], dtype=torch.float32)
    Bt = torch.tensor([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], dtype=torch.float32)
    At = torch.tensor([[1, 1, 1, 0], [0, 1, -1, -1]], dtype=torch.float32)
    d = F.pad(x, (1, 1, 1, 1)).unfold(2, 4, 2).unfold(3, 4, 2)      # [B][ci][H / 2][W / 2][4][4]
    V = Bt @ d @ Bt.t()
    U = G @ w @ G.t()                                               # [co][ci][4][4]
    M = torch.einsum("oiuv,bihwuv->bohwuv", U, V)
    Y = At @ M @ At.t()                                             # [B][co][H / 2][W / 2][2][2]
    B, co, h, w_ = Y.shape[:4]
    y = Y.permute(0, 1, 2, 4, 3, 5).reshape(B, co, 2 * h, 2 * w_) + bias.view(1, -1, 1, 1)
    return torch.relu(y), float(M.abs().max())


def test_winograd_on_the_integer_family_is_exact_in_fp32():
    """The exactness the GPU test relies on, without the kernel: 84 input channels, x in [-3, 3], g in [-2, 2]."""
    name = "w16_84_64"
    inp, ref = C.inputs(name, "b"), C.ref64(name, "b")
    got, top = _restate(inp.xs[0], inp.w, inp.bias)
    assert got.dtype == torch.float32 and A.same_bits(got, ref["y"].float())
    assert torch.equal(ref["y"].float().double(), ref["y"])
    assert 4 * top < 2 ** 24, top      # the largest accumulator, in quarter-units
    # family (a) through the same restatement meets the forward tolerance: the transforms are the convolution
    a, ra = C.inputs(name, "a"), C.ref64(name, "a")
    ya, _ = _restate(a.xs[0], a.w, a.bias)
    assert A.mismatch(ya, ra["y"], **A.TOL_Y)[0] == 0


@pytest.mark.parametrize("name", list(C.CASES))
def test_references(name):
    c = C.case(name)
    o = c["opts"]
    # ---- family (b): exact.  Unit 1 / 64 (bilinear weights are quarters in both directions, the filter transform quarters once more in front of a 16-fold finer product)
    b, rb = C.inputs(name, "b"), C.ref64(name, "b")
    for t in b.xs + [b.w] + [t for t in (b.bias, b.act, b.addend, b.dy2, b.w2) if t is not None]:
        assert torch.equal(t, t.round())
    mx = max(float(t.abs().max()) for t in b.xs)
    assert mx <= 3 and float(b.w.abs().max()) <= 2 and (not c["up"] or min(float(t.min()) for t in b.xs) >= 0)
    extra = (float(b.bias.abs().max()) if b.bias is not None else 0) + (float(b.addend.abs().max()) if b.addend is not None else 0)
    assert extra <= 8
    assert 64 * 9 * C.padded(c["cs"]) * mx * float(b.w.abs().max()) + 64 * extra < 2 ** 24, name
    if b.act is not None:
        assert set(b.act.flatten().tolist()) == {0.0, 1.0, 2.0, 3.0} and float((b.act == 0).float().mean()) > 0.4
    for k, t in rb.items():
        if t.dtype == torch.float64:
            assert torch.equal(t * 16, (t * 16).round()) and float(t.abs().max()) < 2 ** 20, (name, k)      # every reference value is a multiple of 1 / 16 ...
            assert torch.equal(t.float().double(), t)                                                         # ... and a float
    if c["relu"]:
        assert float((rb["pre"] == 0).float().mean()) > (1e-4 if c["up"] else 1e-3), name      # zeros on the ReLU's edge are frequent (an up form's grid is 16 x finer)
    if o.get("pool_code"):
        top = C.blocks(rb["y"]).topk(2, dim=-1).values
        assert float(((top[..., 0] == top[..., 1]) & (top[..., 0] > 0)).float().mean()) > 0.01, name      # ... and so are ties of positive values in a 2 x 2 block
        assert set(rb["code"].flatten().tolist()) > {0, 4 | 0, 8 | 1, 16 | 2, 32 | 3}
    # ---- family (a): a correct fp32 implementation (stock torch on the CPU) meets the tolerances the GPU test uses, so the references are not mistaken as a group
    a, ra = C.inputs(name, "a"), C.ref64(name, "a")
    r32 = C.reference(name, a, torch.float32)
    tol = A.TOL_DX if c["mode"] == 1 else A.TOL_Y
    el, blk = C.ambiguous(name, ra)
    for k in ("y", "pooled"):
        if k in ra:
            assert A.mismatch(r32[k], ra[k], **tol)[0] == 0, (name, k)
    if "gated" in ra:      # (the gate is the fp32 run's own: compared outside the ambiguous elements, as on the device)
        assert A.mismatch(r32["gated"][~el], ra["gated"][~el], **A.TOL_DX)[0] == 0, name
    assert float(ra["y"].abs().max()) > 0.1 and ra["y"].shape == (c["B"], sum(c["sizes"]), c["H"], c["W"])
    if a.act is not None:
        assert 0.3 < float((a.act > 0).float().mean()) < 0.7
    # ---- the exclusion cap of family (a), on the reference alone
    assert (el is not None) == bool(c["relu"] and (o.get("words") or o.get("pool_code"))) and (blk is not None) == bool(o.get("pool_code"))
    if el is not None:
        assert float(el.float().mean()) <= 1e-3, (name, float(el.float().mean()))
    if blk is not None:
        assert float(blk.float().mean()) <= 1e-3, (name, float(blk.float().mean()))
    eb, bb = C.ambiguous(name, rb)      # (family (b) has no value near a gate that is not ON it: nothing is excluded there)
    if eb is not None:
        assert bool((rb["pre"][eb] == 0).all())

"""The hand-over between units, images and sources in the Winograd kernels' per-unit context (csrc/conv_wino.hip: WinoPlace, WinoFeed1, WinoSrcFeed).

A wave decodes a unit's place once, when it takes the unit from the workgroup's counter, and its DMA cursor only steps from chunk to chunk; what can newly break is where the
cursor changes hands: from the unit being computed to the one taken after it (another tile, another image), from one source to the next (a new descriptor, a ragged last
chunk, a batch stride of 0), and the epilogue that now takes the decode the loop made.  The arithmetic itself is guarded by the bit-exact sweeps of test_gpu_wino_edges.py,
test_gpu_conv_alignment.py and test_conv2d_auto_takes_the_launches_of_the_python_dispatcher.

The rows here are SMALL (2 or 3 images of one to four tiles), far below the size gates of the dispatch, and the gates are read from the environment once per process: one
child process with YNET_WINOGRAD_MIN = YNET_WINOGRAD16_MIN = 1 runs every row (this file, as a program, through conftest.launch) and writes one verdict per row; the
parametrised test reads its row's verdict.  A row is driven like a row of test_gpu_wino_edges.py (its _Row: NaN-poisoned buffers with slack between the images, a sliced or a
shared source, guarded code bytes and words) on the exact-integer inputs of tests/_wino_cases.py, and every output -- destinations, pooled copy, pool codes, the word-gated
gradient -- must equal the fp32 restatement C.reference(..., torch.float32) bit for bit; a second call must repeat every bit and nothing around the outputs may change.
The row also names the kernel family ynet_conv2d_auto must take and, where the row is there for an epilogue, its template arguments.

  slice form   B 3 at 32 x 32 (one tile per image: a wave's next unit lies in another image) and 64 x 32 (two tiles), 16 and 64 outputs, sources [5, 33, 1] (12 chunks,
               three descriptors per unit, two ragged last chunks), [84] (21 chunks, the most) and [8] (2 chunks, the fewest: the cursor changes units in the first k-step),
               a shared source, the four epilogues (plain, through a ReLU backward, + addend, + pooled copy)
  cat form     B 3 at 16 x 32 (3 tiles) and 32 x 64 (12 tiles on a grid of 8 walked by XCD: two XCDs are empty), sources [16, 32, 1] and [14], EPI 4 / 5 / 6
  up forms     B 2, one tile per image (all four borders in every unit): 16 x 32 from 8 x 16 (conv_wino_up_kernel), 32 x 32 from 16 x 16 (conv_wino16_up_kernel)
"A grid larger than the tile count" cannot be launched through the C ABI: the host never starts more workgroups than tiles.  What can be reached is the same early
return: 12 tiles on a grid of 8 walked by XCD give per_xcd = 2, so the workgroups of XCDs 6 and 7 have no tile and leave before the barrier (the 32 x 64 cat rows).
The rows are driven through test_gpu_wino_edges._Row and registered in _wino_cases.CASES at run time, in the worker process only: the poisoned-buffer harness and
the references are those of the plan-edge sweep, deliberately not a second copy; a change of _Row's interface fails every row here loudly (no verdict, test_every_row_ran).
conv_wino_kernel keeps its per-chunk decode (the context gained nothing there), so it has no rows here; it runs as the consumer of the cat rows' words."""
import json
import os
import sys

import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
NO_W16, FOR_16 = 2, 4
R, NR = True, False
# name: a row of _wino_cases.CASES (of its plan entry only the family is looked at), then the leading template arguments YnetConvTaken must name for the first launch
# (the slice form: EPI; the cat form: NCB, EPI) or None
ROWS = {
    # ---- conv_wino16_kernel
    "ctx_w16_3src_64": (("auto", 3, 32, 32, [5, 33, 1], [64], R, True, 0, {"shared": 1}, (3, None, None), []), (0,)),
    "ctx_w16_3src_16_two_tiles": (("auto", 3, 64, 32, [5, 33, 1], [16], R, True, 0, {"flags": FOR_16, "slice": 0}, (3, None, None), []), (0,)),
    "ctx_w16_84_64_two_tiles": (("auto", 3, 64, 32, [84], [64], NR, True, 0, {}, (3, None, None), []), (0,)),
    "ctx_w16_84_16": (("auto", 3, 32, 32, [84], [16], R, False, 0, {"flags": FOR_16}, (3, None, None), []), (0,)),
    "ctx_w16_8_64": (("auto", 3, 32, 32, [8], [64], R, True, 0, {}, (3, None, None), []), (0,)),
    "ctx_w16_8_16_two_tiles": (("auto", 3, 64, 32, [8], [16], R, True, 0, {"flags": FOR_16}, (3, None, None), []), (0,)),
    "ctx_w16_relu_of": (("auto", 3, 32, 32, [84], [64], NR, False, 1, {"relu_of": True}, (3, None, None), []), (1,)),
    "ctx_w16_addend": (("auto", 3, 64, 32, [5, 33, 1], [64], R, True, 0, {"addend": 2, "shared": 0}, (3, None, None), []), (2,)),
    "ctx_w16_pooled": (("auto", 3, 32, 32, [8], [16], R, True, 0, {"pooled": True, "flags": FOR_16}, (3, None, None), []), (3,)),
    # ---- conv_wino_cat_kernel
    "ctx_cat_3src_words": (("auto", 3, 16, 32, [16, 32, 1], [32], R, True, 0, {"words": True}, (2, None, None), []), (2, 4)),
    "ctx_cat_14_addend_words": (("auto", 3, 32, 64, [14], [32], R, True, 0, {"words": True, "addend": 2, "flags": NO_W16}, (2, None, None), []), (2, 5)),
    "ctx_cat_3src_pool_code": (("auto", 3, 32, 64, [16, 32, 1], [32], R, True, 0, {"pooled": True, "pool_code": True, "shared": 2}, (2, None, None), []), (2, 6)),
    "ctx_cat_14_pool_code": (("auto", 3, 16, 32, [14], [32], R, True, 0, {"pooled": True, "pool_code": True, "flags": NO_W16}, (2, None, None), []), (2, 6)),
    "ctx_cat_3src_addend_words_12_tiles": (("auto", 3, 32, 64, [16, 32, 1], [32], R, True, 0, {"words": True, "addend": 3, "slice": 1}, (2, None, None), []), (2, 5)),
    # ---- the up-convolutions
    "ctx_up_one_tile": (("auto", 2, 16, 32, [32], [16], NR, True, 0, {"up": True}, (4, None, None), []), None),
    "ctx_up16_one_tile": (("auto", 2, 32, 32, [8], [64], R, True, 0, {"up": True}, (5, None, None), []), None),
    "ctx_up16_84_one_tile": (("auto", 2, 32, 32, [84], [16], NR, True, 0, {"up": True}, (5, None, None), []), None),
}
GATES = {"YNET_WINOGRAD_MIN": "1", "YNET_WINOGRAD16_MIN": "1"}


def _run_row(E, C, A, ops, L, name, dev):
    """One row on the device -> None, or what is wrong with it."""
    import torch
    c = C.case(name)
    o, B, H, W = c["opts"], c["B"], c["H"], c["W"]
    r = E._Row(ops, L, name, "b", dev)
    ref = C.reference(name, C.inputs(name, "b"), torch.float32)
    tk = r.call(True)
    tmpl = tuple(tk.tmpl[0][i] for i in range(3))
    if tk.family != c["plan"][0]:
        return f"family {tk.family} (variant {tk.variant}, {tk.nlaunch} launches, first {tmpl}) instead of {c['plan'][0]}"
    want_t = ROWS[name][1]
    if want_t is not None and tmpl[:len(want_t)] != want_t:
        return f"the first launch is {tmpl}, not {want_t}"
    pairs, c0 = [], 0
    for i, ((v, _, _, _, wanted), n) in enumerate(zip(r.dsts, c["sizes"])):
        if wanted:
            want, got = ref["y"][:, c0:c0 + n].to(dev), v
            if o.get("s2d") and o["s2d"][i]:
                want, got = C.s2d(want.contiguous()), v.view(B, 4 * n, H // 2, W // 2)
            pairs.append((f"destination {i}", got, want))
        c0 += n
    if r.pooled is not None:
        pairs.append(("pooled copy", r.pooled[0], ref["pooled"].to(dev)))
    if r.words is not None:
        pairs.append(("word-gated gradient", r.gated_gradient(), ref["gated"].to(dev)))
    for what, got, want in pairs:
        if not bool(torch.isfinite(got).all()):
            return f"{what}: not finite"
        if not A.same_bits(got, want.float()):
            return f"{what}: {int((got != want).sum())} elements differ from the fp32 restatement, largest {float((got - want).abs().max())}"
    if r.code is not None:
        got, want = r.code.body.view(B, 32, H // 2, W // 2).cpu(), ref["code"]
        if not torch.equal(got, want):
            return f"pool code: {int((got != want).sum())} codes differ"
    first = r.outputs()
    r.repoison()
    tk2 = r.call(False)
    if tk2.transformed != 0:
        return "the second call transformed the filter again"
    for a_, b_ in zip(first, r.outputs()):
        same = torch.equal(torch.nan_to_num(a_, nan=12345.0), torch.nan_to_num(b_, nan=12345.0)) if a_.dtype == torch.float32 else torch.equal(a_, b_)
        if not same:
            return "the second call differs"
    r.nothing_else_changed()
    return None


def _worker(out_path):
    sys.path.insert(0, HERE)
    import torch
    import _align_cases as A
    import _wino_cases as C
    import test_gpu_wino_edges as E
    from conftest import pkg
    for name, (row, _) in ROWS.items():
        C.CASES[name] = row
    ops, L = pkg("ops"), pkg("_lib")
    dev = torch.device("cuda:0")
    verdicts = {}
    for name in ROWS:
        try:
            verdicts[name] = _run_row(E, C, A, ops, L, name, dev)
        except AssertionError as e:
            verdicts[name] = f"assertion: {e}"
        torch.cuda.synchronize()      # (a fault surfaces here and ends the process: the rows behind it have no verdict)
        with open(out_path, "w") as f:
            json.dump(verdicts, f)


@pytest.fixture(scope="module")
def verdicts(tmp_path_factory):
    from conftest import launch
    out = str(tmp_path_factory.mktemp("wino_unit_context") / "verdicts.json")
    rc, tail = launch([sys.executable, os.path.abspath(__file__), "--worker", out], env=GATES, timeout=300)
    got = {}
    if os.path.exists(out):
        with open(out) as f:
            got = json.load(f)
    return rc, tail, got


@pytest.mark.parametrize("name", list(ROWS))
def test_unit_hand_over_matches_the_fp32_restatement_bit_for_bit(dev, verdicts, name):
    rc, tail, got = verdicts
    assert name in got, f"the worker (exit code {rc}) has no verdict for {name}:\n{tail[-2000:]}"
    assert got[name] is None, f"{name}: {got[name]}"


def test_every_row_ran(dev, verdicts):
    rc, tail, got = verdicts
    assert rc == 0 and sorted(got) == sorted(ROWS), f"exit code {rc}, {len(got)} of {len(ROWS)} rows:\n{tail[-2000:]}"


if __name__ == "__main__":
    assert sys.argv[1] == "--worker"
    _worker(sys.argv[2])

"""The hand-over registries of the training step (motion-style-transfer_amd/_handover.py and their use in ops.py), on the host:
which tensor a record is valid for, what a sweep drops, and that one context manager empties every registry of a step."""
import gc

import pytest
import torch

from conftest import pkg


@pytest.fixture
def ops():
    ops = pkg("ops")
    regs = list(ops._ALL_REGISTRIES) + [ops._s2d_produced]
    for r in regs:
        r.clear()
    yield ops
    for r in regs:
        r.clear()


def _new(**kw):
    """A registry that joins neither module-level list (the tests of the type leave the product's lists alone)."""
    H = pkg("_handover")
    n_step, n_all = len(H.STEP), len(H.ALL)
    reg = H.Handover("test", **kw)
    assert len(H.ALL) == n_all + 1 and H.ALL[-1] is reg
    assert len(H.STEP) == n_step + (1 if kw.get("step", True) else 0)
    H.ALL.remove(reg)
    if kw.get("step", True):
        H.STEP.remove(reg)
    return reg


def _same_address_twins():
    base = torch.zeros(8)
    a, b = base[:4], base[:4]
    assert a is not b and a.data_ptr() == b.data_ptr() and a.shape == b.shape
    return base, a, b


def test_the_module_needs_neither_the_library_nor_a_device():
    import ast
    import inspect
    tree = ast.parse(inspect.getsource(pkg("_handover")))
    names = {a.name for n in ast.walk(tree) if isinstance(n, ast.Import) for a in n.names}
    names |= {n.module for n in ast.walk(tree) if isinstance(n, ast.ImportFrom)}
    assert names <= {"weakref", "types"}, names


def test_a_non_weak_registry_knows_a_tensor_by_address_and_shape():
    reg = _new(weak=False, step=False)
    base, a, b = _same_address_twins()
    r = reg.put(a)
    assert r.ref is None and r.shape == (4,) and r.version == a._version
    assert reg.get(b) is r
    del a
    gc.collect()
    assert reg.get(b) is r      # (no reference was kept: the record does not die with the tensor)


def test_a_weak_registry_returns_the_record_while_its_tensor_lives():
    reg = _new(weak=True)
    base, a, b = _same_address_twins()
    r = reg.put(a)
    assert r.ref() is a
    assert reg.get(b) is r and reg.get(a) is r
    key = a.data_ptr()
    del a
    gc.collect()
    assert key in reg           # (still stored: nobody asked)
    assert reg.get(b) is None
    assert key not in reg and len(reg) == 0


@pytest.mark.parametrize("weak", [True, False])
def test_a_view_of_another_shape_at_the_same_address_gets_nothing_and_drops_the_record(weak):
    reg = _new(weak=weak)
    base = torch.zeros(8)
    a = base[:4]
    reg.put(a)
    assert reg.get(base[:2]) is None
    assert a.data_ptr() not in reg and reg.get(a) is None
    # ... unless the registry was made without the shape check (a target consumed as a view of what was registered)
    loose = _new(weak=weak, shape=False)
    r = loose.put(a)
    assert loose.get(base[:4].view(2, 2)) is r and loose.get(a) is r


def test_an_in_place_write_invalidates_a_versioned_record_only():
    versioned, plain = _new(weak=False, version=True), _new(weak=False, version=False)
    t = torch.zeros(4)
    versioned.put(t)
    r = plain.put(t)
    assert versioned.get(t) is not None
    t.add_(1.0)
    assert r.version != t._version
    assert versioned.get(t) is None and t.data_ptr() not in versioned
    assert plain.get(t) is r


def test_named_fields_pop_and_the_container_protocol():
    reg = _new()
    t, bits = torch.zeros(4), torch.ones(3, dtype=torch.int32)
    assert not reg and len(reg) == 0 and t.data_ptr() not in reg
    r = reg.put(t, bits=bits, k=3, wbits=None)
    assert r.bits is bits and r.k == 3 and r.wbits is None
    assert reg and len(reg) == 1 and t.data_ptr() in reg and list(reg.values()) == [r]
    assert reg.get(t) is r and len(reg) == 1        # (get leaves a valid record in place)
    assert reg.pop(t) is r
    assert not reg and t.data_ptr() not in reg and reg.pop(t) is None and reg.get(t) is None
    reg.put(t, k=5)                                  # (a second put under one address replaces the record)
    assert reg.put(t, k=7).k == 7 and len(reg) == 1 and reg.get(t).k == 7
    reg.clear()
    assert not reg


def test_pop_of_an_invalid_record_returns_nothing_and_removes_it():
    reg = _new(weak=False, version=True)
    t = torch.zeros(4)
    reg.put(t, y_ptr=1)
    t.mul_(2.0)
    assert reg.pop(t) is None and not reg


def test_sweep_drops_the_dead_and_what_the_predicate_selects():
    reg = _new()
    live, marked, dead = torch.zeros(3), torch.zeros(5), torch.zeros(7)
    reg.put(live, consumed=False)
    reg.put(marked, consumed=True)
    reg.put(dead, consumed=False)
    del dead
    gc.collect()
    assert len(reg) == 3
    reg.sweep()
    assert len(reg) == 2 and live.data_ptr() in reg and marked.data_ptr() in reg
    reg.sweep(also=lambda r: r.consumed)
    assert len(reg) == 1 and reg.get(live) is not None and reg.get(marked) is None
    # a registry without weak references has no dead records: only the predicate drops
    strong = _new(weak=False)
    a, b = torch.zeros(3), torch.zeros(5)
    strong.put(a, x=1)
    strong.put(b, x=2)
    strong.sweep()
    assert len(strong) == 2
    strong.sweep(also=lambda r: r.x == 2)
    assert a.data_ptr() in strong and b.data_ptr() not in strong


def test_the_ten_registries_check_what_their_protocols_need(ops):
    H = pkg("_handover")
    assert ops._STEP_REGISTRIES is H.STEP and ops._ALL_REGISTRIES is H.ALL
    want = {"_relu_outputs": (True, True, False, True), "_premasked": (False, True, True, True), "_s2d_wanted": (True, True, False, True),
            "_s2d_grads": (False, True, True, True), "_deferred": (True, True, False, True), "_unmaterialized": (False, True, False, True),
            "_pooled_outputs": (True, True, False, False), "_blob_targets": (True, False, True, False), "_skip_registry": (True, True, False, False)}
    for name, (weak, shape, version, step) in want.items():
        reg = getattr(ops, name)
        assert isinstance(reg, H.Handover), name
        assert (reg.weak, reg.shape, reg.version) == (weak, shape, version), name
        assert any(reg is r for r in ops._ALL_REGISTRIES), name
        assert any(reg is r for r in ops._STEP_REGISTRIES) == step, name
    assert type(ops._s2d_produced) is set and any(ops._s2d_produced is r for r in ops._STEP_REGISTRIES)


def _seed_step_registries(ops):
    keep = []
    for reg in ops._STEP_REGISTRIES:
        t = torch.zeros(4)
        keep.append(t)
        if isinstance(reg, set):
            reg.add(t.data_ptr())
        else:
            reg.put(t)
        assert reg
    return keep


@pytest.mark.parametrize("raises", [False, True])
def test_the_context_empties_every_registry_of_a_step(ops, raises):
    keep = _seed_step_registries(ops)
    target, pooled_y = torch.zeros(2, 4, 4), torch.zeros(1, 2, 4, 4)
    ops._blob_targets.put(target, n=2, H=4, W=4, coords=torch.zeros(2, 2), tmpl=None, coords_version=0)
    pooled = ops._pooled_outputs.put(pooled_y, pooled=torch.zeros(1, 2, 2, 2), code=None)
    flags = (ops.skip_fold, ops.premask, ops.wgrad_branch)
    try:
        with ops.fold_skip_gradients():
            assert all(not reg for reg in ops._STEP_REGISTRIES)
            assert ops._blob_targets and ops._pooled_outputs.get(pooled_y) is pooled      # (neither is touched on enter)
            keep += _seed_step_registries(ops)
            if raises:
                raise KeyError("the body fails")
    except KeyError:
        assert raises
    else:
        assert not raises
    assert all(not reg for reg in ops._STEP_REGISTRIES)
    assert not ops._blob_targets
    assert ops._pooled_outputs.get(pooled_y) is pooled and len(ops._pooled_outputs) == 1
    assert (ops.skip_fold, ops.premask, ops.wgrad_branch) == flags


def test_skip_entry_lifecycle(ops):
    base = torch.zeros(2, 4, 4, 4)
    x = base[:]
    ops._skip_register(x)
    e = ops._skip_entry(x)
    assert e is not None and e.stash == [] and e.consumed is False and e.ref() is x and e.shape == (2, 4, 4, 4)
    assert ops._skip_entry(x) is e                                    # (asking does not consume)
    assert ops._skip_entry(base.view(2, 4, 16)) is None               # same address, another shape
    assert x.data_ptr() not in ops._skip_registry and ops._skip_entry(x) is None

    # a gradient handed over to a pool whose backward never ran does not outlive the context; an untouched entry of a live tensor does
    y = torch.zeros(3, 3)
    with ops.fold_skip_gradients():
        ops._skip_register(x)
        ops._skip_register(y)
        ops._skip_entry(x).stash.append((torch.zeros(1), None))
        assert len(ops._skip_registry) == 2
    assert ops._skip_entry(x) is None and ops._skip_entry(y) is not None and len(ops._skip_registry) == 1

    # a consumed entry (the pool's backward ran) goes with the next registration
    ops._skip_entry(y).consumed = True
    assert y.data_ptr() in ops._skip_registry
    z = torch.zeros(5)
    ops._skip_register(z)
    assert y.data_ptr() not in ops._skip_registry and ops._skip_entry(z) is not None and len(ops._skip_registry) == 1
    # ... and so does the entry of a tensor that is gone
    del z
    gc.collect()
    ops._skip_register(x)
    assert len(ops._skip_registry) == 1 and ops._skip_entry(x) is not None


def test_release_stale_entries_drops_the_dead_records_of_every_weak_registry(ops):
    weak = [r for r in ops._ALL_REGISTRIES if r.weak]
    assert {r.name for r in weak} >= {"relu_outputs", "s2d_wanted", "deferred", "pooled_outputs", "blob_targets", "skip_registry"}
    live, dead = [], []
    for reg in ops._ALL_REGISTRIES:
        a, b = torch.zeros(3), torch.zeros(5)
        fields = {"consumed": False, "stash": []} if reg is ops._skip_registry else {}
        reg.put(a, **fields)
        reg.put(b, **fields)
        live.append(a)
        dead.append(b.data_ptr())
        del b
    gc.collect()
    consumed = torch.zeros(7)
    ops._skip_registry.put(consumed, stash=[], consumed=True)
    ops.release_stale_entries()
    for reg, a, gone in zip(ops._ALL_REGISTRIES, live, dead):
        assert reg.get(a) is not None, reg
        assert (gone in reg) == (not reg.weak), reg      # (a registry without weak references cannot tell: its records go with the step)
    assert consumed.data_ptr() not in ops._skip_registry
    assert [len(r) for r in ops._ALL_REGISTRIES] == [1 if r.weak else 2 for r in ops._ALL_REGISTRIES]

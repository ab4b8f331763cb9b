"""Hand-overs between the step's autograd nodes: one producer writes a record under a tensor's address, one consumer
asks for it with the tensor it was handed (ops.py describes each protocol next to its registry; DESIGN.md section 4.6.1
has the table).  An address alone does not name a tensor -- the allocator reuses memory, views share it -- so a record is
only returned to a tensor that passes the checks its registry was made with.  Pure Python: no library, no device."""
import weakref
from types import SimpleNamespace

STEP = []      # the registries of ONE training step: fold_skip_gradients() empties each of them on enter and on exit
ALL = []       # every registry


class Handover:
    """Address of a tensor -> one record (.ref, .shape, .version and the named fields of put()), for ONE producer / consumer
    protocol.  A record is valid for `t` when, as far as this registry checks them: its shape is t's (`shape`), the tensor it
    was written for is alive (`weak`; without it no reference is kept: a gradient returned from a backward belongs to the
    autograd engine), and nobody wrote into t since (`version`)."""

    def __init__(self, name, *, weak=True, shape=True, version=False, step=True):
        self.name, self.weak, self.shape, self.version = name, weak, shape, version
        self._records = {}
        ALL.append(self)
        if step:
            STEP.append(self)

    def put(self, t, **fields):
        r = self._records[t.data_ptr()] = SimpleNamespace(ref=weakref.ref(t) if self.weak else None, shape=tuple(t.shape), version=t._version,
                                                          **fields)
        return r

    def get(self, t):
        """The record valid for `t`, or None; a record found under t's address that is not valid for it is dropped."""
        key = t.data_ptr()
        r = self._records.get(key)
        if r is None:
            return None
        if (self.shape and r.shape != tuple(t.shape)) or (self.weak and r.ref() is None) or (self.version and r.version != t._version):
            del self._records[key]
            return None
        return r

    def pop(self, t):
        r = self.get(t)
        if r is not None:
            del self._records[t.data_ptr()]
        return r

    def sweep(self, also=None):
        """Drop the records whose tensor is gone (weak registries) and those for which also(record) is true."""
        for key in [k for k, r in self._records.items() if (self.weak and r.ref() is None) or (also is not None and also(r))]:
            del self._records[key]

    def clear(self):
        self._records.clear()

    def values(self):
        return self._records.values()

    def __len__(self):
        return len(self._records)

    def __bool__(self):
        return bool(self._records)

    def __contains__(self, address):
        return address in self._records

    def __repr__(self):
        return f"Handover({self.name!r}, {len(self._records)} records)"

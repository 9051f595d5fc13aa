"""The one identity cache for host-side values derived from tensors (sampler keys, decoder tasks, known lists, CSRs, plans).

The rule, written once: a value is keyed by the identity and version of the tensors it was built from, the entry holds
those tensors for as long as it lives -- so an address can never name two different tensors --, and past the limit the
least recently used entry goes.
"""
from collections import OrderedDict

import torch


def identity(tensors):
    """The key of a tuple of tensors: a dense tensor by (storage address, version counter, shape, stride, dtype, device); a
    sparse one, which has no storage address, by the object itself; None, or a hashable given in a tensor's place, by value."""
    key = []
    for t in tensors:
        if not isinstance(t, torch.Tensor):
            key.append(t)
        elif t.layout is torch.strided:
            key.append((t.data_ptr(), t._version, t.shape, t.stride(), t.dtype, t.device))
        else:
            key.append((id(t), t.shape, t.dtype, t.device))
    return tuple(key)


def keyable(x):
    """An argument that is a tensor or a small nested list (a range list) as a member of `tensors`: the tensor itself, the
    list by value -- never the address of a temporary tensor made from the list."""
    return x if isinstance(x, torch.Tensor) else tuple(map(tuple, x))


class DerivedCache(object):
    """At most `limit` values, each built once per (tensors, extra).  `extra` is any hashable the value depends on besides:
    sizes, flags, a small range list by value.  In-place modification of a tensor (its version counter) or another view of
    its storage is another key.  None is a value like any other."""

    def __init__(self, limit):
        self.limit = limit
        self._entries = OrderedDict()                  # key -> (value, the tensors the key names)

    def get(self, tensors, extra, build):
        key = (identity(tensors), extra)
        hit = self._entries.get(key)
        if hit is None:
            hit = self._entries[key] = (build(), tensors)
            if len(self._entries) > self.limit:
                self._entries.popitem(last=False)
        else:
            self._entries.move_to_end(key)
        return hit[0]

    def clear(self):
        self._entries.clear()

    def __len__(self):
        return len(self._entries)

    # Derived state (device arrays, closures) is never pickled or copied: `torch.save(model, ...)`, `copy.deepcopy` and
    # multiprocessing work after a forward pass, and the copy rebuilds on first use.
    def __reduce__(self):
        return (type(self), (self.limit,))

"""Tensors derived from parameters outside the backbone ("shadows": fp16 / bf16 copies that are re-laid-out, padded,
transposed or split), built on first use and rebuilt when a tensor they depend on was written to or moved.

``of(owner).get(slot, params, build)`` is the whole interface.  The holders live in a registry beside the modules, not
on them: nothing here is pickled, deep-copied or listed in a state dict, a copy of a module starts with an empty holder,
and a holder dies with its owner.  (The backbone's ``engine.ShadowCache`` refreshes its copies in place, in one batched
launch per step, and is a mechanism of its own.)"""
import weakref


class Holder:
    """slot name -> (key, value): the key names every tensor the value was built from."""

    def __init__(self):
        self.slots = {}

    def get(self, slot, params, build):
        """The value of ``slot``; ``build()`` runs when an entry of ``params`` (tensors or None) has a new version
        counter, address or dtype since the value was made."""
        key = tuple(None if t is None else (t._version, t.data_ptr(), t.dtype) for t in params)
        hit = self.slots.get(slot)
        if hit is None or hit[0] != key:
            hit = self.slots[slot] = (key, build())
        return hit[1]


# keyed by the owning module (identity hash), never by a tensor: Tensor.__eq__ is element-wise
_holders = weakref.WeakKeyDictionary()


def of(owner):
    """The holder of ``owner``, made on first use."""
    h = _holders.get(owner)
    if h is None:
        h = _holders[owner] = Holder()
    return h

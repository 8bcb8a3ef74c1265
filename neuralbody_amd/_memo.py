"""The memo behind every host-side cache.  The rules of DESIGN.md ("Nothing about a frame lives on the host") hold here once: an
entry holds what it was built from (`tkey` keeps the tensors and storages), so no address can be recycled under its key; an
in-place write is a miss (version counters are part of the key); a caller's `frame_token` is part of a frame's key (the caller
puts it in: a write through a raw pointer bumps no version).  A `Memo` deep-copies and pickles as an empty one."""


class tkey:  # noqa: N801 (called like a function: tkey(t), tkey(*params))
    """Key part for one or more tensors: equal to the `tkey` of the same tensor objects over the same storages, data pointers,
    version counters and shapes.  Holds the tensors and their storages, so no address (and no object id) can be handed to another
    tensor while the key lives."""

    __slots__ = ("tensors", "storages", "sig")

    def __init__(self, *tensors):
        storages = [t.untyped_storage() for t in tensors]
        self.tensors, self.storages = tensors, storages
        self.sig = [(id(t), s._cdata, t.data_ptr(), t._version, t.shape) for t, s in zip(tensors, storages)]

    def __eq__(self, other):
        return isinstance(other, tkey) and self.sig == other.sig

    __hash__ = None


class Memo:
    """Named slots, each of the last `size` (key, value) pairs, most recently used last (size 1 unless given: `Memo(order_full=8)`).
    Keys are tuples whose parts compare with `==`; tensors go in as `tkey(t)`."""

    def __init__(self, **sizes):
        self._sizes = sizes
        self._slots = {}

    def get(self, slot, key, build=None):
        """The value stored under an equal key; otherwise `build()`, stored and returned (nothing is stored if it raises), or None
        without a `build`."""
        entries = self._slots.get(slot, ())
        if entries and entries[-1][0] == key:
            return entries[-1][1]
        for i, (k, v) in enumerate(entries):
            if k == key:
                if i != len(entries) - 1:
                    entries.append(entries.pop(i))
                return v
        if build is None:
            return None
        value = build()
        entries = self._slots.setdefault(slot, [])
        entries.append((key, value))
        del entries[:-self._sizes.get(slot, 1)]
        return value

    def peek(self, slot):
        """The most recently used value of `slot`, None if it is empty (tests, diagnostics)."""
        entries = self._slots.get(slot)
        return entries[-1][1] if entries else None

    def clear(self, slot=None):
        self._slots.clear() if slot is None else self._slots.pop(slot, None)

    def __deepcopy__(self, memo):
        return Memo(**self._sizes)

    def __reduce__(self):
        return Memo, (), {"_sizes": self._sizes}

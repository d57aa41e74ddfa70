"""Device key map: 64-bit feature ids to table rows, in call order (an extension; include/glint_gpu.h, "Key map").

A ``KeyMap`` is an insert-only hash table on one GPU. It stands in front of the row calls for workloads whose
records carry feature ids -- arbitrary, sparse, unbounded int64 values, new ones in every batch -- and not row
numbers, so that no host dictionary and no host synchronisation sits between "which rows?" and the row call:

    ids = KeyMap(capacity)                                          # or client.keymap(capacity)
    rows = ids.insert(ids_dev, sync=False)                          # device tensors, the current stream
    table.updateRowsAdagrad(state, rows, grads_dev, lr, sync=False)  # same stream: no id crosses the link
    ...
    ids.sync()                                                      # raises what an unsynced call refused

Rows are handed out in call order -- the j-th distinct new key of a call, by first occurrence, gets row
``firstRow + size + j`` -- so they are a function of the insert calls and their keys only: not of the table
size, the hash, the launch shape, the host or device form, or of how a call's keys are split over calls.
``INT64_MIN`` is reserved (it marks an empty slot) and is no key.

Calls on one map are ordered by the caller: one stream, or events between streams. Lookups may overlap each
other; nothing may overlap an insert.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .errors import ArrayIndexOutOfBoundsException, KeyMapFullException
from .shard import _host, _is_torch_cuda, check


def _host_keys(x, name: str) -> np.ndarray:
    a = np.asarray(x)
    if a.size and (a.dtype.kind not in "iu" or (a.dtype == np.uint64 and int(a.max()) >= 1 << 63)):
        raise TypeError(f"{name}: expected int64 values, not {a.dtype}")
    return _host(a, np.int64).reshape(-1)


class KeyMap:
    """``KeyMap(capacity, firstRow=0, device=0, slots=None)``: an empty map of up to ``capacity`` keys to the
    rows ``firstRow .. firstRow + capacity - 1``. ``slots`` is the table size, a power of two with ``capacity <
    slots <= 2**30`` (so a miss always ends at an empty slot); the default is the least power of two ``>= 2 *
    capacity``. Anything else raises ValueError."""

    def __init__(self, capacity: int, firstRow: int = 0, device: int = 0, slots=None):
        self.lib = N.load()
        self._h = C.c_void_p()
        check(self.lib.glint_keymap_create(int(device), int(capacity), int(firstRow), 0 if slots is None else int(slots),
                                           C.byref(self._h)))
        self.capacity, self.firstRow, self.slots, self.device = self._static()

    # lifetime -------------------------------------------------------------------------------
    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise ValueError("key map already destroyed")
        return self._h

    def destroy(self) -> None:
        """Frees the map; calls enqueued with ``sync=False`` must have finished."""
        if getattr(self, "_h", None):
            check(self.lib.glint_keymap_destroy(self._h))
            self._h = C.c_void_p()

    close = destroy

    def __del__(self):
        try:
            self.destroy()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.destroy()

    def _static(self) -> tuple:
        cap, fr, sl, dev = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        check(self.lib.glint_keymap_info(self.handle, C.byref(cap), C.byref(fr), C.byref(sl), None, C.byref(dev)))
        return cap.value, fr.value, sl.value, dev.value

    def info(self) -> tuple:
        """(capacity, firstRow, slots, size, device); ``size`` lives on the device, so this waits for the
        device's enqueued work."""
        size = C.c_int64()
        check(self.lib.glint_keymap_info(self.handle, None, None, None, C.byref(size), None))
        return self.capacity, self.firstRow, self.slots, size.value, self.device

    def size(self) -> int:
        """The number of keys in the map. Synchronises, and raises what a ``sync=False`` call on the current
        stream refused, as ``sync`` does."""
        self.sync()
        return self.info()[3]

    def __len__(self) -> int:
        return self.size()

    def sync(self, stream=None) -> None:
        """Waits for ``stream`` (default: the current torch stream of the map's device) and raises if a
        device-form call since the last report was refused: ArrayIndexOutOfBoundsException with the lowest
        refused index in ``.record`` (the reserved key, or a row outside the map for ``keysOf``), or
        KeyMapFullException with the least free row count of an insert that overflowed."""
        if stream is None:
            import torch
            stream = torch.cuda.current_stream(torch.device("cuda", self.device)).cuda_stream
        bad, free = C.c_int64(-1), C.c_int64(-1)
        self._raise(self.lib.glint_keymap_sync(self.handle, stream, C.byref(bad), C.byref(free)), bad, free, "call")

    def _raise(self, rc: int, bad, free, what: str) -> None:
        if rc == N.GLINT_EOUTOFRANGE:
            if bad.value >= 0:
                raise ArrayIndexOutOfBoundsException(f"{what}: record {bad.value} is refused (the reserved key "
                                                     "INT64_MIN, or a row that owns no key)", bad.value)
            raise KeyMapFullException(f"{what}: more new keys than the {free.value} free rows of the key map",
                                      free.value)
        check(rc)

    # calls ----------------------------------------------------------------------------------
    def _call(self, what: str, x, out, sync: bool, host, dev):
        """One call over the int64 values ``x``: the device form (``x`` a contiguous int64 torch tensor on the
        map's device; ``out`` None or such a tensor of its size) launches on the current stream and waits --
        and raises -- only with ``sync``; the host form (anything numpy takes) returns a numpy array, ends
        synchronised and raises at once."""
        if _is_torch_cuda(x) or _is_torch_cuda(out):
            import torch
            if out is None:
                out = torch.empty(x.numel(), dtype=torch.int64, device=x.device)
            for name, t in ((what, x), ("out", out)):
                if not _is_torch_cuda(t):
                    raise TypeError(f"{name}: expected a CUDA tensor (mixing host arrays and device tensors)")
                if t.device.index != self.device:
                    raise ValueError(f"{name} on cuda:{t.device.index}, key map on cuda:{self.device}")
                if t.dtype != torch.int64 or not t.is_contiguous():
                    raise TypeError(f"{name}: expected a contiguous int64 tensor")
            if out.numel() != x.numel():
                raise ValueError(f"out: {out.numel()} elements, expected {x.numel()}")
            stream = torch.cuda.current_stream(x.device).cuda_stream
            check(dev(x.data_ptr(), x.numel(), out.data_ptr(), stream))
            if sync:
                self.sync(stream)
            return out
        k = _host_keys(x, what)
        if out is not None:
            raise TypeError("out: only the device form takes it")
        res = np.empty(k.size, np.int64)
        bad, free = C.c_int64(-1), C.c_int64(-1)
        rc = host(k.ctypes.data if k.size else None, k.size, res.ctypes.data if k.size else None, bad, free)
        self._raise(rc, bad, free, what)
        return res

    def insert(self, keys, out=None, sync: bool = True):
        """One row per record: the row of a key already in the map, and for the distinct new keys of the call,
        numbered ``j = 0, 1, ..`` by first occurrence, row ``firstRow + size + j``; ``size`` then grows by
        their number. A call that names INT64_MIN raises ArrayIndexOutOfBoundsException (lowest index in
        ``.record``); one with more new keys than free rows raises KeyMapFullException (``.free``). Either way
        the map is exactly as before, and a device-form ``out`` holds the rows of the keys already present
        and -1 elsewhere."""
        return self._call("keys", keys, out, sync,
                          lambda k, n, o, bad, free: self.lib.glint_keymap_insert(self.handle, k, n, o, C.byref(bad),
                                                                                  C.byref(free)),
                          lambda k, n, o, st: self.lib.glint_keymap_insert_dev(self.handle, k, n, o, st))

    def lookup(self, keys, missing: int = -1, out=None, sync: bool = True):
        """One row per record, ``missing`` for a key not in the map; reads only. INT64_MIN is refused as by
        ``insert``."""
        missing = int(missing)
        return self._call("keys", keys, out, sync,
                          lambda k, n, o, bad, free: self.lib.glint_keymap_lookup(self.handle, k, n, missing, o,
                                                                                  C.byref(bad)),
                          lambda k, n, o, st: self.lib.glint_keymap_lookup_dev(self.handle, k, n, missing, o, st))

    def keysOf(self, rows, out=None, sync: bool = True):
        """The inverse: the key that owns each row, for rows in ``[firstRow, firstRow + size)`` -- what turns
        ``pullTopK``'s rows back into ids, and what a checkpoint exports. Any other row raises
        ArrayIndexOutOfBoundsException with its index."""
        return self._call("rows", rows, out, sync,
                          lambda r, n, o, bad, free: self.lib.glint_keymap_keys_of(self.handle, r, n, o, C.byref(bad)),
                          lambda r, n, o, st: self.lib.glint_keymap_keys_of_dev(self.handle, r, n, o, st))


__all__ = ["KeyMap"]

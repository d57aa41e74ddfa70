"""Seeded weighted row sampler on the device (an extension; include/glint_gpu.h, "Row sampler").

A ``Sampler`` is an immutable cumulative table on one GPU, built once from integer weights (word counts, or
``round(count ** 0.75 * scale)`` computed by the caller). Draw number ``d`` under seed ``s`` is one fixed key,
whoever asks for it and in whatever batch, so a skip-gram step draws its negatives next to the rows:

    sampler = Sampler(counts)                                   # or Sampler.fromShard(countsShard)
    neg = sampler.draw(n * k, seed, first=step * n * k, exclude=positives, per=k, sync=False)  # device tensors
    scores = syn1.getPairsDot(syn0, neg, centres, sync=False)   # same stream: no id crosses the link

and the later adjusting call regenerates the same ``neg`` from (seed, first). A host caller (numpy arrays)
gets the same keys.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _native as N
from .errors import ArrayIndexOutOfBoundsException
from .shard import PartialVector, _host, _is_torch_cuda, check


def _u64(x, name: str) -> int:
    x = int(x)
    if not 0 <= x < 1 << 64:
        raise ValueError(f"{name}: expected an unsigned 64-bit integer")
    return x


class Sampler:
    """``Sampler(weights, firstKey=0, device=0)``: entry ``i`` of ``weights`` (integers in [0, 2^32), at least
    one of them non-zero) is the weight of global key ``firstKey + i``. ``weights`` is a host array, or an
    int64 torch tensor on ``device`` (read after the work on the current stream; the create ends
    synchronised). A weight outside the range raises ArrayIndexOutOfBoundsException with its index."""

    def __init__(self, weights, firstKey: int = 0, device: int = 0):
        self.lib = N.load()
        self._h = C.c_void_p()
        bad = C.c_int64(-1)
        if _is_torch_cuda(weights):
            import torch
            device = weights.device.index
            if weights.dtype != torch.int64 or not weights.is_contiguous():
                raise TypeError("weights: expected a contiguous int64 device tensor")
            rc = self.lib.glint_sampler_create_dev(device, weights.data_ptr(), weights.numel(), int(firstKey),
                                                   torch.cuda.current_stream(weights.device).cuda_stream,
                                                   C.byref(bad), C.byref(self._h))
        else:
            w = np.asarray(weights)
            if w.dtype.kind not in "iu":
                raise TypeError(f"weights: expected integers, not {w.dtype} (round them first)")
            if w.dtype == np.uint64 and w.size and int(w.max()) >= 1 << 63:
                raise ArrayIndexOutOfBoundsException("weight outside [0, 2^32)", int(np.argmax(w >= 1 << 63)))
            w = _host(w, np.int64).reshape(-1)
            rc = self.lib.glint_sampler_create(int(device), w.ctypes.data if w.size else None, w.size, int(firstKey),
                                               C.byref(bad), C.byref(self._h))
        self._created(rc, bad)

    @classmethod
    def fromShard(cls, counts: PartialVector) -> "Sampler":
        """A sampler over a counts shard -- a range PartialVector of Int or Long, accumulated by ordinary
        pushes -- with the shard's first key and size. The shard is only read; the call is ordered after the
        shard's earlier work and ends synchronised."""
        if not isinstance(counts, PartialVector):
            raise TypeError("fromShard: expected a PartialVector")
        self = cls.__new__(cls)
        self.lib = counts.lib
        self._h = C.c_void_p()
        bad = C.c_int64(-1)
        self._created(self.lib.glint_sampler_create_from_shard(counts.handle, C.byref(bad), C.byref(self._h)), bad)
        return self

    def _created(self, rc: int, bad) -> None:
        if rc == N.GLINT_EOUTOFRANGE:
            raise ArrayIndexOutOfBoundsException(f"weight {bad.value} is outside [0, 2^32)", bad.value)
        check(rc)
        self.m, self.firstKey, self.total, self.device = self.info()

    # lifetime -------------------------------------------------------------------------------
    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise ValueError("sampler already destroyed")
        return self._h

    def destroy(self) -> None:
        """Frees the table; draws enqueued with ``sync=False`` must have finished."""
        if getattr(self, "_h", None):
            check(self.lib.glint_sampler_destroy(self._h))
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

    def info(self) -> tuple:
        """(m, firstKey, total, device)."""
        m, fk, tot, dev = C.c_int64(), C.c_int64(), C.c_int64(), C.c_int()
        check(self.lib.glint_sampler_info(self.handle, C.byref(m), C.byref(fk), C.byref(tot), C.byref(dev)))
        return m.value, fk.value, tot.value, dev.value

    # draws ----------------------------------------------------------------------------------
    def draw(self, n: int, seed: int, first: int = 0, exclude=None, per: int = 1, out=None, sync: bool = True):
        """``n`` global keys, draw ``i`` taken with counter ``first + i`` (mod 2^64) under ``seed``: a function
        of (weights, firstKey, seed, first + i) only, so a range of counters split over calls, ranks or batch
        layouts gives the same keys. With ``exclude`` -- ``ceil(n / per)`` global keys -- draw ``i`` avoids
        ``exclude[i // per]`` (the positive its ``per`` negatives are drawn for) by the retry rule
        include/glint_gpu.h fixes; a key outside the table excludes nothing.

        Host arrays (``exclude`` and ``out`` None or numpy): a numpy int64 array comes back and the call ends
        synchronised. Device tensors (``exclude`` or ``out`` a torch tensor on the sampler's device; with
        neither, host): one launch on the current stream, a device tensor returned or ``out`` (int64,
        contiguous, ``n`` elements) filled; ``sync=False`` leaves the wait to the stream's next consumer."""
        n, per = int(n), int(per)
        seed, first = _u64(seed, "seed"), _u64(first, "first")
        need = -(-n // per) if per >= 1 and n > 0 else 0
        if _is_torch_cuda(exclude) or _is_torch_cuda(out):
            import torch
            for name, t, want in (("exclude", exclude, need), ("out", out, n)):
                if t is None:
                    continue
                if not _is_torch_cuda(t):
                    raise TypeError(f"{name}: expected a CUDA tensor (mixing host arrays and device tensors)")
                if t.device.index != self.device:
                    raise ValueError(f"{name} on cuda:{t.device.index}, sampler on cuda:{self.device}")
                if t.dtype != torch.int64 or not t.is_contiguous():
                    raise TypeError(f"{name}: expected a contiguous int64 tensor")
                if t.numel() != want and per >= 1:
                    raise ValueError(f"{name}: {t.numel()} elements, expected {want}")
            dev = torch.device("cuda", self.device)
            if out is None:
                out = torch.empty(max(n, 0), dtype=torch.int64, device=dev)
            rc = self.lib.glint_sampler_draw_dev(self.handle, seed, first, n,
                                                 None if exclude is None else exclude.data_ptr(), per,
                                                 out.data_ptr(), torch.cuda.current_stream(dev).cuda_stream)
            check(rc)
            if sync:
                torch.cuda.current_stream(dev).synchronize()
            return out
        ex = None
        if exclude is not None:
            ex = _host(exclude, np.int64).reshape(-1)
            if per >= 1 and ex.size != need:
                raise ValueError(f"exclude: {ex.size} keys, expected {need}")
            if ex.size == 0:  # (an empty array's data pointer may be NULL, which would mean no exclusion)
                ex = np.zeros(1, np.int64)
        if out is None:
            out = np.empty(max(n, 0), np.int64)
        elif not isinstance(out, np.ndarray) or out.dtype != np.int64 or out.shape != (n,) \
                or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"out must be a writable C-contiguous int64 array of shape ({n},)")
        # (an empty array's data pointer is passed as it is: n == 0 stores nothing)
        check(self.lib.glint_sampler_draw(self.handle, seed, first, n, None if ex is None else ex.ctypes.data, per,
                                          out.ctypes.data if out.size else None))
        return out


__all__ = ["Sampler"]

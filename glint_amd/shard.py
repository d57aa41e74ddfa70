"""Host-side mirror of Glint's server-side partial models, backed by HBM shards.

``PartialVector`` / ``PartialMatrix`` keep the reference's method names and argument meaning
(src/main/scala/glint/models/server/PartialVector.scala:16-64, PartialMatrix.scala:17-87):

    vec = PartialVector(RangePartition(0, 0, 1000), "double")
    vec.update(keys, values)      # PartialVector.update  -> True
    vec.get(keys)                 # PartialVector.get     -> array of values

Every operation runs the HIP kernels through the C ABI (include/glint_gpu.h). Arguments may be
numpy arrays (host path: staged H2D, synchronous like the actor's ``update``) or torch CUDA tensors
on the shard's device (device-resident path, stream-ordered on torch's current stream; the call
synchronises only when ``sync=True``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np

from . import _native as N
from .errors import ArrayIndexOutOfBoundsException, GlintDeviceError
from .partitioning import CyclicPartition, Partition, RangePartition

_DTYPES = {
    "int": (N.GLINT_I32, np.int32), "int32": (N.GLINT_I32, np.int32), "i32": (N.GLINT_I32, np.int32),
    "long": (N.GLINT_I64, np.int64), "int64": (N.GLINT_I64, np.int64), "i64": (N.GLINT_I64, np.int64),
    "float": (N.GLINT_F32, np.float32), "float32": (N.GLINT_F32, np.float32), "f32": (N.GLINT_F32, np.float32),
    "double": (N.GLINT_F64, np.float64), "float64": (N.GLINT_F64, np.float64), "f64": (N.GLINT_F64, np.float64),
}


def resolve_dtype(dtype) -> tuple:
    """Map a value type ('double', np.float64, 'Int', ...) to (GLINT_* code, numpy dtype)."""
    if isinstance(dtype, str):
        key = dtype.lower()
    else:
        key = np.dtype(dtype).name
    if key not in _DTYPES:
        raise ValueError(f"unsupported value type {dtype!r} (Int, Long, Float or Double)")
    return _DTYPES[key]


def check(rc: int, handle=None, rec: Optional[int] = None) -> None:
    """Translate a C ABI status into the reference's exception types."""
    if rc == N.GLINT_OK:
        return
    if rc == N.GLINT_EOUTOFRANGE:
        if rec is None:  # (wait and sync get the record with the status)
            v = C.c_int64(-1)
            if handle is not None:
                N.load().glint_shard_last_error(handle, C.byref(v))
            rec = v.value
        raise ArrayIndexOutOfBoundsException(f"record {rec} is outside the partition", rec)
    if rc == N.GLINT_EDEVICE:
        raise GlintDeviceError(N.strerror(rc))
    if rc == N.GLINT_ENOMEM:
        raise MemoryError(N.strerror(rc))
    raise ValueError(N.strerror(rc))


def _flags(deterministic: bool, unordered: bool) -> int:
    return (N.GLINT_PUSH_DETERMINISTIC if deterministic else 0) | (N.GLINT_PUSH_UNORDERED if unordered else 0)


def _addr(x) -> int:
    """A raw address (int) as it is, else the tensor's data pointer."""
    return x if isinstance(x, int) else x.data_ptr()


def _is_torch_cuda(x) -> bool:
    return type(x).__module__.startswith("torch") and getattr(x, "is_cuda", False)


def _host(x, dtype) -> np.ndarray:
    return np.ascontiguousarray(np.asarray(x, dtype=dtype))


def _host_offsets(offsets) -> tuple:
    """Host ``offsets`` of a grouped call as (flat int64 array, g)."""
    o = _host(offsets, np.int64).reshape(-1)
    if o.size < 1:
        raise ValueError("offsets needs g + 1 entries")
    return o, o.size - 1


def _check_like(name: str, t, dtype, rows, elems: Optional[int] = None) -> None:
    """A further device argument of a row call: a contiguous ``dtype`` CUDA tensor on the device of ``rows``
    (which _check_dev ties to the shard's), of ``elems`` elements where the call fixes its size -- the kernels
    take raw pointers."""
    if not _is_torch_cuda(t) or t.dtype != dtype or not t.is_contiguous() or t.device != rows.device:
        raise TypeError(f"{name}: expected a contiguous {dtype} CUDA tensor on rows' device")
    if elems is not None and t.numel() != elems:
        raise ValueError(f"{name}: {t.numel()} elements, expected {elems}")


def _check_offsets_dev(offsets, rows) -> int:
    """Device ``offsets`` of a grouped call, as _check_like with at least one entry; returns g."""
    import torch
    if not _is_torch_cuda(offsets) or offsets.dtype != torch.int64 or not offsets.is_contiguous() \
            or offsets.device != rows.device or offsets.numel() < 1:
        raise TypeError("offsets: expected a contiguous int64 CUDA tensor of g + 1 entries on rows' device")
    return offsets.numel() - 1


# wire types of the narrow-format row transport (glint_mat_pull_rows_as / glint_mat_push_rows_as):
# name -> (GLINT_WIRE_* code, numpy dtype of host arrays, torch dtype name of device tensors). numpy has no
# bfloat16, so host arrays hold its 16-bit patterns (to_bfloat16 / from_bfloat16).
_WIRES = {
    "float16": (N.GLINT_WIRE_F16, np.float16, "float16"),
    "bfloat16": (N.GLINT_WIRE_BF16, np.uint16, "bfloat16"),
    "float32": (N.GLINT_WIRE_F32, np.float32, "float32"),
}


def resolve_wire(wire) -> tuple:
    """Map a wire type name to (GLINT_WIRE_* code, numpy dtype, torch dtype name)."""
    if not isinstance(wire, str) or wire not in _WIRES:
        raise ValueError(f"unsupported wire type {wire!r} ('float16', 'bfloat16' or 'float32')")
    return _WIRES[wire]


def to_bfloat16(x) -> np.ndarray:
    """float32 array -> its bfloat16 bit patterns (uint16), the narrowing glint_wire_plan.h fixes: round to
    nearest even on the float's bits u, ``(u + 0x7FFF + ((u >> 16) & 1)) >> 16``; overflow gives an infinity,
    subnormals are kept, a NaN stays a (quiet) NaN."""
    x = np.asarray(x)
    if x.dtype != np.float32:
        raise TypeError(f"to_bfloat16 takes float32, not {x.dtype}")
    u = np.ascontiguousarray(x).view(np.uint32).astype(np.uint64)  # 64 bits: the sum below cannot wrap
    c = np.uint64
    r = (u + c(0x7FFF) + ((u >> c(16)) & c(1))) >> c(16)
    nan = (u & c(0x7FFFFFFF)) > c(0x7F800000)
    return np.where(nan, (u >> c(16)) | c(0x40), r).astype(np.uint16)


def from_bfloat16(b) -> np.ndarray:
    """bfloat16 bit patterns (uint16) -> the equal float32 values: exact, the pattern is the float's upper half."""
    b = np.asarray(b)
    if b.dtype != np.uint16:
        raise TypeError(f"from_bfloat16 takes uint16 bit patterns, not {b.dtype}")
    return (np.ascontiguousarray(b).astype(np.uint32) << np.uint32(16)).view(np.float32)


class HostBuffer:
    """Pinned, device-mapped host memory from glint_host_alloc: the buffers a server answers pulls
    from. A message-sized pull whose ``out`` lies in one is answered by the kernel straight into it
    (no copy out of the ring slot when it retires). ``array(dtype, count, offset)`` views a part of it
    as a numpy array; free() (or leaving the ``with`` block) only once no pull into it is pending."""

    def __init__(self, nbytes: int):
        self.lib = N.load()
        p = C.c_void_p()
        check(self.lib.glint_host_alloc(int(nbytes), C.byref(p)))
        self.ptr, self.nbytes = p.value, int(nbytes)

    def array(self, dtype, count: int, offset: int = 0) -> np.ndarray:
        dt = np.dtype(dtype)
        if offset < 0 or offset + count * dt.itemsize > self.nbytes:
            raise ValueError("outside the buffer")
        raw = (C.c_char * (count * dt.itemsize)).from_address(self.ptr + offset)
        return np.frombuffer(raw, dtype=dt, count=count)

    def free(self) -> None:
        if self.ptr:
            check(self.lib.glint_host_free(self.ptr))
            self.ptr = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()


class _Shard:
    def __init__(self, partition: Partition, dtype, cols: int = 0, device: int = 0):
        self.lib = N.load()
        self.partition = partition
        self.code, self.np_dtype = resolve_dtype(dtype)
        self.device = int(device)
        self._h = C.c_void_p()
        if isinstance(partition, RangePartition):
            rc = self.lib.glint_shard_create(self.device, self.code, partition.start, partition.end, int(cols),
                                             C.byref(self._h))
        elif isinstance(partition, CyclicPartition):
            rc = self.lib.glint_shard_create_cyclic(self.device, self.code, partition.index,
                                                    partition.numberOfPartitions, partition.numberOfKeys,
                                                    int(cols), C.byref(self._h))
        else:
            raise TypeError(f"unsupported partition type {type(partition).__name__}")
        check(rc)
        self._read_info()

    def _read_info(self) -> None:
        sz, cl = C.c_int32(), C.c_int32()
        check(self.lib.glint_shard_info(self._h, C.byref(sz), C.byref(cl), None, None), self._h)
        self.size, self.cols = sz.value, cl.value

    @classmethod
    def view(cls, slab: "_Shard", partition: RangePartition, offset: int):
        """A shard over ``partition`` whose elements are rows [offset, offset + size) of ``slab``
        (glint_shard_create_in): the partitions a server hosts, kept in one allocation so that one
        device-resident call on the slab serves all of them. Destroy views before their slab."""
        if not isinstance(partition, RangePartition):
            raise TypeError("a slab view takes a RangePartition")
        self = cls.__new__(cls)
        self.lib, self.partition, self.device = slab.lib, partition, slab.device
        self.code, self.np_dtype = slab.code, slab.np_dtype
        self._h = C.c_void_p()
        check(self.lib.glint_shard_create_in(slab.handle, int(offset), partition.start, partition.end, C.byref(self._h)))
        self._read_info()
        if self.cols:
            self.rows = self.size
        self.slab = slab
        return self

    # lifetime -------------------------------------------------------------------------------
    @property
    def handle(self) -> C.c_void_p:
        if not self._h:
            raise ValueError("shard already destroyed")
        return self._h

    def destroy(self) -> None:
        if self._h:
            check(self.lib.glint_shard_destroy(self._h))  # (a slab with live views refuses: EINVAL)
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

    def zero(self) -> None:
        """What an Akka restart produces: a freshly constructed, zeroed partial model."""
        check(self.lib.glint_shard_zero(self.handle), self.handle)

    def _init_call(self, name: str, rows, sync: bool, args: tuple) -> bool:
        """fill / initUniform: ``rows`` None names every row (element) of the partition, a numpy array of
        global keys takes the host call, a torch device tensor the device call on the current stream."""
        if rows is None or not _is_torch_cuda(rows):
            if rows is None:
                check(getattr(self.lib, name)(self.handle, None, 0, *args), self.handle)
                return True
            r = _host(rows, np.int64).reshape(-1)
            # (an empty array names nothing, but its data pointer may be NULL, which would name every row)
            p = r if r.size else np.zeros(1, np.int64)
            check(getattr(self.lib, name)(self.handle, p.ctypes.data, r.size, *args), self.handle)
            return True
        n = rows.numel()
        self._check_dev(n, rows)
        if n == 0:  # names nothing (its data pointer may be NULL, which would name every row)
            return True
        rc = getattr(self.lib, name + "_dev")(self.handle, rows.data_ptr(), n, *args, self._stream_of(rows))
        self._dev_done(rc, rows, sync)
        return True

    def fill(self, value, rows=None, sync: bool = True) -> bool:
        """Every element of the named rows = ``value`` (an extension; glint_shard_fill*), written on the
        device: the initial value of an Adagrad accumulator. ``value`` is converted to the shard's type once
        and stored as those bytes: -0.0 and a NaN's payload and sign are kept. ``rows`` None: the whole
        partition. A numpy array of global keys (any order, repeats allowed): every row is checked first,
        one outside the partition raises with the lowest such index and nothing is written. A torch device
        tensor: one stream-ordered launch on the current stream; such a row is skipped and raised by
        ``sync`` (``sync=True``, or a later ``sync()``). Unnamed rows and the row padding are untouched."""
        v = np.asarray(value).astype(self.np_dtype).reshape(1)  # (a value of the shard's type keeps its bits)
        return self._init_call("glint_shard_fill", rows, sync, (v.ctypes.data,))

    def initUniform(self, seed: int, lo: float, hi: float, rows=None, sync: bool = True) -> bool:
        """Seeded uniform init of the named rows (an extension; glint_shard_init_uniform*; Float and
        Double), generated on the device: element (global row g, column c) is ``lo + u * (hi - lo)`` with
        ``u`` in [0, 1) taken from Philox4x32-10 under counter (g, c's block) and key ``seed`` -- a function
        of (seed, g, c, lo, hi, dtype) only, whatever the partition or device (include/glint_gpu.h fixes
        every bit; the result lies in [lo, hi]). ``seed`` is a 64-bit unsigned integer. ``rows`` and
        ``sync`` as for ``fill``; naming a row again writes the same bits."""
        seed = int(seed)
        if not 0 <= seed < 1 << 64:
            raise ValueError("seed: expected an unsigned 64-bit integer")
        return self._init_call("glint_shard_init_uniform", rows, sync, (seed, float(lo), float(hi)))

    def data_ptr(self) -> int:
        p = C.c_void_p()
        check(self.lib.glint_shard_data(self.handle, C.byref(p)), self.handle)
        return p.value or 0

    # pipelined host ingest (include/glint_gpu.h): enqueue now, wait for the ticket before acknowledging
    def push_async(self, *arrays, deterministic: bool = False, unordered: bool = False) -> int:
        """Stage (keys, values) -- or (rows, cols, values) for a matrix -- in a pinned ring slot and
        enqueue the push; returns its ticket (glint_stage_acquire + glint_push_staged). A record outside
        the partition raises ArrayIndexOutOfBoundsException here, at the message (as update() throws in
        the reference), and nothing of the message is applied."""
        mat = self.cols != 0
        if len(arrays) != (3 if mat else 2):
            raise ValueError("push_async(keys, values) for vectors, (rows, cols, values) for matrices")
        keys = _host(arrays[0], np.int64).reshape(-1)
        cols = _host(arrays[1], np.int32).reshape(-1) if mat else None
        vals = _host(arrays[-1], self.np_dtype).reshape(-1)
        if keys.size != vals.size or (mat and cols.size != keys.size):
            raise ValueError("argument lengths differ")
        n = keys.size
        kp, cp, vp, slot = C.c_void_p(), C.c_void_p(), C.c_void_p(), C.c_int(-1)
        check(self.lib.glint_stage_acquire(self.handle, n, C.byref(kp), C.byref(cp), C.byref(vp), C.byref(slot)),
              self.handle)
        if n:
            C.memmove(kp.value, keys.ctypes.data, keys.nbytes)
            if mat:
                C.memmove(cp.value, cols.ctypes.data, cols.nbytes)
            C.memmove(vp.value, vals.ctypes.data, vals.nbytes)
        ticket = C.c_uint64()
        check(self.lib.glint_push_staged(self.handle, slot.value, n, _flags(deterministic, unordered),
                                         C.byref(ticket)), self.handle)
        return ticket.value

    def push_wire_async(self, payload: bytes, deterministic: bool = False):
        """Enqueue a RequestSerializer push image; returns (message id, ticket)."""
        buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
        mid, ticket = C.c_int32(), C.c_uint64()
        flags = N.GLINT_PUSH_DETERMINISTIC if deterministic else N.GLINT_PUSH_DEFAULT
        check(self.lib.glint_push_wire_async(self.handle, buf, len(payload), C.byref(mid), flags, C.byref(ticket)),
              self.handle)
        return mid.value, ticket.value

    def pull_async(self, *arrays, rows: bool = False, out=None):
        """Enqueue a pull -- get(keys) for vectors, get(rows, cols) or getRows(rows) (rows=True) for
        matrices -- behind everything enqueued before it (glint_pull_async). Returns (ticket, out):
        `out` holds the answer once wait(ticket) has returned; keep it alive until then."""
        mat = self.cols != 0
        kind = 0 if not mat else (2 if rows else 1)
        if len(arrays) != (2 if kind == 1 else 1):
            raise ValueError("pull_async(keys) for vectors and row pulls, (rows, cols) for matrix elements")
        keys = _host(arrays[0], np.int64).reshape(-1)
        cols = _host(arrays[1], np.int32).reshape(-1) if kind == 1 else None
        if kind == 1 and cols.size != keys.size:
            raise ValueError("argument lengths differ")
        out = self._host_out(out, (keys.size, self.cols) if kind == 2 else (keys.size,))
        ticket = C.c_uint64()
        check(self.lib.glint_pull_async(self.handle, kind, keys.ctypes.data, None if cols is None else cols.ctypes.data,
                                        out.ctypes.data, keys.size, C.byref(ticket)), self.handle)
        return ticket.value, out

    def wait(self, ticket: int) -> None:
        """Until the push with this ticket (and every earlier one) is applied; raises GlintDeviceError if
        one of them failed to launch (rejected records raise at the enqueueing call instead)."""
        bad = C.c_int64(-1)
        check(self.lib.glint_shard_wait(self.handle, ticket, C.byref(bad)), self.handle, bad.value)

    def sync(self, stream: Optional[int] = None) -> None:
        """Wait for device-resident calls and raise if any of them rejected a record."""
        bad = C.c_int64(-1)
        check(self.lib.glint_shard_sync(self.handle, stream, C.byref(bad)), self.handle, bad.value)

    def _dev_done(self, rc: int, t, sync: bool) -> None:
        """Ends a device-resident call enqueued on tensor ``t``'s stream: raise on ``rc``, then wait if ``sync``."""
        check(rc, self.handle)
        if sync:
            self.sync(self._stream_of(t))

    @staticmethod
    def _stream_of(t) -> int:
        import torch
        return torch.cuda.current_stream(t.device).cuda_stream

    @property
    def torch_dtype(self):
        import torch
        return getattr(torch, np.dtype(self.np_dtype).name)

    def _check_dev(self, n: int, keys, cols=None, values=None, out=None, out_elems=None, value_elems=None,
                   wire_dtype=None) -> None:
        """Device-resident arguments: every tensor on the shard's GPU, contiguous, of the dtype the
        kernels read (keys/rows int64, cols int32, values/out the shard's type, or ``wire_dtype`` for a
        narrow-format call) and long enough -- the kernels take raw pointers, so a mismatch would read or
        write past a buffer."""
        import torch
        vdt = self.torch_dtype if wire_dtype is None else wire_dtype
        spec = [("keys", keys, torch.int64, n)]
        if cols is not None:
            spec.append(("cols", cols, torch.int32, n))
        if values is not None:
            spec.append(("values", values, vdt, n if value_elems is None else value_elems))
        if out is not None:
            spec.append(("out", out, vdt, n if out_elems is None else out_elems))
        for name, t, dt, want in spec:
            if not _is_torch_cuda(t):
                raise TypeError(f"{name}: expected a CUDA tensor (mixing host arrays and device tensors)")
            if t.device.index != self.device:
                raise ValueError(f"{name} on cuda:{t.device.index}, shard on cuda:{self.device}")
            if not t.is_contiguous():
                raise ValueError(f"{name}: device tensors must be contiguous")
            if t.dtype != dt:
                raise TypeError(f"{name}: dtype {t.dtype}, expected {dt}")
            if t.numel() != want:
                raise ValueError(f"{name}: {t.numel()} elements, expected {want}")

    def _host_out(self, out, shape, dtype=None) -> np.ndarray:
        """A caller-provided host result buffer must be a writable C-contiguous array of the shard's
        type (or ``dtype``, a wire type's) and exact shape (the library writes n x sizeof(V) bytes into it)."""
        dtype = self.np_dtype if dtype is None else dtype
        if out is None:
            return np.empty(shape, dtype=dtype)
        if not isinstance(out, np.ndarray) or out.dtype != dtype or out.shape != tuple(shape) \
                or not out.flags.c_contiguous or not out.flags.writeable:
            raise ValueError(f"out must be a writable C-contiguous {np.dtype(dtype).name} array of shape "
                             f"{tuple(shape)}")
        return out

    def _keys(self) -> np.ndarray:
        """The global keys of the partition's elements (rows), in local order."""
        p = self.partition
        if isinstance(p, RangePartition):
            return np.arange(p.start, p.start + self.size, dtype=np.int64)
        return np.arange(self.size, dtype=np.int64) * p.numberOfPartitions + p.index

    def push_wire(self, payload: bytes, deterministic: bool = False) -> int:
        """Apply a RequestSerializer Push*Vector* byte image; returns its message id."""
        buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
        mid = C.c_int32()
        flags = N.GLINT_PUSH_DETERMINISTIC if deterministic else N.GLINT_PUSH_DEFAULT
        check(self.lib.glint_push_wire(self.handle, buf, len(payload), C.byref(mid), flags), self.handle)
        return mid.value

    def pull_wire(self, payload: bytes) -> bytes:
        """Answer a RequestSerializer PullVector byte image with the ResponseSerializer image."""
        return _pull_wire(self, payload)


class PartialVector(_Shard):
    """glint.models.server.PartialVector (PartialVector.scala:16-64) on one MI355X."""

    def __init__(self, partition: Partition, dtype="double", device: int = 0):
        super().__init__(partition, dtype, 0, device)

    def update(self, keys, values, deterministic: bool = False, sync: bool = True, unordered: bool = False,
               gate=None, validate: bool = False) -> bool:
        """PartialVector.update (PartialVector.scala:35-43): data(globalToLocal(k)) += v.
        ``unordered`` is a performance hint (GLINT_PUSH_UNORDERED): skip the order check, bin by slab.
        ``gate`` (device tensors only): a one-element int64 device tensor, or the address of a word in a
        HostBuffer; the push applies nothing if it is nonzero when the push runs
        (glint_vec_push_dev_gated). With ``validate`` the push writes the gate itself
        (GLINT_PUSH_VALIDATE): 0, or ~(first out-of-range record), which cancels it."""
        flags = _flags(deterministic, unordered) | (N.GLINT_PUSH_VALIDATE if validate else 0)
        if _is_torch_cuda(keys):
            self._check_dev(keys.numel(), keys, values=values)
            if gate is not None:
                rc = self.lib.glint_vec_push_dev_gated(self.handle, keys.data_ptr(), values.data_ptr(), keys.numel(),
                                                       flags, _addr(gate), self._stream_of(keys))
            else:
                rc = self.lib.glint_vec_push_dev(self.handle, keys.data_ptr(), values.data_ptr(), keys.numel(), flags,
                                                 self._stream_of(keys))
            self._dev_done(rc, keys, sync)
            return True
        k = _host(keys, np.int64)
        v = _host(values, self.np_dtype)
        if k.shape != v.shape:
            raise ValueError("keys and values differ in length")
        check(self.lib.glint_vec_push(self.handle, k.ctypes.data, v.ctypes.data, k.size, flags), self.handle)
        return True

    def get(self, keys, out=None, sync: bool = True):
        """PartialVector.get (PartialVector.scala:51-60): a new array of data(globalToLocal(k))."""
        if _is_torch_cuda(keys):
            import torch
            if out is None:
                out = torch.empty(keys.numel(), dtype=self.torch_dtype, device=keys.device)
            self._check_dev(keys.numel(), keys, out=out)
            rc = self.lib.glint_vec_pull_dev(self.handle, keys.data_ptr(), out.data_ptr(), keys.numel(),
                                             self._stream_of(keys))
            self._dev_done(rc, keys, sync)
            return out
        k = _host(keys, np.int64)
        res = self._host_out(out, k.shape)
        check(self.lib.glint_vec_pull(self.handle, k.ctypes.data, res.ctypes.data, k.size), self.handle)
        return res

    def to_numpy(self) -> np.ndarray:
        """Whole shard to host (a pull of every local key through the product path)."""
        return self.get(self._keys())


class PartialMatrix(_Shard):
    """glint.models.server.PartialMatrix (PartialMatrix.scala:17-87) on one MI355X."""

    def __init__(self, partition: Partition, cols: int, dtype="double", device: int = 0):
        if int(cols) <= 0:
            raise ValueError("a matrix shard needs cols > 0")
        super().__init__(partition, dtype, int(cols), device)
        self.rows = self.size

    def update(self, rows, cols, values, deterministic: bool = False, sync: bool = True,
               unordered: bool = False, gate=None, validate: bool = False) -> bool:
        """PartialMatrix.update (PartialMatrix.scala:74-83); ``gate`` and ``validate`` as for
        PartialVector.update."""
        flags = _flags(deterministic, unordered) | (N.GLINT_PUSH_VALIDATE if validate else 0)
        if _is_torch_cuda(rows):
            self._check_dev(rows.numel(), rows, cols=cols, values=values)
            if gate is not None:
                rc = self.lib.glint_mat_push_dev_gated(self.handle, rows.data_ptr(), cols.data_ptr(),
                                                       values.data_ptr(), rows.numel(), flags, _addr(gate),
                                                       self._stream_of(rows))
            else:
                rc = self.lib.glint_mat_push_dev(self.handle, rows.data_ptr(), cols.data_ptr(), values.data_ptr(),
                                                 rows.numel(), flags, self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        r = _host(rows, np.int64)
        c = _host(cols, np.int32)
        v = _host(values, self.np_dtype)
        if not (r.shape == c.shape == v.shape):
            raise ValueError("rows, cols and values differ in length")
        check(self.lib.glint_mat_push(self.handle, r.ctypes.data, c.ctypes.data, v.ctypes.data, r.size, flags),
              self.handle)
        return True

    def updateRows(self, rows, values, deterministic: bool = False, sync: bool = True,
                   unordered: bool = False) -> bool:
        """The write counterpart of getRows (an extension; the reference has no such message):
        PartialMatrix.update applied to the triplets (rows[i], c, values[i][c]), for i in order and c
        in [0, cols) inside each i. ``values`` is (n, cols) or flat, dense row-major. Host arrays keep
        the push order for Float/Double unless ``unordered``; device tensors keep it with
        ``deterministic`` (a row that occurs once is bit-exact either way)."""
        flags = _flags(deterministic, unordered)
        if _is_torch_cuda(rows):
            n = rows.numel()
            self._check_dev(n, rows, values=values, value_elems=n * self.cols)
            rc = self.lib.glint_mat_push_rows_dev(self.handle, rows.data_ptr(), values.data_ptr(), n, flags,
                                                  self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        r, v = self._host_rows(rows, values, self.np_dtype)
        check(self.lib.glint_mat_push_rows(self.handle, r.ctypes.data, v.ctypes.data, r.size, flags), self.handle)
        return True

    def _host_rows(self, rows, values, dtype, name: str = "values") -> tuple:
        """Host rows and their dense value rows ((n, cols) or flat, called ``name``) as flat contiguous arrays
        of int64 and ``dtype``."""
        r = _host(rows, np.int64).reshape(-1)
        v = _host(values, dtype).reshape(-1)
        if v.size != r.size * self.cols:
            raise ValueError(f"{name}: {v.size} elements, expected {r.size} rows x {self.cols} columns")
        return r, v

    def updateRowsAs(self, rows, values, wire: str, deterministic: bool = False, sync: bool = True,
                     unordered: bool = False) -> bool:
        """Narrow-format row push (an extension; glint_mat_push_rows_as*): ``updateRows`` of rows that arrive in
        the wire type ``wire`` -- 'float16' or 'bfloat16' for a Float shard, 'float32' for a Double shard --
        widened exactly on the shard, inside the fold, so half the bytes are staged. ``values`` is (n, cols) or
        flat: a numpy array of float16, of uint16 bfloat16 bit patterns (``to_bfloat16``) or of float32, or a
        torch device tensor of that type; another dtype raises ValueError. Order and flags as ``updateRows``."""
        code, np_wire, torch_name = resolve_wire(wire)
        flags = _flags(deterministic, unordered)
        if _is_torch_cuda(rows):
            import torch
            wdt = getattr(torch, torch_name)
            if _is_torch_cuda(values) and values.dtype != wdt:
                raise ValueError(f"values: dtype {values.dtype}, expected {wdt} for wire type {wire!r}")
            n = rows.numel()
            self._check_dev(n, rows, values=values, value_elems=n * self.cols, wire_dtype=wdt)
            rc = self.lib.glint_mat_push_rows_as_dev(self.handle, rows.data_ptr(), values.data_ptr(), n, code, flags,
                                                     self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        if _is_torch_cuda(values):
            raise TypeError("values: a device tensor with host rows (mixing host arrays and device tensors)")
        r = _host(rows, np.int64).reshape(-1)
        v = np.asarray(values)
        if v.dtype != np_wire:
            raise ValueError(f"values: dtype {v.dtype}, expected {np.dtype(np_wire).name} for wire type {wire!r}")
        r, v = self._host_rows(r, v, np_wire)
        check(self.lib.glint_mat_push_rows_as(self.handle, r.ctypes.data, v.ctypes.data, r.size, code, flags),
              self.handle)
        return True

    def updateRowsAxpy(self, rows, coef, x, deterministic: bool = False, sync: bool = True,
                       unordered: bool = False) -> bool:
        """Row axpy push (an extension; glint_mat_push_rows_axpy*): row rows[i] += sum over j of
        ``coef[i, j] * x[j]``, the contribution rows rebuilt on the shard instead of sent. ``x`` is
        (cols,) or (q, cols); ``coef`` is (n,) (only with q == 1) or (n, q). It is ``updateRows`` with
        ``values[i] = ((coef[i, 0] * x[0]) + (coef[i, 1] * x[1])) + ...`` in the shard's type, rounding for
        rounding: every product is rounded before it is added (no fused multiply-add), j ascends, Int/Long
        wrap. Order and errors as ``updateRows``: host arrays keep the push order for Float/Double unless
        ``unordered`` and reject a message with a row outside the partition before anything is applied;
        device tensors keep the order with ``deterministic``, skip such a row and raise at the sync."""
        flags = _flags(deterministic, unordered)
        if _is_torch_cuda(rows):
            n = rows.numel()
            _check_like("coef", coef, self.torch_dtype, rows)
            _check_like("x", x, self.torch_dtype, rows)
            q = self._axpy_q(tuple(x.shape), tuple(coef.shape), n)
            self._check_dev(n, rows)
            rc = self.lib.glint_mat_push_rows_axpy_dev(self.handle, rows.data_ptr(), n, coef.data_ptr(),
                                                       x.data_ptr(), q, flags, self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        r = _host(rows, np.int64).reshape(-1)
        cf = _host(coef, self.np_dtype)
        xs = _host(x, self.np_dtype)
        q = self._axpy_q(xs.shape, cf.shape, r.size)
        check(self.lib.glint_mat_push_rows_axpy(self.handle, r.ctypes.data, r.size, cf.ctypes.data, xs.ctypes.data, q,
                                                flags), self.handle)
        return True

    def updateRowsGrouped(self, rows, offsets, values, weights=None, deterministic: bool = False,
                          sync: bool = True, unordered: bool = False) -> bool:
        """Grouped row push (an extension; glint_mat_push_rows_grouped*), the write side of ``getRowsSum``:
        ``offsets`` has g + 1 int64 entries, non-decreasing from 0 to len(rows), group k is
        ``rows[offsets[k]:offsets[k+1]]``, and every row of group k += ``values[k]`` -- times
        ``weights[i]`` for record i when ``weights`` is given. ``values`` is (g, cols) or flat, ``weights``
        (n,) or None. It is ``updateRows`` with ``values[group of i]`` (``weights[i] * values[group of i]``,
        the product rounded before the add: no fused multiply-add) as record i's row, rounding for
        rounding, without those n rows ever being built or sent; without ``weights`` the value row's bits
        are added as they are. Int/Long wrap. Order and errors as ``updateRows``: host arrays keep the push
        order for Float/Double unless ``unordered`` and reject a message with a row outside the partition
        before anything is applied; device tensors keep the order with ``deterministic``, skip such a row
        and raise at the sync, and their ``offsets`` are clamped to [0, len(rows)] by the kernel (a record
        that no group covers is not applied)."""
        flags = _flags(deterministic, unordered)
        dev = _is_torch_cuda(rows)
        for name, t in (("offsets", offsets), ("values", values)) + ((("weights", weights),) if weights is not None
                                                                     else ()):
            if _is_torch_cuda(t) != dev:
                raise TypeError(f"rows and {name}: mixing host arrays and device tensors")
        if dev:
            n = rows.numel()
            g = _check_offsets_dev(offsets, rows)
            _check_like("values", values, self.torch_dtype, rows, g * self.cols)
            if weights is not None:
                _check_like("weights", weights, self.torch_dtype, rows, n)
            self._check_dev(n, rows)
            rc = self.lib.glint_mat_push_rows_grouped_dev(
                self.handle, rows.data_ptr(), n, offsets.data_ptr(), g, values.data_ptr() if g else None,
                weights.data_ptr() if weights is not None else None, flags, self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        r = _host(rows, np.int64).reshape(-1)
        o, g = _host_offsets(offsets)
        v = _host(values, self.np_dtype).reshape(-1)
        if v.size != g * self.cols:
            raise ValueError(f"values: {v.size} elements, expected {g} groups x {self.cols} columns")
        w = None
        if weights is not None:
            w = _host(weights, self.np_dtype).reshape(-1)
            if w.size != r.size:
                raise ValueError(f"weights: {w.size} values, expected {r.size}")
        check(self.lib.glint_mat_push_rows_grouped(self.handle, r.ctypes.data, r.size, o.ctypes.data, g,
                                                   v.ctypes.data if g else None,
                                                   w.ctypes.data if w is not None else None, flags), self.handle)
        return True

    def updateRowsAdagrad(self, state: "PartialMatrix", rows, grads, lr: float, eps: float = 1e-10,
                          sync: bool = True) -> bool:
        """Adagrad row push (an extension; glint_mat_push_rows_adagrad*): this shard holds the weights and
        ``state`` -- a PartialMatrix of the same type, device, partition and cols -- the accumulated
        squared gradients. ``grads`` is (n, cols) or flat, dense row-major. Per distinct row of ``rows``:
        ``G`` = its gradient rows added to +0 in push order, then ``state += G * G`` and ``weights -=
        (lr * G) / (sqrt(state) + eps)``, every operation rounded on its own in the shard's type
        (include/glint_gpu.h has the contract): duplicates are coalesced, then one step is taken. There
        are no order flags: the call is deterministic. Errors as ``updateRows``: host arrays reject a
        message with a row outside the partition before either shard changes; device tensors skip such a
        row and raise at the weights shard's sync."""
        return self._step_push("updateRowsAdagrad", "glint_mat_push_rows_adagrad", state, PartialMatrix, rows, grads,
                               (float(lr), float(eps)), sync)

    def _step_push(self, name: str, symbol: str, state, state_cls, rows, grads, scalars: tuple, sync: bool) -> bool:
        """What the optimizer row pushes share (as step_push_host / step_push_dev do below the C ABI): method
        ``name`` calls ``symbol`` -- ``symbol + "_dev"`` for device tensors -- with the weights shard, a
        ``state`` shard of class ``state_cls``, the rows, their gradient rows and the step's ``scalars``."""
        if not isinstance(state, state_cls):
            raise TypeError(f"state: expected a {state_cls.__name__}")
        if np.dtype(self.np_dtype).kind != "f":
            raise TypeError(f"{name} needs a Float or Double shard, not {np.dtype(self.np_dtype).name}")
        if _is_torch_cuda(rows) != _is_torch_cuda(grads):
            raise TypeError("rows and grads: mixing host arrays and device tensors")
        if _is_torch_cuda(rows):
            n = rows.numel()
            self._check_dev(n, rows, values=grads, value_elems=n * self.cols)
            rc = getattr(self.lib, symbol + "_dev")(self.handle, state.handle, rows.data_ptr(), grads.data_ptr(), n,
                                                    *scalars, self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        r, g = self._host_rows(rows, grads, self.np_dtype, "grads")
        check(getattr(self.lib, symbol)(self.handle, state.handle, r.ctypes.data, g.ctypes.data, r.size, *scalars),
              self.handle)
        return True

    def updateRowsAdagradRowwise(self, state: "PartialVector", rows, grads, lr: float, eps: float = 1e-10,
                                 sync: bool = True) -> bool:
        """Row-wise Adagrad row push (an extension; glint_mat_push_rows_adagrad_rowwise*): this shard holds
        the weights and ``state`` -- a PartialVector of the same type, device and partition -- one
        accumulator per row, so the optimizer state is ``1 / cols`` of the table; a zeroed vector is the
        initial state. ``grads`` is (n, cols) or flat, dense row-major. Per distinct row of ``rows``: ``G``
        = its gradient rows added to +0 in push order, ``ss`` = the self-dot of ``G`` in ``getRowsDot``'s
        order, then ``state += ss / cols`` and ``weights -= (lr / (sqrt(state) + eps)) * G``, every
        operation rounded on its own in the shard's type (include/glint_gpu.h has the contract):
        duplicates are coalesced, then one step is taken. There are no order flags: the call is
        deterministic. Errors as ``updateRowsAdagrad``."""
        return self._step_push("updateRowsAdagradRowwise", "glint_mat_push_rows_adagrad_rowwise", state, PartialVector,
                               rows, grads, (float(lr), float(eps)), sync)

    def updateRowsAdam(self, state: "PartialMatrix", rows, grads, lr: float, step: int, beta1: float = 0.9,
                       beta2: float = 0.999, eps: float = 1e-8, sync: bool = True) -> bool:
        """Adam row push (an extension; glint_mat_push_rows_adam*): this shard holds the weights and
        ``state`` -- a PartialMatrix of the same type, device and partition with ``2 * cols`` columns --
        both moments, ``m`` in columns ``[0, cols)`` and ``v`` in ``[cols, 2 * cols)``; a zeroed shard is
        the initial state. ``grads`` is (n, cols) or flat, dense row-major. Per distinct row of ``rows``:
        ``G`` = its gradient rows added to +0 in push order, then ``m = beta1 * m + (1 - beta1) * G``,
        ``v = beta2 * v + (1 - beta2) * G * G`` and ``weights -= (alpha * m) / (sqrt(v) / sqrt(c2) + eps)``
        with ``alpha = lr / (1 - beta1 ** step)`` and ``c2 = 1 - beta2 ** step``, every operation rounded
        on its own in the shard's type (include/glint_gpu.h has the contract). This is lazy Adam:
        duplicates are coalesced, then one step is taken; ``step`` is the caller's global count from 1,
        and a row that is not named keeps its moments. There are no order flags: the call is
        deterministic. Errors as ``updateRowsAdagrad``."""
        scalars = (float(lr), float(beta1), float(beta2), float(eps), int(step))
        return self._step_push("updateRowsAdam", "glint_mat_push_rows_adam", state, PartialMatrix, rows, grads,
                               scalars, sync)

    def updateRowsFtrl(self, state: "PartialMatrix", rows, grads, alpha: float, beta: float = 1.0, l1: float = 0.0,
                       l2: float = 0.0, sync: bool = True) -> bool:
        """FTRL-proximal row push (an extension; glint_mat_push_rows_ftrl*): this shard holds the weights
        and ``state`` -- a PartialMatrix of the same type, device and partition with ``2 * cols`` columns
        -- ``z`` in columns ``[0, cols)`` and ``n`` in ``[cols, 2 * cols)``; zeroed weights beside a zeroed
        state are the start. ``grads`` is (n, cols) or flat, dense row-major. Per distinct row of ``rows``:
        ``G`` = its gradient rows added to +0 in push order, then ``n' = n + G * G``, ``z' = z + (G -
        ((sqrt(n') - sqrt(n)) / alpha) * w)`` and ``w' = 0`` where ``|z'| <= l1``, else ``-(z' - sign(z')
        * l1) / ((beta + sqrt(n')) / alpha + l2)``, every operation rounded on its own in the shard's type
        (include/glint_gpu.h has the contract). The weights are a function of ``(z, n)``: a row's first
        step overwrites whatever the weights shard held. Duplicates are coalesced, then one step is
        taken; a row that is not named is not touched. There are no order flags: the call is
        deterministic. Errors as ``updateRowsAdagrad``."""
        scalars = (float(alpha), float(beta), float(l1), float(l2))
        return self._step_push("updateRowsFtrl", "glint_mat_push_rows_ftrl", state, PartialMatrix, rows, grads,
                               scalars, sync)

    def _axpy_q(self, xshape, cshape, n: int) -> int:
        """q of updateRowsAxpy for vectors of shape ``xshape`` and coefficients of shape ``cshape``."""
        if xshape == (self.cols,):
            q = 1
        elif len(xshape) == 2 and xshape[1] == self.cols and 1 <= xshape[0] <= N.GLINT_AXPY_MAX_VECTORS:
            q = xshape[0]
        else:
            raise ValueError(f"x: shape {tuple(xshape)}, expected ({self.cols},) or (q, {self.cols}) with "
                             f"1 <= q <= {N.GLINT_AXPY_MAX_VECTORS}")
        if cshape != (n, q) and not (q == 1 and cshape == (n,)):
            raise ValueError(f"coef: shape {tuple(cshape)}, expected ({n}, {q})" + (f" or ({n},)" if q == 1 else ""))
        return q

    def get(self, rows, cols, out=None, sync: bool = True):
        """PartialMatrix.get (PartialMatrix.scala:55-65)."""
        if _is_torch_cuda(rows):
            import torch
            if out is None:
                out = torch.empty(rows.numel(), dtype=self.torch_dtype, device=rows.device)
            self._check_dev(rows.numel(), rows, cols=cols, out=out)
            rc = self.lib.glint_mat_pull_dev(self.handle, rows.data_ptr(), cols.data_ptr(), out.data_ptr(),
                                             rows.numel(), self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        r = _host(rows, np.int64)
        c = _host(cols, np.int32)
        if r.shape != c.shape:
            raise ValueError("rows and cols differ in length")
        res = self._host_out(out, r.shape)
        check(self.lib.glint_mat_pull(self.handle, r.ctypes.data, c.ctypes.data, res.ctypes.data, r.size),
              self.handle)
        return res

    def getRows(self, rows, out=None, sync: bool = True):
        """PartialMatrix.getRows (PartialMatrix.scala:37-46) as one (n, cols) array -- the flattened
        row-major image ResponseSerializer sends (ResponseSerializer.scala:52-61)."""
        if _is_torch_cuda(rows):
            import torch
            if out is None:
                out = torch.empty((rows.numel(), self.cols), dtype=self.torch_dtype, device=rows.device)
            self._check_dev(rows.numel(), rows, out=out, out_elems=rows.numel() * self.cols)
            rc = self.lib.glint_mat_pull_rows_dev(self.handle, rows.data_ptr(), out.data_ptr(), rows.numel(),
                                                  self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        r = _host(rows, np.int64).reshape(-1)
        res = self._host_out(out, (r.size, self.cols))
        check(self.lib.glint_mat_pull_rows(self.handle, r.ctypes.data, res.ctypes.data, r.size), self.handle)
        return res

    def getRowsAs(self, rows, wire: str, out=None, sync: bool = True):
        """Narrow-format row pull (an extension; glint_mat_pull_rows_as*): ``getRows`` rounded on the shard to
        the wire type ``wire`` -- 'float16' or 'bfloat16' for a Float shard, 'float32' for a Double shard --
        one round-to-nearest-even of each stored value, so half the bytes are copied back. Host rows give an
        (n, cols) numpy array of float16, of uint16 bfloat16 bit patterns (``from_bfloat16`` widens them) or of
        float32; device rows a torch tensor of that type."""
        code, np_wire, torch_name = resolve_wire(wire)
        if _is_torch_cuda(rows):
            import torch
            wdt = getattr(torch, torch_name)
            if out is None:
                out = torch.empty((rows.numel(), self.cols), dtype=wdt, device=rows.device)
            elif _is_torch_cuda(out) and out.dtype != wdt:
                raise ValueError(f"out: dtype {out.dtype}, expected {wdt} for wire type {wire!r}")
            self._check_dev(rows.numel(), rows, out=out, out_elems=rows.numel() * self.cols, wire_dtype=wdt)
            rc = self.lib.glint_mat_pull_rows_as_dev(self.handle, rows.data_ptr(), out.data_ptr(), rows.numel(), code,
                                                     self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        r = _host(rows, np.int64).reshape(-1)
        out = self._host_out(out, (r.size, self.cols), np_wire)
        check(self.lib.glint_mat_pull_rows_as(self.handle, r.ctypes.data, out.ctypes.data, r.size, code), self.handle)
        return out

    def getRowsSparse(self, rows, cap: Optional[int] = None, sync: bool = True):
        """The non-zero elements of the requested rows as a CSR triple ``(indptr, cols, values)`` (an
        extension; glint_mat_pull_rows_sparse*): ``indptr`` has n + 1 int64 entries, request i's entries
        are ``cols[indptr[i]:indptr[i+1]]`` (int32, ascending) and ``values[...]`` (the stored bits).
        Non-zero is the type's ``v != 0``: -0.0 is dropped, NaN kept. Scattered into zeros the triple is
        getRows(rows).

        Host arrays: exact-size numpy arrays (a count-only call, then the pull; with ``cap=k`` one call
        and at most k entries); only the non-zeros cross the link. Device tensors with
        ``cap=None``: a count, one synchronisation to read the total, then exact-size tensors. Device
        tensors with ``cap=k``: one stream-ordered call, returns ``(indptr, cols[:k], values[:k])``;
        entries at positions >= k are not stored, and the caller compares ``indptr[-1]`` with k."""
        if _is_torch_cuda(rows):
            import torch
            n = rows.numel()
            self._check_dev(n, rows)
            if cap is not None and int(cap) < 0:
                raise ValueError("cap must be >= 0")
            st = self._stream_of(rows)
            indptr = torch.empty(n + 1, dtype=torch.int64, device=rows.device)
            if cap is None:
                check(self.lib.glint_mat_pull_rows_sparse_dev(self.handle, rows.data_ptr(), n, indptr.data_ptr(),
                                                              None, None, 0, st), self.handle)
                k = int(indptr[-1].item())
            else:
                k = int(cap)
            cols = torch.empty(k, dtype=torch.int32, device=rows.device)
            vals = torch.empty(k, dtype=self.torch_dtype, device=rows.device)
            rc = N.GLINT_OK
            if k or cap is not None:
                rc = self.lib.glint_mat_pull_rows_sparse_dev(self.handle, rows.data_ptr(), n, indptr.data_ptr(),
                                                             cols.data_ptr() if k else None,
                                                             vals.data_ptr() if k else None, k, st)
            self._dev_done(rc, rows, sync)
            return indptr, cols, vals
        r = _host(rows, np.int64).reshape(-1)
        indptr = np.empty(r.size + 1, np.int64)
        nnz = C.c_int64(0)
        if cap is None:  # a count-only call sizes the arrays (cheaper than faulting in room for n x cols)
            check(self.lib.glint_mat_pull_rows_sparse(self.handle, r.ctypes.data, r.size, indptr.ctypes.data, None,
                                                      None, 0, C.byref(nnz)), self.handle)
            k = nnz.value
            if k == 0:
                return indptr, np.empty(0, np.int32), np.empty(0, self.np_dtype)
        else:
            k = int(cap)
            if k < 0:
                raise ValueError("cap must be >= 0")
        cols = np.empty(k, np.int32)
        vals = np.empty(k, self.np_dtype)
        check(self.lib.glint_mat_pull_rows_sparse(self.handle, r.ctypes.data, r.size, indptr.ctypes.data,
                                                  cols.ctypes.data if k else None, vals.ctypes.data if k else None,
                                                  k, C.byref(nnz)), self.handle)
        if nnz.value < k:
            cols, vals = cols[:nnz.value].copy(), vals[:nnz.value].copy()
        return indptr, cols, vals

    def getRowsSum(self, rows, offsets, out=None, sync: bool = True, *, weights=None):
        """The sums of groups of requested rows as one (g, cols) array (an extension;
        glint_mat_pull_rows_sum*): ``offsets`` has g + 1 int64 entries, non-decreasing from 0 to
        len(rows), and group k is ``rows[offsets[k]:offsets[k+1]]``. Row k of the answer is the
        left-to-right sum of the group's rows in the shard's type, ``((r0 + r1) + r2) + ...`` in the
        caller's order, starting from the first row's stored bits: a group of one row is getRows of
        that row bit for bit, an empty group is zeros, Int/Long wrap. Rows may repeat.

        Host arrays: only the (g, cols) sums cross the link; a row outside the partition raises and
        nothing is written. Device tensors: one stream-ordered launch on the current stream; a row
        outside the partition counts as zeros and is raised by the sync (``sync=True``, or a later
        ``sync()``); ``offsets`` values are clamped to [0, len(rows)] by the kernel.

        ``weights`` (keyword only; (n,) of the shard's dtype, a host array with host rows, a contiguous
        CUDA tensor on rows' device with device rows) makes it the weighted sum (glint_mat_pull_rows_wsum*):
        ``((weights[b] * r_b) + (weights[b+1] * r_b+1)) + ...``, every product rounded before it is added
        (no fused multiply-add) and the first term the first product as computed. On the device a row
        outside the partition is the term zero whatever its weight."""
        if _is_torch_cuda(rows):
            import torch
            n = rows.numel()
            g = _check_offsets_dev(offsets, rows)
            if weights is not None:
                _check_like("weights", weights, self.torch_dtype, rows)
                if weights.numel() != n:
                    raise ValueError(f"weights: {weights.numel()} values, expected {n}")
            if out is None:
                out = torch.empty((g, self.cols), dtype=self.torch_dtype, device=rows.device)
            self._check_dev(n, rows, out=out, out_elems=g * self.cols)
            if weights is None:
                rc = self.lib.glint_mat_pull_rows_sum_dev(self.handle, rows.data_ptr(), n, offsets.data_ptr(), g,
                                                          out.data_ptr(), self._stream_of(rows))
            else:
                rc = self.lib.glint_mat_pull_rows_wsum_dev(self.handle, rows.data_ptr(), n, offsets.data_ptr(), g,
                                                           weights.data_ptr() if n else None, out.data_ptr(),
                                                           self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        if _is_torch_cuda(offsets) or _is_torch_cuda(weights):
            raise TypeError("rows, offsets and weights: mixing host arrays and device tensors")
        r = _host(rows, np.int64).reshape(-1)
        o, g = _host_offsets(offsets)
        w = None
        if weights is not None:
            if isinstance(weights, np.ndarray) and weights.dtype != np.dtype(self.np_dtype):
                raise TypeError(f"weights: expected {np.dtype(self.np_dtype).name}, not {weights.dtype.name}")
            w = _host(weights, self.np_dtype).reshape(-1)
            if w.size != r.size:
                raise ValueError(f"weights: {w.size} values, expected {r.size}")
        res = self._host_out(out, (g, self.cols))
        if w is None:
            check(self.lib.glint_mat_pull_rows_sum(self.handle, r.ctypes.data, r.size, o.ctypes.data, g,
                                                   res.ctypes.data), self.handle)
        else:
            check(self.lib.glint_mat_pull_rows_wsum(self.handle, r.ctypes.data, r.size, o.ctypes.data, g,
                                                    w.ctypes.data if r.size else None, res.ctypes.data), self.handle)
        return res

    def getRowsGroupDot(self, rows, offsets, x, out=None, sync: bool = True):
        """The dot product of every requested row with the one vector of its group, as an (n,) array (an
        extension; glint_mat_pull_rows_gdot*): ``offsets`` is ``getRowsSum``'s, ``x`` is (g, cols) or flat
        with g * cols elements, and ``out[i] = dot(row rows[i], x[k])`` with k the group of record i -- the
        gradient of ``getRowsSum(..., weights=w)`` with respect to ``w``, or each query's scores over its
        own candidates. The arithmetic is ``getRowsDot``'s with one vector, bit for bit: ``out[i]`` is
        ``getRowsDot(rows[i:i+1], x[k])``. Rows may repeat; answers keep the caller's order.

        Host arrays: only the n dots cross the link; a row outside the partition raises and nothing is
        written. Device tensors: one stream-ordered launch on the current stream; a row outside the
        partition answers zero and is raised by the sync; ``offsets`` values are clamped to [0, len(rows)]
        by the kernel and a record that no group covers answers zero."""
        if _is_torch_cuda(rows):
            import torch
            n = rows.numel()
            g = _check_offsets_dev(offsets, rows)
            _check_like("x", x, self.torch_dtype, rows)
            self._gdot_shape(tuple(x.shape), g)
            if out is None:
                out = torch.empty((n,), dtype=self.torch_dtype, device=rows.device)
            self._check_dev(n, rows, out=out, out_elems=n)
            rc = self.lib.glint_mat_pull_rows_gdot_dev(self.handle, rows.data_ptr(), n, offsets.data_ptr(), g,
                                                       x.data_ptr() if g else None, out.data_ptr(),
                                                       self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        if _is_torch_cuda(offsets) or _is_torch_cuda(x):
            raise TypeError("rows, offsets and x: mixing host arrays and device tensors")
        r = _host(rows, np.int64).reshape(-1)
        o, g = _host_offsets(offsets)
        if isinstance(x, np.ndarray) and x.dtype != np.dtype(self.np_dtype):
            raise TypeError(f"x: expected {np.dtype(self.np_dtype).name}, not {x.dtype.name}")
        xs = _host(x, self.np_dtype)
        self._gdot_shape(xs.shape, g)
        res = self._host_out(out, (r.size,))
        check(self.lib.glint_mat_pull_rows_gdot(self.handle, r.ctypes.data, r.size, o.ctypes.data, g,
                                                xs.ctypes.data if g else None, res.ctypes.data), self.handle)
        return res

    def _gdot_shape(self, shape, g: int) -> None:
        """``x`` of a grouped row dot: (g, cols), or flat with g * cols elements."""
        if tuple(shape) != (g, self.cols) and tuple(shape) != (g * self.cols,):
            raise ValueError(f"x: shape {tuple(shape)}, expected ({g}, {self.cols}) or ({g * self.cols},)")

    def getRowsDot(self, rows, x=None, out=None, sync: bool = True):
        """The dot products of the requested rows with caller vectors (an extension;
        glint_mat_pull_rows_dot*), reduced over the columns on the shard: ``x`` of shape (cols,) gives an
        (n,) array, ``x`` of shape (q, cols) an (n, q) array with ``out[i, j] = dot(row rows[i], x[j])``,
        and ``x=None`` the (n,) squared norms ``dot(row, row)``. All arithmetic is in the shard's type:
        Int/Long wrap; Float/Double products are rounded before they are added (no fused multiply-add)
        and added in the fixed order include/glint_gpu.h states, which depends on the type and cols
        only. Rows may repeat; answers keep the caller's order.

        Host arrays: only the n x q dots cross the link; a row outside the partition raises and
        nothing is written. Device tensors: one stream-ordered launch on the current stream; a row
        outside the partition answers zeros and is raised by the sync (``sync=True``, or a later
        ``sync()``)."""
        if _is_torch_cuda(rows):
            import torch
            n = rows.numel()
            q, shape = 1, (n,)
            if x is not None:
                _check_like("x", x, self.torch_dtype, rows)
                q, shape = self._dot_shape(tuple(x.shape), n)
            if out is None:
                out = torch.empty(shape, dtype=self.torch_dtype, device=rows.device)
            self._check_dev(n, rows, out=out, out_elems=n * q)
            rc = self.lib.glint_mat_pull_rows_dot_dev(self.handle, rows.data_ptr(), n,
                                                      x.data_ptr() if x is not None else None, q, out.data_ptr(),
                                                      self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        r = _host(rows, np.int64).reshape(-1)
        q, shape = 1, (r.size,)
        if x is not None:
            x = _host(x, self.np_dtype)
            q, shape = self._dot_shape(x.shape, r.size)
        res = self._host_out(out, shape)
        check(self.lib.glint_mat_pull_rows_dot(self.handle, r.ctypes.data, r.size,
                                               x.ctypes.data if x is not None else None, q, res.ctypes.data),
              self.handle)
        return res

    def _pair_other(self, other, name: str) -> None:
        """The second shard of a row-pair call: a PartialMatrix of this one's type, device and cols."""
        if not isinstance(other, PartialMatrix):
            raise TypeError(f"{name}: expected a PartialMatrix")
        if other.code != self.code or other.cols != self.cols or other.device != self.device:
            raise ValueError(f"{name}: expected a shard of this one's type, device and cols "
                             f"({np.dtype(self.np_dtype).name}, cuda:{self.device}, {self.cols}), not "
                             f"({np.dtype(other.np_dtype).name}, cuda:{other.device}, {other.cols})")

    def _pair_rows_dev(self, rows, other_rows, name: str) -> int:
        """Device-resident row arrays of a row-pair call: both as _check_dev asks, of one length."""
        n = rows.numel()
        self._check_dev(n, rows)
        if not _is_torch_cuda(other_rows):
            raise TypeError(f"{name}: expected a CUDA tensor (mixing host arrays and device tensors)")
        self._check_dev(n, other_rows)
        return n

    def getPairsDot(self, other: "PartialMatrix", rows, other_rows, out=None, sync: bool = True):
        """Row-pair dot pull (an extension; glint_mat_pull_pairs_dot*): ``out[i] = dot(row rows[i] of this
        shard, row other_rows[i] of other)``, an (n,) array, reduced on the device: 2 n row ids go out and n
        values come back, nothing of size cols. ``other`` is a PartialMatrix of this one's type, device and
        cols; its partition is its own, and each row array is translated with its own shard's. ``other``
        may be this shard itself, or a view of the same slab. The arithmetic is ``getRowsDot``'s, word for
        word: the bits are those of ``getRowsDot([rows[i]], x=other.getRows([other_rows[i]]))``. Rows may
        repeat; answers keep the caller's order.

        Host arrays: every pair is checked first; a row of either array outside its shard's partition
        raises with the lowest such index and nothing is written. Device tensors: one stream-ordered launch
        on the current stream; such a pair answers zero and is raised by this shard's sync (``sync=True``,
        or a later ``sync()``)."""
        self._pair_other(other, "other")
        if _is_torch_cuda(rows):
            import torch
            n = self._pair_rows_dev(rows, other_rows, "other_rows")
            if out is None:
                out = torch.empty(n, dtype=self.torch_dtype, device=rows.device)
            self._check_dev(n, rows, out=out)
            rc = self.lib.glint_mat_pull_pairs_dot_dev(self.handle, other.handle, rows.data_ptr(),
                                                       other_rows.data_ptr(), n, out.data_ptr(),
                                                       self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return out
        if _is_torch_cuda(other_rows):
            raise TypeError("rows and other_rows: mixing host arrays and device tensors")
        r = _host(rows, np.int64).reshape(-1)
        o = _host(other_rows, np.int64).reshape(-1)
        if o.size != r.size:
            raise ValueError(f"other_rows: {o.size} rows, expected {r.size}")
        res = self._host_out(out, (r.size,))
        check(self.lib.glint_mat_pull_pairs_dot(self.handle, other.handle, r.ctypes.data, o.ctypes.data, r.size,
                                                res.ctypes.data), self.handle)
        return res

    def updatePairsAxpy(self, src: "PartialMatrix", rows, src_rows, coef, deterministic: bool = False,
                        sync: bool = True, unordered: bool = False) -> bool:
        """Row-pair axpy push (an extension; glint_mat_push_pairs_axpy*): row rows[i] of this shard +=
        ``coef[i] *`` (row src_rows[i] of ``src``), the contribution rows built on the device from the
        second shard instead of sent: 2 n row ids and n coefficients go out, nothing of size cols. ``src``
        is a PartialMatrix of this one's type, device and cols with a partition of its own; it must share
        no memory with this shard (not the same shard, not an overlapping view) and is read as it was before
        the call. ``coef`` is (n,). It is ``updateRows`` with ``values[i] = coef[i] * src.getRows(
        [src_rows[i]])`` in the shard's type, rounding for rounding: the product is rounded before it is
        added (no fused multiply-add), Int/Long wrap. Order and errors as ``updateRows``: host arrays keep
        the push order for Float/Double unless ``unordered`` and reject a message with a row of either array
        outside its partition before anything is applied; device tensors keep the order with
        ``deterministic``, skip such a record -- it contributes nothing -- and raise at this shard's
        sync."""
        self._pair_other(src, "src")
        flags = _flags(deterministic, unordered)
        if _is_torch_cuda(rows):
            n = self._pair_rows_dev(rows, src_rows, "src_rows")
            self._check_dev(n, rows, values=coef)
            rc = self.lib.glint_mat_push_pairs_axpy_dev(self.handle, src.handle, rows.data_ptr(),
                                                        src_rows.data_ptr(), coef.data_ptr(), n, flags,
                                                        self._stream_of(rows))
            self._dev_done(rc, rows, sync)
            return True
        if _is_torch_cuda(src_rows) or _is_torch_cuda(coef):
            raise TypeError("rows, src_rows and coef: mixing host arrays and device tensors")
        r = _host(rows, np.int64).reshape(-1)
        o = _host(src_rows, np.int64).reshape(-1)
        cf = _host(coef, self.np_dtype).reshape(-1)
        if o.size != r.size or cf.size != r.size:
            raise ValueError(f"src_rows: {o.size} rows and coef: {cf.size} values, expected {r.size} of each")
        check(self.lib.glint_mat_push_pairs_axpy(self.handle, src.handle, r.ctypes.data, o.ctypes.data,
                                                 cf.ctypes.data, r.size, flags), self.handle)
        return True

    def _dot_shape(self, xshape, n: int):
        """(q, answer shape) of getRowsDot for query vectors of shape ``xshape``."""
        if xshape == (self.cols,):
            return 1, (n,)
        if len(xshape) == 2 and xshape[1] == self.cols and 1 <= xshape[0] <= N.GLINT_DOT_MAX_QUERIES:
            return xshape[0], (n, xshape[0])
        raise ValueError(f"x: shape {tuple(xshape)}, expected ({self.cols},) or (q, {self.cols}) with "
                         f"1 <= q <= {N.GLINT_DOT_MAX_QUERIES}")

    def getTopK(self, x, k: int, sync: bool = True):
        """The ``k`` rows of the shard that score highest against caller vectors (an extension;
        glint_mat_pull_topk*): ``x`` of shape (cols,) gives ``(rows[k], vals[k])``, ``x`` of shape
        (q, cols) two (q, k) arrays. A score is getRowsDot's ``dot(row, x[j])``, bit for bit. Rows come
        by rank descending, then global row ascending: every NaN ranks below every number, -0 equals +0,
        Int/Long rank by the signed value. ``rows`` holds global keys (int64); a shard of fewer than
        ``k`` rows fills the rest with row -1 and value 0.

        Host array: x goes up, the q x k pairs come back -- nothing of the shard's size crosses the
        link. Device tensor: stream-ordered launches on the current stream, device tensors returned
        (``sync=False`` leaves the wait to the caller)."""
        k = int(k)
        if not 1 <= k <= N.GLINT_TOPK_MAX_K:
            raise ValueError(f"k: {k}, expected 1 <= k <= {N.GLINT_TOPK_MAX_K}")
        if _is_torch_cuda(x):
            import torch
            if x.dtype != self.torch_dtype or not x.is_contiguous() or x.device.index != self.device:
                raise TypeError(f"x: expected a contiguous {self.torch_dtype} CUDA tensor on cuda:{self.device}")
            q, shape = self._topk_shape(tuple(x.shape), k)
            rows = torch.empty(shape, dtype=torch.int64, device=x.device)
            vals = torch.empty(shape, dtype=self.torch_dtype, device=x.device)
            rc = self.lib.glint_mat_pull_topk_dev(self.handle, x.data_ptr(), q, k, rows.data_ptr(), vals.data_ptr(),
                                                  self._stream_of(x))
            self._dev_done(rc, x, sync)
            return rows, vals
        x = _host(x, self.np_dtype)
        q, shape = self._topk_shape(x.shape, k)
        rows = np.empty(shape, np.int64)
        vals = np.empty(shape, self.np_dtype)
        check(self.lib.glint_mat_pull_topk(self.handle, x.ctypes.data, q, k, rows.ctypes.data, vals.ctypes.data),
              self.handle)
        return rows, vals

    def _topk_shape(self, xshape, k: int):
        """(q, answer shape) of getTopK for query vectors of shape ``xshape``."""
        if xshape == (self.cols,):
            return 1, (k,)
        if len(xshape) == 2 and xshape[1] == self.cols and 1 <= xshape[0] <= N.GLINT_TOPK_MAX_QUERIES:
            return xshape[0], (xshape[0], k)
        raise ValueError(f"x: shape {tuple(xshape)}, expected ({self.cols},) or (q, {self.cols}) with "
                         f"1 <= q <= {N.GLINT_TOPK_MAX_QUERIES}")

    def to_numpy(self) -> np.ndarray:
        return self.getRows(self._keys())


def _pull_wire(shard: _Shard, payload: bytes) -> bytes:
    lib = shard.lib
    buf = (C.c_uint8 * len(payload)).from_buffer_copy(payload)
    need = C.c_size_t(0)
    rc = lib.glint_pull_wire(shard.handle, buf, len(payload), None, 0, C.byref(need))
    if rc != N.GLINT_OK and need.value == 0:
        check(rc, shard.handle)
    out = (C.c_uint8 * need.value)()
    check(lib.glint_pull_wire(shard.handle, buf, len(payload), out, need.value, C.byref(need)), shard.handle)
    return bytes(out)

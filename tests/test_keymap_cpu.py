"""Device key map, the parts that need no GPU: the ABI's symbols and version, the argument checks every entry
point makes before it touches a device, and the Python surface."""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N

# glint_version() at the parent of the key map ("Key map")
PARENT_VERSION = 1700
NAMES = ("glint_keymap_create", "glint_keymap_destroy", "glint_keymap_info", "glint_keymap_insert",
         "glint_keymap_insert_dev", "glint_keymap_lookup", "glint_keymap_lookup_dev", "glint_keymap_keys_of",
         "glint_keymap_keys_of_dev", "glint_keymap_sync")


def test_abi():
    lib = N.load()
    for name in NAMES:
        assert callable(getattr(lib, name)) and name in N.SIGNATURES
    assert lib.glint_version() > PARENT_VERSION
    assert N.GLINT_K_COUNT == 13  # no new kernel id


@pytest.mark.parametrize("capacity,first_row,slots", [
    (0, 0, 0), (-1, 0, 0), (4, 0, 4), (4, 0, 6), (4, 0, 2), (1, 0, 1), (4, -1, 8), (4, (1 << 62) - 3, 8),
    (1 << 29, 0, 1 << 31), ((1 << 29) + 1, 0, 0), (1 << 30, 0, 1 << 30)])
def test_create_refuses_bad_geometry(capacity, first_row, slots):
    h = C.c_void_p(1)
    assert N.load().glint_keymap_create(0, capacity, first_row, slots, C.byref(h)) == N.GLINT_EINVAL and not h.value


def test_argument_checks_without_device():
    lib = N.load()
    assert lib.glint_keymap_create(0, 4, 0, 8, None) == N.GLINT_EINVAL
    buf = np.zeros(4, np.int64)
    p, bad, free = buf.ctypes.data, C.c_int64(5), C.c_int64(5)
    # a NULL map
    assert lib.glint_keymap_destroy(None) == N.GLINT_EINVAL
    assert lib.glint_keymap_info(None, None, None, None, None, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_sync(None, None, C.byref(bad), C.byref(free)) == N.GLINT_EINVAL
    assert bad.value == free.value == -1
    assert lib.glint_keymap_insert(None, p, 4, p, None, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_insert_dev(None, p, 4, p, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_lookup(None, p, 4, -1, p, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_lookup_dev(None, p, 4, -1, p, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_keys_of(None, p, 4, p, None) == N.GLINT_EINVAL
    assert lib.glint_keymap_keys_of_dev(None, p, 4, p, None) == N.GLINT_EINVAL
    # a bad n or a NULL array is refused before the map is looked at: the handle here is not a map
    fake = C.c_void_p(buf.ctypes.data)
    for n, a, o in ((-1, p, p), (1 << 31, p, p), (4, None, p), (4, p, None)):
        assert lib.glint_keymap_insert(fake, a, n, o, None, None) == N.GLINT_EINVAL
        assert lib.glint_keymap_insert_dev(fake, a, n, o, None) == N.GLINT_EINVAL
        assert lib.glint_keymap_lookup(fake, a, n, -1, o, None) == N.GLINT_EINVAL
        assert lib.glint_keymap_lookup_dev(fake, a, n, -1, o, None) == N.GLINT_EINVAL
        assert lib.glint_keymap_keys_of(fake, a, n, o, None) == N.GLINT_EINVAL
        assert lib.glint_keymap_keys_of_dev(fake, a, n, o, None) == N.GLINT_EINVAL
    # n == 0 touches nothing
    assert lib.glint_keymap_insert(fake, None, 0, None, C.byref(bad), C.byref(free)) == N.GLINT_OK
    assert lib.glint_keymap_lookup_dev(fake, None, 0, -1, None, None) == N.GLINT_OK


def test_python_surface():
    assert glint_amd.KeyMap is glint_amd.keymap.KeyMap and "KeyMap" in glint_amd.__all__
    assert issubclass(glint_amd.KeyMapFullException, glint_amd.ArrayIndexOutOfBoundsException)
    e = glint_amd.KeyMapFullException("full", 3)
    assert e.free == 3 and e.record == -1
    for name in ("insert", "lookup", "keysOf", "size", "info", "sync", "destroy"):
        assert callable(getattr(glint_amd.KeyMap, name))
    assert callable(glint_amd.Client.keymap)
    with pytest.raises(ValueError):
        glint_amd.KeyMap(4, slots=6)
    blank = object.__new__(glint_amd.KeyMap)  # the type check comes before the map is touched
    for fn in (blank.insert, blank.lookup, blank.keysOf):
        with pytest.raises(TypeError):
            fn(np.array([0.5, 1.5]))
    if N.load().glint_device_count() == 0:
        with pytest.raises(glint_amd.GlintDeviceError):
            glint_amd.KeyMap(4)

"""rsk_bloom_pool_*: argument errors need no GPU -- a NULL handle (or NULL ctx /
keys) is refused with RSK_ERR_INVALID_ARG and a message before any device call."""
import ctypes

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from redisson_amd import _lib

    return _lib.load()


def _keys(n=4):
    from redisson_amd import KeyBatch

    return KeyBatch.from_numpy(np.zeros((n, 16), np.uint8))


def _refused(L, rc):
    from redisson_amd import _lib

    assert rc == _lib.RSK_ERR_INVALID_ARG
    assert L.rsk_last_error()


def test_null_handle_refused_by_every_entry_point(L):
    kb = _keys()
    ks = kb.as_struct()
    groups = np.zeros(4, np.uint32)
    out = np.zeros(8, np.uint8)
    u64 = np.zeros(4, np.uint64)
    i32 = np.zeros(4, np.int32)
    n = ctypes.c_size_t()
    nf, st = ctypes.c_uint64(), ctypes.c_uint64()
    size, k = ctypes.c_int64(), ctypes.c_int32()
    h = ctypes.c_void_p()
    _refused(L, L.rsk_bloom_pool_create(None, 3, 729, 5, ctypes.byref(h)))
    assert not h.value
    _refused(L, L.rsk_bloom_pool_destroy(None))
    _refused(L, L.rsk_bloom_pool_info(None, ctypes.byref(nf), ctypes.byref(size), ctypes.byref(k), ctypes.byref(st)))
    _refused(L, L.rsk_bloom_pool_add(None, ctypes.byref(ks), groups.ctypes.data, out.ctypes.data))
    _refused(L, L.rsk_bloom_pool_add(None, ctypes.byref(ks), groups.ctypes.data, None))
    _refused(L, L.rsk_bloom_pool_add(None, None, groups.ctypes.data, out.ctypes.data))
    _refused(L, L.rsk_bloom_pool_contains(None, ctypes.byref(ks), groups.ctypes.data, out.ctypes.data))
    _refused(L, L.rsk_bloom_pool_contains(None, None, None, out.ctypes.data))
    _refused(L, L.rsk_bloom_pool_bitcount(None, None, 4, u64.ctypes.data))
    _refused(L, L.rsk_bloom_pool_count(None, None, 4, i32.ctypes.data))
    _refused(L, L.rsk_bloom_pool_export_bits(None, 0, out.ctypes.data, out.size, ctypes.byref(n)))
    _refused(L, L.rsk_bloom_pool_import_bits(None, 0, out.ctypes.data, out.size))
    _refused(L, L.rsk_bloom_pool_clear(None))
    assert L.rsk_bloom_pool_device_bits(None) is None
    assert L.rsk_last_error()
    assert not out.any()  # nothing written


def test_create_refuses_null_out_and_resets_it(L):
    h = ctypes.c_void_p(1234)
    _refused(L, L.rsk_bloom_pool_create(None, 3, 729, 5, ctypes.byref(h)))
    assert not h.value  # no stale handle left behind
    _refused(L, L.rsk_bloom_pool_create(None, 3, 729, 5, None))


def test_python_class_exported():
    import redisson_amd

    assert "GroupedBloomFilter" in redisson_amd.__all__
    cls = redisson_amd.GroupedBloomFilter
    for m in ("add", "contains", "count", "bitcount", "toByteArray", "fromByteArray", "clear", "close"):
        assert callable(getattr(cls, m))

"""rsk_hll_add_grouped_each: argument errors need no GPU -- a NULL handle is
refused with RSK_ERR_INVALID_ARG and a message before any device call, whatever
the other arguments are, and nothing is written.  (NULL keys / groups / out on a
live pool: tests/test_gpu_hll_grouped_each.py.)"""
import ctypes
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def L():
    from redisson_amd import _lib

    return _lib.load()


def _refused(L, rc):
    from redisson_amd import _lib

    assert rc == _lib.RSK_ERR_INVALID_ARG
    assert L.rsk_last_error()


def test_null_handle_refused(L):
    from redisson_amd import KeyBatch

    kb = KeyBatch.from_numpy(np.zeros((4, 16), np.uint8))
    ks = kb.as_struct()
    groups = np.zeros(4, np.uint32)
    out = np.full(8, 0xAA, np.uint8)
    fn = L.rsk_hll_add_grouped_each
    _refused(L, fn(None, ctypes.byref(ks), groups.ctypes.data, out.ctypes.data))
    _refused(L, fn(None, None, groups.ctypes.data, out.ctypes.data))
    _refused(L, fn(None, ctypes.byref(ks), None, out.ctypes.data))
    _refused(L, fn(None, ctypes.byref(ks), groups.ctypes.data, None))
    _refused(L, fn(None, None, None, None))
    assert (out == 0xAA).all()  # nothing written
    assert not groups.any()


def test_signature_follows_header():
    """The binding's argument list is the header's: handle, keys, groups, out."""
    import os

    from redisson_amd import _lib

    res, args = _lib.SIGNATURES["rsk_hll_add_grouped_each"]
    assert res is ctypes.c_int and len(args) == 4
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    hdr = open(os.path.join(root, "include", "rsketch.h")).read()
    m = re.search(r"int rsk_hll_add_grouped_each\(([^)]*)\);", hdr)
    assert m and m.group(1).count(",") == 3
    assert re.search(r"#define RSK_ABI_VERSION 2\b", hdr)


def test_python_method_exported():
    import redisson_amd

    cls = redisson_amd.GroupedHyperLogLog
    assert callable(getattr(cls, "addEach"))
    assert callable(getattr(cls, "add"))

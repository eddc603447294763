"""Bloom filter pools (rsk_bloom_pool_*): F equal filters as rows of one bit
string, key i added to / queried in row groups[i].  Everything is bit-exact
against the CPU oracle composed per filter (test_bloom_pool_model.py): every
row's bytes, every reply, every row's BITCOUNT and count(), and the padding of
the row stride stays zero."""
import ctypes

import numpy as np
import pytest

from test_bloom_pool_model import pool_add, pool_contains

pytestmark = pytest.mark.gpu

POP8 = np.array([bin(i).count("1") for i in range(256)], np.uint8)
P10K = (95850, 7)  # rsk_bloom_params(10000, 0.01): test_shape_constants_are_the_library_params


@pytest.fixture(scope="module")
def L():
    from redisson_amd import _lib

    return _lib.load()


class Pool:
    """The C ABI of one pool, as the tests drive it."""

    def __init__(self, L, engine, F, size, k):
        from redisson_amd import _lib

        self.L, self.engine, self.lib = L, engine, _lib
        h = ctypes.c_void_p()
        _lib.check(L.rsk_bloom_pool_create(engine.ctx, F, size, k, ctypes.byref(h)))
        self.h = h
        nf, st, sz, kk = ctypes.c_uint64(), ctypes.c_uint64(), ctypes.c_int64(), ctypes.c_int32()
        _lib.check(L.rsk_bloom_pool_info(h, ctypes.byref(nf), ctypes.byref(sz), ctypes.byref(kk), ctypes.byref(st)))
        assert (nf.value, sz.value, kk.value) == (F, size, k)
        assert st.value % 32 == 0 and size <= st.value < size + 32
        self.F, self.size, self.k, self.stride = F, size, k, st.value
        self.nbytes = (size + 7) // 8

    def close(self):
        self.lib.check(self.L.rsk_bloom_pool_destroy(self.h))

    def _call(self, fn, kb, groups, want_out=True):
        """Host batches: numpy groups / replies.  Device batches: the groups go
        up to a DeviceBuffer and the replies are read back from one."""
        from redisson_amd import devmem

        ks = kb.as_struct()
        groups = np.ascontiguousarray(groups, np.uint32)
        if kb.on_device:
            dg = devmem.DeviceBuffer.from_numpy(self.engine, groups)
            do = devmem.DeviceBuffer(self.engine, max(1, kb.n)) if want_out else None
            self.lib.check(fn(self.h, ctypes.byref(ks), dg.ptr, do.ptr if do else None))
            out = do.to_numpy()[: kb.n] if do else None
            dg.free()
            if do:
                do.free()
            return out
        out = np.zeros(max(1, kb.n), np.uint8)
        self.lib.check(fn(self.h, ctypes.byref(ks), groups.ctypes.data, out.ctypes.data if want_out else None))
        return out[: kb.n] if want_out else None

    def add(self, kb, groups, replies=True):
        return self._call(self.L.rsk_bloom_pool_add, kb, groups, replies)

    def contains(self, kb, groups):
        return self._call(self.L.rsk_bloom_pool_contains, kb, groups)

    def raw(self):
        """The device rows read through rsk_memcpy: uint8 [F, stride / 8]."""
        out = np.empty(self.F * self.stride // 8, np.uint8)
        p = self.L.rsk_bloom_pool_device_bits(self.h)
        self.lib.check(self.L.rsk_memcpy(self.engine.ctx, out.ctypes.data, p, out.size, 1))
        return out.reshape(self.F, self.stride // 8)

    def bitcount(self, ids=None):
        n = self.F if ids is None else len(ids)
        out = np.zeros(max(1, n), np.uint64)
        ids = None if ids is None else np.ascontiguousarray(ids, np.uint64)
        self.lib.check(self.L.rsk_bloom_pool_bitcount(self.h, None if ids is None else ids.ctypes.data, n,
                                                      out.ctypes.data))
        return out[:n]

    def count(self, ids=None):
        n = self.F if ids is None else len(ids)
        out = np.zeros(max(1, n), np.int32)
        ids = None if ids is None else np.ascontiguousarray(ids, np.uint64)
        self.lib.check(self.L.rsk_bloom_pool_count(self.h, None if ids is None else ids.ctypes.data, n,
                                                   out.ctypes.data))
        return out[:n]

    def export(self, r):
        out = np.zeros(self.nbytes, np.uint8)
        n = ctypes.c_size_t()
        self.lib.check(self.L.rsk_bloom_pool_export_bits(self.h, r, out.ctypes.data, out.size, ctypes.byref(n)))
        assert n.value == self.nbytes
        return out

    def import_(self, r, data):
        data = np.ascontiguousarray(data, np.uint8)
        self.lib.check(self.L.rsk_bloom_pool_import_bits(self.h, r, data.ctypes.data, data.size))


def check_rows(orc, pool, ref):
    """Every row's bytes, the stride's padding, every BITCOUNT and count()."""
    raw = pool.raw()
    assert np.array_equal(raw[:, : pool.nbytes], ref)
    assert not raw[:, pool.nbytes:].any()  # whole padding bytes
    if pool.size % 8:  # bits beyond `size` in the last byte of the string
        assert not (raw[:, pool.nbytes - 1] & (0xFF >> (pool.size % 8))).any()
    bc = POP8[ref].sum(axis=1, dtype=np.uint64)
    assert np.array_equal(pool.bitcount(), bc)
    want = np.array([orc.bloom_count(pool.size, pool.k, int(b)) for b in bc], np.int32)
    assert np.array_equal(pool.count(), want)
    some = np.array([pool.F - 1, 0, pool.F // 2, 0], np.uint64)  # any order, repeats
    assert np.array_equal(pool.bitcount(some), bc[some.astype(np.int64)])
    assert np.array_equal(pool.count(some), want[some.astype(np.int64)])
    assert np.array_equal(pool.export(pool.F - 1), ref[pool.F - 1])


def test_shape_constants_are_the_library_params():
    from redisson_amd.bloom import bloom_params

    assert bloom_params(10000, 0.01) == P10K
    assert bloom_params(100, 0.03) == (729, 5)  # the JUnit pair


def host16(keys):
    from redisson_amd import KeyBatch

    return KeyBatch.from_numpy(keys.reshape(-1, 16))


# ---------------------------------------------------------------- 1. shapes
SHAPES = [(729, 5, F) for F in (1, 3, 1000, 70000)] + [P10K + (F,) for F in (1, 3, 1000)] + \
         [(524288, 7, F) for F in (1, 3, 1000)]


@pytest.mark.parametrize("n", [0, 1, 200000])
@pytest.mark.parametrize("size,k,F", SHAPES)
def test_shapes(L, engine, orc, size, k, F, n):
    """Rows that are no multiple of 32 bits (729: the stride padding), the
    (10000, 0.01) filter, rows of exactly one 2^19-bit slice; 1, 3, 1000 and
    70000 filters (more than a 16-bit row id; rows straddling slice boundaries);
    empty, single-key and 200000-key batches with uniform groups."""
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    want = pool_add(orc, ref, size, k, groups, keys, None, 16)
    got = pool.add(host16(keys), groups)
    assert np.array_equal(got, want)
    check_rows(orc, pool, ref)
    pool.close()


# ------------------------------------------------------ 2. sequential replies
def _key_with_repeated_bit(orc, size, k):
    """A generated key two of whose first k-1 probes hit one bit, or None."""
    keys = orc.gen_keys16(0x5EED0009, 0, 100000).reshape(-1, 16)
    for i in range(keys.shape[0]):
        idx = orc.bloom_indexes(keys[i].tobytes(), k, size)[: k - 1]
        if len(set(idx)) < len(idx):
            return keys[i]
    return None


@pytest.mark.parametrize("knobs", ["", "reply=1", "reply=-1"])
def test_sequential_replies_under_collisions(L, engine, orc, route, knobs):
    """5000 keys into 2 rows of 729 bits: the rows saturate and most bits are
    probed many times inside one tile.  The same key twice to one filter (the
    second reply is 0), the same key to two filters (both 1), and a key whose
    own probes repeat a bit, at the head of the batch."""
    route(knobs)
    size, k, F = 729, 5, 2
    groups, keys = orc.gen_grouped(0x5EED0006, F, 0, 5000)
    keys = keys.reshape(-1, 16)
    rep = _key_with_repeated_bit(orc, size, k)
    assert rep is not None, "no generated key repeats a bit at size 729 (searched 100000)"
    head = np.stack([keys[0], keys[0], keys[1], keys[1], rep, rep])
    hg = np.array([0, 0, 0, 1, 1, 0], np.uint32)
    keys = np.ascontiguousarray(np.concatenate([head, keys]))
    groups = np.concatenate([hg, groups]).astype(np.uint32)
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    want = pool_add(orc, ref, size, k, groups, keys.reshape(-1), None, 16)
    got = pool.add(host16(keys), groups)
    assert got[:6].tolist() == [1, 0, 1, 1, 1, 1]
    assert np.array_equal(got, want)
    assert not want[-1000:].all() and POP8[ref].sum(dtype=np.uint64) > 0.9 * 2 * size  # saturated rows
    check_rows(orc, pool, ref)
    pool.close()


# ------------------------------------------------------------------- 3. skew
@pytest.mark.parametrize("knobs", ["", "reply=1", "bloom_stream=1"])
@pytest.mark.parametrize("dist", ["hot", "zipf"])
def test_skewed_groups(L, engine, orc, route, dist, knobs):
    """Every key to row 7 of 1000 (the single-filter case inside a pool), and
    Zipf(1.1) groups: replies and rows exact."""
    route(knobs)
    size, k = P10K
    F, n = 1000, 200000
    keys = orc.gen_keys16(0x5EED0003, 0, n)
    groups = np.full(n, 7, np.uint32) if dist == "hot" else orc.gen_grouped_zipf_groups(0x5EED0005, F, 1.1, 0, n)
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    want = pool_add(orc, ref, size, k, groups, keys, None, 16)
    replies = knobs != "bloom_stream=1"  # that knob forces the reply-less insert's routes
    got = pool.add(host16(keys), groups, replies=replies)
    if replies:
        assert np.array_equal(got, want)
    check_rows(orc, pool, ref)
    if dist == "hot":
        assert not np.delete(ref, 7, axis=0).any()
    pool.close()


# ------------------------------------------------- 4. key forms and locations
@pytest.mark.parametrize("device", [False, True])
@pytest.mark.parametrize("form", ["fixed16", "fixed8", "varlen"])
def test_key_forms_and_locations(L, engine, orc, form, device):
    from redisson_amd import KeyBatch, devmem

    size, k, F, n = 729, 5, 37, 6000
    groups = orc.gen_grouped_groups(0x5EED0005, F, 0, n)
    bufs = []
    if form == "varlen":
        blob, offs = orc.gen_varlen(0x5EED0004, 0, n)
        blob = np.ascontiguousarray(blob[: int(offs[-1]) + 1])
        args = (blob, offs, 0)
        if device:
            bufs = [devmem.DeviceBuffer.from_numpy(engine, blob), devmem.DeviceBuffer.from_numpy(engine, offs)]
            kb = bufs[0].keys_var(bufs[1], n)
        else:
            kb = KeyBatch.from_numpy(blob, offs)
    else:
        w = 16 if form == "fixed16" else 8
        data = orc.gen_keys16(0x5EED0003, 0, n).reshape(-1, 16)[:, :w]
        data = np.ascontiguousarray(data).reshape(-1)
        args = (data, None, w)
        if device:
            bufs = [devmem.DeviceBuffer.from_numpy(engine, data)]
            kb = bufs[0].keys_fixed(n, w)
        else:
            kb = KeyBatch.from_numpy(data.reshape(-1, w))
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    want = pool_add(orc, ref, size, k, groups, *args)
    assert np.array_equal(pool.add(kb, groups), want)
    check_rows(orc, pool, ref)
    wrong = ((groups + 1) % F).astype(np.uint32)
    assert np.array_equal(pool.contains(kb, groups), pool_contains(orc, ref, size, k, groups, *args))
    assert pool.contains(kb, groups).all()
    assert np.array_equal(pool.contains(kb, wrong), pool_contains(orc, ref, size, k, wrong, *args))
    assert pool.add(kb, groups, replies=False) is None  # re-adding changes nothing
    check_rows(orc, pool, ref)
    pool.close()
    for b in bufs:
        b.free()


# ------------------------------------------------------------ 5. state carries
def test_state_carries_across_calls(L, engine, orc):
    """Two adds on one pool (the second answered against the rows the first
    left), then contains on inserted and fresh keys mixed, with groups that hit
    the right and the wrong row."""
    size, k = P10K
    F, n, nq = 3, 20000, 30000
    keys = orc.gen_keys16(0x5EED0003, 0, n)
    groups = orc.gen_grouped_groups(0x5EED0005, F, 0, n)
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    h = n // 2
    for a, b in ((0, h + 3000), (h, n)):  # the second call repeats 3000 keys of the first
        want = pool_add(orc, ref, size, k, groups[a:b], keys[16 * a:16 * b], None, 16)
        assert np.array_equal(pool.add(host16(keys[16 * a:16 * b]), groups[a:b]), want)
        if a:
            assert not want[:3000].any()
    check_rows(orc, pool, ref)
    q = orc.gen_queries16(0x5EED0004, 0x5EED0003, n, 0, nq)
    qg = np.random.default_rng(5).integers(0, F, nq).astype(np.uint32)
    want = pool_contains(orc, ref, size, k, qg, q, None, 16)
    assert np.array_equal(pool.contains(host16(q), qg), want)
    assert 0.1 < want.mean() < 0.5  # inserted keys asked in their own row only a third of the time
    pool.close()


# ---------------------------------------------------------------- 6. routes
STAGES = ("bloom_add_each", "bloom_rp1", "bloom_rp2", "bloom_rp_apply", "bloom_rp_reply", "bloom_rp_fallback",
          "bloom_st1", "bloom_st2", "bloom_st_apply", "bloom_part_hist", "bloom_part1", "bloom_part2",
          "bloom_slice_apply")
SORT = {"bloom_add_each"}
TAGS = {"bloom_rp1", "bloom_rp2", "bloom_rp_apply", "bloom_rp_reply"}
ONE = {"bloom_st1", "bloom_st_apply"}
TWO = {"bloom_st1", "bloom_st2", "bloom_st_apply"}
EXACT1 = {"bloom_part_hist", "bloom_part1", "bloom_slice_apply"}
EXACT2 = EXACT1 | {"bloom_part2"}
ROUTES = [
    # (route knobs, replies wanted, F, size, k, the profiler stages that must have run -- and no other of STAGES).
    # Pools of <= 256 slices take the one-level forms, larger ones the two-level ones: 1000 rows of 200003
    # bits = 382 slices, rows straddling them; 70000 rows (a row id above 16 bits) of 729 bits = 99 slices,
    # of 2001 bits = 270 slices.
    ("reply=-1", True, 50, 95851, 7, SORT),                      # the (bit, sequence) sort path
    ("reply=1", True, 50, 95851, 7, TAGS),                       # the group-tag reply pipeline, one coarse level
    ("reply=1", True, 1000, 200003, 7, TAGS),                    # ... over 382 slices
    ("reply=1", True, 70000, 729, 5, TAGS),
    ("reply=1", True, 70000, 2001, 5, TAGS),
    ("reply=1,reply_chunk=300000", True, 50, 95851, 7, TAGS),    # ... in chunks, applied in input order
    ("reply=1,reply_s=4,reply_u=4", True, 1000, 200003, 7, TAGS),  # ... its kernel forms, as the single filter's
    ("reply=1,reply_s=1,reply_u=1,reply_v=3", True, 1000, 200003, 7, TAGS),
    ("reply=1,sa_tiny=1", True, 1000, 200003, 7, {"bloom_rp1"} | SORT),  # rp1 overflows: the sort fallback
    ("bloom_stream=1", False, 50, 95851, 7, ONE),                # st1 -> apply
    ("bloom_stream=1", False, 70000, 729, 5, ONE),
    ("bloom_stream=1", False, 1000, 200003, 7, TWO),             # sa1 -> sa2 -> apply
    ("bloom_stream=1", False, 70000, 2001, 5, TWO),
    ("bloom_stream=1", False, 1000, 200003, 12, TWO),            # ... with 16 probe slots per key
    ("bloom_stream=1,sa_tiny=1,bloom_part=1", False, 1000, 200003, 7, TWO | EXACT2),  # sa1 overflows: the chunk redone by the exact-offset pipeline
    ("bloom_part=1,bloom_stream=-1", False, 50, 95851, 7, EXACT1),       # the exact-offset pipeline, one level
    ("bloom_part=1,bloom_stream=-1", False, 1000, 200003, 7, EXACT2),    # ... two levels
    ("bloom_part=-1,bloom_stream=-1", False, 1000, 200003, 7, set()),    # direct atomics
]


@pytest.mark.parametrize("knobs,replies,F,size,k,stages", ROUTES)
def test_every_route(L, engine, orc, route, knobs, replies, F, size, k, stages):
    """Each pipeline forced on a pool small enough for seconds, and seen to
    have run (the profiler's stage counts; no chunk of a group-tag case
    answered by the fallback): 16-byte keys, then variable-length ones that
    repeat keys of the first batch."""
    from redisson_amd import KeyBatch

    route(knobs)
    n = 100000
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    pool = Pool(L, engine, F, size, k)
    ref = np.zeros((F, pool.nbytes), np.uint8)
    want = pool_add(orc, ref, size, k, groups, keys, None, 16)
    fb0 = engine.reply_stats()[1]
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        got = pool.add(host16(keys), groups, replies=replies)
    finally:
        engine.prof_enable(False)
    ran = {s for s in STAGES if engine.prof_read(s)[1]}
    assert ran == stages, (sorted(ran), sorted(stages))
    assert engine.reply_stats()[1] == fb0
    if replies:
        assert np.array_equal(got, want)
    raw = pool.raw()
    assert np.array_equal(raw[:, : pool.nbytes], ref)
    rng = np.random.default_rng(k + F)
    vk = [rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8).tobytes() for _ in range(3000)]
    vk += vk[:500] + [b""] + [bytes(keys[16 * i: 16 * i + 16]) for i in range(0, 3000, 3)]
    vg = np.concatenate([rng.integers(0, F, 3501), groups[0:3000:3]]).astype(np.uint32)
    blob, offs = orc.pack_keys(vk)
    want = pool_add(orc, ref, size, k, vg, blob, offs)
    got = pool.add(KeyBatch.from_bytes_list(vk), vg, replies=replies)
    if replies:
        assert np.array_equal(got, want)
        assert not want[-1000:].any()  # the 16-byte keys again, in their own rows
    check_rows(orc, pool, ref)
    pool.close()


# ---------------------------------------------------------------- 7. interop
def test_rows_move_to_and_from_single_filters(L, engine, orc):
    from redisson_amd import _lib
    from test_gpu_bloom import _bits, _contains, _filter

    size, k = P10K
    F, n, r = 5, 20000, 2
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    pool = Pool(L, engine, F, size, k)
    pool.add(host16(keys), groups, replies=False)
    q = host16(orc.gen_queries16(0x5EED0004, 0x5EED0005, n, 0, 5000))
    # row r -> an rsk_bloom of the same (size, k): contains agrees
    b = _filter(L, engine, size, k)
    row = pool.export(r)
    _lib.check(L.rsk_bloom_import_bits(b, row.ctypes.data, row.size))
    mine = np.ascontiguousarray(keys.reshape(-1, 16)[groups == r])
    for kb in (q, host16(mine)):
        assert np.array_equal(_contains(L, b, kb), pool.contains(kb, np.full(kb.n, r, np.uint32)))
    assert _contains(L, b, host16(mine)).all()
    # an rsk_bloom's string -> row r: the row is replaced, its neighbours stay
    other = orc.gen_keys16(0x5EED0007, 0, 3000)
    b2 = _filter(L, engine, size, k)
    ks = host16(other).as_struct()
    _lib.check(L.rsk_bloom_add(b2, ctypes.byref(ks), None))
    before = pool.raw().copy()
    pool.import_(r, _bits(L, b2, size))
    after = pool.raw()
    assert np.array_equal(after[r, : pool.nbytes], _bits(L, b2, size)) and not after[r, pool.nbytes:].any()
    assert np.array_equal(np.delete(after, r, axis=0), np.delete(before, r, axis=0))
    for kb in (q, host16(other)):
        assert np.array_equal(_contains(L, b2, kb), pool.contains(kb, np.full(kb.n, r, np.uint32)))
    assert np.array_equal(pool.export(r - 1), before[r - 1, : pool.nbytes])
    assert np.array_equal(pool.export(r + 1), before[r + 1, : pool.nbytes])
    # a shorter string replaces the whole row (SET); clear zeroes every row
    pool.import_(r, np.array([0x80], np.uint8))
    assert pool.bitcount([r])[0] == 1
    _lib.check(L.rsk_bloom_pool_clear(pool.h))
    assert not pool.raw().any()
    L.rsk_bloom_destroy(b)
    L.rsk_bloom_destroy(b2)
    pool.close()


# ------------------------------------------------------ 8. all-or-nothing errors
@pytest.mark.parametrize("device", [False, True])
def test_bad_group_id_changes_nothing(L, engine, orc, device):
    from redisson_amd import _lib, devmem

    size, k, F, n = 729, 5, 40, 10000
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    pool = Pool(L, engine, F, size, k)
    pool.add(host16(keys[: 16 * 500]), groups[:500], replies=False)
    before = pool.raw().copy()
    bad = groups.copy()
    bad[n // 2] = F
    if device:
        dk = devmem.DeviceBuffer.from_numpy(engine, keys)
        dg = devmem.DeviceBuffer.from_numpy(engine, bad)
        out = devmem.DeviceBuffer.from_numpy(engine, np.full(n, 0xAA, np.uint8))
        ks = dk.keys_fixed(n, 16).as_struct()
        gp, op = dg.ptr, out.ptr
        read = out.to_numpy
    else:
        kb = host16(keys)
        ks = kb.as_struct()
        out = np.full(n, 0xAA, np.uint8)
        gp, op = bad.ctypes.data, out.ctypes.data
        read = lambda: out  # noqa: E731
    for fn, o in ((L.rsk_bloom_pool_add, op), (L.rsk_bloom_pool_add, None), (L.rsk_bloom_pool_contains, op)):
        assert fn(pool.h, ctypes.byref(ks), gp, o) == _lib.RSK_ERR_INVALID_ARG
        assert b"out of range" in L.rsk_last_error()
        assert (read() == 0xAA).all()
        assert np.array_equal(pool.raw(), before)
    for ids in ([F], [0, F + 5]):
        a = np.array(ids, np.uint64)
        o64 = np.zeros(2, np.uint64)
        assert L.rsk_bloom_pool_bitcount(pool.h, a.ctypes.data, a.size, o64.ctypes.data) == _lib.RSK_ERR_INVALID_ARG
    n_ = ctypes.c_size_t()
    row = np.zeros(pool.nbytes + 1, np.uint8)
    assert L.rsk_bloom_pool_export_bits(pool.h, F, row.ctypes.data, row.size, ctypes.byref(n_)) == _lib.RSK_ERR_INVALID_ARG
    assert L.rsk_bloom_pool_export_bits(pool.h, 0, row.ctypes.data, pool.nbytes - 1, ctypes.byref(n_)) \
        == _lib.RSK_ERR_INVALID_ARG
    assert L.rsk_bloom_pool_import_bits(pool.h, 0, row.ctypes.data, row.size) == _lib.RSK_ERR_INVALID_ARG
    assert L.rsk_bloom_pool_add(pool.h, ctypes.byref(ks), None, None) == _lib.RSK_ERR_INVALID_ARG  # groups NULL
    assert np.array_equal(pool.raw(), before)
    pool.close()


def test_create_refuses_bad_shapes(L, engine):
    from redisson_amd import _lib

    h = ctypes.c_void_p()
    for F, size, k in ((3, 0, 5), (3, -7, 5), (3, 729, 0), (3, 729, 4097), (0, 729, 5)):
        assert L.rsk_bloom_pool_create(engine.ctx, F, size, k, ctypes.byref(h)) == _lib.RSK_ERR_INVALID_ARG
        assert not h.value and L.rsk_last_error()


# ------------------------------------------------------------ 9. determinism
@pytest.mark.parametrize("knobs", ["", "reply=1"])
def test_same_call_twice_is_identical(L, engine, orc, route, knobs):
    route(knobs)
    size, k = P10K
    F, n = 5, 150000  # 30000 keys per filter sized for 10000: both replies occur
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    res = []
    for _ in range(2):
        pool = Pool(L, engine, F, size, k)
        got = pool.add(host16(keys), groups)
        res.append((got.copy(), pool.raw().copy()))
        pool.close()
    assert np.array_equal(res[0][0], res[1][0]) and np.array_equal(res[0][1], res[1][1])
    assert 0 < res[0][0].sum() < n

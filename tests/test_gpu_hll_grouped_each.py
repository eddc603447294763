"""Grouped PFADD with per-element replies (rsk_hll_add_grouped_each,
rsk_hll_geach.hip): element i goes to sketch groups[i] and out[i] is the reply
Redis gives the i-th PFADD when the n commands run one by one in input order.

References: small cases replay RedisModel.pfadd(str(g), element); larger ones
run a plain loop over the oracle's records (index << 6 | rank) and the group
ids.  Checked after every call: replies, registers, and what the host keeps
per sketch (existence, card cache, kept SET string)."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 16384
SEED_C2 = 0x5EED0002
SEED_G = 0x5EED0006


@pytest.fixture(scope="module")
def L():
    from redisson_amd import _lib

    return _lib.load()


# ------------------------------------------------------------------ helpers
def _pool(L, engine, n):
    from redisson_amd import _lib

    h = ctypes.c_void_p()
    _lib.check(L.rsk_hll_create(engine.ctx, n, ctypes.byref(h)))
    return h


def _regs(L, h, i):
    from redisson_amd import _lib

    out = np.zeros(R, np.uint8)
    _lib.check(L.rsk_hll_get_registers(h, i, out.ctypes.data, _lib.RSK_MEM_HOST))
    return out


def _exists(L, h, i):
    from redisson_amd import _lib

    v = ctypes.c_int(-1)
    _lib.check(L.rsk_hll_exists(h, i, ctypes.byref(v)))
    return v.value


def _export(L, h, i):
    from redisson_amd import _lib

    buf = (ctypes.c_uint8 * 12304)()
    n = ctypes.c_size_t()
    _lib.check(L.rsk_hll_export_redis(h, i, buf, 12304, ctypes.byref(n)))
    return bytes(buf[: n.value])


def _counts(L, h, G):
    from redisson_amd import _lib

    out = np.zeros(G, np.uint64)
    _lib.check(L.rsk_hll_count(h, None, G, out.ctypes.data))
    return out


def _call(L, h, kb, gptr, optr):
    ks = kb.as_struct()
    return L.rsk_hll_add_grouped_each(h, ctypes.byref(ks), gptr, optr)


def _each_host(L, h, kb, groups):
    from redisson_amd import _lib

    groups = np.ascontiguousarray(groups, np.uint32)
    out = np.full(max(1, kb.n), 0xAA, np.uint8)
    _lib.check(_call(L, h, kb, groups.ctypes.data, out.ctypes.data))
    return out[: kb.n]


def _each_dev(L, engine, h, kb, dgroups, goff=0):
    """Device batch: replies read back from a device buffer pre-filled with 0xAA."""
    from redisson_amd import _lib
    from redisson_amd.devmem import DeviceBuffer

    dout = DeviceBuffer.from_numpy(engine, np.full(max(1, kb.n), 0xAA, np.uint8))
    _lib.check(_call(L, h, kb, dgroups.ptr + 4 * goff, dout.ptr))
    out = dout.to_numpy(np.uint8, kb.n)
    dout.free()
    return out


def _ref(state, recs, groups):
    """The n PFADDs one by one over `state` ({sketch << 14 | index: register},
    updated in place): the replies by the register rule."""
    pos = ((groups.astype(np.int64) << 14) | (recs >> 6).astype(np.int64)).tolist()
    rk = (recs & 63).tolist()
    out = bytearray(len(pos))
    get = state.get
    for i, (p, r) in enumerate(zip(pos, rk)):
        if r > get(p, 0):
            state[p] = r
            out[i] = 1
    return np.frombuffer(bytes(out), np.uint8)


class _State:
    """A reference state as arrays, for the registers of single sketches."""

    def __init__(self, state):
        self.p = np.fromiter(state.keys(), np.int64, len(state))
        self.v = np.fromiter(state.values(), np.uint8, len(state))

    def regs(self, g):
        m = (self.p >> 14) == g
        out = np.zeros(R, np.uint8)
        out[self.p[m] & (R - 1)] = self.v[m]
        return out


def _prof(engine, fn):
    """fn() with the profiler on: {stage: launches} of the three stages."""
    engine.prof_reset()
    engine.prof_enable(True)
    try:
        res = fn()
    finally:
        engine.prof_enable(False)
    return res, {s: engine.prof_read("hll_geach_" + s)[1] for s in ("filter", "sort", "scan")}


# --------------------------------------------------- 1. mixed small batch
G1 = 257
UNUSED1 = (3, 128, 256)


@pytest.fixture(scope="module")
def mixed(orc):
    """About 20,000 variable-length elements (1-40 bytes) for 257 sketches: ~30 %
    repeat an earlier (key, sketch) pair, ~5 % send an earlier key to another
    sketch, three sketches are never used; the model's replies and final state."""
    rng = np.random.default_rng(0x6EAC)
    used = np.array([g for g in range(G1) if g not in UNUSED1])
    keys, groups = [], []
    for i in range(20000):
        u = rng.random()
        if i and u < 0.30:
            j = int(rng.integers(i))
            keys.append(keys[j])
            groups.append(groups[j])
        elif i and u < 0.35:
            keys.append(keys[int(rng.integers(i))])
            groups.append(int(rng.choice(used)))
        else:
            keys.append(rng.integers(0, 256, int(rng.integers(1, 41)), dtype=np.uint8).tobytes())
            groups.append(int(rng.choice(used)))
    model = orc.RedisModel()
    replies = np.array([model.pfadd(str(g), k) for g, k in zip(groups, keys)], np.uint8)
    regs = {g: model.db[str(g)].regs.copy() for g in set(groups)}
    assert max(int((r != 0).sum()) for r in regs.values()) < 500  # every sketch stays sparse
    counts = np.array([model.pfcount(str(g)) for g in range(G1)], np.uint64)
    strings = [model.get(str(g)) or b"" for g in range(G1)]  # (after PFCOUNT: caches valid)
    return keys, np.array(groups, np.uint32), replies, regs, counts, strings


def _check_mixed(L, h, mixed, got):
    keys, groups, replies, regs, counts, strings = mixed
    assert np.array_equal(got, replies)
    for g in range(G1):
        assert np.array_equal(_regs(L, h, g), regs.get(g, np.zeros(R, np.uint8))), g
        assert _exists(L, h, g) == (0 if g in UNUSED1 else 1), g
    assert np.array_equal(_counts(L, h, G1), counts)
    for g in range(G1):
        assert _export(L, h, g) == strings[g], g


def test_mixed_batch_host(L, engine, mixed):
    from redisson_amd import GroupedHyperLogLog, KeyBatch

    pool = GroupedHyperLogLog(engine, G1)
    try:
        kb = KeyBatch.from_bytes_list(mixed[0])
        assert kb.offsets is not None  # the blob + offsets form
        out = np.full(kb.n, 0xAA, np.uint8)
        got = pool.addEach(kb, mixed[1], out=out)
        assert got.base is out or got is out
        _check_mixed(L, pool.pool, mixed, got)
    finally:
        pool.close()


def test_mixed_batch_device(L, engine, orc, mixed):
    from redisson_amd import GroupedHyperLogLog
    from redisson_amd.devmem import DeviceBuffer

    pool = GroupedHyperLogLog(engine, G1)
    try:
        blob, offs = orc.pack_keys(mixed[0])
        dblob, doffs = DeviceBuffer.from_numpy(engine, blob), DeviceBuffer.from_numpy(engine, offs)
        dgroups = DeviceBuffer.from_numpy(engine, mixed[1])
        dout = pool.addEach(dblob.keys_var(doffs, len(mixed[0])), dgroups)
        _check_mixed(L, pool.pool, mixed, dout.to_numpy(np.uint8, len(mixed[0])))
    finally:
        pool.close()


# ------------------------------------------ 2. dense sketches, fresh then warm
N2 = 400000
H2 = N2 // 2


@pytest.fixture(scope="module")
def dense(orc, engine):
    """gen_grouped(0x5EED0006, 4, 0, 400000) as device keys; the record loop's
    replies and states after the first and after the second 200,000 pairs."""
    from redisson_amd.devmem import DeviceBuffer

    groups, keys = orc.gen_grouped(SEED_G, 4, 0, N2)
    recs = orc.hll_records(keys, 16, N2)
    state = {}
    r1 = _ref(state, recs[:H2], groups[:H2])
    s1 = _State(state)
    r2 = _ref(state, recs[H2:], groups[H2:])
    s2 = _State(state)
    # (the filter's survivors of the warm call: rank above the register after the first half)
    d = {"groups": groups, "keys": keys.reshape(-1, 16), "recs": recs, "r1": r1, "r2": r2, "s1": s1, "s2": s2,
         "dkeys": DeviceBuffer.from_numpy(engine, keys), "dgroups": DeviceBuffer.from_numpy(engine, groups)}
    yield d
    d["dkeys"].free()
    d["dgroups"].free()


def _half(d, which):
    return d["dkeys"].keys_fixed(H2, 16, offset=16 * H2 * which)


def _two_halves(L, engine, d):
    h = _pool(L, engine, 4)
    a = _each_dev(L, engine, h, _half(d, 0), d["dgroups"], 0)
    b = _each_dev(L, engine, h, _half(d, 1), d["dgroups"], H2)
    return h, a, b


def test_dense_fresh_then_warm(L, engine, orc, dense):
    d = dense
    assert abs(d["r1"].mean() - 0.483) < 0.002 and abs(d["r2"].mean() - 0.163) < 0.002  # both outcomes well represented
    h = _pool(L, engine, 4)
    try:
        a, pa = _prof(engine, lambda: _each_dev(L, engine, h, _half(d, 0), d["dgroups"], 0))
        assert np.array_equal(a, d["r1"])
        for g in range(4):
            assert np.array_equal(_regs(L, h, g), d["s1"].regs(g)), g
        b, pb = _prof(engine, lambda: _each_dev(L, engine, h, _half(d, 1), d["dgroups"], H2))
        assert np.array_equal(b, d["r2"])
        assert pa["sort"] >= 1 and pb["sort"] >= 1 and pa["scan"] >= 1 and pb["scan"] >= 1
        for g in range(4):
            regs = d["s2"].regs(g)
            assert np.array_equal(_regs(L, h, g), regs), g
            assert _exists(L, h, g) == 1
            s = _export(L, h, g)
            assert len(s) == 12304 and s == orc.hll_encode_dense(regs)  # dense, cache invalid
    finally:
        L.rsk_hll_destroy(h)


# --------------------------------------- 3. replay is free and changes nothing
def test_replay_changes_nothing(L, engine, dense):
    d = dense
    h, _, _ = _two_halves(L, engine, d)
    try:
        counts = _counts(L, h, 4)  # PFCOUNT: the caches are valid from here on
        before = [_export(L, h, g) for g in range(4)]
        assert all(s[15] & 0x80 == 0 for s in before)
        out, p = _prof(engine, lambda: _each_dev(L, engine, h, _half(d, 1), d["dgroups"], H2))
        assert not out.any()
        assert p["filter"] >= 1 and p["sort"] == 0 and p["scan"] == 0
        assert [_export(L, h, g) for g in range(4)] == before
        assert np.array_equal(_counts(L, h, 4), counts)
        for g in range(4):
            assert np.array_equal(_regs(L, h, g), d["s2"].regs(g)), g
    finally:
        L.rsk_hll_destroy(h)


def test_kept_set_string_survives_covered_elements(L, engine, orc):
    """SET of a non-canonical sparse string, then elements its registers already
    cover: GET returns the string byte for byte.  One element that raises a
    register then ends that, for its sketch only."""
    from redisson_amd import KeyBatch, _lib

    r2 = np.zeros(R, np.uint8)
    r2[10:14] = 5
    hdr = bytes(orc.hll_encode_sparse(r2)[:16])
    rest = R - 14  # registers 0-9 zero (ZERO 5 + ZERO 5), 10-13 = 5 (VAL 2 + VAL 2), 14.. zero (XZERO)
    nonc = hdr + bytes([4, 4, 0x80 | (4 << 2) | 1, 0x80 | (4 << 2) | 1, 0x40 | ((rest - 1) >> 8), (rest - 1) & 0xFF])
    n = 1 << 18
    keys = orc.gen_keys16(SEED_C2, 0, n).reshape(-1, 16)
    recs = orc.hll_records(keys, 16, n)
    idx, rank = recs >> 6, recs & 63
    covered = keys[(idx >= 10) & (idx < 14) & (rank <= 5)]
    raising = keys[(idx >= 10) & (idx < 14) & (rank > 5)]
    assert covered.shape[0] >= 20 and raising.shape[0] >= 1
    h = _pool(L, engine, 3)
    try:
        for g in (0, 1):
            b = (ctypes.c_uint8 * len(nonc)).from_buffer_copy(nonc)
            _lib.check(L.rsk_hll_import_redis(h, g, b, len(nonc)))
        both = np.concatenate([covered, covered])
        grp = np.repeat(np.array([0, 1], np.uint32), covered.shape[0])
        assert not _each_host(L, h, KeyBatch.from_numpy(both), grp).any()
        assert _export(L, h, 0) == nonc and _export(L, h, 1) == nonc
        assert _exists(L, h, 2) == 0 and _export(L, h, 2) == b""
        out = _each_host(L, h, KeyBatch.from_numpy(np.concatenate([covered[:3], raising[:1]])),
                         np.array([0, 0, 0, 1], np.uint32))
        assert out.tolist() == [0, 0, 0, 1]
        assert _export(L, h, 0) == nonc  # untouched by the other sketch's change
        s1 = _export(L, h, 1)
        assert s1 != nonc and s1[15] & 0x80  # re-encoded, cache invalid
    finally:
        L.rsk_hll_destroy(h)


# ------------------- 4. one register, a run longer than any tile; 9. determinism
@pytest.fixture(scope="module")
def one_register(orc):
    n = 1 << 20
    keys = orc.gen_keys16(SEED_C2, 0, n).reshape(-1, 16)
    recs = orc.hll_records(keys, 16, n)
    sel = np.flatnonzero((recs >> 6) == 7996)
    rank = (recs[sel] & 63).astype(np.int64)
    assert sel.size == 100 and sorted(set(rank.tolist())) == [1, 2, 3, 4, 5, 6, 10]
    low, r3 = sel[rank <= 2], sel[rank == 3]
    high = sel[rank >= 4][np.argsort(rank[rank >= 4], kind="stable")]
    rng = np.random.default_rng(4)
    seq = np.concatenate([rng.choice(low, 30000), r3[:1], rng.choice(low, 30000), high, rng.choice(sel, 40000)])
    assert seq.size == 100014
    return keys[seq], recs[seq], keys[low], recs[low]


def _one_register_run(L, engine, one_register, warm):
    """The sequence into sketch 1 of a pool of 2, empty or first fed the rank <= 2 keys."""
    from redisson_amd import KeyBatch, _lib
    from redisson_amd.devmem import DeviceBuffer

    keys, recs, low, low_recs = one_register
    n = keys.shape[0]
    h = _pool(L, engine, 2)
    state = {}
    try:
        if warm:
            ks = KeyBatch.from_numpy(low).as_struct()
            _lib.check(L.rsk_hll_add(h, 1, ctypes.byref(ks), None))
            _ref(state, low_recs, np.ones(low_recs.size, np.uint32))
        dk = DeviceBuffer.from_numpy(engine, keys)
        dg = DeviceBuffer.from_numpy(engine, np.ones(n, np.uint32))
        got = _each_dev(L, engine, h, dk.keys_fixed(n, 16), dg)
        want = _ref(state, recs, np.ones(n, np.uint32))
        regs = _regs(L, h, 1)
        assert not _regs(L, h, 0).any() and _exists(L, h, 0) == 0
        dk.free()
        dg.free()
        return got, want, regs, _State(state).regs(1)
    finally:
        L.rsk_hll_destroy(h)


def test_one_register_long_run_fresh(L, engine, one_register):
    """Every element survives the filter: one segment spans ~98 scan tiles, so the
    replies deep inside it come from the carry."""
    got, want, regs, want_regs = _one_register_run(L, engine, one_register, warm=False)
    assert want[0] == 1 and want[30000] == 1 and want[60001] == 1 and want[60013] == 1 and not want[60014:].any()
    assert np.array_equal(got, want)
    assert np.array_equal(regs, want_regs) and regs[7996] == 10


def test_one_register_long_run_warm_and_deterministic(L, engine, one_register):
    """The rank <= 2 keys are in already: the survivors are sparse and sit in many
    filter tiles, so the compaction's order decides the replies.  Twice on equal
    pools: byte-identical."""
    got, want, regs, want_regs = _one_register_run(L, engine, one_register, warm=True)
    assert want[30000] == 1 and not want[:30000].any() and want.sum() >= 4
    assert np.array_equal(got, want)
    assert np.array_equal(regs, want_regs)
    again = _one_register_run(L, engine, one_register, warm=True)[0]
    assert got.tobytes() == again.tobytes()


# ------------------------------------------------ 5. many sketches, wide keys
def test_many_sketches_wide_keys(L, engine, orc):
    from redisson_amd.devmem import DeviceBuffer

    G = 262149  # above 2^18: the sort key is above 32 bits
    rng = np.random.default_rng(5)
    n = 160000
    groups = rng.integers(0, G, n).astype(np.uint32)
    groups[rng.choice(n, 10000, replace=False)] = G - 1
    keys = orc.gen_keys16(SEED_C2, 0, n)
    keys.reshape(-1, 16)[5000:9000] = keys.reshape(-1, 16)[1000:5000]  # some repeats, to their own sketches
    groups[5000:9000] = groups[1000:5000]
    recs = orc.hll_records(keys, 16, n)
    state = {}
    want = _ref(state, recs, groups)
    st = _State(state)
    h = _pool(L, engine, G)
    try:
        dk, dg = DeviceBuffer.from_numpy(engine, keys), DeviceBuffer.from_numpy(engine, groups)
        got = _each_dev(L, engine, h, dk.keys_fixed(n, 16), dg)
        dk.free()
        dg.free()
        assert np.array_equal(got, want)
        for g in [G - 1] + rng.choice(groups, 48).tolist() + rng.integers(0, G, 16).tolist():
            assert np.array_equal(_regs(L, h, int(g)), st.regs(int(g))), g
        received = np.zeros(G, bool)
        received[groups] = True
        for g in rng.choice(groups, 500).tolist() + rng.integers(0, G, 500).tolist():
            assert _exists(L, h, int(g)) == int(received[g]), g
    finally:
        L.rsk_hll_destroy(h)


# ------------------------------------- 6. sub-chunks and staged chunks compose
def test_sub_chunks_compose(L, engine, route, dense):
    d = dense
    h0, _, b0 = _two_halves(L, engine, d)
    h1 = _pool(L, engine, 4)
    try:
        _each_dev(L, engine, h1, _half(d, 0), d["dgroups"], 0)
        route(geach_chunk=4096)  # 200,000 elements: 49 sub-chunks
        b1, p = _prof(engine, lambda: _each_dev(L, engine, h1, _half(d, 1), d["dgroups"], H2))
        assert p["filter"] == 49
        assert np.array_equal(b1, b0) and np.array_equal(b1, d["r2"])
        for g in range(4):
            assert np.array_equal(_regs(L, h1, g), _regs(L, h0, g)), g
            assert np.array_equal(_regs(L, h1, g), d["s2"].regs(g)), g
    finally:
        L.rsk_hll_destroy(h0)
        L.rsk_hll_destroy(h1)


def test_staged_host_chunks_compose(L, dense):
    """150,000 host 16-byte keys through a 1 MiB stage: three staged chunks, the
    group ids uploaded and the replies read back per chunk."""
    from redisson_amd import KeyBatch, _lib

    d = dense
    n = 150000
    state = {}
    want = _ref(state, d["recs"][:n], d["groups"][:n])
    st = _State(state)
    e = _lib.Engine(0, staging_bytes=1 << 20)
    try:
        h = _pool(L, e, 4)
        got = _each_host(L, h, KeyBatch.from_numpy(d["keys"][:n]), d["groups"][:n])
        assert np.array_equal(got, want)
        for g in range(4):
            assert np.array_equal(_regs(L, h, g), st.regs(g)), g
        L.rsk_hll_destroy(h)
    finally:
        e.close()


# ------------------------------------------------------------ 7. bad group id
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_bad_group_id_refused_nothing_changed(L, engine, dense, device):
    from redisson_amd import KeyBatch, _lib
    from redisson_amd.devmem import DeviceBuffer

    d = dense
    G, n = 5, 1000
    h = _pool(L, engine, G)
    try:
        _each_host(L, h, KeyBatch.from_numpy(d["keys"][:300]), d["groups"][:300] % 3)  # sketches 0-2 exist
        regs = [_regs(L, h, g) for g in range(G)]
        ex = [_exists(L, h, g) for g in range(G)]
        assert ex == [1, 1, 1, 0, 0]
        keys = d["keys"][1000:1000 + n]
        groups = (np.arange(n) % G).astype(np.uint32)
        groups[n // 2] = G
        if device:
            dk, dg = DeviceBuffer.from_numpy(engine, keys), DeviceBuffer.from_numpy(engine, groups)
            dout = DeviceBuffer.from_numpy(engine, np.full(n, 0xAA, np.uint8))
            rc = _call(L, h, dk.keys_fixed(n, 16), dg.ptr, dout.ptr)
            err = L.rsk_last_error()
            out = dout.to_numpy(np.uint8, n)
        else:
            out = np.full(n, 0xAA, np.uint8)
            rc = _call(L, h, KeyBatch.from_numpy(keys), groups.ctypes.data, out.ctypes.data)
            err = L.rsk_last_error()
        assert rc == _lib.RSK_ERR_INVALID_ARG and b"out of range" in err
        assert (out == 0xAA).all()
        assert [_exists(L, h, g) for g in range(G)] == ex
        for g in range(G):
            assert np.array_equal(_regs(L, h, g), regs[g]), g
    finally:
        L.rsk_hll_destroy(h)


def test_null_arguments_and_empty_batch(L, engine, dense):
    from redisson_amd import KeyBatch, _lib

    h = _pool(L, engine, 2)
    try:
        kb = KeyBatch.from_numpy(dense["keys"][:8])
        groups = np.zeros(8, np.uint32)
        out = np.full(8, 0xAA, np.uint8)
        ks = kb.as_struct()
        for args in ((None, groups.ctypes.data, out.ctypes.data), (ctypes.byref(ks), None, out.ctypes.data),
                     (ctypes.byref(ks), groups.ctypes.data, None)):
            assert L.rsk_hll_add_grouped_each(h, *args) == _lib.RSK_ERR_INVALID_ARG
            assert L.rsk_last_error()
        assert (out == 0xAA).all() and _exists(L, h, 0) == 0
        # a pageable pointer with device keys is refused, not dereferenced
        from redisson_amd.devmem import DeviceBuffer

        dk = DeviceBuffer.from_numpy(engine, dense["keys"][:8])
        assert _call(L, h, dk.keys_fixed(8, 16), groups.ctypes.data, out.ctypes.data) == _lib.RSK_ERR_INVALID_ARG
        dk.free()
        # n = 0: OK, nothing changes (no groups or out needed)
        empty = KeyBatch.from_numpy(np.zeros((0, 16), np.uint8))
        assert _call(L, h, empty, None, None) == _lib.RSK_OK
        assert _exists(L, h, 0) == 0 and _exists(L, h, 1) == 0
    finally:
        L.rsk_hll_destroy(h)


# --------------------------------------- 8. agreement with the existing calls
def test_agrees_with_add_each_and_add_grouped(L, engine, orc, dense):
    from redisson_amd import KeyBatch, _lib

    d = dense
    keys = np.concatenate([d["keys"][:30000], d["keys"][:20000]])
    n = keys.shape[0]
    ha, hb = _pool(L, engine, 1), _pool(L, engine, 1)
    hc, hd = _pool(L, engine, 4), _pool(L, engine, 4)
    try:
        want = np.zeros(n, np.uint8)
        ks = KeyBatch.from_numpy(keys).as_struct()
        _lib.check(L.rsk_hll_add_each(ha, 0, ctypes.byref(ks), want.ctypes.data))
        got = _each_host(L, hb, KeyBatch.from_numpy(keys), np.zeros(n, np.uint32))
        assert np.array_equal(got, want) and got[0] == 1
        assert np.array_equal(_regs(L, hb, 0), _regs(L, ha, 0))
        _each_dev(L, engine, hc, d["dkeys"].keys_fixed(N2, 16), d["dgroups"])
        ks = d["dkeys"].keys_fixed(N2, 16).as_struct()
        _lib.check(L.rsk_hll_add_grouped(hd, ctypes.byref(ks), d["dgroups"].ptr))
        for g in range(4):
            assert np.array_equal(_regs(L, hc, g), _regs(L, hd, g)), g
        assert np.array_equal(_counts(L, hc, 4), _counts(L, hd, 4))
    finally:
        for h in (ha, hb, hc, hd):
            L.rsk_hll_destroy(h)


# ------------------------- the precomputed PFCOUNT of a changed sketch is retired
def test_precomputed_counts_kept_only_where_nothing_grew(L, engine, orc, route, dense):
    """The partitioned grouped add leaves an estimate per sketch; a call that raises
    registers of sketches 0 and 1 only must retire theirs (a stale one would be the
    count before the call) and PFCOUNT of all four must be the oracle's."""
    from redisson_amd import _lib
    from redisson_amd.devmem import DeviceBuffer

    d = dense
    h = _pool(L, engine, 4)
    try:
        route(gpart=1)  # the partitioned add at this size: it estimates every row it writes
        ks = _half(d, 0).as_struct()
        _lib.check(L.rsk_hll_add_grouped(h, ctypes.byref(ks), d["dgroups"].ptr))
        sel = np.flatnonzero(d["groups"][H2:] < 2)[:3000] + H2
        state = {}
        _ref(state, d["recs"][:H2], d["groups"][:H2])
        before = [orc.hll_count_dense(_State(state).regs(g)) for g in range(4)]
        want = _ref(state, d["recs"][sel], d["groups"][sel])
        st = _State(state)
        after = [orc.hll_count_dense(st.regs(g)) for g in range(4)]
        assert after[0] != before[0] and after[1] != before[1] and after[2:] == before[2:]
        dk = DeviceBuffer.from_numpy(engine, d["keys"][sel])
        dg = DeviceBuffer.from_numpy(engine, d["groups"][sel])
        got = _each_dev(L, engine, h, dk.keys_fixed(sel.size, 16), dg)
        dk.free()
        dg.free()
        assert np.array_equal(got, want)
        assert _counts(L, h, 4).tolist() == after
        for g in range(4):
            assert np.array_equal(_regs(L, h, g), st.regs(g)), g
    finally:
        L.rsk_hll_destroy(h)

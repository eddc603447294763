"""The yardstick of the Bloom pool tests: the existing CPU oracle composed per
filter.  A pool call on (keys, groups) must equal: the batch stable-partitioned
by group, oracle.bloom_add_batch / bloom_contains_batch run on each filter's
own bit array, the replies scattered back to input order.  This file holds
that helper and checks it against OracleBloomFilter replayed key by key on
RedisModel (no GPU; passes with or without the pool)."""
import numpy as np


def _sub_keys(idx, data, offsets, fixed_len):
    """Keys idx (input order kept) as (data, offsets, fixed_len, n) for the oracle."""
    if offsets is None:
        sub = np.ascontiguousarray(data.reshape(-1, fixed_len)[idx]).reshape(-1)
        return sub, None, fixed_len, idx.size
    lens = (offsets[1:] - offsets[:-1]).astype(np.int64)
    so = np.zeros(idx.size + 1, np.uint64)
    so[1:] = np.cumsum(lens[idx])
    sub = np.zeros(int(so[-1]) + 1, np.uint8)
    for j, i in enumerate(idx):
        sub[int(so[j]):int(so[j + 1])] = data[int(offsets[i]):int(offsets[i + 1])]
    return sub, so, 0, idx.size


def _per_filter(groups):
    """(filter id, indices of its keys in input order) for every filter with keys."""
    groups = np.asarray(groups, np.uint32)
    order = np.argsort(groups, kind="stable")
    ids, starts = np.unique(groups[order], return_index=True)
    ends = np.append(starts[1:], groups.size)
    return [(int(g), order[a:b]) for g, a, b in zip(ids, starts, ends)]


def pool_add(orc, rows, size, k, groups, data, offsets=None, fixed_len=0):
    """rows: uint8 [F, ceil(size/8)], updated in place; returns add()'s replies in input order."""
    out = np.zeros(len(groups), np.uint8)
    for g, idx in _per_filter(groups):
        d, o, fl, n = _sub_keys(idx, data, offsets, fixed_len)
        out[idx] = orc.bloom_add_batch(rows[g], size, k, d, o, fl, n)
    return out


def pool_contains(orc, rows, size, k, groups, data, offsets=None, fixed_len=0):
    out = np.zeros(len(groups), np.uint8)
    for g, idx in _per_filter(groups):
        d, o, fl, n = _sub_keys(idx, data, offsets, fixed_len)
        out[idx] = orc.bloom_contains_batch(rows[g], size, k, d, o, fl, n)
    return out


def test_helper_matches_redis_model(orc):
    """3 filters f0..f2, a 200-key stream with repeats, replayed key by key."""
    rng = np.random.default_rng(7)
    base = [rng.integers(0, 256, int(rng.integers(1, 40)), dtype=np.uint8).tobytes() for _ in range(120)]
    keys = base + [base[int(i)] for i in rng.integers(0, 120, 80)]  # 200 keys, 80 of them repeats
    order = rng.permutation(200)
    keys = [keys[int(i)] for i in order]
    groups = rng.integers(0, 3, 200).astype(np.uint32)
    redis = orc.RedisModel()
    fs = [orc.OracleBloomFilter(redis, "f%d" % i, lambda b: b) for i in range(3)]
    for f in fs:
        assert f.try_init(100, 0.03)
    size, k = fs[0].size, fs[0].k
    assert (size, k) == (729, 5)
    want_add = np.array([fs[g].add(key) for key, g in zip(keys, groups)], np.uint8)
    blob, offs = orc.pack_keys(keys)
    rows = np.zeros((3, (size + 7) // 8), np.uint8)
    got_add = pool_add(orc, rows, size, k, groups, blob, offs)
    assert np.array_equal(got_add, want_add)
    assert 0 < want_add.sum() < 200
    # queries: every key against the next filter too (right and wrong rows)
    qg = np.concatenate([groups, (groups + 1) % 3]).astype(np.uint32)
    qk = keys + keys
    want_q = np.array([fs[g].contains(key) for key, g in zip(qk, qg)], np.uint8)
    qb, qo = orc.pack_keys(qk)
    assert np.array_equal(pool_contains(orc, rows, size, k, qg, qb, qo), want_q)
    assert want_q[:200].all() and not want_q[200:].all()
    for i, f in enumerate(fs):
        assert f.count() == orc.bloom_count(size, k, orc.bitcount(rows[i]))
    # fixed-length keys take the same path
    fk = orc.gen_keys16(0x5EED0003, 0, 50)
    fg = (np.arange(50) % 3).astype(np.uint32)
    r2 = rows.copy()
    got = pool_add(orc, r2, size, k, fg, fk, None, 16)
    want = np.array([fs[int(g)].add(bytes(fk[16 * i:16 * i + 16])) for i, g in enumerate(fg)], np.uint8)
    assert np.array_equal(got, want)

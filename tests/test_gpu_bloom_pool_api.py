"""redisson_amd.GroupedBloomFilter: the Python face of rsk_bloom_pool_*."""
import numpy as np
import pytest

from test_bloom_pool_model import pool_add, pool_contains

pytestmark = pytest.mark.gpu


def test_round_trip_add_contains_count(engine, orc):
    from redisson_amd import GroupedBloomFilter, KeyBatch, devmem

    F, n = 64, 30000
    gbf = GroupedBloomFilter(engine, F, 1000, 0.01)
    size, k = gbf.getSize(), gbf.getHashIterations()
    assert (size, k) == (orc.bloom_optimal_bits(1000, 0.01), orc.bloom_optimal_k(1000, size))
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    ref = np.zeros((F, (size + 7) // 8), np.uint8)
    want = pool_add(orc, ref, size, k, groups, keys, None, 16)
    kb = KeyBatch.from_numpy(keys.reshape(-1, 16))
    got = gbf.add(kb, groups)
    assert got == [bool(x) for x in want]
    assert all(gbf.contains(kb, groups))
    wrong = ((groups + 1) % F).astype(np.uint32)
    assert gbf.contains(kb, wrong) == [bool(x) for x in pool_contains(orc, ref, size, k, wrong, keys, None, 16)]
    bc = np.array([orc.bitcount(r) for r in ref], np.uint64)
    assert np.array_equal(gbf.bitcount(), bc)
    assert gbf.count().tolist() == [orc.bloom_count(size, k, int(b)) for b in bc]
    assert gbf.count([5, 2]).tolist() == [orc.bloom_count(size, k, int(bc[5])), orc.bloom_count(size, k, int(bc[2]))]
    # device-resident batches answer into device buffers
    dk = devmem.DeviceBuffer.from_numpy(engine, keys)
    dg = devmem.DeviceBuffer.from_numpy(engine, groups)
    out = gbf.contains(dk.keys_fixed(n, 16), dg)
    assert out.to_numpy()[:n].all()
    again = gbf.add(dk.keys_fixed(n, 16), dg)
    assert not again.to_numpy()[:n].any()
    assert gbf.add(dk.keys_fixed(n, 16), dg, replies=False) is None
    for b in (dk, dg, out, again):
        b.free()
    gbf.clear()
    assert not gbf.bitcount().any()
    gbf.close()


def test_row_bytes_feed_a_plain_rbloomfilter(engine, client, orc):
    """toByteArray(i) is the string an RBloomFilter of the same parameters
    holds: a plain filter given those bytes answers the same."""
    from redisson_amd import GroupedBloomFilter, KeyBatch, _lib

    F, n, r = 8, 8000, 3
    gbf = GroupedBloomFilter(engine, F, 1000, 0.01)
    groups, keys = orc.gen_grouped(0x5EED0005, F, 0, n)
    kb = KeyBatch.from_numpy(keys.reshape(-1, 16))
    gbf.add(kb, groups, replies=False)
    bf = client.getBloomFilter("pool-row")
    assert bf.tryInit(1000, 0.01)
    assert (bf.getSize(), bf.getHashIterations()) == (gbf.getSize(), gbf.getHashIterations())
    data = gbf.toByteArray(r)
    a = np.frombuffer(data, np.uint8)
    _lib.check(_lib.load().rsk_bloom_import_bits(bf._filter(), a.ctypes.data, a.size))
    assert bf.toByteArray() == data
    q = KeyBatch.from_numpy(orc.gen_queries16(0x5EED0004, 0x5EED0005, n, 0, 4000).reshape(-1, 16))
    for batch in (kb, q):
        assert bf.containsAll(batch) == gbf.contains(batch, np.full(batch.n, r, np.uint32))
    assert bf.count() == int(gbf.count([r])[0])
    # and back: the plain filter's bytes into another row
    gbf.fromByteArray(r + 1, bf.toByteArray())
    assert gbf.toByteArray(r + 1) == data
    assert gbf.contains(kb, np.full(kb.n, r + 1, np.uint32)) == gbf.contains(kb, np.full(kb.n, r, np.uint32))
    gbf.close()

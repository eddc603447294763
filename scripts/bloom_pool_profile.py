"""Bloom pool (rsk_bloom_pool_*) against what a caller had to do before it: one
rsk_bloom handle per filter and one rsk_bloom_add / rsk_bloom_contains call per
filter over the same keys, pre-partitioned by filter on the device.

One GPU, F = 65536 filters sized for (1000, 0.01), 2^24 uniform 16-byte
device-resident keys.  Timed: pool add without replies, pool add with replies,
pool contains (warm-up, then `reps` steps, rsk_prof stage times), and the
per-filter loop of the same three, and the pool steps again with every key in
one row (a hot row: reported only).  Every loop runs in a fresh process.
--baseline-lib PATH interleaves loops on another build of librsketch.so (the
parent commit's) with this tree's: the builds must agree within the spread
one build shows from process to process, or the single-filter path moved.

  python scripts/bloom_pool_profile.py [--reps 3] [--filters 65536] [--log2n 24]
         [--baseline-lib PATH [--rounds 2]] [--out profiles/bloom_pool.json]"""
import argparse
import ctypes
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import oracle as O  # noqa: E402
from redisson_amd import _lib  # noqa: E402

POOL_STAGES = ("bloom_pool_check", "bloom_add16", "bloom_st1", "bloom_st_mid", "bloom_st2", "bloom_st_apply",
               "bloom_rp1", "bloom_rp_mid", "bloom_rp2", "bloom_rp_apply", "bloom_rp_reply", "bloom_rp_fallback",
               "bloom_add_each", "bloom_contains16", "bloom_part_hist", "bloom_part1", "bloom_part2",
               "bloom_slice_apply")
HOT_ROW = 7


def bind(path):
    """librsketch.so at `path` with every signature it exports (an older build
    lacks the pool's entry points: the per-filter loop does not need them)."""
    L = ctypes.CDLL(path)
    comgr = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "libamd_comgr.so.3")
    if os.path.exists(comgr):
        ctypes.CDLL(comgr, mode=ctypes.RTLD_GLOBAL)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


class Ctx:
    def __init__(self, L):
        self.L = L
        opts = _lib.rsk_options(0, 320, 0)
        self.ctx = ctypes.c_void_p()
        self.ok(L.rsk_init(ctypes.byref(opts), ctypes.byref(self.ctx)))

    def ok(self, rc):
        if rc != 0:
            raise RuntimeError(self.L.rsk_last_error().decode(errors="replace"))

    def alloc(self, nbytes):
        p = ctypes.c_void_p()
        self.ok(self.L.rsk_dev_alloc(self.ctx, max(1, nbytes), ctypes.byref(p)))
        return p.value

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes)
        self.ok(self.L.rsk_memcpy(self.ctx, p, arr.ctypes.data, arr.nbytes, 0))
        return p

    def stages(self, names, reps):
        out = {}
        for s in names:
            ms, cnt = ctypes.c_double(), ctypes.c_uint64()
            self.ok(self.L.rsk_prof_read(self.ctx, s.encode(), ctypes.byref(ms), ctypes.byref(cnt)))
            if cnt.value:
                out[s] = ms.value / reps
        return out


def keys_struct(ptr, n):
    return _lib.rsk_keys(ptr, None, n, 16, _lib.RSK_MEM_DEVICE)


def stream(F, n):
    groups, keys = O.gen_grouped(0x5EED0005, F, 0, n)
    return groups, keys.reshape(-1, 16)


def run_pool(c, F, size, k, groups, keys, reps):
    L, n = c.L, groups.size
    d_keys, d_groups, d_out = c.upload(keys), c.upload(groups), c.alloc(n)
    ks = keys_struct(d_keys, n)
    pool = ctypes.c_void_p()
    c.ok(L.rsk_bloom_pool_create(c.ctx, F, size, k, ctypes.byref(pool)))
    stride = ctypes.c_uint64()
    c.ok(L.rsk_bloom_pool_info(pool, None, None, None, ctypes.byref(stride)))
    res = {"stride_bits": stride.value, "pool_bytes": F * stride.value // 8}

    def timed(name, call, clear):
        ts = []
        for i in range(reps + 1):  # the first is the warm-up (scratch grows)
            if clear:
                c.ok(L.rsk_bloom_pool_clear(pool))
            if i == 1:
                c.ok(L.rsk_prof_reset(c.ctx))
                c.ok(L.rsk_prof_enable(c.ctx, 1))
            t0 = time.perf_counter()
            c.ok(call())
            c.ok(L.rsk_sync(c.ctx))
            ts.append((time.perf_counter() - t0) * 1e3)
        c.ok(L.rsk_prof_enable(c.ctx, 0))
        res[name] = {"call_ms": min(ts[1:]), "call_ms_each": ts[1:], "stage_ms_per_call": c.stages(POOL_STAGES, reps)}

    timed("add", lambda: L.rsk_bloom_pool_add(pool, ctypes.byref(ks), d_groups, None), True)
    timed("add_replies", lambda: L.rsk_bloom_pool_add(pool, ctypes.byref(ks), d_groups, d_out), True)
    timed("contains", lambda: L.rsk_bloom_pool_contains(pool, ctypes.byref(ks), d_groups, d_out), False)
    bc = np.zeros(F, np.uint64)
    c.ok(L.rsk_bloom_pool_bitcount(pool, None, F, bc.ctypes.data))
    res["bits_set"] = int(bc.sum())
    # a hot row (every key to one filter): reported, not compared -- the sub-regions sized for evenly
    # spread probes overflow, the insert is redone by the exact-offset pipeline and the sort path replies
    d_hot = c.upload(np.full(n, HOT_ROW, np.uint32))
    timed("hot_add", lambda: L.rsk_bloom_pool_add(pool, ctypes.byref(ks), d_hot, None), True)
    timed("hot_add_replies", lambda: L.rsk_bloom_pool_add(pool, ctypes.byref(ks), d_hot, d_out), True)
    timed("hot_contains", lambda: L.rsk_bloom_pool_contains(pool, ctypes.byref(ks), d_hot, d_out), False)
    L.rsk_dev_free(c.ctx, d_hot)
    c.ok(L.rsk_bloom_pool_destroy(pool))
    for p in (d_keys, d_groups, d_out):
        L.rsk_dev_free(c.ctx, p)
    return res


def run_loop(c, F, size, k, groups, keys, reps):
    """One handle and one call per filter; the keys partitioned by filter on the device beforehand."""
    L, n = c.L, groups.size
    order = np.argsort(groups, kind="stable")
    starts = np.searchsorted(groups[order], np.arange(F + 1))
    d_keys, d_out = c.upload(keys[order]), c.alloc(n)
    structs = [keys_struct(d_keys + 16 * int(starts[f]), int(starts[f + 1] - starts[f])) for f in range(F)]
    refs = [ctypes.byref(s) for s in structs]
    handles = []
    for _ in range(F):
        h = ctypes.c_void_p()
        c.ok(L.rsk_bloom_create(c.ctx, size, k, ctypes.byref(h)))
        handles.append(h)
    res = {}

    # (the filters are not cleared between steps: a per-filter clear is another F calls, and
    # neither the direct insert nor the sort path's work depends on the bits already set)
    def timed(name, fn, out):
        ts = []
        for _ in range(reps + 1):
            t0 = time.perf_counter()
            for f in range(F):
                rc = fn(handles[f], refs[f], (d_out + int(starts[f])) if out else None)
                if rc:
                    c.ok(rc)
            c.ok(L.rsk_sync(c.ctx))  # the reply-less add only queues its kernel
            ts.append((time.perf_counter() - t0) * 1e3)
        res[name] = {"call_ms": min(ts[1:]), "call_ms_each": ts[1:]}

    timed("add", L.rsk_bloom_add, False)
    timed("add_replies", L.rsk_bloom_add, True)
    timed("contains", L.rsk_bloom_contains, True)
    total = 0
    bc = ctypes.c_uint64()
    for h in handles:
        c.ok(L.rsk_bloom_bitcount(h, ctypes.byref(bc)))
        total += bc.value
        L.rsk_bloom_destroy(h)
    res["bits_set"] = total
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--filters", type=int, default=65536)
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=2, help="(baseline, this tree) loop pairs after the first loop")
    ap.add_argument("--loop-only", metavar="LIB", help="(internal) the per-filter loop on LIB, JSON on stdout")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bloom_pool.json"))
    a = ap.parse_args()
    F, n = a.filters, 1 << a.log2n
    size = O.bloom_optimal_bits(1000, 0.01)
    k = O.bloom_optimal_k(1000, size)
    groups, keys = stream(F, n)
    if a.loop_only:
        c = Ctx(bind(a.loop_only))
        print(json.dumps(run_loop(c, F, size, k, groups, keys, a.reps)), flush=True)
        c.L.rsk_shutdown(c.ctx)
        return
    c = Ctx(bind(_lib.LIB_PATH))
    rec = {"filters": F, "keys": n, "size": size, "k": k, "reps": a.reps}
    rec["pool"] = run_pool(c, F, size, k, groups, keys, a.reps)
    c.L.rsk_shutdown(c.ctx)

    def loop(lib):  # each loop in a fresh process of its own: the same conditions for every build
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--loop-only", lib, "--reps", str(a.reps),
                            "--filters", str(F), "--log2n", str(a.log2n)], capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("per-filter loop on %s failed: %s" % (lib, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    # this tree, then `rounds` times (baseline, this tree): the loops are launch-bound and one build's
    # loop moves from process to process by far more than inside a process, so each build runs several
    # times, interleaved, and the builds are compared range against range
    rec["loop_this_tree"] = [loop(_lib.LIB_PATH)]
    rec["loop_baseline"] = []
    for _ in range(a.rounds if a.baseline_lib else 0):
        rec["loop_baseline"].append(loop(a.baseline_lib))
        rec["loop_this_tree"].append(loop(_lib.LIB_PATH))
    # DESIGN.md's byte model of the pool add without replies (two partition levels): 16 B key +
    # 4 B row id + 12 k of records (sa1 write 4k, sa2 read 4k + write 2k, apply read 2k) per key,
    # plus the pool read and written once
    pool = rec["pool"]
    model = n * (16 + 4 + 12 * k) + 2 * pool["pool_bytes"]
    pool["add"]["model_bytes"] = model
    pool["add"]["model_gbps"] = model / (pool["add"]["call_ms"] * 1e-3) / 1e9
    ops = ("add", "add_replies", "contains")
    for op in ops:  # against the slowest-measured pool step and the fastest loop: the speedup is at least this
        rec["speedup_" + op] = min(r[op]["call_ms"] for r in rec["loop_this_tree"]) / max(pool[op]["call_ms_each"])
    assert all(r["bits_set"] == pool["bits_set"] for r in rec["loop_this_tree"] + rec["loop_baseline"]), \
        "pool and per-filter loop set different bits"
    if rec["loop_baseline"]:
        # per op: each build's best time per process (ms), the spread of the repeats inside one process
        # ((max - min) / min, the largest seen) and from process to process of one build
        agree = {}
        for op in ops:
            this = [r[op]["call_ms"] for r in rec["loop_this_tree"]]
            base = [r[op]["call_ms"] for r in rec["loop_baseline"]]
            every = rec["loop_this_tree"] + rec["loop_baseline"]
            agree[op] = {"this_tree_ms": this, "baseline_ms": base,
                         "spread_within_process": max((max(r[op]["call_ms_each"]) - r[op]["call_ms"]) / r[op]["call_ms"]
                                                      for r in every),
                         "spread_this_tree_between_processes": (max(this) - min(this)) / min(this),
                         "spread_baseline_between_processes": (max(base) - min(base)) / min(base),
                         "ranges_overlap": min(this) <= max(base) and min(base) <= max(this),
                         "best_this_tree_over_best_baseline": min(this) / min(base)}
        rec["loop_agreement"] = agree
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

"""Grouped PFADD with replies (rsk_hll_add_grouped_each) against what a caller
had to do before it: the pairs pre-sorted by sketch, then one rsk_hll_add_each
call per sketch.

One GPU, G = 65536 sketches, 2^24 uniform 16-byte device pairs from
rsk_gen_grouped per batch.  Timed (warm-up, then `reps` steps, rsk_prof stage
times): the new call on a fresh pool (every element survives the filter), on a
warm pool (the second 2^24 pairs of the stream after the first), the same batch
replayed (no survivor), rsk_hll_add_grouped of the same pairs (the floor
without replies), and the per-sketch loop.  Every GPU step runs in a fresh
child process under its own time limit; a step that fails stops the rest.
--baseline-lib PATH runs the loop on another build of librsketch.so (the
parent commit's), interleaved with this tree's: the speed-up is quoted against
the loop on that build.

  python scripts/hll_grouped_each_profile.py [--reps 3] [--sketches 65536] [--log2n 24]
         [--baseline-lib PATH [--rounds 2]] [--out profiles/hll_grouped_each.json]"""
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

SEED = 0x5EED0005
STAGES = ("bloom_pool_check", "hll_geach_filter", "hll_geach_sort", "hll_geach_scan", "hll_clear", "hll_add_grouped16",
          "hll_gpart1", "hll_gpart2", "hll_gpart_count", "hll_gapply")


def bind(path):
    """librsketch.so at `path` with every signature it exports (an older build
    lacks the new entry point: the per-sketch loop does not need it)."""
    L = ctypes.CDLL(path)
    for name, (res, args) in _lib.SIGNATURES.items():
        if hasattr(L, name):
            fn = getattr(L, name)
            fn.restype, fn.argtypes = res, args
    return L


def ok(L, rc):
    if rc != 0:
        raise RuntimeError(L.rsk_last_error().decode(errors="replace"))


def keys_struct(ptr, n):
    return _lib.rsk_keys(ptr, None, n, 16, _lib.RSK_MEM_DEVICE)


def step_pool(G, n, reps):
    """The new call and the reply-less grouped add, this tree's library."""
    from redisson_amd import devmem

    e = _lib.Engine(0)
    L = e.lib
    dg, dk = devmem.gen_grouped(e, SEED, G, 0, 2 * n)  # both batches, back to back
    dout = devmem.DeviceBuffer(e, n)
    ks = [keys_struct(dk.ptr + 16 * n * i, n) for i in (0, 1)]
    gp = [dg.ptr + 4 * n * i for i in (0, 1)]
    h = ctypes.c_void_p()
    ok(L, L.rsk_hll_create(e.ctx, G, ctypes.byref(h)))
    one = np.zeros(16384, np.uint8)
    res = {}

    def fresh():  # an empty pool with the lazy clear completed outside the timed call
        ok(L, L.rsk_hll_clear(h))
        ok(L, L.rsk_hll_get_registers(h, 0, one.ctypes.data, _lib.RSK_MEM_HOST))
        e.sync()

    def warm():
        fresh()
        ok(L, L.rsk_hll_add_grouped(h, ctypes.byref(ks[0]), gp[0]))
        e.sync()

    def timed(name, prepare, call):
        ts = []
        for i in range(reps + 1):  # the first is the warm-up (scratch grows)
            if prepare:
                prepare()
            if i == 1:
                e.prof_reset()
            e.prof_enable(i >= 1)
            t0 = time.perf_counter()
            ok(L, call())
            e.sync()
            ts.append((time.perf_counter() - t0) * 1e3)
            e.prof_enable(False)
        st = {}
        for s in STAGES:
            ms, cnt = e.prof_read(s)
            if cnt:
                st[s] = ms / reps
        res[name] = {"call_ms": min(ts[1:]), "call_ms_each": ts[1:], "stage_ms_per_call": st}

    each = [lambda i=i: L.rsk_hll_add_grouped_each(h, ctypes.byref(ks[i]), gp[i], dout.ptr) for i in (0, 1)]
    plain = [lambda i=i: L.rsk_hll_add_grouped(h, ctypes.byref(ks[i]), gp[i]) for i in (0, 1)]
    timed("each_fresh", fresh, each[0])
    res["each_fresh"]["reply_share"] = float(dout.to_numpy(np.uint8, n).mean())
    timed("each_warm", warm, each[1])
    res["each_warm"]["reply_share"] = float(dout.to_numpy(np.uint8, n).mean())
    timed("each_replay", None, each[1])  # the pool holds both batches: nothing survives
    res["each_replay"]["reply_share"] = float(dout.to_numpy(np.uint8, n).mean())
    counts = np.zeros(G, np.uint64)
    ok(L, L.rsk_hll_count(h, None, G, counts.ctypes.data))
    res["count_sum_two_batches"] = int(counts.sum())
    timed("grouped_fresh", fresh, plain[0])
    ok(L, L.rsk_hll_count(h, None, G, counts.ctypes.data))
    res["count_sum_first_batch"] = int(counts.sum())
    timed("grouped_warm", warm, plain[1])
    ok(L, L.rsk_hll_count(h, None, G, counts.ctypes.data))
    assert int(counts.sum()) == res["count_sum_two_batches"], "the two grouped adds disagree"
    L.rsk_hll_destroy(h)
    e.close()
    return res


def step_loop(lib, G, n, reps):
    """One rsk_hll_add_each per sketch over the first batch, pre-sorted by sketch, on `lib`."""
    L = bind(lib)
    opts = _lib.rsk_options(0, 320, 0)
    ctx = ctypes.c_void_p()
    ok(L, L.rsk_init(ctypes.byref(opts), ctypes.byref(ctx)))
    groups, keys = O.gen_grouped(SEED, G, 0, n)
    order = np.argsort(groups, kind="stable")
    starts = np.searchsorted(groups[order], np.arange(G + 1))
    sorted_keys = np.ascontiguousarray(keys.reshape(-1, 16)[order])
    d_keys, d_out = ctypes.c_void_p(), ctypes.c_void_p()
    ok(L, L.rsk_dev_alloc(ctx, sorted_keys.nbytes, ctypes.byref(d_keys)))
    ok(L, L.rsk_dev_alloc(ctx, n, ctypes.byref(d_out)))
    ok(L, L.rsk_memcpy(ctx, d_keys.value, sorted_keys.ctypes.data, sorted_keys.nbytes, 0))
    structs = [keys_struct(d_keys.value + 16 * int(starts[g]), int(starts[g + 1] - starts[g])) for g in range(G)]
    refs = [ctypes.byref(s) for s in structs]
    h = ctypes.c_void_p()
    ok(L, L.rsk_hll_create(ctx, G, ctypes.byref(h)))
    one = np.zeros(16384, np.uint8)
    ts = []
    for _ in range(reps + 1):
        ok(L, L.rsk_hll_clear(h))
        ok(L, L.rsk_hll_get_registers(h, 0, one.ctypes.data, _lib.RSK_MEM_HOST))
        ok(L, L.rsk_sync(ctx))
        t0 = time.perf_counter()
        for g in range(G):
            if structs[g].n:
                rc = L.rsk_hll_add_each(h, g, refs[g], d_out.value + int(starts[g]))
                if rc:
                    ok(L, rc)
        ok(L, L.rsk_sync(ctx))
        ts.append((time.perf_counter() - t0) * 1e3)
    replies = np.zeros(n, np.uint8)
    ok(L, L.rsk_memcpy(ctx, replies.ctypes.data, d_out.value, n, 1))
    counts = np.zeros(G, np.uint64)
    ok(L, L.rsk_hll_count(h, None, G, counts.ctypes.data))
    L.rsk_hll_destroy(h)
    L.rsk_shutdown(ctx)
    return {"call_ms": min(ts[1:]), "call_ms_each": ts[1:], "reply_share": float(replies.mean()),
            "count_sum": int(counts.sum())}


def survivor_share(G, n):
    """The share of the second batch whose rank is above its register after the first (host)."""
    regs = np.zeros((G, 16384), np.uint8)
    O.hll_add_gen_grouped(regs, G, SEED, 0, n)
    groups, keys = O.gen_grouped(SEED, G, n, n)
    recs = O.hll_records(keys, 16, n)
    return float(((recs & 63) > regs[groups, recs >> 6]).mean())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--sketches", type=int, default=65536)
    ap.add_argument("--log2n", type=int, default=24)
    ap.add_argument("--baseline-lib")
    ap.add_argument("--rounds", type=int, default=2, help="(baseline, this tree) loop pairs")
    ap.add_argument("--step-limit", type=int, default=420, help="seconds per GPU step")
    ap.add_argument("--step", help="(internal) pool | loop: one GPU step, JSON on stdout")
    ap.add_argument("--lib", default=_lib.LIB_PATH, help="(internal) the loop's library")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "hll_grouped_each.json"))
    a = ap.parse_args()
    G, n = a.sketches, 1 << a.log2n
    if a.step == "pool":
        print(json.dumps(step_pool(G, n, a.reps)), flush=True)
        return
    if a.step == "loop":
        print(json.dumps(step_loop(a.lib, G, n, a.reps)), flush=True)
        return

    def child(step, lib=None):  # a fresh process under its own time limit; a failure ends the run
        cmd = ["timeout", "-k", "10", str(a.step_limit), sys.executable, os.path.abspath(__file__), "--step", step,
               "--reps", str(a.reps), "--sketches", str(G), "--log2n", str(a.log2n)]
        if lib:
            cmd += ["--lib", lib]
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise SystemExit("step %s%s failed (exit %d), nothing further is run: %s"
                             % (step, " on " + lib if lib else "", r.returncode, r.stderr[-2000:]))
        return json.loads(r.stdout.strip().splitlines()[-1])

    rec = {"sketches": G, "pairs_per_batch": n, "reps": a.reps}
    rec["pool"] = child("pool")
    rec["pool"]["each_warm"]["survivor_share"] = survivor_share(G, n)
    rec["pool"]["each_fresh"]["survivor_share"] = 1.0
    rec["pool"]["each_replay"]["survivor_share"] = 0.0
    rec["loop_baseline"], rec["loop_this_tree"] = [], []
    for _ in range(a.rounds if a.baseline_lib else 0):
        rec["loop_baseline"].append(child("loop", a.baseline_lib))
        rec["loop_this_tree"].append(child("loop", _lib.LIB_PATH))
    if not rec["loop_this_tree"]:
        rec["loop_this_tree"].append(child("loop", _lib.LIB_PATH))
    loops = rec["loop_baseline"] + rec["loop_this_tree"]
    assert all(r["count_sum"] == rec["pool"]["count_sum_first_batch"] for r in loops), "pool and loop disagree"
    assert all(abs(r["reply_share"] - rec["pool"]["each_fresh"]["reply_share"]) < 1e-12 for r in loops), \
        "pool and loop reply differently"
    ref = rec["loop_baseline"] or rec["loop_this_tree"]  # the comparison: the loop on the parent's build
    # the slowest-measured call against the fastest loop: the speed-up is at least this
    rec["speedup_fresh_vs_loop"] = min(r["call_ms"] for r in ref) / max(rec["pool"]["each_fresh"]["call_ms_each"])
    rec["each_fresh_over_grouped_fresh"] = rec["pool"]["each_fresh"]["call_ms"] / rec["pool"]["grouped_fresh"]["call_ms"]
    rec["each_warm_over_grouped_warm"] = rec["pool"]["each_warm"]["call_ms"] / rec["pool"]["grouped_warm"]["call_ms"]
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec), flush=True)


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""A run proven in segments at blow-up 2, 4 and 8 (stark.prove_rate_segment) and verified as one run, and many whole-run rate proofs verified in one stage run.
  1. the fib loop run for 8 (S - 1) + 1 cycles, S = 2^(K-3) (default K = 20: the 2^20-cycle run less seven rows), in G = 8 row shards of S rows — neighbours share a
     row, as in INTEGRATION.md's recipe — at log_blowup 1, 2, 3 with the default queries and 12 bits: prove time per
     segment (wall, median over the segments of --prove-rounds rounds; the first proof on a context sizes its workspace and is not counted), proof words; the chain verified
     by zkir_verify_rate_chain (host) and zkir_verify_rate_chain_device, alternating call by call after a warm-up, --calls calls each.
  2. 8 whole-run rate proofs of 2^(K-3) rows (log_blowup 2): ONE zkir_verify_rate_many_device call against 8 zkir_verify_rate_device calls of the library --parent
     names (a build of the parent commit, zkir_amd.build.build_variant; the tree's when not given), alternating in one process as scripts/time_verify.py --queries does.
Times are host clocks around calls that synchronise before they return.  Prints what profiles/r23_rate_chain.txt records.
    python scripts/time_rate_chain.py [--k 20] [--calls 200] [--prove-rounds 3] [--parent LIB.so] [--out FILE]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, HERE)
import numpy as np  # noqa: E402
import torch  # noqa: E402
from zkir_amd import pipeline as pl, runtime as rt, spec, stark  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--prove-rounds", type=int, default=3)
ap.add_argument("--parent", default=None)
ap.add_argument("--out", default=None)
a = ap.parse_args()
G = 8
lines = []


def say(t):
    print(t, flush=True); lines.append(t)


def mmm(xs):
    return f"median {statistics.median(xs):.3f} ms (min {min(xs):.3f}, max {max(xs):.3f})"


V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
NEW = rt.lib()                                                       # the tree's build: the prover and the new entries
NEW.zkir_verify_rate_chain.restype = C.c_int; NEW.zkir_verify_rate_chain.argtypes = [V, V, U32, V, U32, U32]
NEW.zkir_verify_rate_chain_device.restype = C.c_int; NEW.zkir_verify_rate_chain_device.argtypes = [V, V, U32, V, U32, U32, V]
NEW.zkir_verify_rate_many_device.restype = C.c_int; NEW.zkir_verify_rate_many_device.argtypes = [V, V, V, V, V, U32, V, V]
NEW.zkir_verify_queries_last.restype = C.c_int; NEW.zkir_verify_queries_last.argtypes = [V, V, V, V]
OLD = C.CDLL(a.parent) if a.parent else NEW                          # the parent's zkir_verify_rate_device
OLD.zkir_verify_rate_device.restype = C.c_int; OLD.zkir_verify_rate_device.argtypes = [V, U64, V, U32, U32, V]
say(f"device {torch.cuda.get_device_name(0)}; single-proof entry from {'a build of the parent commit' if a.parent else 'the tree (no --parent)'}; {a.calls} calls per verifier figure")


def arrays(ps):
    return (C.c_void_p * len(ps))(*[p.ctypes.data for p in ps]), (C.c_uint64 * len(ps))(*[len(p) for p in ps])


blob = spec.fib_endless_program().to_bytes()
seg = (1 << a.k) // G
n = G * (seg - 1) + 1
log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, max_cycles=n))
run_pub = rt.public_inputs(log, blob, [])
cuts = [(g * (seg - 1), g * (seg - 1) + seg) for g in range(G)]      # neighbouring segments share a row
traces = []
for lo, hi in cuts:
    sh = log.shard(lo, hi)
    ddl = pl.upload(sh); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    pub = rt.PublicInputsC.from_buffer_copy(run_pub); pub.n_real = hi - lo
    traces.append((sh, ddl, tr, pub))
log_n = stark.padded_log_n(seg)
assert log.n_rows == n and cuts[-1][1] == n
say(f"\n1. fib, {n} cycles in {G} segments of {seg} rows, context log_n {log_n}; default queries, 12 bits")
for b in (1, 2, 3):
    ctx = stark.StarkContext(log_n, b)
    nq = rt.RATE_DEFAULT_QUERIES[b]
    stark.prove_rate_segment(ctx, traces[0][2], traces[0][3])          # (sizes the workspace)
    walls, proofs = [], []
    for rnd in range(a.prove_rounds):
        proofs = []
        for sh, ddl, tr, pub in traces:
            torch.cuda.synchronize()
            t0 = time.perf_counter(); p = stark.prove_rate_segment(ctx, tr, pub); walls.append((time.perf_counter() - t0) * 1e3)
            proofs.append(np.ascontiguousarray(p, dtype=np.uint32))
    ctx.close()
    ptrs, lens = arrays(proofs)
    e = C.byref(run_pub)
    for _ in range(3):
        assert NEW.zkir_verify_rate_chain(ptrs, lens, G, e, nq, 12) == 0 and NEW.zkir_verify_rate_chain_device(ptrs, lens, G, e, nq, 12, None) == 0
    host, dev = [], []
    for _ in range(a.calls):
        t0 = time.perf_counter(); rc = NEW.zkir_verify_rate_chain(ptrs, lens, G, e, nq, 12); host.append((time.perf_counter() - t0) * 1e3); assert rc == 0, rc
        t0 = time.perf_counter(); rc = NEW.zkir_verify_rate_chain_device(ptrs, lens, G, e, nq, 12, None); dev.append((time.perf_counter() - t0) * 1e3); assert rc == 0, rc
    h, v, l, u = C.c_uint64(), C.c_uint64(), C.c_uint32(), C.c_uint64()
    NEW.zkir_verify_queries_last(C.byref(h), C.byref(v), C.byref(l), C.byref(u))
    say(f"  b={b} queries={nq}: prove per segment {mmm(walls)} over {len(walls)} proofs; proof words per segment {len(proofs[1])}, chain total {sum(len(p) for p in proofs)}")
    say(f"     chain of {G}: zkir_verify_rate_chain (host) {mmm(host)}; zkir_verify_rate_chain_device {mmm(dev)}; stage: {h.value} hash jobs, {v.value} value jobs, {l.value} launches, {u.value} words up")
for sh, ddl, tr, pub in traces:
    sh.close()
del traces
torch.cuda.empty_cache()

# ---- 2. eight independent whole-run proofs: one batch against eight single calls ----
rows = seg
wlog = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, max_cycles=rows))
wpub = rt.public_inputs(wlog, blob, [])
ddl = pl.upload(wlog); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
ctx = stark.StarkContext(stark.padded_log_n(rows), 2)
whole = [np.ascontiguousarray(stark.prove_rate(ctx, tr, wpub, 25, 12 + (i % 3)), dtype=np.uint32) for i in range(G)]      # (three grinding settings: the proofs are not all the same words)
ctx.close()
ptrs, lens = arrays(whole)
exps = (C.c_void_p * G)(*[C.addressof(wpub)] * G)
verdicts = (C.c_int32 * G)()
for _ in range(3):
    assert NEW.zkir_verify_rate_many_device(ptrs, lens, exps, None, None, G, verdicts, None) == 0 and not any(verdicts)
    assert all(OLD.zkir_verify_rate_device(p.ctypes.data, len(p), C.byref(wpub), 1, 0, None) == 0 for p in whole)
one, many = [], []
for _ in range(a.calls):
    t0 = time.perf_counter()
    for p in whole:
        rc = OLD.zkir_verify_rate_device(p.ctypes.data, len(p), C.byref(wpub), 1, 0, None); assert rc == 0, rc
    one.append((time.perf_counter() - t0) * 1e3)
    t0 = time.perf_counter(); rc = NEW.zkir_verify_rate_many_device(ptrs, lens, exps, None, None, G, verdicts, None); many.append((time.perf_counter() - t0) * 1e3)
    assert rc == 0 and not any(verdicts)
say(f"\n2. {G} whole-run proofs of {rows} rows at b=2, 25 queries ({len(whole[0])} words each)")
say(f"     {G} x zkir_verify_rate_device, one call each: {mmm(one)}")
say(f"     1 x zkir_verify_rate_many_device:           {mmm(many)}")
r = statistics.median(many) / statistics.median(one)
say(f"     batch / sum of single calls = {r:.3f}" + ("" if r < 1 else "  (the batch is NOT below the sum of the single calls)"))
if a.out:
    open(a.out, "w").write("\n".join(lines) + "\n")

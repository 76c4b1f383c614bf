#!/usr/bin/env python3
"""zkir_verify_many_memory_device / zkir_verify_rate_many_memory_device (the memory sections of MANY proofs as one GPU batch) against the many-proof entries that keep a
mode-3 front's section on the host (zkir_verify_many_on_device / zkir_verify_rate_many_device, from the library --parent names, else this build's), against n calls of the
single-proof zkir_verify_memory_device, and against themselves on their host route — in one process, the entries of a block alternating call by call:
  1. --big N proofs of the array loop at 2^K cycles (mode 3, 65 535 cells at K = 20) in one call: the 'ZKIR' proofs, and the 'ZKSR' proofs at blow-up 4;
  2. --small N proofs of spec.memory_loop_program(300) in one call (the per-proof device route is off at this size);
  3. --cross: batches of 1, 2, 4, .. proofs of 64-cell sections, device route (ZKIR_VERIFY_DEVICE_MIN_CELLS = 0) against host route (2^30), until the device route wins.
A block whose calls take more than 100 ms runs fewer rounds (at least 20).
    python scripts/time_verify_many_memory.py [--calls 200] [--k 20] [--big 8] [--small 64] [--cross 64] [--parent PATH/libzkir_amd.so]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from zkir_amd import pipeline as pl, runtime as rt, spec, stark  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--big", type=int, default=8)
ap.add_argument("--small", type=int, default=64)
ap.add_argument("--cross", type=int, default=64, help="cells of the crossing's sections (0: skip)")
ap.add_argument("--parent", default="")
a = ap.parse_args()
med = statistics.median
V, U32 = C.c_void_p, C.c_uint32
OLD = C.CDLL(a.parent) if a.parent else rt.lib()
OLD.zkir_verify_many_on_device.restype = C.c_int; OLD.zkir_verify_many_on_device.argtypes = [V, V, V, U32, V, V]
OLD.zkir_verify_rate_many_device.restype = C.c_int; OLD.zkir_verify_rate_many_device.argtypes = [V, V, V, V, V, U32, V, V]
OLD.zkir_verify_memory_device.restype = C.c_int; OLD.zkir_verify_memory_device.argtypes = [V, C.c_uint64, V, C.c_int, V]
PARENT = " (parent)" if a.parent else ""


def device_run(blob, cycles):
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=cycles, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    return log, ddl, tr


def alternate(fns, calls):
    """fns: [(label, callable -> True)]; every callable once per round; prints median and minimum and returns them"""
    ms = [[] for _ in fns]
    for _, f in fns:
        t0 = time.perf_counter(); assert f(); warm = (time.perf_counter() - t0) * 1e3
        if warm > 100:
            calls = max(20, min(calls, int(calls * 100 / warm)))
    for _ in range(calls):
        for i, (_, f) in enumerate(fns):
            t0 = time.perf_counter(); ok = f(); ms[i].append((time.perf_counter() - t0) * 1e3); assert ok
    for (label, _), m in zip(fns, ms):
        print(f"     {label}: median {med(m):.3f} ms, min {min(m):.3f}, max {max(m):.3f}  ({calls} calls)", flush=True)
    return [med(m) for m in ms], [min(m) for m in ms]


def many_args(proofs, pubs):
    n = len(proofs)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in proofs]); lens = (C.c_uint64 * n)(*[len(p) for p in proofs])
    exps = (C.c_void_p * n)(*[C.addressof(e) for e in pubs]); out = (C.c_int32 * n)()
    return n, ptrs, lens, exps, out


def route(min_cells, f):
    def g():
        os.environ["ZKIR_VERIFY_DEVICE_MIN_CELLS"] = str(min_cells)
        try:
            return f()
        finally:
            os.environ.pop("ZKIR_VERIFY_DEVICE_MIN_CELLS", None)
    return g


def zkir_block(label, proof, pub, n, with_single=True):
    proofs, pubs = [proof] * n, [pub] * n
    n, ptrs, lens, exps, out = many_args(proofs, pubs)
    ok = [0] * n
    def parent_many():
        return OLD.zkir_verify_many_on_device(ptrs, lens, exps, n, out, None) == 0 and list(out) == ok
    def one_by_one():
        return all(OLD.zkir_verify_memory_device(proof.ctypes.data, len(proof), C.byref(pub), 1, None) == 0 for _ in range(n))
    new = lambda: rt.verify_many(proofs, pubs, memory=True) == ok  # noqa: E731
    print(f"   {label}: {n} proofs in one call")
    fns = [("zkir_verify_many_on_device" + PARENT, parent_many), ("zkir_verify_many_memory_device", new),
           ("zkir_verify_many_memory_device, host route (threshold above the total)", route(1 << 40, new))]
    if with_single:
        fns.append((f"{n} calls of zkir_verify_memory_device(queries = 1)" + PARENT, one_by_one))
    m, lo = alternate(fns, a.calls)
    assert new()
    print(f"     zkir_verify_memory_last: {rt.verify_memory_last()}; queries: {rt.verify_queries_last()}")
    print(f"     new median / parent minimum: {m[1]:.3f} / {lo[0]:.3f} = {m[1] / lo[0]:.3f}" + (f"; new median / one-by-one median: {m[1]:.3f} / {m[3]:.3f} = {m[1] / m[3]:.3f}" if with_single else ""), flush=True)
    return m, lo


def rate_block(label, rp, pub, nq, n):
    proofs, pubs = [rp] * n, [pub] * n
    n, ptrs, lens, exps, out = many_args(proofs, pubs)
    mq, mb = (U32 * n)(*[nq] * n), (U32 * n)(*[12] * n)
    ok = [0] * n
    def parent_many():
        return OLD.zkir_verify_rate_many_device(ptrs, lens, exps, mq, mb, n, out, None) == 0 and list(out) == ok
    new = lambda: rt.verify_rate_many(proofs, pubs, [nq] * n, [12] * n, memory=True) == ok  # noqa: E731
    print(f"   {label}: {n} proofs in one call")
    m, lo = alternate([("zkir_verify_rate_many_device" + PARENT, parent_many), ("zkir_verify_rate_many_memory_device", new)], a.calls)
    print(f"     new median / parent minimum: {m[1]:.3f} / {lo[0]:.3f} = {m[1] / lo[0]:.3f}", flush=True)


def prove_loop(cells, cycles, rate_b=0):
    blob = spec.memory_loop_program(cells).to_bytes()
    log, ddl, tr = device_run(blob, cycles)
    pub = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="device")
    log_n = stark.padded_log_n(log.n_rows)
    ctx = stark.StarkContext(log_n)
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    rp = None
    if rate_b:
        rctx = stark.StarkContext(log_n, rate_b)
        rp = stark.prove_rate_modes(rctx, tr, pub)
        rctx.close()
    rows = log.n_rows
    log.close()
    del ddl, tr
    torch.cuda.empty_cache()
    return proof, rp, pub, rows


print(f"device {torch.cuda.get_device_name(0)}; up to {a.calls} calls per figure, alternating; parent library: {a.parent or '(this build)'}")
if a.big:
    n_cycles = 1 << a.k
    proof, rp, pub, rows = prove_loop(min(65535, n_cycles // 13), n_cycles, rate_b=2)
    cells = int(proof[stark.proof_layout(proof)["mem_section"]])
    print(f"\n1. array loop (spec.memory_loop_program): {rows} rows, mode 3, {cells} cells, proof words {len(proof)} ('ZKIR') / {len(rp)} ('ZKSR', blow-up 4)", flush=True)
    zkir_block("'ZKIR' proofs (blow-up 2)", proof, pub, a.big)
    rate_block(f"'ZKSR' proofs at blow-up 4 ({rt.RATE_DEFAULT_QUERIES[2]} queries, 12 bits)", rp, pub, rt.RATE_DEFAULT_QUERIES[2], a.big)
    del proof, rp
if a.small:
    proof, _, pub, rows = prove_loop(300, 1 << 24)
    print(f"\n2. spec.memory_loop_program(300): {rows} rows, mode 3, 300 cells, proof words {len(proof)}", flush=True)
    zkir_block("'ZKIR' proofs", proof, pub, a.small)
if a.cross:
    proof, _, pub, rows = prove_loop(a.cross, 1 << 24)
    print(f"\n3. the routing crossing: batches of proofs of spec.memory_loop_program({a.cross}) ({rows} rows, {a.cross} cells each); device route = threshold 0, host route = threshold 2^40", flush=True)
    n = 1
    while n <= 64:
        proofs, pubs = [proof] * n, [pub] * n
        ok = [0] * n
        new = lambda: rt.verify_many(proofs, pubs, memory=True) == ok  # noqa: E731
        print(f"   {n} proofs, {n * a.cross} cells in all:")
        m, lo = alternate([("host route  ", route(1 << 40, new)), ("device route", route(0, new))], a.calls)
        print(f"     device median - host median: {m[1] - m[0]:+.3f} ms", flush=True)
        n *= 2

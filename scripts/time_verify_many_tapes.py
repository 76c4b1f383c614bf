#!/usr/bin/env python3
"""zkir_verify_many_tapes_device (the hash and wide tapes of MANY mode-4 proofs as one GPU batch beside the memory batch) against zkir_verify_many_memory_device, which
gives every mode-4 front its own device tape stages (from the library --parent names, else this build's), and against n calls of the single-proof
zkir_verify_memory_device — in one process, the entries of a block alternating call by call:
  1. --mixed N mode-4 proofs of the SHA chain stopped after 1 .. 20 hash calls, in one call;
  2. --chain N proofs of the SHA chain at 2^12 cycles, in one call;
  3. --wide N proofs of the signed-division loop (wide records, no hash call), in one call.
A block whose calls take more than 100 ms runs fewer rounds (at least 20).
    python scripts/time_verify_many_tapes.py [--calls 200] [--mixed 64] [--chain 8] [--wide 64] [--parent PATH/libzkir_amd.so]"""
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
ap.add_argument("--mixed", type=int, default=64)
ap.add_argument("--chain", type=int, default=8)
ap.add_argument("--wide", type=int, default=64)
ap.add_argument("--parent", default="")
a = ap.parse_args()
med = statistics.median
V, U32 = C.c_void_p, C.c_uint32
OLD = C.CDLL(a.parent) if a.parent else rt.lib()
OLD.zkir_verify_many_memory_device.restype = C.c_int; OLD.zkir_verify_many_memory_device.argtypes = [V, V, V, U32, V, V]
OLD.zkir_verify_memory_device.restype = C.c_int; OLD.zkir_verify_memory_device.argtypes = [V, C.c_uint64, V, C.c_int, V]
PARENT = " (parent)" if a.parent else ""


def prove_mode4(blob, cycles):
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=cycles, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    pub = rt.public_inputs(log, blob, [], wide_mode=True, hash_witness="device")
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    log.close()
    lay = stark.proof_layout(proof)
    return proof, pub, int(proof[lay["hash_section"]]), int(proof[lay["wide_section"]])


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


def block(label, proofs, pubs):
    n = len(proofs)
    ptrs = (C.c_void_p * n)(*[p.ctypes.data for p in proofs]); lens = (C.c_uint64 * n)(*[len(p) for p in proofs])
    exps = (C.c_void_p * n)(*[C.addressof(e) for e in pubs]); out = (C.c_int32 * n)()
    ok = [0] * n
    def parent_many():
        return OLD.zkir_verify_many_memory_device(ptrs, lens, exps, n, out, None) == 0 and list(out) == ok
    def one_by_one():
        return all(OLD.zkir_verify_memory_device(p.ctypes.data, len(p), C.byref(e), 1, None) == 0 for p, e in zip(proofs, pubs))
    new = lambda: rt.verify_many(proofs, pubs, tapes=True) == ok  # noqa: E731
    print(f"   {label}: {n} proofs in one call")
    m, lo = alternate([("zkir_verify_many_memory_device" + PARENT, parent_many), ("zkir_verify_many_tapes_device", new),
                       (f"{n} calls of zkir_verify_memory_device(queries = 1)" + PARENT, one_by_one)], a.calls)
    assert new()
    print(f"     zkir_verify_tapes_last: {rt.verify_tapes_last()}; memory: {rt.verify_memory_last()}; queries: {rt.verify_queries_last()}")
    print(f"     new median / parent minimum: {m[1]:.3f} / {lo[0]:.3f} = {m[1] / lo[0]:.3f}; new median / one-by-one median: {m[1]:.3f} / {m[2]:.3f} = {m[1] / m[2]:.3f}", flush=True)


print(f"device {torch.cuda.get_device_name(0)}; up to {a.calls} calls per figure, alternating; parent library: {a.parent or '(this build)'}")
chain = spec.sha256_chain_program().to_bytes()
if a.mixed:
    made, cycles = {}, 8
    while len(made) < 20 and cycles < 4096:                      # the chain stopped after 1, 2, .. 20 calls: one proof per call count
        proof, pub, nh, nw = prove_mode4(chain, cycles)
        if 1 <= nh <= 20 and nh not in made:
            made[nh] = (proof, pub)
        cycles += 2
    ks = sorted(made)
    pick = [made[ks[i % len(ks)]] for i in range(a.mixed)]
    print(f"\n1. the SHA chain stopped after {ks[0]} .. {ks[-1]} hash calls ({len(ks)} different proofs, mode 4, proof words {len(made[ks[0]][0])} .. {len(made[ks[-1]][0])})", flush=True)
    block("mixed call counts", [p for p, _ in pick], [e for _, e in pick])
if a.chain:
    proof, pub, nh, nw = prove_mode4(chain, 1 << 12)
    print(f"\n2. the SHA chain at 2^12 cycles: {nh} hash calls, {nw} wide records, proof words {len(proof)}", flush=True)
    block("2^12-cycle chains", [proof] * a.chain, [pub] * a.chain)
if a.wide:
    proof, pub, nh, nw = prove_mode4(spec.signed_division_loop_program().to_bytes(), 300)
    print(f"\n3. the signed-division loop, 300 cycles: {nh} hash calls, {nw} wide records, proof words {len(proof)}", flush=True)
    block("wide arithmetic", [proof] * a.wide, [pub] * a.wide)

#!/usr/bin/env python3
"""Proofs of mode-3 and mode-4 runs at blow-up 2, 4 and 8 (stark.prove_rate_modes, 'ZKSR') beside zkir_prove in the same process, on bench.py's prove_by_mode workloads:
the array loop (852 k rows, mode 3, witness on the device) and the wide-arithmetic loop (2^20 rows, mode 4).  Per rate: wall and device ms (medians, alternating with
zkir_prove), proof words, the eleven stage times; at b = 1 the quotient stage against zkir_prove's of the same run; zkir_verify_rate on the host against the device form
(medians of alternating calls).  --sha K adds the SHA-256 chain at 2^K rows (mode 4, tape on the device) at b = 2, 3.
    python scripts/time_prove_rate_modes.py [--calls 7] [--verify-calls 50] [--k 20] [--sha K] [--modes 3,4]"""
import argparse
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from zkir_amd import pipeline as pl, runtime as rt, spec, stark  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=7)
ap.add_argument("--verify-calls", type=int, default=50)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--sha", type=int, default=0)
ap.add_argument("--modes", default="3,4")
ap.add_argument("--rates", default="1,2,3")
a = ap.parse_args()
n = 1 << a.k
med = statistics.median
RATE = ["main trace", "LDE", "trace Merkle", "lookup arg", "quotient+Merkle", "weights", "evaluations", "eval quotient", "FRI commit", "grinding", "queries"]


def device_run(blob, cycles):
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=cycles, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    return log, ddl, tr


def timed(fn, calls):
    walls, stages = [], []
    for _ in range(calls):
        t0 = time.perf_counter(); proof, ms = fn(); walls.append((time.perf_counter() - t0) * 1e3); stages.append(ms)
    k = walls.index(sorted(walls)[len(walls) // 2])
    return med(walls), min(walls), max(walls), stages[k], proof


def measure(label, blob, cycles, mode, rates, hash_witness="host"):
    log, ddl, tr = device_run(blob, cycles)
    log_n = stark.padded_log_n(log.n_rows)
    pub = rt.public_inputs(log, blob, [], mem_mode=mode == 3, wide_mode=mode == 4, mem_witness="device", hash_witness=hash_witness)
    print(f"\n{label}: {log.n_rows} rows (log_n {log_n}), mode {mode}", flush=True)
    base = stark.StarkContext(log_n) if 1 in rates else None
    for b in rates:
        ctx = base if b == 1 else stark.StarkContext(log_n, b)
        nq = rt.RATE_DEFAULT_QUERIES[b]
        stark.prove_rate_modes(ctx, tr, pub)                                # (the first call sizes the workspace)
        w = timed(lambda: stark.prove_rate_modes(ctx, tr, pub, want_stage_ms=True), a.calls)
        proof = w[4]
        print(f"  b={b} queries={nq} bits=12: prove_rate_modes wall median {w[0]:.2f} ms (min {w[1]:.2f} max {w[2]:.2f}), device sum {sum(w[3]):.2f} ms, proof words {len(proof)}")
        print("     stages [" + ", ".join(RATE) + "] ms: " + " ".join(f"{x:.3f}" for x in w[3]), flush=True)
        if b == 1:
            stark.prove(ctx, tr, pub)
            z = timed(lambda: stark.prove(ctx, tr, pub, want_stage_ms=True), a.calls)
            print(f"     zkir_prove beside it: wall median {z[0]:.2f} ms (min {z[1]:.2f} max {z[2]:.2f}), device sum {sum(z[3]):.2f} ms, proof words {len(z[4])}; stages: " + " ".join(f"{x:.3f}" for x in z[3]))
            print(f"     quotient stage at b=1: quotient_rate_kernel<{mode}> + Merkle {w[3][4]:.3f} ms vs quotient_kernel<{mode}> + Merkle {z[3][4]:.3f} ms: ratio {w[3][4] / z[3][4]:.3f}")
            print(f"     lookup-argument stage at b=1 {w[3][3]:.3f} vs {z[3][3]:.3f} ms; LDE {w[3][1]:.3f} vs {z[3][1]:.3f}; trace Merkle {w[3][2]:.3f} vs {z[3][2]:.3f}", flush=True)
        host, dev = [], []
        for _ in range(a.verify_calls):
            t0 = time.perf_counter(); rc = rt.verify_rate(proof, pub, nq, 12); host.append((time.perf_counter() - t0) * 1e3); assert rc == 0, rc
            t0 = time.perf_counter(); rc = stark.verify_rate(proof, pub, nq, 12, device=True); dev.append((time.perf_counter() - t0) * 1e3); assert rc == 0, rc
        print(f"     verify b={b}: zkir_verify_rate host median {med(host):.3f} ms, device {med(dev):.3f} ms ({a.verify_calls} calls each, alternating)", flush=True)
        if ctx is not base:
            ctx.close()
    if base is not None:
        base.close()
    log.close()
    del ddl, tr
    torch.cuda.empty_cache()


print(f"device {torch.cuda.get_device_name(0)}; {a.calls} proofs and {a.verify_calls} verifications per figure")
rates = [int(x) for x in a.rates.split(",")]
if "3" in a.modes.split(","):
    measure("array loop (spec.memory_loop_program), witness on the device", spec.memory_loop_program(min(65535, n // 13)).to_bytes(), n, 3, rates)
if "4" in a.modes.split(","):
    measure("wide-arithmetic loop (spec.wide_loop_program: 6 of 18 rows MULH / DIVU / REMU / DIV / REM)", spec.wide_loop_program().to_bytes(), n, 4, rates)
if a.sha:
    measure("SHA-256 hash chain (spec.sha256_chain_program), witness and tape on the device", spec.sha256_chain_program().to_bytes(), 1 << a.sha, 4, [b for b in rates if b > 1], hash_witness="device")

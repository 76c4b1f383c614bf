#!/usr/bin/env python3
"""zkir_verify_memory_device / zkir_verify_rate_memory_device (the touched-cell section's stages on the GPU) against the host verifier and against the entries that keep a
mode-3 front on the host (zkir_verify_on_device / zkir_verify_rate_device, from the library --parent names, else this build's), in one process, alternating:
  1. the array loop at 2^K cycles (mode 3, 65 535 cells at K = 20): the 'ZKIR' proof and the 'ZKSR' proofs at blow-up 2, 4 and 8;
  2. --sha K: the SHA-256 chain at 2^K cycles (mode 4);
  3. the stages on their own (the stand-alone entries on the proof's section: each launch form allocates, uploads, runs and synchronises) and the verifier's host clocks;
  4. small sections (array loops of 1, 64, 1000 and 8000 cells): the new entry with every section on the device against the same entry with
     ZKIR_VERIFY_DEVICE_MIN_CELLS above the section (its host route).
    python scripts/time_verify_memory.py [--calls 200] [--k 20] [--sha 20] [--parent PATH/libzkir_amd.so] [--sweep 1,64,1000,8000] [--sweep-only]"""
import argparse
import ctypes as C
import os
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402
from zkir_amd import pipeline as pl, runtime as rt, spec, stark  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--calls", type=int, default=200)
ap.add_argument("--k", type=int, default=20)
ap.add_argument("--sha", type=int, default=0)
ap.add_argument("--parent", default="")
ap.add_argument("--rates", default="1,2,3")
ap.add_argument("--sweep", default="1,64,1000,8000", help="cells of the small sections")
ap.add_argument("--sweep-only", action="store_true")
a = ap.parse_args()
med = statistics.median
V, U64, U32 = C.c_void_p, C.c_uint64, C.c_uint32
OLD = C.CDLL(a.parent) if a.parent else rt.lib()
OLD.zkir_verify_on_device.restype = C.c_int; OLD.zkir_verify_on_device.argtypes = [V, U64, V, V]
OLD.zkir_verify_rate_device.restype = C.c_int; OLD.zkir_verify_rate_device.argtypes = [V, U64, V, U32, U32, V]


def device_run(blob, cycles):
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=cycles, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    return log, ddl, tr


def alternate(fns, calls):
    """fns: [(label, callable -> verdict)]; every callable once per round, `calls` rounds; prints median and minimum"""
    ms = [[] for _ in fns]
    for _, f in fns:
        assert f() == 0                                            # (sizes the per-device block and the staging)
    for _ in range(calls):
        for i, (_, f) in enumerate(fns):
            t0 = time.perf_counter(); rc = f(); ms[i].append((time.perf_counter() - t0) * 1e3); assert rc == 0, rc
    for (label, _), m in zip(fns, ms):
        print(f"     {label}: median {med(m):.3f} ms, min {min(m):.3f}, max {max(m):.3f}", flush=True)
    return [med(m) for m in ms], [min(m) for m in ms]


def stages(proof, pub):
    lay = stark.proof_layout(proof)
    n = int(proof[lay["mem_section"]])
    sec = np.ascontiguousarray(proof[lay["mem_section"]:lay["mem_section"] + 1 + 7 * n])
    blob, mode, n_code = lay["blob"], lay["mode"], lay["n_rom"]
    al, lm = [1234567891, 987654321, 5, 77], [3, 2, 1357911, 1 << 30]
    print(f"   the stages on their own, {n} cells ({len(sec)} words; image {max(len(blob) - 32, 0)} bytes):")
    alternate([("cell checks   host", lambda: rt.mem_section_check(sec, mode, n_code, device=False)), ("cell checks   launch (malloc + upload + kernel)", lambda: rt.mem_section_check(sec, mode, n_code, device=True))], a.calls)
    alternate([("table side    host", lambda: 0 * int(rt.mem_table_side(sec, blob, al, lm, device=False)[0])), ("table side    launch (malloc + upload + 2 kernels)", lambda: 0 * int(rt.mem_table_side(sec, blob, al, lm, device=True)[0]))], a.calls)
    for label, f in (("zkir_verify", lambda: rt.verify(proof, pub)), ("zkir_verify_memory_device, queries", lambda: rt.verify(proof, pub, device=True, memory=True, queries=True))):
        clocks = []
        for _ in range(min(a.calls, 50)):
            assert f() == 0
            clocks.append(rt.verify_last_stages())
        print(f"     {label}: host clocks, medians: parse + cell checks {med(c['parse'] for c in clocks):.3f} ms | section digests {med(c['section_digests'] for c in clocks):.3f} | rest (table side among it) {med(c['rest'] for c in clocks):.3f}")
    assert rt.verify(proof, pub, device=True, memory=True, queries=True) == 0
    print(f"     zkir_verify_memory_last: {rt.verify_memory_last()}, device stages {rt.verify_last_stages()['device_stages']}", flush=True)


def measure(label, blob, cycles, mode, rates, hash_witness="host", with_stages=True):
    log, ddl, tr = device_run(blob, cycles)
    log_n = stark.padded_log_n(log.n_rows)
    pub = rt.public_inputs(log, blob, [], mem_mode=mode == 3, wide_mode=mode == 4, mem_witness="device", hash_witness=hash_witness)
    e = C.byref(pub)
    base = stark.StarkContext(log_n)
    proof = stark.prove(base, tr, pub)
    lay = stark.proof_layout(proof)
    print(f"\n{label}: {log.n_rows} rows (log_n {log_n}), mode {mode}, {int(proof[lay['mem_section']])} cells, proof words {len(proof)}", flush=True)
    print("   'ZKIR' proof (blow-up 2):")
    m, lo = alternate([("zkir_verify (host)", lambda: rt.verify(proof, pub)),
                       ("zkir_verify_on_device" + (" (parent)" if a.parent else ""), lambda: OLD.zkir_verify_on_device(proof.ctypes.data, len(proof), e, None)),
                       ("zkir_verify_memory_device, queries = 1", lambda: rt.verify(proof, pub, device=True, memory=True, queries=True)),
                       ("zkir_verify_memory_device, queries = 0", lambda: rt.verify(proof, pub, device=True, memory=True))], a.calls)
    print(f"     new median / parent minimum: {m[2]:.3f} / {lo[1]:.3f} = {m[2] / lo[1]:.3f}")
    if with_stages:
        stages(proof, pub)
    for b in rates:
        ctx = base if b == 1 else stark.StarkContext(log_n, b)
        nq = rt.RATE_DEFAULT_QUERIES[b]
        rp = stark.prove_rate_modes(ctx, tr, pub)
        print(f"   'ZKSR' proof at blow-up {1 << b} ({nq} queries, 12 bits), proof words {len(rp)}:")
        m, lo = alternate([("zkir_verify_rate (host)", lambda: rt.verify_rate(rp, pub, nq, 12)),
                           ("zkir_verify_rate_device" + (" (parent)" if a.parent else ""), lambda: OLD.zkir_verify_rate_device(rp.ctypes.data, len(rp), e, nq, 12, None)),
                           ("zkir_verify_rate_memory_device", lambda: rt.verify_rate(rp, pub, nq, 12, device=True, memory=True))], a.calls)
        print(f"     new median / parent minimum: {m[2]:.3f} / {lo[1]:.3f} = {m[2] / lo[1]:.3f}")
        if ctx is not base:
            ctx.close()
    base.close(); log.close()
    del ddl, tr
    torch.cuda.empty_cache()


def sweep():
    print("\nsmall sections: zkir_verify_memory_device (queries = 1) with the section on the device against its host route (ZKIR_VERIFY_DEVICE_MIN_CELLS = 2^30)")
    for n in [int(x) for x in a.sweep.split(",") if x]:
        blob = spec.memory_loop_program(n).to_bytes()
        log, ddl, tr = device_run(blob, 1 << 24)
        pub = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="device")
        ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
        proof = stark.prove(ctx, tr, pub)
        ctx.close()
        def route(min_cells):
            os.environ["ZKIR_VERIFY_DEVICE_MIN_CELLS"] = str(min_cells)
            return rt.verify(proof, pub, device=True, memory=True, queries=True)
        print(f"   {n} cells ({log.n_rows} rows):")
        alternate([("host route  ", lambda: route(1 << 30)), ("device route", lambda: route(0)), ("zkir_verify (host entry)", lambda: rt.verify(proof, pub))], a.calls)
        os.environ.pop("ZKIR_VERIFY_DEVICE_MIN_CELLS", None)
        log.close()
        del ddl, tr


print(f"device {torch.cuda.get_device_name(0)}; {a.calls} calls per figure, alternating; parent library: {a.parent or '(this build)'}")
rates = [int(x) for x in a.rates.split(",") if x]
n = 1 << a.k
if a.sweep_only:
    sweep()
    sys.exit(0)
measure("array loop (spec.memory_loop_program), witness on the device", spec.memory_loop_program(min(65535, n // 13)).to_bytes(), n, 3, rates)
if a.sha:
    measure("SHA-256 hash chain (spec.sha256_chain_program), witness and tape on the device", spec.sha256_chain_program().to_bytes(), 1 << a.sha, 4, [], hash_witness="device", with_stages=False)
sweep()

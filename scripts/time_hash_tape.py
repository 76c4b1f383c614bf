#!/usr/bin/env python3
"""Mode-4 proof of the SHA-256 hash chain (BASELINE configs[4]'s program) at 2^k cycles: host witness, prove (best of 3, stage split), both costs of the hash tape
(ZKIR_PROVE_TIMES=1 prints the prover's host phases), the host verifier.  --witness host (default): the host's sequential replay, timed on its own, feeds the proof;
--witness device: the public inputs bring no witness and zkir_prove builds the memory witness and the hash tape on the GPU (memcheck.hip) — its time is inside "prove".
--program chain (default) | hello (tests' sha256_hello: one call, the small case; k is ignored) | wide (the signed-division loop: the wide tape, no hash call);
--repeats N (default 3): every repeat's total and lookup stage are printed, so that two builds can be compared with their spread."""
import os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
from zkir_amd import pipeline as pl, runtime as rt, spec, stark
args = sys.argv[1:]
witness = "host"
if "--witness" in args:
    i = args.index("--witness"); witness = args[i + 1]; del args[i:i + 2]
assert witness in ("host", "device"), "--witness host|device"
program, repeats = "chain", 3
if "--program" in args:
    i = args.index("--program"); program = args[i + 1]; del args[i:i + 2]
if "--repeats" in args:
    i = args.index("--repeats"); repeats = int(args[i + 1]); del args[i:i + 2]
assert program in ("chain", "hello", "wide"), "--program chain|hello|wide"
k = int(args[0]) if args else 20
if program == "hello":
    code = [spec.addi(5, 0, 0x2000)] + [w for i, b in enumerate(b"hello") for w in (spec.addi(6, 0, b), spec.encode(spec.Opcode.SB, rs1=5, rs2=6, imm=i))]
    code += [spec.addi(11, 0, 0x2000), spec.addi(12, 0, 5), spec.addi(13, 0, 0x3000), spec.addi(10, 0, 3), spec.ecall(), spec.ebreak()]
    blob = spec.Program.from_code(code).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True))
    k = stark.padded_log_n(int(log.n_rows))
else:
    blob = (spec.sha256_chain_program() if program == "chain" else spec.signed_division_loop_program()).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=1 << k, enable_execution_trace=True))
ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
t0 = time.perf_counter()
pub = rt.public_inputs(log, blob, [], wide_mode=True, mem_witness="host") if witness == "host" else rt.public_inputs(log, blob, [], wide_mode=True, hash_witness="device")
t_wit = (time.perf_counter() - t0) * 1e3
ctx = stark.StarkContext(k)
best, totals, lookups = None, [], []
stark.prove(ctx, tr, pub)                                     # warm-up: code objects, the context's workspace and its pinned staging
for _ in range(repeats):
    t0 = time.perf_counter(); proof, st = stark.prove(ctx, tr, pub, want_stage_ms=True); dt = (time.perf_counter() - t0) * 1e3
    best = dt if best is None else min(best, dt)
    totals.append(dt); lookups.append(st[3])
print(f"{program} 2^{k} ({witness} witness): prove totals ms " + " ".join(f"{x:.2f}" for x in totals) + " | lookup stage ms " + " ".join(f"{x:.2f}" for x in lookups))
t0 = time.perf_counter(); rc = rt.verify(proof, pub); t_ver = (time.perf_counter() - t0) * 1e3
if witness == "device":
    print(f"{program} 2^{k}: {int(proof[stark.proof_layout(proof)['hash_section']])} hash calls, device witness (inside prove; public inputs in {t_wit:.1f} ms), prove {best:.1f} ms (device stages {sum(st):.1f} ms), "
          f"proof {len(proof) * 4 / 1e6:.1f} MB, verify {t_ver:.1f} ms -> {rc}")
    sys.exit(0)
print(f"{program} 2^{k}: {pub._mem_ref.n_hash_calls} hash calls, host witness {t_wit:.1f} ms, prove {best:.1f} ms (device stages {sum(st):.1f} ms), proof {len(proof) * 4 / 1e6:.1f} MB, verify {t_ver:.1f} ms -> {rc}")

#!/usr/bin/env python3
"""Verifier timing on a mode-4 proof: zkir_verify (host) against zkir_verify_device (the tape stages on the GPU), with the stage clocks of zkir_verify_last_stages.
Two steps, so that a verifying process does nothing but verify:
  time_verify.py --make PROOF.npy [--program chain|hello|wide] [K]     prove the program at 2^K cycles (device witness) and save the proof's words
  time_verify.py --proof PROOF.npy --verify host|device [--repeats N]  one warm-up call, then N timed calls (default 3); prints one JSON line
  time_verify.py --digests KIND LEN N [--repeats R]                    zkir_hash_tape_new_bytes_launch against _host on N calls of LEN bytes of kind 3 | 5 | 6
                                                                       (LEN <= 1024: a lane per call; longer: host threads) — what the L_dev decision rests on
The library is the tree's, or the one ZKIR_AMD_LIB names (a build of another commit to time against: its host verifier has no stage clocks, which is reported as null)."""
import json, os, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
args = sys.argv[1:]


def opt(name, default=None):
    if name in args:
        i = args.index(name); v = args[i + 1]; del args[i:i + 2]
        return v
    return default


make, proof_path, which, repeats, program = opt("--make"), opt("--proof"), opt("--verify", "host"), int(opt("--repeats", "3")), opt("--program", "chain")
if "--digests" in args:
    from zkir_amd import runtime as rt
    kind, length, n = (int(x) for x in args[args.index("--digests") + 1:][:3])
    assert kind in (3, 5, 6) and 0 < length <= 1 << 20 and n > 0
    rng = np.random.default_rng(1)
    n_in, stride = (length + 7) // 8, (length + 7) // 8 * 8 + 64     # inputs from 16 MiB up, outputs from 2^39 up: the input's cells come first
    parts = [np.array([n], np.uint32)]
    for j in range(n):
        in_ptr, out_ptr = (1 << 24) + stride * j, (1 << 39) + 64 * j
        rec = np.zeros((n_in + 4, 5), np.uint32); rec[:, 1:] = rng.integers(0, 1 << 16, (n_in + 4, 4))
        parts += [np.array([1 + j, in_ptr & 0xFFFFF, in_ptr >> 20, length, out_ptr & 0xFFFFF, out_ptr >> 20, kind, n_in + 4], np.uint32), rec.reshape(-1)]
    tape = np.concatenate(parts)
    res = {"digests": {"kind": kind, "len": length, "calls": n, "tape_mb": round(tape.nbytes / 1e6, 2)}}
    ref = None
    for name, dev in (("host", False), ("device", True)):
        out = rt.hash_tape_new_bytes(tape, device=dev); ts = []      # warm-up
        for _ in range(repeats):
            t0 = time.perf_counter(); out = rt.hash_tape_new_bytes(tape, device=dev); ts.append(round((time.perf_counter() - t0) * 1e3, 3))
        res[name + "_ms"] = ts
        ref = out if ref is None else ref
        res["equal"] = bool(np.array_equal(ref, out))
    print(json.dumps(res))
    sys.exit(0)
assert which in ("host", "device") and program in ("chain", "hello", "wide") and bool(make) != bool(proof_path), __doc__
if make:
    import torch
    from zkir_amd import pipeline as pl, runtime as rt, spec, stark
    k = int(args[0]) if args else 20
    if program == "hello":
        code = [spec.addi(5, 0, 0x2000)] + [w for i, b in enumerate(b"hello") for w in (spec.addi(6, 0, b), spec.encode(spec.Opcode.SB, rs1=5, rs2=6, imm=i))]
        code += [spec.addi(11, 0, 0x2000), spec.addi(12, 0, 5), spec.addi(13, 0, 0x3000), spec.addi(10, 0, 3), spec.ecall(), spec.ebreak()]
        blob = spec.Program.from_code(code).to_bytes()
        log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True))
    else:
        blob = (spec.sha256_chain_program() if program == "chain" else spec.signed_division_loop_program()).to_bytes()
        log = rt.interpret(blob, [], rt.VMConfig(max_cycles=1 << k, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    ctx = stark.StarkContext(stark.padded_log_n(int(log.n_rows)))
    proof = stark.prove(ctx, tr, rt.public_inputs(log, blob, [], wide_mode=True, hash_witness="device"))
    lay = stark.proof_layout(proof)
    np.save(make, proof)
    print(json.dumps({"made": make, "program": program, "rows": int(log.n_rows), "proof_mb": round(len(proof) * 4 / 1e6, 2), "hash_calls": int(proof[lay["hash_section"]]),
                      "wide_records": int(proof[lay["wide_section"]])}))
    sys.exit(0)
from zkir_amd import runtime as rt
proof = np.ascontiguousarray(np.load(proof_path), dtype=np.uint32)
if which == "device" and not hasattr(rt.lib(), "zkir_verify_device"):
    sys.exit("this library has no zkir_verify_device")
call = (lambda: rt.verify(proof, device=True)) if which == "device" else (lambda: rt.verify(proof))
rc = call()                                                   # warm-up: code objects, the device block and the pinned staging (device); page-ins (host)
times, clocks = [], []
for _ in range(repeats):
    t0 = time.perf_counter(); rc |= call(); times.append((time.perf_counter() - t0) * 1e3)
    clocks.append(rt.verify_last_stages() if hasattr(rt.lib(), "zkir_verify_last_stages") else None)
print(json.dumps({"proof": os.path.basename(proof_path), "lib": os.environ.get("ZKIR_AMD_LIB", "tree"), "verify": which, "rc": int(rc), "ms": [round(t, 2) for t in times],
                  "stages": [None if c is None else {k: (v if k == "device_stages" else round(v, 2)) for k, v in c.items()} for c in clocks]}))

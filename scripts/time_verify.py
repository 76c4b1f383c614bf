#!/usr/bin/env python3
"""Verifier timing on a mode-4 proof: zkir_verify (host) against zkir_verify_device (the tape stages on the GPU), with the stage clocks of zkir_verify_last_stages.
Two steps, so that a verifying process does nothing but verify:
  time_verify.py --make PROOF.npy [--program chain|hello|wide] [K]     prove the program at 2^K cycles (device witness) and save the proof's words
  time_verify.py --proof PROOF.npy --verify host|device [--repeats N]  one warm-up call, then N timed calls (default 3); prints one JSON line
  time_verify.py --digests KIND LEN N [--repeats R]                    zkir_hash_tape_new_bytes_launch against _host on N calls of LEN bytes of kind 3 | 5 | 6
                                                                       (LEN <= 1024: a lane per call; longer: host threads) — what the L_dev decision rests on
  time_verify.py --queries [--cases fib16,fib20,hello,many,segments,mode3,chain20,fib24,chain22] [--calls 200] [--out FILE]
                                                                       the host verifier against the entries with the QUERY STAGE on the device (zkir_verify_on_device,
                                                                       zkir_verify_many_on_device, zkir_verify_chain_on_device), in ONE process: the host entry is the library's
                                                                       that ZKIR_AMD_LIB names (a build of the parent commit; the tree's when unset), the new entries are the
                                                                       tree's, alternating call by call after a warm-up; medians with min and max over --calls calls (9 for the
                                                                       2^22 and 2^24 cases); a second loop under ZKIR_VERIFY_QUERIES_TIMES splits the device entry into host
                                                                       part | upload | kernels | download.  Writes what profiles/r20_verify_queries_device.txt records.
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


if "--queries" in args:
    import ctypes as C
    import torch
    from zkir_amd import pipeline as pl, runtime as rt, spec, stark
    args.remove("--queries")
    cases, calls, out_path = opt("--cases", "fib16,fib20,hello,many,segments").split(","), int(opt("--calls", "200")), opt("--out")
    HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    NEW = C.CDLL(os.path.join(HERE, "zkir_amd", "libzkir_amd.so"))      # the tree's build: the new entries, whatever library serves the host entry
    V, U64 = C.c_void_p, C.c_uint64
    NEW.zkir_verify_on_device.restype = C.c_int; NEW.zkir_verify_on_device.argtypes = [V, U64, V, V]
    NEW.zkir_verify_many_on_device.restype = C.c_int; NEW.zkir_verify_many_on_device.argtypes = [V, V, V, C.c_uint32, V, V]
    NEW.zkir_verify_chain_on_device.restype = C.c_int; NEW.zkir_verify_chain_on_device.argtypes = [V, V, C.c_uint32, V, V]
    NEW.zkir_verify_queries_last.restype = C.c_int; NEW.zkir_verify_queries_last.argtypes = [V, V, V, V]
    NEW.zkir_verify_queries_last_stage_ms.restype = C.c_int; NEW.zkir_verify_queries_last_stage_ms.argtypes = [V]
    NEW.zkir_verify_last_stages.restype = C.c_int; NEW.zkir_verify_last_stages.argtypes = [V, V]
    lines = []

    def say(t):
        print(t, flush=True); lines.append(t)

    def mmm(xs):
        xs = sorted(xs)
        return xs[len(xs) // 2], xs[0], xs[-1]

    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"

    def prove(blob, n, seg=None, **mode):
        """a run of n cycles proven whole, or (seg = rows a segment) in overlapping segments"""
        log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True, **({"max_cycles": n} if n else {})))
        run_pub = rt.public_inputs(log, blob, [], **mode)
        cuts, a = [], 0
        while seg and a < log.n_rows - 1:
            b = min(a + seg, log.n_rows); cuts.append((a, b)); a = b - 1
        proofs = []
        for a, b in (cuts or [(0, log.n_rows)]):
            sh = log.shard(a, b) if cuts else log
            ddl = pl.upload(sh); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
            pub = run_pub
            if cuts:
                pub = rt.PublicInputsC.from_buffer_copy(run_pub); pub.n_real = b - a
            ctx = stark.StarkContext(stark.padded_log_n(b - a))
            proofs.append(np.ascontiguousarray(stark.prove(ctx, tr, pub), dtype=np.uint32))
            ctx.close()
            del tr, ddl
        torch.cuda.empty_cache()
        return proofs

    def arrays(ps):
        return (C.c_void_p * len(ps))(*[p.ctypes.data for p in ps]), (C.c_uint64 * len(ps))(*[len(p) for p in ps])

    def measure(name, host, dev, n_calls):
        for _ in range(3):
            assert host() == 0 and dev() == 0, name
        h, v, l, u = C.c_uint64(0), C.c_uint64(0), C.c_uint32(0), C.c_uint64(0)
        NEW.zkir_verify_queries_last(C.byref(h), C.byref(v), C.byref(l), C.byref(u))
        th, td = [], []
        for _ in range(n_calls):                                     # alternating: a drift of the machine meets both alike
            t0 = time.perf_counter(); rc = host(); th.append((time.perf_counter() - t0) * 1e3); assert rc == 0
            t0 = time.perf_counter(); rc = dev(); td.append((time.perf_counter() - t0) * 1e3); assert rc == 0
        os.environ["ZKIR_VERIFY_QUERIES_TIMES"] = "1"
        parts, ms, clocks = [], (C.c_double * 3)(), (C.c_double * 5)()
        for _ in range(n_calls):
            t0 = time.perf_counter(); rc = dev(); dt = (time.perf_counter() - t0) * 1e3; assert rc == 0
            NEW.zkir_verify_queries_last_stage_ms(ms); NEW.zkir_verify_last_stages(clocks, None)
            parts.append((dt - ms[0] - ms[1] - ms[2], ms[0], ms[1], ms[2], clocks[0], clocks[1] + clocks[2] + clocks[3], clocks[4]))
        del os.environ["ZKIR_VERIFY_QUERIES_TIMES"]
        H, D = mmm(th), mmm(td)
        spread = max(H[2] - H[1], D[2] - D[1])
        say(f"{name:>34s} | {h.value:8d} {u.value:9d} | {f3(H):>27s} | {f3(D):>27s} | {'yes' if H[0] - D[0] > spread else 'NO':>6s} | "
            + " | ".join(f"{f3(mmm([p[i] for p in parts])):>22s}" for i in range(7)))

    say(f"# python scripts/time_verify.py --queries --cases {','.join(cases)} --calls {calls}")
    say(f"# {torch.cuda.get_device_name(0)}; host entry: {os.environ.get('ZKIR_AMD_LIB') or 'the tree build (ZKIR_AMD_LIB unset)'}; new entries: the tree build; alternating call by call after "
        f"3 warm-up pairs; wall ms, median (min .. max).  'faster': the host median exceeds the device median by more than the larger of the two spreads (max - min).")
    say(f"{'case':>34s} | {'hash jobs':>8s} {'uploaded':>9s} | {'host entry ms':>27s} | {'device entry ms':>27s} | faster | device entry, stage synchronising: "
        f"host part | upload | kernels | download | of the host part (last proof of a call): parse | tape stages | rest = transcript, constraints at zeta, table side")
    fib = spec.fib_endless_program().to_bytes()
    single = {"fib16": (fib, 1 << 16, {}), "fib20": (fib, 1 << 20, {}), "fib24": (fib, 1 << 24, {}), "mode3": (spec.memory_loop_program(65535).to_bytes(), 1 << 20, {"mem_mode": True}),
              "chain20": (spec.sha256_chain_program().to_bytes(), 1 << 20, {"wide_mode": True, "hash_witness": "device"}),
              "chain22": (spec.sha256_chain_program().to_bytes(), 1 << 22, {"wide_mode": True, "hash_witness": "device"})}
    for case in cases:
        few = 9 if case in ("fib24", "chain22") else calls
        if case in single or case == "hello":
            if case == "hello":
                code = [spec.addi(5, 0, 0x2000)] + [w for i, b in enumerate(b"hello") for w in (spec.addi(6, 0, b), spec.encode(spec.Opcode.SB, rs1=5, rs2=6, imm=i))]
                code += [spec.addi(11, 0, 0x2000), spec.addi(12, 0, 5), spec.addi(13, 0, 0x3000), spec.addi(10, 0, 3), spec.ecall(), spec.ebreak()]
                p, = prove(spec.Program.from_code(code).to_bytes(), 0, wide_mode=True, hash_witness="device")
            else:
                blob, n, mode = single[case]
                p, = prove(blob, n, **mode)
            measure(f"{case} (mode {int(p[9])}, log_n {int(p[2])}, {len(p)} words)", lambda: rt.verify(p), lambda: NEW.zkir_verify_on_device(p.ctypes.data, len(p), None, None), few)
        elif case == "many":
            ps = [prove(fib, (1 << 16) - 64 + k)[0] for k in range(64)]
            for n in (1, 4, 16, 64):
                ptrs, lens = arrays(ps[:n]); verdicts = (C.c_int32 * n)()
                one_by_one = lambda: max(NEW.zkir_verify_on_device(q.ctypes.data, len(q), None, None) for q in ps[:n])
                many = lambda: NEW.zkir_verify_many_on_device(ptrs, lens, None, n, verdicts, None) or max(verdicts)
                host = lambda: max(rt.verify(q) for q in ps[:n])
                measure(f"many: {n} x fib 2^16, ONE call", host, many, calls)
                measure(f"many: {n} x fib 2^16, one by one", host, one_by_one, calls)
        elif case == "segments":
            ps = prove(fib, 8 * ((1 << 17) - 1) + 1, seg=1 << 17)
            assert len(ps) == 8
            ptrs, lens = arrays(ps)
            measure("chain: 8 segments of 2^17 rows", lambda: rt.verify_chain(ps), lambda: NEW.zkir_verify_chain_on_device(ptrs, lens, 8, None, None), calls)
        else:
            sys.exit(f"no such case: {case}")
    if out_path:
        with open(out_path, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    sys.exit(0)
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

#!/usr/bin/env python3
"""Times of the low-degree proof of a commitment (stark.lowdeg_prove) over a 2^log_n x 152 matrix committed at blow-up 2, 4, 8, with about the same conjectured bits at
every rate (num_queries 50 / 25 / 17, 12 grinding bits): device ms per stage (HIP events inside the library), wall ms, proof words, host verify ms; the combine kernel alone
(HIP events around one launch) as achieved GB/s of its algorithmic bytes, next to zkir_hbm_copy_peak_gbs of the same process and to the DEEP stage of a mode-0 proof at the
same size in the same run.  Writes what profiles/r12_lowdeg.txt records.

    python scripts/time_lowdeg.py [--log-n 20] [--reps 7] [--out FILE]
    python scripts/time_lowdeg.py --trace-pass      # five mode-0 proofs and five low-degree proofs at blow-up 2 in one process: for a profiler's kernel trace, which
                                                    # times deep_kernel and lowdeg_combine_kernel themselves over the same 2^(log_n + 1) rows
"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = 152
QUERIES = {1: 50, 2: 25, 3: 17}
POW_BITS = 12


def _timed(f, reps):
    """HIP events around one call, after three warm-up calls: (median, min, max) in us"""
    import numpy as np, torch
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); e.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(e) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def _mmm(xs):
    import numpy as np
    return float(np.median(xs)), min(xs), max(xs)


def lowdeg_rows(log_n, reps, say):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    rows = []
    for b in (1, 2, 3):
        ctx = stark.StarkContext(log_n, b)
        g = torch.Generator(device="cuda"); g.manual_seed(b)
        mat = stark.lde(ctx, torch.randint(0, stark.P, (W // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
        tree = stark.merkle_commit(ctx, mat, W)
        M = mat.shape[1]
        nq = QUERIES[b]
        stages, walls = [], []
        for it in range(reps + 2):
            t0 = time.perf_counter(); proof, ms = stark.lowdeg_prove(ctx, mat, tree, W, nq, POW_BITS, want_stage_ms=True); dt = (time.perf_counter() - t0) * 1e3
            if it >= 2:
                stages.append(ms); walls.append(dt)
        again = stark.lowdeg_prove(ctx, mat, tree, W, nq, POW_BITS)
        assert np.array_equal(again, proof)
        root = tree[-4:].cpu().numpy().view(np.uint32)
        vs = []
        for _ in range(3):
            t0 = time.perf_counter(); rc = rt.lowdeg_verify(proof, root); vs.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        gamma = [3, 1, 4, 1]
        scratch = torch.empty(32 * (W // 8), dtype=torch.int32, device="cuda"); cw = torch.empty((4, M), dtype=torch.int32, device="cuda")
        ga = (C.c_uint32 * 4)(*gamma)
        def comb():
            assert rt.lib().zkir_lowdeg_combine_launch(ctx.handle, mat.data_ptr(), W, ga, scratch.data_ptr(), cw.data_ptr(), C.c_void_p(torch.cuda.current_stream().cuda_stream)) == 0
        c_us = _timed(comb, 3 * reps)
        bytes_ = M * (32 * (W // 8) + 16)                                # 4 * 8 * ceil(width / 8) B read, 16 B written per row
        row = {"b": b, "M": M, "num_queries": nq, "stage_ms": [_mmm([s[i] for s in stages]) for i in range(4)], "wall_ms": _mmm(walls), "proof_words": int(len(proof)),
               "verify_ms": _mmm(vs), "combine_us": c_us, "combine_bytes": bytes_, "combine_gbs": tuple(bytes_ / (u * 1e-6) / 1e9 for u in c_us)}
        say(f"# b={b}: {row}")
        rows.append(row)
        ctx.close(); del mat, tree, cw
        torch.cuda.empty_cache()
    return rows


def trace_pass(log_n):
    import torch
    from zkir_amd import stark
    ctx = stark.StarkContext(log_n, 1)
    g = torch.Generator(device="cuda"); g.manual_seed(1)
    mat = stark.lde(ctx, torch.randint(0, stark.P, (W // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
    tree = stark.merkle_commit(ctx, mat, W)
    for _ in range(5):
        stark.lowdeg_prove(ctx, mat, tree, W, QUERIES[1], POW_BITS)
    ctx.close()
    return 0


def deep_row(log_n, reps):
    """the DEEP stage (stage 6 of zkir_prove's stage_ms: the host's gamma powers and their upload, then deep_kernel) of a mode-0 proof at 2^log_n rows"""
    import torch
    from zkir_amd import pipeline as pl, runtime as rt, spec, stark
    n = 1 << log_n
    blob = spec.fib_endless_program().to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    ctx = stark.StarkContext(log_n)
    pub = rt.public_inputs(log, blob)
    ms = []
    for it in range(reps + 2):
        out = stark.prove(ctx, tr, pub, want_stage_ms=True)
        if it >= 2:
            ms.append(float(out[1][6]))
    ctx.close(); log.close()
    n2 = 2 * n
    bytes_ = n2 * (32 * ((W + stark.W_AUX) // 8) + 16 + 2 * 16 + 16)     # the two matrices' blocks, the quotient's four words, 1 / (zeta - x) twice, 16 B written
    return {"stage_ms": _mmm(ms), "bytes": bytes_, "gbs": tuple(bytes_ / (m * 1e-3) / 1e9 for m in _mmm(ms))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    ap.add_argument("--trace-pass", action="store_true")
    args = ap.parse_args()
    if args.trace_pass:
        QUERIES.pop(2); QUERIES.pop(3)
        deep_row(args.log_n, 3)
        return trace_pass(args.log_n)
    import torch
    from zkir_amd import runtime as rt
    lines = []
    def say(s):
        print(s, flush=True); lines.append(s)
    lib = rt.lib()
    lib.zkir_hbm_copy_peak_gbs.restype = C.c_double; lib.zkir_hbm_copy_peak_gbs.argtypes = [C.c_uint64, C.c_void_p]
    sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    copy = [float(lib.zkir_hbm_copy_peak_gbs(1 << 30, sp())) for _ in range(5)]
    say(f"# {torch.cuda.get_device_name(0)}; 2^{args.log_n} x {W}; pow_bits {POW_BITS}; {args.reps} proofs a rate after 2 warm-up ones; every figure: median (min .. max)")
    say(f"zkir_hbm_copy_peak_gbs (1 GiB, 5 runs): {max(copy):.0f} GB/s best ({min(copy):.0f} .. {max(copy):.0f})")
    rows = lowdeg_rows(args.log_n, args.reps, lambda s: None)
    f3 = lambda t, u="": f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f}){u}"
    say(f"{'b':>2s} {'queries':>7s} | {'combine ms':>24s} | {'FRI commit ms':>24s} | {'grinding ms':>24s} | {'queries ms':>24s} | {'wall ms':>24s} | {'words':>7s} | {'verify ms':>22s}")
    for r in rows:
        s = r["stage_ms"]
        say(f"{r['b']:2d} {r['num_queries']:7d} | {f3(s[0]):>24s} | {f3(s[1]):>24s} | {f3(s[2]):>24s} | {f3(s[3]):>24s} | {f3(r['wall_ms']):>24s} | {r['proof_words']:7d} | {f3(r['verify_ms']):>22s}")
    say("lowdeg_combine_kernel alone (HIP events around one launch; algorithmic bytes = M (32 ceil(width / 8) + 16)):")
    for r in rows:
        u, gb = r["combine_us"], r["combine_gbs"]
        say(f"  b={r['b']} M=2^{r['M'].bit_length() - 1}: {u[0]:.1f} us ({u[1]:.1f} .. {u[2]:.1f}) for {r['combine_bytes'] / 1e9:.3f} GB = {gb[0]:.0f} GB/s ({gb[2]:.0f} .. {gb[1]:.0f}); "
            f"{100 * gb[0] / max(copy):.0f} % of the copy peak; run-to-run spread {100 * (u[2] - u[1]) / u[0]:.1f} % of the median")
    d = deep_row(args.log_n, args.reps)
    say(f"DEEP stage of a mode-0 proof at 2^{args.log_n} (zkir_prove stage_ms[6]: the host's gamma powers and their upload with the GPU idle, then deep_kernel; M = 2^{args.log_n + 1}): "
        f"{f3(d['stage_ms'], ' ms')} for {d['bytes'] / 1e9:.3f} GB = {d['gbs'][0]:.0f} GB/s ({d['gbs'][2]:.0f} .. {d['gbs'][1]:.0f}) — a LOWER bound on deep_kernel's own rate: the stage holds host time")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

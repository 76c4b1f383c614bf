#!/usr/bin/env python3
"""Times of the evaluation proof of a commitment (stark.eval_prove) over a 2^log_n x 152 matrix committed at blow-up 2, 4, 8, for one and two points (num_queries
50 / 25 / 17, 12 grinding bits): device ms per stage (HIP events inside the library), wall ms, proof words, host verify ms.  Two comparisons: the quotient kernel's launch
(inverse table + eval_quotient_kernel) and the inverse table alone against lowdeg_combine_kernel on the same matrix, in matrix bytes read per second; the evaluations stage
against the openings stage of a mode-0 zkir_prove proof at the same row count (bary_weights + bary_dot + bary_sum at blow-up 2).  Writes what profiles/r13_eval.txt records.

    python scripts/time_eval.py [--log-n 20] [--reps 7] [--out FILE]
"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.time_lowdeg import POW_BITS, QUERIES, W, _mmm, _timed      # noqa: E402

POINTS = [[5, 7, 11, 13], [2013265920, 3, 1, 4]]


def eval_rows(log_n, reps):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    rows = []
    for b in (1, 2, 3):
        ctx = stark.StarkContext(log_n, b)
        g = torch.Generator(device="cuda"); g.manual_seed(b)
        mat = stark.lde(ctx, torch.randint(0, stark.P, (W // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
        tree = stark.merkle_commit(ctx, mat, W)
        M, nq = mat.shape[1], QUERIES[b]
        root = tree[-4:].cpu().numpy().view(np.uint32)
        sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        gamma = (C.c_uint32 * 4)(3, 1, 4, 1)
        scratch = torch.empty(32 * (W // 8), dtype=torch.int32, device="cuda"); cw = torch.empty((4, M), dtype=torch.int32, device="cuda")
        comb = _timed(lambda: rt.lib().zkir_lowdeg_combine_launch(ctx.handle, mat.data_ptr(), W, gamma, scratch.data_ptr(), cw.data_ptr(), sp()), 3 * reps)
        for n_points in (1, 2):
            pts = np.array(POINTS[:n_points], np.uint32)
            stages, walls = [], []
            for it in range(reps + 2):
                t0 = time.perf_counter(); proof, ms = stark.eval_prove(ctx, mat, tree, W, pts, nq, POW_BITS, want_stage_ms=True); dt = (time.perf_counter() - t0) * 1e3
                if it >= 2:
                    stages.append(ms); walls.append(dt)
            assert np.array_equal(stark.eval_prove(ctx, mat, tree, W, pts, nq, POW_BITS), proof)
            vs = []
            for _ in range(3):
                t0 = time.perf_counter(); rc = rt.eval_verify(proof, root, pts); vs.append((time.perf_counter() - t0) * 1e3)
                assert rc == 0
            at = stark.eval_layout(proof)
            ys = proof[at["evals"]:at["layer_roots"]].copy()
            qs = torch.empty(int(rt.lib().zkir_eval_quotient_scratch_words(log_n + b, W, n_points)), dtype=torch.int32, device="cuda")
            def quot():
                assert rt.lib().zkir_eval_quotient_launch(ctx.handle, mat.data_ptr(), W, gamma, pts.ctypes.data, n_points, ys.ctypes.data, qs.data_ptr(), cw.data_ptr(), sp()) == 0
            q_us = _timed(quot, 3 * reps)
            rows.append({"b": b, "M": M, "n_points": n_points, "num_queries": nq, "stage_ms": [_mmm([s[i] for s in stages]) for i in range(6)], "wall_ms": _mmm(walls),
                         "proof_words": int(len(proof)), "verify_ms": _mmm(vs), "quotient_launch_us": q_us, "combine_us": comb, "matrix_bytes": M * 32 * (W // 8)})
            del qs
        ctx.close(); del mat, tree, cw
        torch.cuda.empty_cache()
    return rows


def openings_row(log_n, reps):
    """the openings stage (stage 5 of zkir_prove's stage_ms: bary_weights_kernel, bary_dot_kernel over main + aux + quotient, bary_sum_kernel, the download) of a mode-0 proof"""
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
            ms.append(float(out[1][5]))
    ctx.close(); log.close()
    return {"stage_ms": _mmm(ms), "columns": W + stark.W_AUX + 4}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    from zkir_amd import runtime as rt
    lines = []
    def say(s):
        print(s, flush=True); lines.append(s)
    lib = rt.lib()
    lib.zkir_hbm_copy_peak_gbs.restype = C.c_double; lib.zkir_hbm_copy_peak_gbs.argtypes = [C.c_uint64, C.c_void_p]
    copy = [float(lib.zkir_hbm_copy_peak_gbs(1 << 30, C.c_void_p(torch.cuda.current_stream().cuda_stream))) for _ in range(5)]
    say(f"# {torch.cuda.get_device_name(0)}; 2^{args.log_n} x {W}; pow_bits {POW_BITS}; {args.reps} proofs a case after 2 warm-up ones; every figure: median (min .. max)")
    say(f"zkir_hbm_copy_peak_gbs (1 GiB, 5 runs): {max(copy):.0f} GB/s best ({min(copy):.0f} .. {max(copy):.0f})")
    rows = eval_rows(args.log_n, args.reps)
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    names = ["weights", "evaluations", "quotient", "FRI commit", "grinding", "queries"]
    say(f"{'b':>2s} {'pts':>3s} {'q':>3s} | " + " | ".join(f"{n + ' ms':>22s}" for n in names) + f" | {'wall ms':>22s} | {'words':>7s} | {'verify ms':>22s}")
    for r in rows:
        say(f"{r['b']:2d} {r['n_points']:3d} {r['num_queries']:3d} | " + " | ".join(f"{f3(s):>22s}" for s in r["stage_ms"]) + f" | {f3(r['wall_ms']):>22s} | {r['proof_words']:7d} | {f3(r['verify_ms']):>22s}")
    say("quotient against combine on the same matrix (HIP events around one launch; bytes = the matrix's M * 32 * ceil(width / 8) read by both):")
    say("  zkir_eval_quotient_launch = eval_weights_kernel (the inverse table, n_points * M inversions: the proof's 'weights' stage) + eval_quotient_kernel; the kernel's own time is")
    say("  taken as the launch minus the weights stage (the proof's 'quotient' stage holds the host's transcript up to gamma with the GPU idle, so it is not the kernel's time)")
    for r in rows:
        gb = lambda us: r["matrix_bytes"] / (us * 1e-6) / 1e9
        qk = r["quotient_launch_us"][0] - r["stage_ms"][0][0] * 1e3
        say(f"  b={r['b']} points={r['n_points']}: lowdeg_combine_kernel {r['combine_us'][0]:.1f} us = {gb(r['combine_us'][0]):.0f} GB/s | table + quotient launch {r['quotient_launch_us'][0]:.1f} us, "
            f"eval_quotient_kernel {qk:.1f} us = {gb(qk):.0f} GB/s of matrix bytes, {qk / r['combine_us'][0]:.2f} x the combine's time")
    o = openings_row(args.log_n, args.reps)
    say(f"openings stage of a mode-0 zkir_prove proof at 2^{args.log_n} rows, blow-up 2 ({o['columns']} columns, two points, its own weights kernel and download inside): {f3(o['stage_ms'])} ms "
        f"= {o['stage_ms'][0] * 1e3 / o['columns']:.2f} us a column")
    for r in rows:
        if r["n_points"] == 2:
            e, w_ = r["stage_ms"][1][0], r["stage_ms"][0][0]
            say(f"  eval_prove b={r['b']} two points: evaluations {e:.3f} ms = {e * 1e3 / W:.2f} us a column; weights + evaluations {e + w_:.3f} ms = {(e + w_) * 1e3 / W:.2f} us a column")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

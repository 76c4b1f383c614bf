#!/usr/bin/env python3
"""Times of the batched evaluation proof (stark.batch_eval_prove) of three matrices of 2^log_n rows — 152 columns opened at both points, 40 at both, 8 at the first point only:
a trace, an auxiliary matrix and a quotient — committed at blow-up 2, 4, 8 (num_queries 50 / 25 / 17, 12 grinding bits): device ms per stage (HIP events inside the library),
wall ms, proof words, host verify ms.  Two comparisons in the same process: the batch proof against the three separate stark.eval_prove calls on the same matrices (sum of
device ms, sum of words), and batch_quotient_kernel over the three matrices (25 blocks) against eval_quotient_kernel on a single 200-column matrix (25 blocks), in matrix
bytes read per second.  Writes what profiles/r14_batch_eval.txt records.

    python scripts/time_batch_eval.py [--log-n 20] [--reps 7] [--out FILE]
"""
import argparse, ctypes as C, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.time_lowdeg import POW_BITS, QUERIES, _mmm, _timed      # noqa: E402
from scripts.time_eval import POINTS                                 # noqa: E402

WIDTHS, MASKS = [152, 40, 8], [3, 3, 1]
SINGLE = 200                                                         # one matrix of as many B8 blocks as the three together
NAMES = ["weights", "evaluations", "quotient", "FRI commit", "grinding", "queries"]


def _proofs(f, reps):
    """(proof, per-stage (median, min, max) ms, total device ms (median, min, max), wall ms (median, min, max)) of reps calls of f after two warm-up ones"""
    stages, walls = [], []
    for it in range(reps + 2):
        t0 = time.perf_counter(); proof, ms = f(); dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            stages.append(ms); walls.append(dt)
    return proof, [_mmm([s[i] for s in stages]) for i in range(6)], _mmm([sum(s) for s in stages]), _mmm(walls), stages


def rows_for(log_n, reps):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    pts = np.array(POINTS, np.uint32)
    rows = []
    for b in (1, 2, 3):
        ctx = stark.StarkContext(log_n, b)
        g = torch.Generator(device="cuda"); g.manual_seed(10 + b)
        def committed(width):
            mat = stark.lde(ctx, torch.randint(0, stark.P, ((width + 7) // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
            return mat, stark.merkle_commit(ctx, mat, width)
        pairs = [committed(w) for w in WIDTHS]
        mats, trees = [p[0] for p in pairs], [p[1] for p in pairs]
        M, nq = mats[0].shape[1], QUERIES[b]
        roots = np.concatenate([t[-4:].cpu().numpy().view(np.uint32) for t in trees])
        # ---- the batch proof ----
        proof, st, dev, wall, _ = _proofs(lambda: stark.batch_eval_prove(ctx, mats, trees, WIDTHS, MASKS, pts, nq, POW_BITS, want_stage_ms=True), reps)
        assert np.array_equal(stark.batch_eval_prove(ctx, mats, trees, WIDTHS, MASKS, pts, nq, POW_BITS), proof)
        vs = []
        for _ in range(3):
            t0 = time.perf_counter(); rc = rt.batch_eval_verify(proof, roots, pts); vs.append((time.perf_counter() - t0) * 1e3)
            assert rc == 0
        # ---- the three separate proofs on the same matrices: each at the points its mask selects ----
        sep, sep_words, sep_verify = [], 0, 0.0
        for m in range(3):
            p_m = pts[[i for i in range(2) if (MASKS[m] >> i) & 1]]
            pr_m, st_m, dev_m, wall_m, raw = _proofs(lambda: stark.eval_prove(ctx, mats[m], trees[m], WIDTHS[m], p_m, nq, POW_BITS, want_stage_ms=True), reps)
            t0 = time.perf_counter(); assert rt.eval_verify(pr_m, roots[4 * m:4 * m + 4], p_m) == 0; sep_verify += (time.perf_counter() - t0) * 1e3
            sep.append({"stage_ms": st_m, "device_ms": dev_m, "wall_ms": wall_m, "raw": raw}); sep_words += len(pr_m)
            # the batch's evaluations are the separate proofs'
            at, lay = stark.eval_layout(pr_m), stark.batch_eval_layout(proof)
            for li, i in enumerate([i for i in range(2) if (MASKS[m] >> i) & 1]):
                assert np.array_equal(pr_m[at["evals"] + 4 * li * WIDTHS[m]:at["evals"] + 4 * (li + 1) * WIDTHS[m]], proof[lay["evals_of"][(i, m)]:lay["evals_of"][(i, m)] + 4 * WIDTHS[m]])
        sum_raw = [sum(sum(s["raw"][k]) for s in sep) for k in range(reps)]
        # ---- the quotient kernels alone: the three matrices in one pass against one matrix of as many blocks ----
        sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
        lay = stark.batch_eval_layout(proof)
        ys = proof[lay["evals"]:lay["layer_roots"]].copy()
        gamma = np.array([3, 1, 4, 1], np.uint32)
        cw = torch.empty((4, M), dtype=torch.int32, device="cuda")
        ws, ks = np.array(WIDTHS, np.uint32), np.array(MASKS, np.uint32)
        ptrs = (C.c_void_p * 3)(*[m.data_ptr() for m in mats])
        qs = torch.empty(int(rt.lib().zkir_batch_eval_quotient_scratch_words(log_n + b, 3, ws.ctypes.data, 2)), dtype=torch.int32, device="cuda")
        def bq():
            assert rt.lib().zkir_batch_eval_quotient_launch(ctx.handle, 3, ptrs, ws.ctypes.data, ks.ctypes.data, gamma.ctypes.data, pts.ctypes.data, 2, ys.ctypes.data, qs.data_ptr(), cw.data_ptr(), sp()) == 0
        bq_us = _timed(bq, 3 * reps)
        del qs
        single = stark.lde(ctx, torch.randint(0, stark.P, (SINGLE // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
        ys1 = np.random.default_rng(b).integers(0, stark.P, (2, SINGLE, 4), dtype=np.uint32)
        qs = torch.empty(int(rt.lib().zkir_eval_quotient_scratch_words(log_n + b, SINGLE, 2)), dtype=torch.int32, device="cuda")
        def eq():
            assert rt.lib().zkir_eval_quotient_launch(ctx.handle, single.data_ptr(), SINGLE, gamma.ctypes.data, pts.ctypes.data, 2, ys1.ctypes.data, qs.data_ptr(), cw.data_ptr(), sp()) == 0
        eq_us = _timed(eq, 3 * reps)
        rows.append({"b": b, "M": M, "num_queries": nq, "stage_ms": st, "device_ms": dev, "wall_ms": wall, "proof_words": int(len(proof)), "verify_ms": _mmm(vs), "separate": sep,
                     "separate_device_ms": _mmm(sum_raw), "separate_words": int(sep_words), "separate_verify_ms": sep_verify, "batch_quotient_us": bq_us, "eval_quotient_us": eq_us,
                     "matrix_bytes": M * 32 * sum((w + 7) // 8 for w in WIDTHS)})
        ctx.close(); del mats, trees, pairs, single, cw, qs
        torch.cuda.empty_cache()
    return rows


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
    say(f"# {torch.cuda.get_device_name(0)}; 2^{args.log_n} rows; matrices {WIDTHS} columns, masks {MASKS} (bit i: opened at point i), two points; pow_bits {POW_BITS}; "
        f"{args.reps} proofs a case after 2 warm-up ones; every figure: median (min .. max)")
    say(f"zkir_hbm_copy_peak_gbs (1 GiB, 5 runs): {max(copy):.0f} GB/s best ({min(copy):.0f} .. {max(copy):.0f})")
    rows = rows_for(args.log_n, args.reps)
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    say("batch proof (stark.batch_eval_prove), device ms per stage:")
    say(f"{'b':>2s} {'q':>3s} | " + " | ".join(f"{n + ' ms':>22s}" for n in NAMES) + f" | {'device ms':>22s} | {'wall ms':>22s} | {'words':>7s} | {'verify ms':>22s}")
    for r in rows:
        say(f"{r['b']:2d} {r['num_queries']:3d} | " + " | ".join(f"{f3(s):>22s}" for s in r["stage_ms"]) + f" | {f3(r['device_ms']):>22s} | {f3(r['wall_ms']):>22s} | {r['proof_words']:7d} | {f3(r['verify_ms']):>22s}")
    say("the three separate proofs (stark.eval_prove on the same matrices in the same process: 152 columns at two points, 40 at two, 8 at one), device ms per stage, medians:")
    for r in rows:
        for m, s in enumerate(r["separate"]):
            say(f"{r['b']:2d} {r['num_queries']:3d} | width {WIDTHS[m]:3d} | " + " | ".join(f"{s['stage_ms'][i][0]:8.3f}" for i in range(6)) + f" | device {f3(s['device_ms'])} | wall {f3(s['wall_ms'])}")
    say("batch against the sum of the three (device ms: the sum of the six stages of a proof; sum of the three: repetition k of each added up, then median (min .. max)):")
    for r in rows:
        d, s = r["device_ms"], r["separate_device_ms"]
        say(f"  b={r['b']}: batch {f3(d)} ms, three proofs {f3(s)} ms: {d[0] / s[0]:.2f} x | words {r['proof_words']} against {r['separate_words']}: {r['proof_words'] / r['separate_words']:.2f} x | "
            f"host verify {r['verify_ms'][0]:.1f} ms against {r['separate_verify_ms']:.1f} ms")
        per = [sum(x["stage_ms"][i][0] for x in r["separate"]) for i in range(6)]
        say("        per stage, batch / sum of three medians: " + ", ".join(f"{NAMES[i]} {r['stage_ms'][i][0]:.3f} / {per[i]:.3f}" for i in range(6)))
    say("quotient kernels alone (HIP events around one launch of the test entry: the synchronous upload of the gamma table, eval_weights_kernel for the inverse table of two")
    say("  points, the quotient kernel; the kernel's own time is taken as the launch minus the batch proof's 'weights' stage, the same kernel on the same points; bytes = the")
    say(f"  M * 32 * 25 matrix bytes both read: {WIDTHS} in three matrices for batch_quotient_kernel, one matrix of {SINGLE} columns for eval_quotient_kernel):")
    for r in rows:
        gb = lambda us: r["matrix_bytes"] / (us * 1e-6) / 1e9
        w_us = r["stage_ms"][0][0] * 1e3
        bk, ek = [x - w_us for x in r["batch_quotient_us"]], [x - w_us for x in r["eval_quotient_us"]]
        say(f"  b={r['b']}: batch launch {r['batch_quotient_us'][0]:.1f} us ({r['batch_quotient_us'][1]:.1f} .. {r['batch_quotient_us'][2]:.1f}), kernel {bk[0]:.1f} us = {gb(bk[0]):.0f} GB/s "
            f"({gb(bk[2]):.0f} .. {gb(bk[1]):.0f}) | single launch {r['eval_quotient_us'][0]:.1f} us ({r['eval_quotient_us'][1]:.1f} .. {r['eval_quotient_us'][2]:.1f}), kernel {ek[0]:.1f} us = "
            f"{gb(ek[0]):.0f} GB/s ({gb(ek[2]):.0f} .. {gb(ek[1]):.0f}) | batch / single kernel time {bk[0] / ek[0]:.2f}")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

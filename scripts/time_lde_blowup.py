#!/usr/bin/env python3
"""HIP-event timing of the commitment at blow-up 2, 4 and 8 (StarkContext(log_n, log_blowup = 1, 2, 3)) on a random 152-column matrix: the LDE stage, the leaf
hash, and the step (LDE + Merkle tree), with the algorithmic-byte and per-output-word figures of profiles/r10_lde_blowup.txt.

    python scripts/time_lde_blowup.py [--log-n 20] [--blowups 1,2,3] [--reps 20] [--json]
    python scripts/time_lde_blowup.py --compare OTHER_LIB.so [--rounds 3]     # blow-up 2 only: this build against another one (ZKIR_AMD_LIB), alternated, a fresh process each

Per-kernel times come from a profiler's kernel trace over the first form, one blow-up per run (the strided kernels have the same names at every rate).
Algorithmic bytes per element of the N x W input: the middle kernel reads 4 and writes 4 * 2^b; every strided pass moves 8 per word it covers
(N words on the inverse side, N * 2^b on the forward side); the leaf hash reads 4 * 2^b.
"""
import argparse, ctypes as C, json, os, subprocess, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = 152


def passes(stages):
    """kernels run_strided_stages picks for `stages` radix-2 stages (ntt.hip)"""
    n = 0
    while stages > 0:
        take = 10 if stages >= 10 and stages != 11 else {11: 8, 9: 6, 7: 4, 5: 3}.get(stages, stages)
        stages -= take; n += 1
    return n


def measure(log_n, blowups, reps):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    n = 1 << log_n
    lib = rt.lib(); sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
    src = torch.from_numpy(np.random.default_rng(log_n).integers(0, stark.P, (W // 8, n, 8), dtype=np.uint32).view(np.int32)).cuda()
    out = []
    for b in blowups:
        m_rows = n << b
        ctx = stark.StarkContext(log_n, b)
        m = src.clone(); L = torch.empty((W // 8, m_rows, 8), dtype=torch.int32, device="cuda"); tree = torch.empty(4 * (2 * m_rows - 1), dtype=torch.int32, device="cuda")
        def lde():
            m.copy_(src)                                               # the extension clobbers its input; the copy stays outside the timed region
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); rc = lib.zkir_lde_launch(ctx.handle, m.data_ptr(), W, L.data_ptr(), sp()); e.record()
            assert rc == 0
            return a, e
        def leaves():
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); rc = lib.zkir_merkle_leaves_launch(ctx.handle, L.data_ptr(), W, m_rows, tree.data_ptr(), sp()); e.record()
            assert rc == 0
            return a, e
        def step():
            m.copy_(src)
            a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(); rc = lib.zkir_lde_launch(ctx.handle, m.data_ptr(), W, L.data_ptr(), sp()) or lib.zkir_merkle_commit_launch(ctx.handle, L.data_ptr(), W, m_rows, tree.data_ptr(), sp()); e.record()
            assert rc == 0
            return a, e
        row = {"log_n": log_n, "log_blowup": b}
        for name, f in [("lde", lde), ("leaves", leaves), ("step", step)]:
            for _ in range(3):
                f()
            torch.cuda.synchronize()
            ts = []
            for _ in range(reps):
                a, e = f(); torch.cuda.synchronize(); ts.append(a.elapsed_time(e))
            row[name] = {"median_ms": float(np.median(ts)), "min_ms": min(ts), "max_ms": max(ts)}
        words_out = W * m_rows
        strided = passes(max(log_n - 10, 0))
        lde_bytes = W * n * (4 + (4 << b)) + 8 * W * n * strided + 8 * words_out * strided if log_n >= 10 else W * n * (4 + (4 << b))
        row["lde_algorithmic_gb"] = lde_bytes / 1e9
        row["lde_gbs"] = lde_bytes / 1e9 / (row["lde"]["median_ms"] * 1e-3)
        row["lde_ns_per_output_word"] = row["lde"]["median_ms"] * 1e6 / words_out
        row["leaves_ns_per_output_word"] = row["leaves"]["median_ms"] * 1e6 / words_out
        row["step_ns_per_output_word"] = row["step"]["median_ms"] * 1e6 / words_out
        out.append(row)
        ctx.close(); del m, L, tree
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--blowups", default="1,2,3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--json", action="store_true")
    ap.add_argument("--compare", metavar="LIB", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    args = ap.parse_args()
    if args.compare:
        import numpy as np
        res = {"other": [], "this": []}
        for _ in range(args.rounds):                                   # alternated, each in a fresh process (a library is loaded once per process)
            for who in ("other", "this"):
                env = dict(os.environ)
                env.pop("ZKIR_AMD_LIB", None)
                if who == "other":
                    env["ZKIR_AMD_LIB"] = os.path.abspath(args.compare)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--log-n", str(args.log_n), "--blowups", "1", "--reps", str(args.reps), "--json"], env=env, capture_output=True, text=True,
                                   timeout=120)                        # every GPU step under its own limit; a failed child ends the comparison with its own words
                if r.returncode != 0:
                    sys.stderr.write(r.stderr)
                    sys.exit(f"{who}: the timing child ended with status {r.returncode}")
                res[who].append(json.loads(r.stdout.strip().split("\n")[-1])[0])
        for stage in ("lde", "step"):
            for who in ("other", "this"):
                med = [r[stage]["median_ms"] for r in res[who]]
                print(f"{stage:5s} {who:5s} medians of {args.rounds} runs x {args.reps} reps: {' '.join(f'{x:.4f}' for x in med)} ms   median {np.median(med):.4f}  spread {max(med) - min(med):.4f}")
            a, t = [np.median([r[stage]["median_ms"] for r in res[w]]) for w in ("other", "this")]
            sp = max(max(x) - min(x) for x in ([r[stage]["median_ms"] for r in res[w]] for w in ("other", "this")))
            print(f"{stage:5s} this - other = {t - a:+.4f} ms; larger spread {sp:.4f} ms: {'inside' if abs(t - a) <= sp else 'OUTSIDE'}")
        return 0
    rows = measure(args.log_n, [int(x) for x in args.blowups.split(",")], args.reps)
    if args.json:
        print(json.dumps(rows))
        return 0
    print(f"# 2^{args.log_n} x {W}, {args.reps} reps, HIP events; ms = median (min .. max)")
    print(f"{'b':>2s} {'lde ms':>24s} {'alg GB':>7s} {'GB/s':>7s} {'ns/word':>8s} | {'leaf hash ms':>24s} {'ns/word':>8s} | {'step ms':>24s} {'ns/word':>8s}")
    for r in rows:
        f = lambda k: f"{r[k]['median_ms']:8.3f} ({r[k]['min_ms']:.3f} .. {r[k]['max_ms']:.3f})"
        print(f"{r['log_blowup']:2d} {f('lde'):>24s} {r['lde_algorithmic_gb']:7.3f} {r['lde_gbs']:7.0f} {r['lde_ns_per_output_word']:8.4f} | {f('leaves'):>24s} {r['leaves_ns_per_output_word']:8.4f} | {f('step'):>24s} {r['step_ns_per_output_word']:8.4f}")
    return 0


if __name__ == "__main__":
    sys.exit(main())

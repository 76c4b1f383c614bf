#!/usr/bin/env python3
"""HIP-event timing of zkir_merkle_open_launch and zkir_merkle_verify_launch (both verifier forms and the library's rule) over a committed 2^20 x 152 matrix at blow-up 2
and 8 (n_leaves 2^21 and 2^23) for n_idx = 50 .. 65536; zkir_merkle_verify_host on the same records; and, with --compare, bench.py's step and
stark.prove (mode 0, 2^20) of this build against another build of the library, alternated, a fresh process each.  Writes what profiles/r11_merkle_open.txt records.

    python scripts/time_merkle_open.py [--log-n 20] [--blowups 1,3] [--reps 20] [--host-cap 4096]
    python scripts/time_merkle_open.py --compare OTHER_LIB.so [--rounds 3]
    python scripts/time_merkle_open.py --once N_IDX --form lane|row16|rule      # one open + one verify launch: for a profiler's kernel trace
"""
import argparse, ctypes as C, json, os, subprocess, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
W = 152
N_IDX = [50, 300, 1024, 4096, 8192, 12288, 16384, 65536]                  # the sizes asked for, and three between the last two of them: where the forms cross


def _timed(f, reps):
    import numpy as np, torch
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); f(); e.record(); torch.cuda.synchronize(); ts.append(a.elapsed_time(e) * 1e3)
    return float(np.median(ts)), min(ts), max(ts)


def _setup(log_n, b):
    import numpy as np, torch
    from zkir_amd import stark
    n = (1 << log_n) << b
    ctx = stark.StarkContext(min(log_n, 20), 1)                          # any context serves: the calls use nothing that depends on its size or rate
    g = torch.Generator(device="cuda"); g.manual_seed(b)
    mat = torch.randint(0, stark.P, (W // 8, n, 8), dtype=torch.int32, device="cuda", generator=g)
    tree = stark.merkle_commit(ctx, mat, W)
    return ctx, n, mat, tree


def measure(log_n, blowups, reps, host_cap):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    lib = rt.lib()
    rows = []
    for b in blowups:
        ctx, n, mat, tree = _setup(log_n, b)
        words = stark.opening_words(W, n)
        for n_idx in N_IDX:
            idx = torch.from_numpy(np.random.default_rng(n_idx).integers(0, n, n_idx).astype(np.int64)).cuda()
            out = torch.empty((n_idx, words), dtype=torch.int32, device="cuda")
            v = torch.empty(n_idx, dtype=torch.int32, device="cuda"); s = torch.empty(2, dtype=torch.int32, device="cuda")
            sp = lambda: C.c_void_p(torch.cuda.current_stream().cuda_stream)
            def op():
                assert lib.zkir_merkle_open_launch(ctx.handle, mat.data_ptr(), W, n, tree.data_ptr(), idx.data_ptr(), n_idx, out.data_ptr(), sp()) == 0
            def ver(flags):
                def f():
                    assert lib.zkir_merkle_verify_launch(ctx.handle, tree[-4:].data_ptr(), W, n, idx.data_ptr(), n_idx, out.data_ptr(), flags, v.data_ptr(), s.data_ptr(), sp()) == 0
                return f
            row = {"log_blowup": b, "n_leaves": n, "n_idx": n_idx, "open_us": _timed(op, reps)}
            for name, flags in [("lane", stark.VERIFY_FORM_LANE), ("row16", stark.VERIFY_FORM_ROW16), ("rule", 0)]:
                row[name + "_us"] = _timed(ver(flags), reps)
                assert not v.cpu().numpy().any() and [int(x) for x in s.cpu()] == [0, -1], (name, n_idx)
            k = min(n_idx, host_cap)                                     # the host verifier: one thread, ~40 permutations a record
            h_idx, h_rec, root = idx[:k].cpu().numpy().view(np.uint64), out[:k].cpu().numpy().view(np.uint32), tree[-4:].cpu().numpy().view(np.uint32)
            t0 = time.perf_counter(); hv, hs = rt.merkle_verify_host(root, W, n, h_idx, h_rec); dt = time.perf_counter() - t0
            assert not hv.any()
            row["host_records"], row["host_ms"] = k, dt * 1e3
            rows.append(row)
        ctx.close(); del mat, tree
    return rows


def once(log_n, b, n_idx, form):
    import numpy as np, torch
    from zkir_amd import stark
    ctx, n, mat, tree = _setup(log_n, b)
    idx = np.random.default_rng(n_idx).integers(0, n, n_idx).astype(np.uint64)
    flags = {"lane": stark.VERIFY_FORM_LANE, "row16": stark.VERIFY_FORM_ROW16, "rule": 0}[form]
    for _ in range(3):
        rec = stark.merkle_open(ctx, mat, tree, idx, W)
        v, s = stark.merkle_verify(ctx, tree[-4:], W, n, idx, rec, flags)
    torch.cuda.synchronize()
    assert not v.cpu().numpy().any()
    ctx.close()


def parent_side(log_n, reps):
    """bench.py's step and a mode-0 proof at 2^log_n with whichever library ZKIR_AMD_LIB names: one JSON line"""
    import numpy as np, torch
    from zkir_amd import pipeline as pl, runtime as rt, spec, stark
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "100", "--warmup", "10"], capture_output=True, text=True, timeout=300)
    if r.returncode != 0:
        sys.stderr.write(r.stderr); sys.exit(f"bench.py ended with status {r.returncode}")
    bench = json.loads(r.stdout.strip().split("\n")[-1])
    n = 1 << log_n
    blob = spec.fib_endless_program().to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(max_cycles=n, enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr)); torch.cuda.synchronize()
    ctx = stark.StarkContext(log_n)
    pub = rt.public_inputs(log, blob)
    ts = []
    for it in range(reps + 2):
        t0 = time.perf_counter(); proof = stark.prove(ctx, tr, pub); dt = (time.perf_counter() - t0) * 1e3
        if it >= 2:
            ts.append(dt)
    t0 = time.perf_counter(); assert rt.verify(proof) == 0; verify_ms = (time.perf_counter() - t0) * 1e3
    stages = rt.verify_last_stages() if hasattr(rt.lib(), "zkir_verify_last_stages") else {}
    print(json.dumps({"bench_ms_per_step": bench.get("ms_per_step"), "bench_stage_ms": bench.get("stage_ms"), "prove_ms_median": float(np.median(ts)), "prove_ms_min": min(ts),
                      "verify_ms": verify_ms, "verify_stages": stages, "proof_words": int(len(proof))}, default=str))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--blowups", default="1,3")
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--host-cap", type=int, default=4096)
    ap.add_argument("--compare", metavar="LIB", default=None)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--once", type=int, default=0)
    ap.add_argument("--form", default="rule")
    ap.add_argument("--parent-side", action="store_true", help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.parent_side:
        return parent_side(args.log_n, 5)
    if args.once:
        return once(args.log_n, int(args.blowups.split(",")[0]), args.once, args.form)
    if args.compare:
        import numpy as np
        res = {"other": [], "this": []}
        for _ in range(args.rounds):                                     # alternated, each in a fresh process (a library is loaded once per process)
            for who in ("other", "this"):
                env = dict(os.environ)
                env.pop("ZKIR_AMD_LIB", None)
                if who == "other":
                    env["ZKIR_AMD_LIB"] = os.path.abspath(args.compare)
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--parent-side", "--log-n", str(args.log_n)], env=env, capture_output=True, text=True, timeout=420)
                if r.returncode != 0:                                    # every GPU step under its own limit; a failed child ends the comparison with its own words
                    sys.stderr.write(r.stderr)
                    sys.exit(f"{who}: the timing child ended with status {r.returncode}")
                res[who].append(json.loads(r.stdout.strip().split("\n")[-1]))
                print(f"# {who}: {r.stdout.strip().splitlines()[-1]}", flush=True)
        for key in ("bench_ms_per_step", "prove_ms_median"):
            for who in ("other", "this"):
                x = [r[key] for r in res[who]]
                print(f"{key:18s} {who:5s} {' '.join(f'{v:.4f}' for v in x)} ms   median {np.median(x):.4f}  spread {max(x) - min(x):.4f}")
            a, t = [np.median([r[key] for r in res[w]]) for w in ("other", "this")]
            sp = max(max(x) - min(x) for x in ([r[key] for r in res[w]] for w in ("other", "this")))
            print(f"{key:18s} this - other = {t - a:+.4f} ms; larger spread {sp:.4f} ms: {'inside' if abs(t - a) <= sp else 'OUTSIDE'}")
        return 0
    rows = measure(args.log_n, [int(x) for x in args.blowups.split(",")], args.reps, args.host_cap)
    print(f"# 2^{args.log_n} x {W} committed at blow-up 2^b; {args.reps} reps, HIP events around one launch; us = median (min .. max); host = zkir_merkle_verify_host, one thread")
    print(f"{'b':>2s} {'n_leaves':>9s} {'n_idx':>6s} | {'open us':>26s} | {'verify lane us':>30s} | {'verify row16 us':>30s} | {'verify rule us':>30s} | {'host ms (records)':>20s}")
    for r in rows:
        f = lambda k: f"{r[k][0]:9.1f} ({r[k][1]:.1f} .. {r[k][2]:.1f})"
        print(f"{r['log_blowup']:2d} {r['n_leaves']:9d} {r['n_idx']:6d} | {f('open_us'):>26s} | {f('lane_us'):>30s} | {f('row16_us'):>30s} | {f('rule_us'):>30s} | {r['host_ms']:10.1f} ({r['host_records']})")
    return 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python3
"""Host against device verification of the commitment layer's three proofs, in one process, on the proofs of time_lowdeg.py, time_eval.py and time_batch_eval.py: a matrix of
2^log_n rows x 152 columns ('ZKLD'; 'ZKEV' at two points) and the three-matrix batch 152 / 40 / 8 ('ZKBE'), committed at blow-up 2, 4, 8 (num_queries 50 / 25 / 17, 12
grinding bits).  The host entry and the device entry ALTERNATE, call by call, after a warm-up; every figure is a median (min .. max) of wall ms over --calls calls each.
A second loop with ZKIR_PCS_VERIFY_TIMES set (the stage then synchronises after its upload and after its kernels) splits the device entry into host part | upload | kernels |
download.  Writes what profiles/r16_pcs_verify_device.txt records.

    python scripts/time_pcs_verify.py [--log-n 20] [--calls 200] [--out FILE]

--mixed times the FOURTH proof the same way and nothing else: the mixed-height proof ('ZKMH') of time_mixed_eval.py — 2^20 x 152 and 2^16 x 40 at two points each, 2^12 x 8
at one — with zkir_mixed_eval_verify against zkir_mixed_eval_verify_device.  Writes what profiles/r19_mixed_verify_device.txt records.

    python scripts/time_pcs_verify.py --mixed [--log-ns 20,16,12] [--calls 200] [--out FILE]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.time_lowdeg import POW_BITS, QUERIES, _mmm            # noqa: E402
from scripts.time_eval import POINTS                                 # noqa: E402
from scripts.time_batch_eval import WIDTHS, MASKS                    # noqa: E402

W = 152


def proofs_for(log_n, b):
    """[(name, host call, device call, proof words, hash jobs)] on matrices committed on a context of its own"""
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    ctx = stark.StarkContext(log_n, b)
    g = torch.Generator(device="cuda"); g.manual_seed(20 + b)
    def committed(width):
        mat = stark.lde(ctx, torch.randint(0, stark.P, ((width + 7) // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
        return mat, stark.merkle_commit(ctx, mat, width)
    pairs = [committed(w) for w in WIDTHS]
    mats, trees = [p[0] for p in pairs], [p[1] for p in pairs]
    roots = np.concatenate([t[-4:].cpu().numpy().view(np.uint32) for t in trees])
    pts, nq = np.array(POINTS, np.uint32), QUERIES[b]
    ld = stark.lowdeg_prove(ctx, mats[0], trees[0], W, nq, POW_BITS)
    ev = stark.eval_prove(ctx, mats[0], trees[0], W, pts, nq, POW_BITS)
    be = stark.batch_eval_prove(ctx, mats, trees, WIDTHS, MASKS, pts, nq, POW_BITS)
    ctx.close(); del mats, trees, pairs
    torch.cuda.empty_cache()
    return [("lowdeg", lambda d: rt.lowdeg_verify(ld, roots[:4], device=d), len(ld)),
            ("eval", lambda d: rt.eval_verify(ev, roots[:4], pts, device=d), len(ev)),
            ("batch_eval", lambda d: rt.batch_eval_verify(be, roots, pts, device=d), len(be))]


def mixed_proof_for(log_ns, b):
    """[(name, call, proof words)] of the mixed-height proof of time_mixed_eval.py's groups, each committed on a context of its own"""
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    from scripts.time_mixed_eval import WIDTHS as MW, MASKS as MM, N_POINTS as MP
    g = torch.Generator(device="cuda"); g.manual_seed(20 + b)
    rng = np.random.default_rng(30 + b)
    groups = []
    for log_n, width, mask, n_points in zip(log_ns, MW, MM, MP):
        ctx = stark.StarkContext(log_n, b)
        mat = stark.lde(ctx, torch.randint(0, stark.P, ((width + 7) // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
        groups.append(stark.EvalGroup(ctx, [mat], [stark.merkle_commit(ctx, mat, width)], [width], [mask], rng.integers(1, stark.P, (n_points, 4), dtype=np.uint32)))
    pr = stark.mixed_eval_prove(groups, QUERIES[b], POW_BITS)
    lay = stark.mixed_eval_layout(pr)
    roots, pts = pr[lay["roots"]:lay["points"]].copy(), np.concatenate([gr.points.reshape(-1) for gr in groups]).astype(np.uint32)
    for gr in groups:
        gr.ctx.close()
    del groups
    torch.cuda.empty_cache()
    return [("mixed_eval", lambda d: rt.mixed_eval_verify(pr, roots, pts, device=d), len(pr))]


def measure(call, calls):
    from zkir_amd import runtime as rt
    for _ in range(10):
        assert call(False) == 0 and call(True) == 0
    jobs = rt.pcs_verify_last_jobs()
    host, dev = [], []
    for _ in range(calls):                                          # alternating: a drift of the machine meets both alike
        t0 = time.perf_counter(); rc = call(False); host.append((time.perf_counter() - t0) * 1e3); assert rc == 0
        t0 = time.perf_counter(); rc = call(True); dev.append((time.perf_counter() - t0) * 1e3); assert rc == 0
    os.environ["ZKIR_PCS_VERIFY_TIMES"] = "1"
    parts = []
    for _ in range(calls):
        t0 = time.perf_counter(); rc = call(True); dt = (time.perf_counter() - t0) * 1e3; assert rc == 0
        up, kern, down = rt.pcs_verify_last_stage_ms()
        parts.append((dt - up - kern - down, up, kern, down))
    del os.environ["ZKIR_PCS_VERIFY_TIMES"]
    return _mmm(host), _mmm(dev), [_mmm([p[i] for p in parts]) for i in range(4)], jobs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-n", type=int, default=20)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=None)
    ap.add_argument("--mixed", action="store_true", help="time the mixed-height proof ('ZKMH') and nothing else")
    ap.add_argument("--log-ns", default="20,16,12", help="--mixed: the three heights")
    args = ap.parse_args()
    log_ns = [int(x) for x in args.log_ns.split(",")]
    import torch
    lines = []
    def say(s):
        print(s, flush=True); lines.append(s)
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    if args.mixed:
        from scripts.time_mixed_eval import WIDTHS as MW, MASKS as MM, N_POINTS as MP
        say(f"# python scripts/time_pcs_verify.py --mixed --log-ns {args.log_ns} --calls {args.calls}")
        say(f"# {torch.cuda.get_device_name(0)}; mixed_eval: groups of 2^{log_ns} rows x {MW} columns, masks {MM}, {MP} points; pow_bits {POW_BITS}; "
            f"host and device entries alternating, {args.calls} calls each after 10 warm-up pairs; wall ms, median (min .. max)")
    else:
        say(f"# {torch.cuda.get_device_name(0)}; 2^{args.log_n} rows; lowdeg / eval: {W} columns (eval at two points); batch_eval: {WIDTHS} columns, masks {MASKS}; pow_bits {POW_BITS}; "
            f"host and device entries alternating, {args.calls} calls each after 10 warm-up pairs; wall ms, median (min .. max)")
    say(f"{'proof':>10s} {'b':>2s} {'q':>3s} {'words':>7s} {'hash jobs':>9s} | {'host entry ms':>24s} | {'device entry ms':>24s} | device median < host min | "
        f"device entry split (stage synchronising): {'host part':>22s} | {'upload':>22s} | {'kernels':>22s} | {'download':>22s}")
    for b in (1, 2, 3):
        for name, call, words in (mixed_proof_for(log_ns, b) if args.mixed else proofs_for(args.log_n, b)):
            host, dev, parts, jobs = measure(call, args.calls)
            say(f"{name:>10s} {b:2d} {QUERIES[b]:3d} {words:7d} {jobs[0]:9d} | {f3(host):>24s} | {f3(dev):>24s} | {'yes' if dev[0] < host[1] else 'NO':>23s} | "
                + " " * 43 + " | ".join(f"{f3(p):>22s}" for p in parts))
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

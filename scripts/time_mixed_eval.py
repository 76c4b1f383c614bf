#!/usr/bin/env python3
"""Times of the evaluation proof over several heights (stark.mixed_eval_prove): a main trace of 2^20 x 152 (mask 3, two points), a chip of 2^16 x 40 (mask 3, two points of its
own) and a table of 2^12 x 8 (mask 1, one point), committed at blow-up 2, 4, 8 (num_queries 50 / 25 / 17, 12 grinding bits), against the three separate
stark.batch_eval_prove proofs of the same matrices at their own heights.  Same process, the four proofs ALTERNATING repetition by repetition (mixed, then the three separate
ones), medians and spread: device ms per stage (HIP events inside the library), their sum, wall ms; proof words from the words functions (exact).  The FRI commit phase is named
separately: the lower groups' own commit phases are what the mixed proof removes.  Writes what profiles/r18_mixed_eval.txt records.

    python scripts/time_mixed_eval.py [--log-ns 20,16,12] [--reps 7] [--out FILE]
"""
import argparse, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from scripts.time_lowdeg import POW_BITS, QUERIES, _mmm      # noqa: E402

WIDTHS, MASKS, N_POINTS = [152, 40, 8], [3, 3, 1], [2, 2, 1]
NAMES = ["weights", "evaluations", "quotient", "FRI commit", "grinding", "queries"]


def rows_for(log_ns, reps):
    import numpy as np, torch
    from zkir_amd import runtime as rt, stark
    rows = []
    for b in (1, 2, 3):
        g = torch.Generator(device="cuda"); g.manual_seed(20 + b)
        rng = np.random.default_rng(30 + b)
        groups = []
        for log_n, width, mask, n_points in zip(log_ns, WIDTHS, MASKS, N_POINTS):
            ctx = stark.StarkContext(log_n, b)
            mat = stark.lde(ctx, torch.randint(0, stark.P, ((width + 7) // 8, 1 << log_n, 8), dtype=torch.int32, device="cuda", generator=g), clobber=True)
            groups.append(stark.EvalGroup(ctx, [mat], [stark.merkle_commit(ctx, mat, width)], [width], [mask], rng.integers(1, stark.P, (n_points, 4), dtype=np.uint32)))
        nq = QUERIES[b]
        calls = [lambda: stark.mixed_eval_prove(groups, nq, POW_BITS, want_stage_ms=True)] + \
                [lambda gr=gr: stark.batch_eval_prove(gr.ctx, gr.mats, gr.trees, gr.widths, gr.masks, gr.points, nq, POW_BITS, want_stage_ms=True) for gr in groups]
        stages, walls, proofs = [[] for _ in calls], [[] for _ in calls], [None] * len(calls)
        for it in range(reps + 2):                                   # two warm-up rounds; within a round the four proofs follow each other
            for k, f in enumerate(calls):
                torch.cuda.synchronize()
                t0 = time.perf_counter(); proofs[k], ms = f(); dt = (time.perf_counter() - t0) * 1e3
                if it >= 2:
                    stages[k].append(ms); walls[k].append(dt)
        assert rt.mixed_eval_verify(proofs[0]) == 0 and all(rt.batch_eval_verify(p) == 0 for p in proofs[1:])
        lay = stark.mixed_eval_layout(proofs[0])                     # the mixed proof's evaluations are the separate proofs'
        for gl, p in zip(lay["groups"], proofs[1:]):
            at = stark.batch_eval_layout(p)
            assert np.array_equal(proofs[0][gl["evals"]:gl["evals"] + 4 * gl["n_evals"]], p[at["evals"]:at["layer_roots"]])
        shapes = [([w], [k], n) for w, k, n in zip(WIDTHS, MASKS, N_POINTS)]
        words = rt.mixed_eval_proof_words(log_ns, b, shapes, nq)
        sep_words = [rt.batch_eval_proof_words(log_n, b, *shape, nq) for log_n, shape in zip(log_ns, shapes)]
        assert words == len(proofs[0]) and sep_words == [len(p) for p in proofs[1:]]
        rows.append({"b": b, "num_queries": nq, "words": words, "separate_words": sep_words,
                     "stage_ms": [[_mmm([s[i] for s in st]) for i in range(6)] for st in stages], "device_ms": [_mmm([sum(s) for s in st]) for st in stages],
                     "wall_ms": [_mmm(w) for w in walls],
                     "separate_device_ms": _mmm([sum(sum(stages[k][r]) for k in (1, 2, 3)) for r in range(reps)]),
                     "separate_wall_ms": _mmm([sum(walls[k][r] for k in (1, 2, 3)) for r in range(reps)]),
                     "separate_fri_ms": _mmm([sum(stages[k][r][3] for k in (1, 2, 3)) for r in range(reps)])})
        for gr in groups:
            gr.ctx.close()
        del groups, calls
        torch.cuda.empty_cache()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--log-ns", default="20,16,12")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    log_ns = [int(x) for x in args.log_ns.split(",")]
    assert len(log_ns) == 3
    lines = []
    def say(s):
        print(s, flush=True); lines.append(s)
    say(f"# {torch.cuda.get_device_name(0)}; groups of 2^{log_ns} rows x {WIDTHS} columns, masks {MASKS}, {N_POINTS} points; pow_bits {POW_BITS}; {args.reps} rounds after 2 warm-up ones,")
    say("# a round = the mixed proof, then the three separate batch_eval_prove proofs, in this order; every figure: median (min .. max)")
    rows = rows_for(log_ns, args.reps)
    f3 = lambda t: f"{t[0]:.3f} ({t[1]:.3f} .. {t[2]:.3f})"
    who = ["mixed"] + [f"2^{n} alone" for n in log_ns]
    say(f"{'b':>2s} {'q':>3s} {'proof':>11s} | " + " | ".join(f"{n + ' ms':>22s}" for n in NAMES) + f" | {'device ms':>22s} | {'wall ms':>22s} | {'words':>7s}")
    for r in rows:
        for k in range(4):
            say(f"{r['b']:2d} {r['num_queries']:3d} {who[k]:>11s} | " + " | ".join(f"{f3(s):>22s}" for s in r["stage_ms"][k]) + f" | {f3(r['device_ms'][k]):>22s} | {f3(r['wall_ms'][k]):>22s} | "
                f"{(r['words'] if k == 0 else r['separate_words'][k - 1]):7d}")
    say("mixed against the sum of the three (round k of each added up, then median (min .. max)):")
    for r in rows:
        d, s, w, sw = r["device_ms"][0], r["separate_device_ms"], r["wall_ms"][0], r["separate_wall_ms"]
        fri, sfri = r["stage_ms"][0][3], r["separate_fri_ms"]
        say(f"  b={r['b']}: device {f3(d)} against {f3(s)} ms: {d[0] / s[0]:.2f} x | wall {f3(w)} against {f3(sw)} ms: {w[0] / sw[0]:.2f} x | FRI commit phase {f3(fri)} against {f3(sfri)} ms: "
            f"{fri[0] / sfri[0]:.2f} x | words {r['words']} against {sum(r['separate_words'])} = {' + '.join(str(x) for x in r['separate_words'])}: {r['words'] / sum(r['separate_words']):.3f} x")
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(lines) + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())

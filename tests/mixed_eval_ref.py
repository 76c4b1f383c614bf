"""Reference prover and verifier of the EVALUATION PROOF OVER SEVERAL HEIGHTS (zkir_mixed_eval_prove / zkir_mixed_eval_verify), for the mixed-eval tests.  Nothing here imports
the product: batch_eval_ref (shape, evaluations, quotient), eval_ref (e_inv, points_ok), lowdeg_ref (field, fold, trees, paths, challenger), oracle.stark_api and numpy.

Statement: n_groups (2 or 3) groups at one rate b, of strictly decreasing heights log_n_0 > log_n_1 > .. (each >= 3, log_n_0 + b <= 27).  Group h is what a 'ZKBE' proof states
at its own height: 1 .. 4 matrices over 31 <w_{M_h}>, M_h = N_h << b, each under its own root, widths summing to at most 512, its own 1 or 2 points, a mask per matrix.
ONE gamma, drawn after the header and all roots, points and evaluations.  Its exponent runs consecutively through the groups in order and inside a group in 'ZKBE''s order;
F_h is batch_eval_ref.quotient of group h with those exponents (= gamma^(the group's first exponent) times the quotient with exponents from 0).
FRI: layer 0 is F_0.  The schedule is lowdeg_ref's with one more cap — whenever some log M_h < log_m the step is at most log_m - max{log M_h < log_m} — so every M_h is the
size of a committed layer and ks[0] stays 1.  When a fold leaves a layer of size M_h, F_h is added to it BY INDEX before the layer is hashed: L[i] = fold[i] + F_h[i].

Proof words (all canonical):
    [0..7)   MAGIC 'ZKMH', VERSION, b, n_groups, num_queries, pow_bits, n_layers
    then     per group: log_n, n_mats, n_points, (width, mask) per matrix | all roots (groups in order, matrices in order) | all points | all evaluations in the exponent
             order | n_layers x 4 layer roots | n_fin x 4 final layer | the nonce | the queries
    query:   q, group 0's matrices record_m(q), record_m(q + M_0/2), each lower group's matrices ONE record_m(q mod M_h) (width_m + 4 log M_h words), per layer values and path
Transcript: every word up to and including the evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log M_0 - 1).

Codes of verify_ref, first failing check in this order, lowest query first: 1 malformed (exact length, magic, version, ranges, group order, a group's shape, n_layers), 2 not
the expected roots, 13 not the expected points / evaluations, 3 a word >= p, 12 a point in the base field or two equal points within a group, 4 final layer not of degree < 4,
5 grinding, 6 a query's index word, 7 a record (in the order they stand in the query), 8 layer-0 values != F_0 at the two rows, 9 a FRI leaf's path, 10 carried value !=
v[slot] — before the step into the layer of size M_h the carried value becomes carried + F_h(q mod M_h), recomputed from group h's records — 11 final value."""
from __future__ import annotations

import numpy as np

import batch_eval_ref as be
import eval_ref as ev
import lowdeg_ref as ld
from oracle import stark_api as so

P, GEN, U64 = ld.P, ld.GEN, ld.U64
MAGIC, VERSION = 0x484D4B5A, 1
HEAD = 7
MIN_GROUPS, MAX_GROUPS = 2, 3


def schedule(log_ns, b: int):
    log_ms = [int(x) + b for x in log_ns]
    ks, log_m = [], log_ms[0]
    while log_m > 2 + b:
        k = 1 if not ks else min(ld.LOG_ARITY, log_m - (2 + b))
        lower = [x for x in log_ms[1:] if x < log_m]
        if lower:
            k = min(k, log_m - max(lower))
        ks.append(k)
        log_m -= k
    return ks


def params_ok(log_ns, b, shapes, num_queries) -> bool:
    """shapes[h] = (widths, masks, n_points) of group h"""
    log_ns = [int(x) for x in log_ns]
    if not MIN_GROUPS <= len(log_ns) <= MAX_GROUPS or len(shapes) != len(log_ns) or not 1 <= b <= 3 or not 1 <= num_queries <= ld.MAX_QUERIES:
        return False
    if any(not 3 <= x <= 26 or x + b > 27 for x in log_ns) or any(x >= y for x, y in zip(log_ns[1:], log_ns)):
        return False
    return all(be.shape_ok([int(x) for x in w], [int(x) for x in k], n) for w, k, n in shapes)


def query_words(log_ns, b: int, shapes) -> int:
    q, lm = 1, log_ns[0] + b
    for h, (widths, _, _) in enumerate(shapes):
        q += (1 if h else 2) * sum(w + 4 * (log_ns[h] + b) for w in widths)
    for k in schedule(log_ns, b):
        q += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    return q


def proof_words(log_ns, b: int, shapes, num_queries: int) -> int:
    if not params_ok(log_ns, b, shapes, num_queries):
        return 0
    n_mats, n_points = sum(len(w) for w, _, _ in shapes), sum(n for _, _, n in shapes)
    n_evals = sum(be.selected(list(w), list(k), n)[1] for w, k, n in shapes)
    return HEAD + sum(3 + 2 * len(w) for w, _, _ in shapes) + 4 * n_mats + 4 * n_points + 4 * n_evals + 4 * len(schedule(log_ns, b)) + 4 * (4 << b) + 1 + \
        num_queries * query_words(log_ns, b, shapes)


def e_pow_from(first, gamma, n: int) -> np.ndarray:
    """first, first gamma, .. first gamma^(n-1) (so.emul: the oracle's product)"""
    out = np.zeros((n, 4), U64)
    cur = np.asarray(first, np.uint32)
    for k in range(n):
        out[k] = cur
        cur = so.emul(cur, np.asarray(gamma, np.uint32))
    return out


def evaluate(groups, b: int) -> np.ndarray:
    """all evaluations uint64[n_evals][4] in the exponent order: batch_eval_ref's, group after group.  groups[h] = (mats, masks, points)"""
    return np.concatenate([be.evaluate(mats, b, masks, pts) for mats, masks, pts in groups])


def prove_ref(groups, b: int, num_queries: int, pow_bits: int, evals=None, low_q=None, quotient_evals=None, final_add=None) -> np.ndarray:
    """The proof for groups[h] = (mats, masks, points): mats[m] uint32[width_m][M_h] extended matrices, points [n_points_h][4] canonical.  A cheating prover for the tests:
    `evals` ([n_evals][4], all groups in the exponent order) takes the place of the evaluations; everything after follows the honest procedure.  Two more cheats:
    quotient_evals — the codewords F_h are built from THESE evaluations while `evals` are stated (a prover that keeps the low-degree codewords of the true values under a
    false statement) — low_q(q, M_h) in the place of q mod M_h as the row a lower group's records open — and final_add (an E4 value, four words) added to every value of the
    final layer before it is observed: still of degree < 4, and not what the last committed layer folds to."""
    groups = [([np.ascontiguousarray(c, dtype=np.uint32) for c in mats], [int(k) for k in masks], np.asarray(pts, np.uint32).reshape(-1, 4)) for mats, masks, pts in groups]
    Ms = [mats[0].shape[1] for mats, _, _ in groups]
    log_ns = [M.bit_length() - 1 - b for M in Ms]
    shapes = [([len(c) for c in mats], masks, len(pts)) for mats, masks, pts in groups]
    assert all(c.shape[1] == M for (mats, _, _), M in zip(groups, Ms) for c in mats) and params_ok(log_ns, b, shapes, num_queries)
    assert 0 <= pow_bits <= ld.MAX_POW and all(ev.points_ok(pts) for _, _, pts in groups)
    ks = schedule(log_ns, b)
    committed = [[so.merkle(c, want_layers=True) for c in mats] for mats, _, _ in groups]
    counts = [be.selected(w, k, n)[1] for w, k, n in shapes]
    y = (evaluate(groups, b) if evals is None else np.asarray(evals, U64).reshape(-1, 4)).astype(np.uint32)
    assert len(y) == sum(counts)
    head = [MAGIC, VERSION, b, len(groups), num_queries, pow_bits, len(ks)]
    for log_n, (widths, masks, n_points) in zip(log_ns, shapes):
        head += [log_n, len(widths), n_points] + [x for wk in zip(widths, masks) for x in wk]
    out = [np.array(head, np.uint32)] + [r for trees in committed for r, _ in trees] + [pts.reshape(-1) for _, _, pts in groups] + [y.reshape(-1)]
    ch = ld.Challenger()
    ch.observe_n(np.concatenate(out))
    gamma = ch.sample_ext()
    yq = y if quotient_evals is None else np.asarray(quotient_evals, U64).reshape(-1, 4)
    F, first, e0 = [], np.array([1, 0, 0, 0], np.uint32), 0
    for (mats, masks, pts), n in zip(groups, counts):                # F_h with the exponents e0 .. e0 + n - 1: gamma^e0 times the quotient with exponents from 0
        F.append(ld.e_mul(be.quotient(mats, masks, pts, yq[e0:e0 + n], gamma), first.astype(U64)))
        for _ in range(n):
            first = so.emul(first, gamma)
        e0 += n
    layers, trees, roots = [F[0]], [], []
    shift, log_m = GEN, log_ns[0] + b
    for j, k in enumerate(ks):
        r, t = ld.layer_tree(layers[j], k)
        roots.append(r); trees.append(t)
        ch.observe_n(r)
        nxt, shift = ld.fold(layers[j], k, shift, log_m, ch.sample_ext())
        log_m -= k
        for h in range(1, len(groups)):
            if Ms[h] == 1 << log_m:
                nxt = ld.e_add(nxt, F[h])                            # by index, before the layer is hashed
        layers.append(nxt)
    if final_add is not None:
        layers[-1] = ld.e_add(layers[-1], np.asarray(final_add, U64).reshape(1, 4))
    fin = layers[-1]
    assert len(fin) == 4 << b and all(any(len(L) == M for L in layers[1:-1]) for M in Ms[1:])
    ch.observe_n(fin)
    nonce = ch.grind(pow_bits)
    assert ch.check_pow(nonce, pow_bits)
    out += roots + [fin.astype(np.uint32).reshape(-1), np.array([nonce], np.uint32)]
    for _ in range(num_queries):
        q = ch.sample_bits(log_ns[0] + b - 1)
        out.append(np.array([q], np.uint32))
        for h, ((mats, _, _), trees_h) in enumerate(zip(groups, committed)):
            rows = (q, q + Ms[0] // 2) if h == 0 else ((q % Ms[h] if low_q is None else low_q(q, Ms[h])),)
            for cols, (_, tree) in zip(mats, trees_h):
                for pos in rows:
                    out += [cols[:, pos], ld.tree_path(tree, Ms[h], pos)]
        log_m = log_ns[0] + b
        for j, k in enumerate(ks):
            g = (1 << log_m) >> k
            idx = q & (g - 1)
            out += [layers[j][idx + t * g].astype(np.uint32) for t in range(1 << k)] + [ld.tree_path(trees[j], g, idx)]
            log_m -= k
    proof = np.concatenate(out).astype(np.uint32)
    assert len(proof) == proof_words(log_ns, b, shapes, num_queries)
    return proof


def layout(proof) -> dict:
    """Word offsets of a well-formed proof: groups (per group: log_n, log_M, widths, masks, n_points, shape = where its three words stand, roots, points, evals, n_evals,
    evals_of {(i, m): offset}, records [m] = offsets relative to a query's start (two for group 0, one below), recs [m] = words a record), roots, points, evals, layer_roots,
    final, nonce, queries, qsize, ks, n_fin; layers (relative): (values, path, depth)"""
    b, n_groups, nq = int(proof[2]), int(proof[3]), int(proof[4])
    groups, at_w = [], HEAD
    for _ in range(n_groups):
        log_n, n_mats, n_points = (int(x) for x in proof[at_w:at_w + 3])
        widths = [int(x) for x in proof[at_w + 3:at_w + 3 + 2 * n_mats:2]]
        masks = [int(x) for x in proof[at_w + 4:at_w + 3 + 2 * n_mats:2]]
        groups.append({"log_n": log_n, "log_M": log_n + b, "widths": widths, "masks": masks, "n_points": n_points, "shape": at_w})
        at_w += 3 + 2 * n_mats
    log_ns = [g["log_n"] for g in groups]
    ks = schedule(log_ns, b)
    at = {"b": b, "n_groups": n_groups, "num_queries": nq, "ks": ks, "n_fin": 4 << b, "groups": groups, "log_ns": log_ns, "roots": at_w}
    at["points"] = at["roots"] + 4 * sum(len(g["widths"]) for g in groups)
    at["evals"] = at["points"] + 4 * sum(g["n_points"] for g in groups)
    r_at, p_at, e, rel = at["roots"], at["points"], 0, 1
    for h, g in enumerate(groups):
        sel, n = be.selected(g["widths"], g["masks"], g["n_points"])
        g["roots"], g["points"], g["evals"], g["n_evals"], g["first_e"] = r_at, p_at, at["evals"] + 4 * e, n, e
        g["evals_of"] = {(i, m): at["evals"] + 4 * (e + e1) for i, m, e1 in sel}
        g["recs"] = [w + 4 * g["log_M"] for w in g["widths"]]
        g["records"] = []
        for rec in g["recs"]:
            g["records"].append((rel, rel + rec) if h == 0 else (rel,))
            rel += (2 if h == 0 else 1) * rec
        r_at += 4 * len(g["widths"]); p_at += 4 * g["n_points"]; e += n
    at["n_evals"] = e
    at["layer_roots"] = at["evals"] + 4 * e
    at["final"] = at["layer_roots"] + 4 * len(ks)
    at["nonce"] = at["final"] + 4 * at["n_fin"]
    at["queries"] = at["nonce"] + 1
    lm, lay = log_ns[0] + b, []
    for k in ks:
        lay.append((rel, rel + 4 * (1 << k), lm - k))
        rel += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    at["layers"], at["qsize"] = lay, rel
    return at


def _parse(w):
    """(b, nq, pow_bits, n_layers, log_ns, shapes) of a header a proof can have, else None"""
    if len(w) < HEAD or int(w[0]) != MAGIC or int(w[1]) != VERSION:
        return None
    b, n_groups, nq, pow_bits, n_layers = (int(x) for x in w[2:7])
    if not 1 <= b <= 3 or not MIN_GROUPS <= n_groups <= MAX_GROUPS or not 1 <= nq <= ld.MAX_QUERIES or pow_bits > ld.MAX_POW:
        return None
    log_ns, shapes, at_w = [], [], HEAD
    for _ in range(n_groups):
        if len(w) < at_w + 3:
            return None
        log_n, n_mats, n_points = (int(x) for x in w[at_w:at_w + 3])
        if not 1 <= n_mats <= be.MAX_MATS or len(w) < at_w + 3 + 2 * n_mats:
            return None
        log_ns.append(log_n)
        shapes.append(([int(x) for x in w[at_w + 3:at_w + 3 + 2 * n_mats:2]], [int(x) for x in w[at_w + 4:at_w + 3 + 2 * n_mats:2]], n_points))
        at_w += 3 + 2 * n_mats
    if not params_ok(log_ns, b, shapes, nq) or n_layers != len(schedule(log_ns, b)) or len(w) != proof_words(log_ns, b, shapes, nq):
        return None
    return b, nq, pow_bits, n_layers, log_ns, shapes


def verify_ref(proof, roots=None, points=None, evals=None) -> int:
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    parsed = _parse(w)
    if parsed is None:
        return 1
    b, nq, pow_bits, n_layers, log_ns, shapes = parsed
    at = layout(w)
    ks, G = at["ks"], at["groups"]
    w_roots, w_pts, w_y = w[at["roots"]:at["points"]], w[at["points"]:at["evals"]], w[at["evals"]:at["layer_roots"]]
    if roots is not None and not np.array_equal(w_roots, np.asarray(roots, np.uint32).reshape(-1)):
        return 2
    if points is not None and not np.array_equal(w_pts, np.asarray(points, np.uint32).reshape(-1)):
        return 13
    if evals is not None and not np.array_equal(w_y, np.asarray(evals, np.uint32).reshape(-1)):
        return 13
    if (w >= P).any():
        return 3
    for g in G:
        if not ev.points_ok(w[g["points"]:g["points"] + 4 * g["n_points"]].reshape(-1, 4)):
            return 12
    log_M = log_ns[0] + b
    M, n_fin = 1 << log_M, 4 << b
    fin = w[at["final"]:at["final"] + 4 * n_fin].astype(U64).reshape(n_fin, 4)
    winv = pow(ld.root_of_unity(2 + b), P - 2, P)
    for k in range(4, n_fin):
        if (ld.e_scale(fin, ld.powers(pow(winv, k, P), n_fin)).sum(axis=0) % U64(P)).any():
            return 4
    ch = ld.Challenger()
    ch.observe_n(w[:at["layer_roots"]])
    gamma = ch.sample_ext()
    betas = []
    for j in range(n_layers):
        ch.observe_n(w[at["layer_roots"] + 4 * j:at["layer_roots"] + 4 * j + 4])
        betas.append(ch.sample_ext())
    ch.observe_n(w[at["final"]:at["nonce"]])
    if not ch.check_pow(int(w[at["nonce"]]), pow_bits):
        return 5
    qs = [ch.sample_bits(log_M - 1) for _ in range(nq)]
    gp = e_pow_from([1, 0, 0, 0], gamma, at["n_evals"])
    ys = w_y.astype(U64).reshape(-1, 4)
    for g in G:                                                      # a_i of every group, with the group's exponents
        g["sel"] = [(i, m, g["first_e"] + e1) for i, m, e1 in be.selected(g["widths"], g["masks"], g["n_points"])[0]]
        g["pts"] = w[g["points"]:g["points"] + 4 * g["n_points"]].astype(U64).reshape(-1, 4)
        g["a"] = np.zeros((g["n_points"], 4), U64)
        for i, m, e in g["sel"]:
            g["a"][i] = (g["a"][i] + ld.e_mul(gp[e:e + g["widths"][m]], ys[e:e + g["widths"][m]]).sum(axis=0)) % U64(P)

    def F_at(g, pos, rows):
        """F_h at row pos of its own domain from the opened rows (rows[m]: uint64[width_m])"""
        x = GEN * pow(ld.root_of_unity(g["log_M"]), pos, P) % P
        A = np.zeros((g["n_points"], 4), U64)
        for i, m, e in g["sel"]:
            A[i] = (A[i] + (rows[m][:, None] * gp[e:e + g["widths"][m]] % U64(P)).sum(axis=0)) % U64(P)
        F = np.zeros((1, 4), U64)
        for i in range(g["n_points"]):
            F = ld.e_add(F, ld.e_mul(ld.e_sub(g["a"][i], A[i]).reshape(1, 4), ev.e_inv(ev._z_minus_x(g["pts"][i], [x]))))
        return F[0]

    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = qs[t]
        if int(w[p0]) != q:
            return 6
        rows = []
        for h, g in enumerate(G):
            positions = (q, q + M // 2) if h == 0 else (q % (1 << g["log_M"]),)
            rows.append([[None] * len(g["widths"]) for _ in positions])
            for m, width in enumerate(g["widths"]):
                for s2, pos in enumerate(positions):
                    r = w[p0 + g["records"][m][s2]:p0 + g["records"][m][s2] + g["recs"][m]]
                    if not ld._path_ok(so.hash_elems(r[:width]), pos, r[width:], g["log_M"], w[g["roots"] + 4 * m:g["roots"] + 4 * m + 4]):
                        return 7
                    rows[h][s2][m] = r[:width].astype(U64)
        want = [F_at(G[0], q, rows[0][0]), F_at(G[0], q + M // 2, rows[0][1])]
        carried, carried_idx, shift, log_m = None, q, GEN, log_M
        for j, k in enumerate(ks):
            v_at, p_at, depth = at["layers"][j]
            nv, gsz = 1 << k, 1 << depth
            for h in range(1, len(G)):
                if G[h]["log_M"] == log_m:
                    carried = ld.e_add(carried, F_at(G[h], carried_idx, rows[h][0]))
            idx, slot = carried_idx & (gsz - 1), carried_idx >> depth
            vals = w[p0 + v_at:p0 + v_at + 4 * nv]
            v = [x for x in vals.astype(U64).reshape(nv, 4)]
            if j == 0 and not (np.array_equal(v[0], want[0]) and np.array_equal(v[1], want[1])):
                return 8
            if not ld._path_ok(so.hash_elems(vals), idx, w[p0 + p_at:p0 + p_at + 4 * depth], depth, w[at["layer_roots"] + 4 * j:at["layer_roots"] + 4 * j + 4]):
                return 9
            if j > 0 and not np.array_equal(v[slot], carried):
                return 10
            beta = betas[j]
            for f in range(k):
                half = nv >> (f + 1)
                wm = ld.root_of_unity(log_m)
                for t2 in range(half):
                    v[t2] = ld._fold_pair(v[t2], v[t2 + half], shift * pow(wm, idx + t2 * gsz, P) % P, beta)
                shift, log_m, beta = shift * shift % P, log_m - 1, so.emul(beta, beta)
            carried, carried_idx = v[0], idx
        if not np.array_equal(fin[carried_idx & (n_fin - 1)], carried):
            return 11
    return 0

"""Reference prover and verifier of the BATCHED EVALUATION PROOF (zkir_batch_eval_prove / zkir_batch_eval_verify), for the batch-eval tests.  Nothing here imports the
product: eval_ref (evaluate, e_inv, points_ok), lowdeg_ref (field, fold, trees, paths, challenger), oracle.stark_api (merkle, hash_elems, emul) and numpy.

Statement: n_mats (1 .. 4) matrices committed over the same coset 31 <w_M>, M = N << b, each under its own root; matrix m has width_m (1 .. 512) columns and a mask_m
(1 .. 2^n_points - 1) saying at which of the n_points (1 or 2) shared points z_i of E4 it is opened.  Every point is used by some matrix and the widths sum to at most 512.
Every column is close to a polynomial of degree < N, and p_{m,k}(z_i) = y[i][m][k] for every selected (i, m).  The evaluations are eval_ref's barycentric sums.
The gamma exponent e runs consecutively: for i over the points, for m over the matrices with bit i of mask_m set, in order, for k < width_m.
    A_i(x) = sum gamma^e col_{m,k}(x),  a_i = sum gamma^e y[i][m][k]   (over the selected (m, k) of point i)
    F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j)   over all M rows; batched FRI over F exactly as in lowdeg_ref.

Proof words (all canonical):
    [0..9)   MAGIC 'ZKBE', VERSION, log_n, b, n_mats, n_points, num_queries, pow_bits, n_layers
    then     (width_m, mask_m) per matrix | the n_mats roots | 4 n_points point words | the evaluations in the exponent order, 4 words each | lowdeg_ref's layout: n_layers x 4
             layer roots | n_fin x 4 final layer | the nonce | the queries
    query:   q, then for each matrix in order record_m(q), record_m(q + M/2) (width_m + 4 log_M words each), then per layer values and path
Transcript: every word up to and including the evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log_n + b - 1).

Codes of verify_ref, first failing check in this order, lowest query first: 1 malformed (also n_mats, a width, the width total, a mask, an unused point), 2 not the expected
roots, 13 not the expected points / evaluations, 3 a word >= p, 12 a point in the base field or two equal points, 4 final layer not of degree < 4, 5 grinding, 6 a query's
index word, 7 a matrix record (lowest matrix first within a query, q before q + M/2), 8 layer-0 values != F at the two rows (recomputed from ALL the matrices' records;
BEFORE layer 0's path), 9 a FRI leaf's path, 10 carried value != v[slot], 11 final value."""
from __future__ import annotations

import numpy as np

import eval_ref as ev
import lowdeg_ref as ld
from oracle import stark_api as so

P, GEN, U64 = ld.P, ld.GEN, ld.U64
MAGIC, VERSION = 0x45424B5A, 1
HEAD = 9
MAX_MATS, MAX_POINTS, MAX_TOTAL_WIDTH = 4, 2, 512


def shape_ok(widths, masks, n_points) -> bool:
    """1 .. 4 matrices of width 1 .. 512 summing to at most 512, masks in 1 .. 2^n_points - 1, every point used"""
    if not 1 <= n_points <= MAX_POINTS or not 1 <= len(widths) <= MAX_MATS or len(masks) != len(widths):
        return False
    if any(not 1 <= w <= ld.MAX_WIDTH for w in widths) or sum(widths) > MAX_TOTAL_WIDTH or any(not 1 <= k < (1 << n_points) for k in masks):
        return False
    used = 0
    for k in masks:
        used |= k
    return used == (1 << n_points) - 1


def params_ok(log_n, b, widths, masks, n_points, num_queries) -> bool:
    return shape_ok(widths, masks, n_points) and ld.params_ok(log_n, b, 1, num_queries)


def selected(widths, masks, n_points):
    """[(i, m, first exponent)] in the exponent order, and the number of evaluations"""
    out, e = [], 0
    for i in range(n_points):
        for m, (w, k) in enumerate(zip(widths, masks)):
            if (k >> i) & 1:
                out.append((i, m, e))
                e += w
    return out, e


def query_words(log_n: int, b: int, widths) -> int:
    return ld.query_words(log_n, b, 1) - 2 + 2 * sum(widths) + 8 * (log_n + b) * (len(widths) - 1)


def proof_words(log_n: int, b: int, widths, masks, n_points: int, num_queries: int) -> int:
    widths, masks = [int(x) for x in widths], [int(x) for x in masks]
    if not params_ok(log_n, b, widths, masks, n_points, num_queries):
        return 0
    n_evals = selected(widths, masks, n_points)[1]
    return HEAD + 6 * len(widths) + 4 * n_points + 4 * n_evals + 4 * len(ld.schedule(log_n, b)) + 4 * (4 << b) + 1 + num_queries * query_words(log_n, b, widths)


def evaluate(mats, b: int, masks, points) -> np.ndarray:
    """the evaluations uint64[n_evals][4] in the exponent order: eval_ref's sums for the (point, matrix) pairs the masks select, and for no others"""
    pts = np.asarray(points, U64).reshape(-1, 4)
    widths = [len(c) for c in mats]
    per = {}
    for m, cols in enumerate(mats):
        idx = [i for i in range(len(pts)) if (masks[m] >> i) & 1]
        for i, y in zip(idx, ev.evaluate(cols, b, pts[idx])):
            per[(i, m)] = y
    return np.concatenate([per[(i, m)] for i, m, _ in selected(widths, masks, len(pts))[0]])


def quotient(mats, masks, points, evals, gamma) -> np.ndarray:
    """F uint64[M][4] over all M rows; evals [n_evals][4] in the exponent order"""
    mats = [np.asarray(c, dtype=np.uint32) for c in mats]
    widths, M = [len(c) for c in mats], mats[0].shape[1]
    pts = np.asarray(points, U64).reshape(-1, 4)
    sel, n_evals = selected(widths, masks, len(pts))
    evals = np.asarray(evals, U64).reshape(n_evals, 4)
    gp = ld.e_pow_table(gamma, n_evals)
    x = ld.powers(ld.root_of_unity(M.bit_length() - 1), M) * U64(GEN) % U64(P)
    F = np.zeros((M, 4), U64)
    for i, z in enumerate(pts):
        A, a = np.zeros((M, 4), U64), np.zeros(4, U64)
        for i2, m, e in sel:
            if i2 != i:
                continue
            for k in range(widths[m]):
                A = (A + mats[m][k].astype(U64)[:, None] * gp[e + k][None, :] % U64(P)) % U64(P)
            a = (a + ld.e_mul(gp[e:e + widths[m]], evals[e:e + widths[m]]).sum(axis=0)) % U64(P)      # at most 512 terms below p
        F = ld.e_add(F, ld.e_mul(ld.e_sub(a.reshape(1, 4), A), ev.e_inv(ev._z_minus_x(z, x))))
    return F


def prove_ref(mats, b: int, masks, points, num_queries: int, pow_bits: int, evals=None) -> np.ndarray:
    """The proof for the extended matrices mats[m] (uint32[width_m][M]) at `points` ([n_points][4] canonical).  A cheating prover for the tests: `evals` ([n_evals][4]) takes
    the place of the evaluations; everything after follows the honest procedure."""
    mats = [np.ascontiguousarray(c, dtype=np.uint32) for c in mats]
    widths, masks, M = [len(c) for c in mats], [int(k) for k in masks], mats[0].shape[1]
    pts = np.asarray(points, np.uint32).reshape(-1, 4)
    log_n = M.bit_length() - 1 - b
    assert all(c.shape[1] == M for c in mats) and M == 1 << (log_n + b) and params_ok(log_n, b, widths, masks, len(pts), num_queries)
    assert 0 <= pow_bits <= ld.MAX_POW and ev.points_ok(pts)
    ks = ld.schedule(log_n, b)
    committed = [so.merkle(c, want_layers=True) for c in mats]
    y = (evaluate(mats, b, masks, pts) if evals is None else np.asarray(evals, U64).reshape(-1, 4)).astype(np.uint32)
    assert len(y) == selected(widths, masks, len(pts))[1]
    head = [MAGIC, VERSION, log_n, b, len(mats), len(pts), num_queries, pow_bits, len(ks)]
    out = [np.array(head, np.uint32), np.array([[w, k] for w, k in zip(widths, masks)], np.uint32).reshape(-1)] + [r for r, _ in committed] + [pts.reshape(-1), y.reshape(-1)]
    ch = ld.Challenger()
    ch.observe_n(np.concatenate(out))
    gamma = ch.sample_ext()
    layers, trees, roots = [quotient(mats, masks, pts, y, gamma)], [], []
    shift, log_m = GEN, log_n + b
    for j, k in enumerate(ks):
        r, t = ld.layer_tree(layers[j], k)
        roots.append(r); trees.append(t)
        ch.observe_n(r)
        nxt, shift = ld.fold(layers[j], k, shift, log_m, ch.sample_ext())
        log_m -= k
        layers.append(nxt)
    fin = layers[-1]
    assert len(fin) == 4 << b
    ch.observe_n(fin)
    nonce = ch.grind(pow_bits)
    assert ch.check_pow(nonce, pow_bits)                             # (observes the nonce: the queries are drawn after it)
    out += roots + [fin.astype(np.uint32).reshape(-1), np.array([nonce], np.uint32)]
    for _ in range(num_queries):
        q = ch.sample_bits(log_n + b - 1)
        out.append(np.array([q], np.uint32))
        for cols, (_, tree) in zip(mats, committed):
            for pos in (q, q + M // 2):
                out += [cols[:, pos], ld.tree_path(tree, M, pos)]
        log_m = log_n + b
        for j, k in enumerate(ks):
            g = (1 << log_m) >> k
            idx = q & (g - 1)
            out += [layers[j][idx + t * g].astype(np.uint32) for t in range(1 << k)] + [ld.tree_path(trees[j], g, idx)]
            log_m -= k
    proof = np.concatenate(out).astype(np.uint32)
    assert len(proof) == proof_words(log_n, b, widths, masks, len(pts), num_queries)
    return proof


def layout(proof) -> dict:
    """Word offsets of a well-formed proof: shape (the (width, mask) pairs), roots, points, evals, layer roots, final layer, nonce, queries, qsize; `evals_of`: {(i, m): offset
    of y[i][m][0]}; inside a query (relative): `records` [m] = (record(q) at, record(q + M/2) at), per layer (values, path, depth)"""
    log_n, b, n_mats, n_points, nq = (int(x) for x in proof[2:7])
    widths = [int(x) for x in proof[HEAD:HEAD + 2 * n_mats:2]]
    masks = [int(x) for x in proof[HEAD + 1:HEAD + 2 * n_mats:2]]
    ks = ld.schedule(log_n, b)
    sel, n_evals = selected(widths, masks, n_points)
    n_fin = 4 << b
    at = {"log_n": log_n, "b": b, "n_mats": n_mats, "n_points": n_points, "num_queries": nq, "ks": ks, "widths": widths, "masks": masks, "n_evals": n_evals, "n_fin": n_fin,
          "shape": HEAD, "roots": HEAD + 2 * n_mats, "points": HEAD + 6 * n_mats, "evals": HEAD + 6 * n_mats + 4 * n_points, "recs": [w + 4 * (log_n + b) for w in widths]}
    at["evals_of"] = {(i, m): at["evals"] + 4 * e for i, m, e in sel}
    at["layer_roots"] = at["evals"] + 4 * n_evals
    at["final"] = at["layer_roots"] + 4 * len(ks)
    at["nonce"] = at["final"] + 4 * n_fin
    at["queries"] = at["nonce"] + 1
    at["qsize"] = query_words(log_n, b, widths)
    rel, records = 1, []
    for rec in at["recs"]:
        records.append((rel, rel + rec))
        rel += 2 * rec
    at["records"] = records
    lm, lay = log_n + b, []
    for k in ks:
        lay.append((rel, rel + 4 * (1 << k), lm - k))
        rel += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    at["layers"] = lay
    return at


def verify_ref(proof, roots=None, points=None, evals=None) -> int:
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    if len(w) < HEAD or int(w[0]) != MAGIC or int(w[1]) != VERSION:
        return 1
    log_n, b, n_mats, n_points, nq, pow_bits, n_layers = (int(x) for x in w[2:9])
    if not 1 <= n_mats <= MAX_MATS or not 1 <= n_points <= MAX_POINTS or len(w) < HEAD + 2 * n_mats:
        return 1
    widths, masks = [int(x) for x in w[HEAD:HEAD + 2 * n_mats:2]], [int(x) for x in w[HEAD + 1:HEAD + 2 * n_mats:2]]
    if not params_ok(log_n, b, widths, masks, n_points, nq) or pow_bits > ld.MAX_POW:
        return 1
    ks = ld.schedule(log_n, b)
    if n_layers != len(ks) or len(w) != proof_words(log_n, b, widths, masks, n_points, nq):
        return 1
    at = layout(w)
    w_roots, w_pts, w_y = w[at["roots"]:at["points"]], w[at["points"]:at["evals"]], w[at["evals"]:at["layer_roots"]]
    if roots is not None and not np.array_equal(w_roots, np.asarray(roots, np.uint32).reshape(-1)):
        return 2
    if points is not None and not np.array_equal(w_pts, np.asarray(points, np.uint32).reshape(-1)):
        return 13
    if evals is not None and not np.array_equal(w_y, np.asarray(evals, np.uint32).reshape(-1)):
        return 13
    if (w >= P).any():
        return 3
    if not ev.points_ok(w_pts.reshape(-1, 4)):
        return 12
    log_M = log_n + b
    M, n_fin = 1 << log_M, 4 << b
    fin = w[at["final"]:at["final"] + 4 * n_fin].astype(U64).reshape(n_fin, 4)
    winv = pow(ld.root_of_unity(2 + b), P - 2, P)
    for k in range(4, n_fin):
        if (ld.e_scale(fin, ld.powers(pow(winv, k, P), n_fin)).sum(axis=0) % U64(P)).any():
            return 4
    ch = ld.Challenger()
    ch.observe_n(w[:at["layer_roots"]])                              # header, shape, roots, points, evaluations
    gamma = ch.sample_ext()
    betas = []
    for j in range(n_layers):
        ch.observe_n(w[at["layer_roots"] + 4 * j:at["layer_roots"] + 4 * j + 4])
        betas.append(ch.sample_ext())
    ch.observe_n(w[at["final"]:at["nonce"]])
    if not ch.check_pow(int(w[at["nonce"]]), pow_bits):
        return 5
    qs = [ch.sample_bits(log_M - 1) for _ in range(nq)]
    pts = w_pts.astype(U64).reshape(n_points, 4)
    ys = w_y.astype(U64).reshape(-1, 4)
    sel = selected(widths, masks, n_points)[0]
    gp = ld.e_pow_table(gamma, at["n_evals"])
    a = np.zeros((n_points, 4), U64)
    for i, m, e in sel:
        a[i] = (a[i] + ld.e_mul(gp[e:e + widths[m]], ys[e:e + widths[m]]).sum(axis=0)) % U64(P)
    wM = ld.root_of_unity(log_M)
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = qs[t]
        if int(w[p0]) != q:
            return 6
        rows = [[None, None] for _ in range(n_mats)]
        for m in range(n_mats):
            for s2 in range(2):
                r = w[p0 + at["records"][m][s2]:p0 + at["records"][m][s2] + at["recs"][m]]
                if not ld._path_ok(so.hash_elems(r[:widths[m]]), q + s2 * (M // 2), r[widths[m]:], log_M, w_roots[4 * m:4 * m + 4]):
                    return 7
                rows[m][s2] = r[:widths[m]].astype(U64)
        want = []
        for s2 in range(2):
            x = GEN * pow(wM, q + s2 * (M // 2), P) % P
            A = np.zeros((n_points, 4), U64)
            for i, m, e in sel:
                A[i] = (A[i] + (rows[m][s2][:, None] * gp[e:e + widths[m]] % U64(P)).sum(axis=0)) % U64(P)
            F = np.zeros((1, 4), U64)
            for i in range(n_points):
                F = ld.e_add(F, ld.e_mul(ld.e_sub(a[i], A[i]).reshape(1, 4), ev.e_inv(ev._z_minus_x(pts[i], [x]))))
            want.append(F[0])
        carried, carried_idx, shift, log_m = None, q, GEN, log_M
        for j, k in enumerate(ks):
            v_at, p_at, depth = at["layers"][j]
            nv, g = 1 << k, 1 << depth
            idx, slot = carried_idx & (g - 1), carried_idx >> depth
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
                    v[t2] = ld._fold_pair(v[t2], v[t2 + half], shift * pow(wm, idx + t2 * g, P) % P, beta)
                shift, log_m, beta = shift * shift % P, log_m - 1, so.emul(beta, beta)
            carried, carried_idx = v[0], idx
        if not np.array_equal(fin[carried_idx & (n_fin - 1)], carried):
            return 11
    return 0

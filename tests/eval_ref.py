"""Reference prover and verifier of the EVALUATION PROOF OF A COMMITMENT (zkir_eval_prove / zkir_eval_verify), for the eval tests.  Nothing here imports the product:
lowdeg_ref (field, fold, trees, paths, challenger), oracle.stark_api (merkle, hash_elems, emul) and numpy.

Statement: every column k of a committed matrix over the coset 31 <w_M>, M = N << b, is close to a polynomial p_k of degree < N, and p_k(z_i) = y[i][k] at n_points (1 or 2)
points z_i of E4 outside the base field.  The evaluations are DEFINED as the barycentric sums over the rows j 2^b (the sub-coset 31 <w_N>), whatever the matrix holds:
    y[i][k] = ((z_i / 31)^N - 1) / N * sum_j mat[k][j 2^b] x_j / (z_i - x_j),   x_j = 31 w_N^j
Codeword: F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j) over all M rows, A_i(x) = sum_k gamma^(i width + k) col_k(x), a_i = sum_k gamma^(i width + k) y[i][k]; batched FRI
over F exactly as in lowdeg_ref.

Proof words (all canonical):
    [0..9)   MAGIC 'ZKEV', VERSION, log_n, b, width, n_points, num_queries, pow_bits, n_layers
    [9..13)  the matrix root | 4 n_points point words | 4 n_points width evaluation words (point-major) | then lowdeg_ref's layout: n_layers x 4 layer roots | n_fin x 4 final
             layer | the nonce | the queries (q, record(q), record(q + M/2), per layer values and path)
Transcript: header, root, points, evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log_n + b - 1).

Codes of verify_ref, first failing check in this order, lowest query first: 1 malformed, 2 not the expected root, 13 not the expected points / evaluations, 3 a word >= p,
12 a point in the base field or two equal points, 4 final layer not of degree < 4, 5 grinding, 6 a query's index word, 7 a matrix record, 8 layer-0 values != F at the two
rows (recomputed from the records, the points and the evaluations; BEFORE layer 0's path), 9 a FRI leaf's path, 10 carried value != v[slot], 11 final value."""
from __future__ import annotations

import numpy as np

import lowdeg_ref as ld
from oracle import stark_api as so

P, GEN, U64 = ld.P, ld.GEN, ld.U64
MAGIC, VERSION = 0x56454B5A, 1
HEAD = 9
MAX_POINTS = 2


def f_inv(a) -> np.ndarray:
    """a^(p-2) for a vector of base-field values (uint64), by square and multiply"""
    a = np.asarray(a, U64) % U64(P)
    out = np.ones(a.shape, U64)
    e = P - 2
    while e:
        if e & 1:
            out = out * a % U64(P)
        a = a * a % U64(P)
        e >>= 1
    return out


def e_inv(a) -> np.ndarray:
    """Inverse of E4 values [n][4] through the norm to F[Y]/(Y^2 - 11), Y = X^2: a = A(Y) + X B(Y), a (A - X B) = A^2 - Y B^2 = n0 + n1 Y, whose inverse is
    (n0 - n1 Y) / (n0^2 - 11 n1^2)"""
    a = np.asarray(a, U64).reshape(-1, 4) % U64(P)
    p, a0, a1, a2, a3 = U64(P), a[:, 0], a[:, 1], a[:, 2], a[:, 3]
    A0, A1 = (a0 * a0 + U64(11) * (a2 * a2 % p)) % p, U64(2) * (a0 * a2 % p) % p
    B0, B1 = (a1 * a1 + U64(11) * (a3 * a3 % p)) % p, U64(2) * (a1 * a3 % p) % p
    n0, n1 = (A0 + p - U64(11) * B1 % p) % p, (A1 + p - B0) % p
    d = f_inv((n0 * n0 % p + p - U64(11) * (n1 * n1 % p) % p) % p)
    i0, i1 = n0 * d % p, (p - n1 * d % p) % p
    conj = np.stack([a0, (p - a1) % p, a2, (p - a3) % p], axis=1)
    ninv = np.stack([i0, np.zeros_like(i0), i1, np.zeros_like(i0)], axis=1)
    return ld.e_mul(conj, ninv)


def e_pow(a, e: int) -> np.ndarray:
    a, out = np.asarray(a, U64).reshape(1, 4), np.array([[1, 0, 0, 0]], U64)
    while e:
        if e & 1:
            out = ld.e_mul(out, a)
        a = ld.e_mul(a, a)
        e >>= 1
    return out[0]


def points_ok(points) -> bool:
    """one or two canonical points, each outside the base field (a coordinate 1 .. 3 is not zero), two of them different"""
    pts = np.asarray(points, U64).reshape(-1, 4)
    if not 1 <= len(pts) <= MAX_POINTS or (pts >= P).any() or not all(p[1:].any() for p in pts):
        return False
    return len(pts) == 1 or not np.array_equal(pts[0], pts[1])


def _z_minus_x(z, x) -> np.ndarray:
    out = np.tile(np.asarray(z, U64).reshape(1, 4), (len(x), 1))
    out[:, 0] = (out[:, 0] + U64(P) - np.asarray(x, U64)) % U64(P)
    return out


def evaluate(cols_lde, b: int, points) -> np.ndarray:
    """y uint64[n_points][width][4]: the barycentric sums over the rows j 2^b of cols_lde (uint32[width][M], canonical)"""
    cols = np.asarray(cols_lde, dtype=np.uint32)
    width, M = cols.shape
    N = M >> b
    log_n = N.bit_length() - 1
    sub = cols[:, ::1 << b].astype(U64)
    x = ld.powers(ld.root_of_unity(log_n), N) * U64(GEN) % U64(P)
    out = np.zeros((len(points), width, 4), U64)
    for i, z in enumerate(np.asarray(points, U64).reshape(-1, 4)):
        wts = ld.e_scale(e_inv(_z_minus_x(z, x)), x)                                 # x_j / (z - x_j)
        scale = e_pow(ld.e_scale(z.reshape(1, 4), pow(GEN, P - 2, P))[0], N)         # (z / 31)^N
        scale[0] = (scale[0] + U64(P - 1)) % U64(P)
        scale = ld.e_scale(scale.reshape(1, 4), pow(N, P - 2, P))[0]
        for k in range(width):
            s = np.zeros(4, U64)
            for lo in range(0, N, 1 << 16):                                          # 2^16 terms below p: the sum fits 64 bits
                s = (s + (sub[k, lo:lo + (1 << 16), None] * wts[lo:lo + (1 << 16)] % U64(P)).sum(axis=0)) % U64(P)
            out[i, k] = ld.e_mul(s.reshape(1, 4), scale)[0]
    return out


def quotient(cols_lde, b: int, points, evals, gamma) -> np.ndarray:
    """F uint64[M][4] over all M rows (b is implied by nothing here: the rows are those of the whole domain 31 <w_M>)"""
    cols = np.asarray(cols_lde, dtype=np.uint32)
    width, M = cols.shape
    pts = np.asarray(points, U64).reshape(-1, 4)
    evals = np.asarray(evals, U64).reshape(len(pts), width, 4)
    gp = ld.e_pow_table(gamma, len(pts) * width)
    x = ld.powers(ld.root_of_unity(M.bit_length() - 1), M) * U64(GEN) % U64(P)
    F = np.zeros((M, 4), U64)
    for i, z in enumerate(pts):
        g = gp[i * width:(i + 1) * width]
        A = np.zeros((M, 4), U64)
        for k in range(width):
            A = (A + cols[k].astype(U64)[:, None] * g[k][None, :] % U64(P)) % U64(P)
        a = ld.e_mul(g, evals[i]).sum(axis=0) % U64(P)                               # at most 512 terms below p
        F = ld.e_add(F, ld.e_mul(ld.e_sub(a.reshape(1, 4), A), e_inv(_z_minus_x(z, x))))
    return F


def query_words(log_n: int, b: int, width: int) -> int:
    return ld.query_words(log_n, b, width)


def params_ok(log_n, b, width, n_points, num_queries) -> bool:
    return ld.params_ok(log_n, b, width, num_queries) and 1 <= n_points <= MAX_POINTS


def proof_words(log_n: int, b: int, width: int, n_points: int, num_queries: int) -> int:
    if not params_ok(log_n, b, width, n_points, num_queries):
        return 0
    return HEAD + 4 + 4 * n_points * (1 + width) + 4 * len(ld.schedule(log_n, b)) + 4 * (4 << b) + 1 + num_queries * query_words(log_n, b, width)


def prove_ref(cols_lde, b: int, points, num_queries: int, pow_bits: int, evals=None) -> np.ndarray:
    """The proof for the extended matrix cols_lde (uint32[width][M]) at `points` ([n_points][4] canonical).  A cheating prover for the tests: `evals` takes the place of the
    evaluations; everything after follows the honest procedure."""
    cols = np.ascontiguousarray(cols_lde, dtype=np.uint32)
    width, M = cols.shape
    pts = np.asarray(points, np.uint32).reshape(-1, 4)
    log_n = M.bit_length() - 1 - b
    assert M == 1 << (log_n + b) and params_ok(log_n, b, width, len(pts), num_queries) and 0 <= pow_bits <= ld.MAX_POW and points_ok(pts)
    ks = ld.schedule(log_n, b)
    root, tree = so.merkle(cols, want_layers=True)
    y = (evaluate(cols, b, pts) if evals is None else np.asarray(evals, U64).reshape(len(pts), width, 4)).astype(np.uint32)
    head = [MAGIC, VERSION, log_n, b, width, len(pts), num_queries, pow_bits, len(ks)]
    ch = ld.Challenger()
    ch.observe_n(head)
    ch.observe_n(root)
    ch.observe_n(pts)
    ch.observe_n(y)
    gamma = ch.sample_ext()
    layers, trees, roots = [quotient(cols, b, pts, y, gamma)], [], []
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
    out = [np.array(head, np.uint32), root, pts.reshape(-1), y.reshape(-1)] + roots + [fin.astype(np.uint32).reshape(-1), np.array([nonce], np.uint32)]
    for _ in range(num_queries):
        q = ch.sample_bits(log_n + b - 1)
        out.append(np.array([q], np.uint32))
        for pos in (q, q + M // 2):
            out += [cols[:, pos], ld.tree_path(tree, M, pos)]
        log_m = log_n + b
        for j, k in enumerate(ks):
            g = (1 << log_m) >> k
            idx = q & (g - 1)
            out += [layers[j][idx + t * g].astype(np.uint32) for t in range(1 << k)] + [ld.tree_path(trees[j], g, idx)]
            log_m -= k
    proof = np.concatenate(out).astype(np.uint32)
    assert len(proof) == proof_words(log_n, b, width, len(pts), num_queries)
    return proof


def layout(proof) -> dict:
    """Word offsets of a well-formed proof: root, points, evals, layer roots, final layer, nonce, queries, qsize, and inside a query (relative): the records, per layer
    (values, path, depth)"""
    log_n, b, width, n_points, nq = (int(x) for x in proof[2:7])
    ks = ld.schedule(log_n, b)
    n_fin, rec = 4 << b, width + 4 * (log_n + b)
    at = {"log_n": log_n, "b": b, "width": width, "n_points": n_points, "num_queries": nq, "ks": ks, "root": HEAD, "points": HEAD + 4, "evals": HEAD + 4 + 4 * n_points,
          "n_fin": n_fin, "rec": rec}
    at["layer_roots"] = at["evals"] + 4 * n_points * width
    at["final"] = at["layer_roots"] + 4 * len(ks)
    at["nonce"] = at["final"] + 4 * n_fin
    at["queries"] = at["nonce"] + 1
    at["qsize"] = query_words(log_n, b, width)
    rel, lm, lay = 1 + 2 * rec, log_n + b, []
    for k in ks:
        lay.append((rel, rel + 4 * (1 << k), lm - k))
        rel += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    at["layers"] = lay
    return at


def verify_ref(proof, root=None, points=None, evals=None) -> int:
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    if len(w) < HEAD or int(w[0]) != MAGIC or int(w[1]) != VERSION:
        return 1
    log_n, b, width, n_points, nq, pow_bits, n_layers = (int(x) for x in w[2:9])
    if not params_ok(log_n, b, width, n_points, nq) or pow_bits > ld.MAX_POW:
        return 1
    ks = ld.schedule(log_n, b)
    if n_layers != len(ks) or len(w) != proof_words(log_n, b, width, n_points, nq):
        return 1
    at = layout(w)
    w_root = w[at["root"]:at["root"] + 4]
    w_pts, w_y = w[at["points"]:at["evals"]], w[at["evals"]:at["layer_roots"]]
    if root is not None and not np.array_equal(w_root, np.asarray(root, np.uint32)):
        return 2
    if points is not None and not np.array_equal(w_pts, np.asarray(points, np.uint32).reshape(-1)):
        return 13
    if evals is not None and not np.array_equal(w_y, np.asarray(evals, np.uint32).reshape(-1)):
        return 13
    if (w >= P).any():
        return 3
    if not points_ok(w_pts.reshape(-1, 4)):
        return 12
    log_M = log_n + b
    M, n_fin = 1 << log_M, 4 << b
    fin = w[at["final"]:at["final"] + 4 * n_fin].astype(U64).reshape(n_fin, 4)
    winv = pow(ld.root_of_unity(2 + b), P - 2, P)
    for k in range(4, n_fin):
        if (ld.e_scale(fin, ld.powers(pow(winv, k, P), n_fin)).sum(axis=0) % U64(P)).any():
            return 4
    ch = ld.Challenger()
    ch.observe_n(w[:at["layer_roots"]])                              # header, root, points, evaluations
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
    ys = w_y.astype(U64).reshape(n_points, width, 4)
    gp = ld.e_pow_table(gamma, n_points * width).reshape(n_points, width, 4)
    a = [ld.e_mul(gp[i], ys[i]).sum(axis=0) % U64(P) for i in range(n_points)]
    wM = ld.root_of_unity(log_M)
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = qs[t]
        if int(w[p0]) != q:
            return 6
        want = []
        for s2 in range(2):
            pos = q + s2 * (M // 2)
            r = w[p0 + 1 + s2 * at["rec"]:p0 + 1 + (s2 + 1) * at["rec"]]
            if not ld._path_ok(so.hash_elems(r[:width]), pos, r[width:], log_M, w_root):
                return 7
            x = GEN * pow(wM, pos, P) % P
            F = np.zeros((1, 4), U64)
            for i in range(n_points):
                A = (r[:width].astype(U64)[:, None] * gp[i] % U64(P)).sum(axis=0) % U64(P)
                F = ld.e_add(F, ld.e_mul(ld.e_sub(a[i], A).reshape(1, 4), e_inv(_z_minus_x(pts[i], [x]))))
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

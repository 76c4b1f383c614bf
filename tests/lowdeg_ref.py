"""Reference prover and verifier of the LOW-DEGREE PROOF OF A COMMITMENT (zkir_lowdeg_prove / zkir_lowdeg_verify), for the lowdeg tests.  Nothing here imports the product:
oracle.stark_api (lde, merkle, hash_elems, compress, permute, emul, einv) and numpy.

Statement: every column of a committed matrix over the coset 31 <w_M>, M = N << b, is close to a polynomial of degree < N.  Batched FRI over C(x) = sum_k gamma^k col_k(x).

Proof words (all canonical):
    [0..8)   MAGIC, VERSION, log_n, b, width, num_queries, pow_bits, n_layers
    [8..12)  the matrix root | n_layers x 4 layer roots | n_fin x 4 final layer (n_fin = 4 << b) | the grinding nonce (the smallest that passes)
    query:   q (< M/2), record(q), record(q + M/2) (row words, then one sibling a level, leaf level first), per layer 4 * 2^k values (value t = c[idx + t g]) and 4 * depth siblings
Transcript: header, root, gamma; per layer root, beta; the 4 n_fin final words; check_pow(nonce); q_t = sample_bits(log_n + b - 1).

Codes of verify_ref, first failing check in this order, lowest query first: 1 malformed, 2 not the expected root, 3 a word >= p, 4 final layer not of degree < 4, 5 grinding,
6 a query's index word, 7 a matrix record, 8 layer-0 values != sum gamma^k row, 9 a FRI leaf's path, 10 carried value != v[slot], 11 final value.
ORDER INSIDE A LAYER: at layer 0 the equality with the rows (8) is checked BEFORE the leaf's path (9) — a changed layer-0 value is an 8; at later layers the path (9) comes
before the carried value (10)."""
from __future__ import annotations

import numpy as np

from oracle import stark_api as so

P = 0x78000001
GEN = 31
ROOT27 = 0x1A427A41
MAGIC, VERSION = 0x444C4B5A, 1
LOG_ARITY = 3
MAX_WIDTH, MAX_QUERIES, MAX_POW = 512, 128, 24
U64 = np.uint64


def root_of_unity(log_m: int) -> int:
    assert 0 <= log_m <= 27
    return pow(ROOT27, 1 << (27 - log_m), P)


def powers(w: int, n: int) -> np.ndarray:
    """w^0 .. w^(n-1) mod p (uint64), by doubling"""
    out = np.ones(1, U64)
    step = w % P
    while len(out) < n:
        out = np.concatenate([out, out * U64(step) % U64(P)])
        step = step * step % P
    return out[:n]


def schedule(log_n: int, b: int):
    ks, log_m = [], log_n + b
    while log_m > 2 + b:
        k = 1 if not ks else min(LOG_ARITY, log_m - (2 + b))
        ks.append(k)
        log_m -= k
    return ks


def params_ok(log_n, b, width, num_queries) -> bool:
    return 3 <= log_n <= 26 and 1 <= b <= 3 and log_n + b <= 27 and 1 <= width <= MAX_WIDTH and 1 <= num_queries <= MAX_QUERIES


def query_words(log_n: int, b: int, width: int) -> int:
    q, lm = 1 + 2 * (width + 4 * (log_n + b)), log_n + b
    for k in schedule(log_n, b):
        q += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    return q


def proof_words(log_n: int, b: int, width: int, num_queries: int) -> int:
    if not params_ok(log_n, b, width, num_queries):
        return 0
    return 12 + 4 * len(schedule(log_n, b)) + 4 * (4 << b) + 1 + num_queries * query_words(log_n, b, width)


# ---- E4 = F_p[X] / (X^4 - 11): vectors are uint64[n][4], scalars length-4 ------------------------------------------------------------------------
def e_add(a, b):
    return (np.asarray(a, U64) + np.asarray(b, U64)) % U64(P)


def e_sub(a, b):
    return (np.asarray(a, U64) + U64(P) - np.asarray(b, U64)) % U64(P)


def e_scale(a, f):
    """a (E4 vector [n][4]) times base-field values f ([n] or a scalar)"""
    f = np.asarray(f, U64)
    return np.asarray(a, U64) * (f[:, None] if f.ndim == 1 else f) % U64(P)


def e_mul(a, b):
    """E4 vector [n][4] times E4 vector or scalar, schoolbook over X^4 = 11"""
    a = np.asarray(a, U64).reshape(-1, 4)
    b = np.broadcast_to(np.asarray(b, U64).reshape(-1, 4), a.shape)
    out = np.zeros(a.shape, U64)
    for i in range(4):
        for j in range(4):
            t = a[:, i] * b[:, j] % U64(P)
            if i + j >= 4:
                t = t * U64(11) % U64(P)
            out[:, (i + j) % 4] = (out[:, (i + j) % 4] + t) % U64(P)
    return out


def e_pow_table(g, n: int) -> np.ndarray:
    """g^0 .. g^(n-1), E4 scalars [n][4] (so.emul: the oracle's product)"""
    out = np.zeros((n, 4), U64)
    cur = np.array([1, 0, 0, 0], np.uint32)
    for k in range(n):
        out[k] = cur
        cur = so.emul(cur, np.asarray(g, np.uint32))
    return out


class Challenger:
    """The duplex sponge of verify.cpp / so::Challenger over so.permute: canonical words in and out, rate 8 of 12, sample() pops from the back of the rate."""

    def __init__(self):
        self.st = np.zeros(12, np.uint32)
        self.inp, self.out = [], []

    def duplex(self):
        for i, v in enumerate(self.inp):
            self.st[i] = v
        self.inp = []
        self.st = so.permute(self.st)
        self.out = [int(x) for x in self.st[:8]]

    def observe(self, x):
        self.out = []
        self.inp.append(int(x))
        if len(self.inp) == 8:
            self.duplex()

    def observe_n(self, xs):
        for x in np.asarray(xs).reshape(-1):
            self.observe(x)

    def sample(self) -> int:
        if self.inp or not self.out:
            self.duplex()
        return self.out.pop()

    def sample_ext(self) -> np.ndarray:
        return np.array([self.sample() for _ in range(4)], np.uint32)

    def sample_bits(self, b: int) -> int:
        return self.sample() & ((1 << b) - 1)

    def flush(self):
        if self.inp:
            self.duplex()
        self.out = []

    def check_pow(self, nonce: int, bits: int) -> bool:
        self.flush()
        self.observe(nonce)
        return self.sample() & ((1 << bits) - 1) == 0

    def grind(self, bits: int) -> int:
        """the SMALLEST nonce check_pow accepts (the state is left as it was)"""
        self.flush()
        mask = (1 << bits) - 1
        for nonce in range(P):
            s = self.st.copy()
            s[0] = nonce
            if int(so.permute(s)[7]) & mask == 0:
                return nonce
        raise AssertionError("no nonce")


# ---- the codeword and its folds -------------------------------------------------------------------------------------------------------------------
def combine(cols, gamma) -> np.ndarray:
    """C[j] = sum_k gamma^k cols[k][j]: cols uint32[width][M] canonical -> uint64[M][4]"""
    cols = np.asarray(cols, dtype=np.uint32)
    gp = e_pow_table(gamma, cols.shape[0])
    out = np.zeros((cols.shape[1], 4), U64)
    for k in range(cols.shape[0]):
        out = (out + cols[k].astype(U64)[:, None] * gp[k][None, :] % U64(P)) % U64(P)
    return out


def sum_diff(cur, shift: int, log_m: int):
    """The two halves of one binary fold of a layer of m = 2^log_m values over shift <w_m>: S[i] = (c[i] + c[i + h]) / 2, D[i] = (c[i] - c[i + h]) / (2 x_i), x_i = shift w_m^i."""
    cur = np.asarray(cur, U64)
    h = len(cur) // 2
    assert len(cur) == 1 << log_m
    a, b = cur[:h], cur[h:]
    inv2x = powers(pow(root_of_unity(log_m), P - 2, P), h) * U64(pow(2 * shift % P, P - 2, P)) % U64(P)
    return e_scale(e_add(a, b), (P + 1) // 2), e_scale(e_sub(a, b), inv2x)


def fold(cur, k: int, shift: int, log_m: int, beta):
    """k binary folds with beta, beta^2, beta^4 (the shift squares each time): returns (layer of m >> k values, the next shift)"""
    beta = np.asarray(beta, np.uint32)
    for _ in range(k):
        s, d = sum_diff(cur, shift, log_m)
        cur = e_add(s, e_mul(d, beta))
        shift, log_m, beta = shift * shift % P, log_m - 1, so.emul(beta, beta)
    return cur, shift


def layer_tree(layer, k: int):
    """(root, tree words) of a layer committed at 2^k values a leaf: leaf i = (c[i + t g])_t, 4 * 2^k words, hashed and compressed as a matrix of that width (so.merkle)"""
    layer = np.asarray(layer, U64)
    g = len(layer) >> k
    mat = np.zeros((4 << k, g), np.uint32)
    for t in range(1 << k):
        for e in range(4):
            mat[4 * t + e] = layer[t * g:(t + 1) * g, e]
    return so.merkle(mat, want_layers=True)


def tree_path(tree, n: int, idx: int) -> np.ndarray:
    out = [tree[4 * (2 * n - ((2 * n) >> lvl)) + 4 * ((idx >> lvl) ^ 1):][:4] for lvl in range(n.bit_length() - 1)]
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def prove_ref(cols_lde, b: int, num_queries: int, pow_bits: int, codeword=None, layer_hook=None) -> np.ndarray:
    """The proof for the extended matrix cols_lde (uint32[width][M], canonical, M = N << b).  A cheating prover for the tests: `codeword` (uint64[M][4]) takes the place of the
    combination, and layer_hook(j, layer) may replace layer j >= 1 (j = n_layers: the final layer) before it is committed; everything after follows the honest procedure."""
    cols = np.ascontiguousarray(cols_lde, dtype=np.uint32)
    width, M = cols.shape
    log_n = M.bit_length() - 1 - b
    assert M == 1 << (log_n + b) and params_ok(log_n, b, width, num_queries) and 0 <= pow_bits <= MAX_POW
    ks = schedule(log_n, b)
    root, tree = so.merkle(cols, want_layers=True)
    head = [MAGIC, VERSION, log_n, b, width, num_queries, pow_bits, len(ks)]
    ch = Challenger()
    ch.observe_n(head)
    ch.observe_n(root)
    gamma = ch.sample_ext()
    layers, trees, roots = [combine(cols, gamma) if codeword is None else np.asarray(codeword, U64)], [], []
    shift, log_m = GEN, log_n + b
    for j, k in enumerate(ks):
        r, t = layer_tree(layers[j], k)
        roots.append(r); trees.append(t)
        ch.observe_n(r)
        beta = ch.sample_ext()
        nxt, shift = fold(layers[j], k, shift, log_m, beta)
        log_m -= k
        if layer_hook is not None:
            nxt = np.asarray(layer_hook(j + 1, nxt), U64)
        layers.append(nxt)
    fin = layers[-1]
    assert len(fin) == 4 << b
    ch.observe_n(fin)
    nonce = ch.grind(pow_bits)
    assert ch.check_pow(nonce, pow_bits)
    out = [np.array(head, np.uint32), root] + roots + [fin.astype(np.uint32).reshape(-1), np.array([nonce], np.uint32)]
    for _ in range(num_queries):
        q = ch.sample_bits(log_n + b - 1)
        out.append(np.array([q], np.uint32))
        for pos in (q, q + M // 2):
            out += [cols[:, pos], tree_path(tree, M, pos)]
        log_m = log_n + b
        for j, k in enumerate(ks):
            g = (1 << log_m) >> k
            idx = q & (g - 1)
            out += [layers[j][idx + t * g].astype(np.uint32) for t in range(1 << k)] + [tree_path(trees[j], g, idx)]
            log_m -= k
    proof = np.concatenate(out).astype(np.uint32)
    assert len(proof) == proof_words(log_n, b, width, num_queries)
    return proof


def layout(proof) -> dict:
    """Word offsets of a well-formed proof: root, layer roots, final layer, nonce, queries, qsize, and inside a query (relative): the records, per layer (values, path)"""
    log_n, b, width, nq = (int(x) for x in proof[2:6])
    ks = schedule(log_n, b)
    n_fin, rec = 4 << b, width + 4 * (log_n + b)
    at = {"log_n": log_n, "b": b, "width": width, "num_queries": nq, "ks": ks, "root": 8, "layer_roots": 12, "final": 12 + 4 * len(ks), "n_fin": n_fin, "rec": rec}
    at["nonce"] = at["final"] + 4 * n_fin
    at["queries"] = at["nonce"] + 1
    at["qsize"] = query_words(log_n, b, width)
    rel, lm, lay = 1 + 2 * rec, log_n + b, []
    for k in ks:
        lay.append((rel, rel + 4 * (1 << k), lm - k))                # (values at, path at, depth)
        rel += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    at["layers"] = lay
    return at


def _path_ok(leaf, idx: int, path, depth: int, root) -> bool:
    node = np.asarray(leaf, np.uint32)
    for lvl in range(depth):
        sib = path[4 * lvl:4 * lvl + 4]
        node = so.compress(sib, node) if (idx >> lvl) & 1 else so.compress(node, sib)
    return np.array_equal(node, np.asarray(root, np.uint32))


def _fold_pair(a, b, x: int, beta):
    s = e_scale(e_add(a, b).reshape(1, 4), (P + 1) // 2)
    d = e_scale(e_sub(a, b).reshape(1, 4), pow(2 * x % P, P - 2, P))
    return e_add(s, e_mul(d, beta))[0]


def verify_ref(proof, root=None) -> int:
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    if len(w) < 12 or int(w[0]) != MAGIC or int(w[1]) != VERSION:
        return 1
    log_n, b, width, nq, pow_bits, n_layers = (int(x) for x in w[2:8])
    if not params_ok(log_n, b, width, nq) or pow_bits > MAX_POW:
        return 1
    ks = schedule(log_n, b)
    if n_layers != len(ks) or len(w) != proof_words(log_n, b, width, nq):
        return 1
    if root is not None and not np.array_equal(w[8:12], np.asarray(root, np.uint32)):
        return 2
    if (w >= P).any():
        return 3
    at = layout(w)
    log_M = log_n + b
    M, n_fin = 1 << log_M, 4 << b
    fin = w[at["final"]:at["final"] + 4 * n_fin].astype(U64).reshape(n_fin, 4)
    winv = pow(root_of_unity(2 + b), P - 2, P)
    for k in range(4, n_fin):                                         # coefficients 4 .. n_fin - 1 of the plain inverse DFT (unscaled)
        if (e_scale(fin, powers(pow(winv, k, P), n_fin)).sum(axis=0) % U64(P)).any():                # (at most 32 terms below p: the sum fits 64 bits)
            return 4
    ch = Challenger()
    ch.observe_n(w[:8])
    ch.observe_n(w[8:12])
    gamma = ch.sample_ext()
    betas = []
    for j in range(n_layers):
        ch.observe_n(w[12 + 4 * j:16 + 4 * j])
        betas.append(ch.sample_ext())
    ch.observe_n(w[at["final"]:at["nonce"]])
    if not ch.check_pow(int(w[at["nonce"]]), pow_bits):
        return 5
    qs = [ch.sample_bits(log_M - 1) for _ in range(nq)]
    gp = e_pow_table(gamma, width)
    for t in range(nq):
        p0 = at["queries"] + t * at["qsize"]
        q = qs[t]
        if int(w[p0]) != q:
            return 6
        comb = []
        for s2 in range(2):
            r = w[p0 + 1 + s2 * at["rec"]:p0 + 1 + (s2 + 1) * at["rec"]]
            if not _path_ok(so.hash_elems(r[:width]), q + s2 * (M // 2), r[width:], log_M, w[8:12]):
                return 7
            comb.append((r[:width].astype(U64)[:, None] * gp % U64(P)).sum(axis=0) % U64(P))
        carried, carried_idx, shift, log_m = None, q, GEN, log_M
        for j, k in enumerate(ks):
            v_at, p_at, depth = at["layers"][j]
            nv, g = 1 << k, 1 << depth
            idx, slot = carried_idx & (g - 1), carried_idx >> depth
            vals = w[p0 + v_at:p0 + v_at + 4 * nv]
            v = [x for x in vals.astype(U64).reshape(nv, 4)]
            if j == 0 and not (np.array_equal(v[0], comb[0]) and np.array_equal(v[1], comb[1])):
                return 8
            if not _path_ok(so.hash_elems(vals), idx, w[p0 + p_at:p0 + p_at + 4 * depth], depth, w[12 + 4 * j:16 + 4 * j]):
                return 9
            if j > 0 and not np.array_equal(v[slot], carried):
                return 10
            beta = betas[j]
            for f in range(k):
                half = nv >> (f + 1)
                wm = root_of_unity(log_m)
                for t2 in range(half):
                    v[t2] = _fold_pair(v[t2], v[t2 + half], shift * pow(wm, idx + t2 * g, P) % P, beta)
                shift, log_m, beta = shift * shift % P, log_m - 1, so.emul(beta, beta)
            carried, carried_idx = v[0], idx
        if not np.array_equal(fin[carried_idx & (n_fin - 1)], carried):
            return 11
    return 0

"""Reference forms of an opening record and of its check, for the merkle-open tests.  Nothing here imports the product: numpy indexing of a column-major matrix and an
oracle-layout tree (4 (2n - 1) words, leaves first, root last; level lvl starts at word 4 (2n - (2n >> lvl))), so.hash_elems / so.compress, and a parser of the query
section of a mode-0 proof (the proof's own per-position records ARE opening records: row words, then one sibling a level, leaf level first)."""
from __future__ import annotations

import numpy as np

from oracle import stark_api as so

P = 0x78000001
FILL = 0xFFFFFFFF
LEAF_DIGEST = 1
LOG_FINAL, LOG_ARITY, NUM_QUERIES = 3, 3, 50


def depth_of(n_leaves: int) -> int:
    assert n_leaves >= 1 and n_leaves & (n_leaves - 1) == 0
    return n_leaves.bit_length() - 1


def record_words(width: int, n_leaves: int, flags: int = 0) -> int:
    return (4 if flags & LEAF_DIGEST else width) + 4 * depth_of(n_leaves)


def level_start(n: int, lvl: int) -> int:
    return 4 * (2 * n - ((2 * n) >> lvl))


def path_ref(layers: np.ndarray, idx: int) -> np.ndarray:
    n = (len(layers) // 4 + 1) // 2
    out = []
    for lvl in range(depth_of(n)):
        at = level_start(n, lvl) + 4 * ((idx >> lvl) ^ 1)
        out.append(layers[at:at + 4])
    return np.concatenate(out).astype(np.uint32) if out else np.zeros(0, np.uint32)


def open_ref(mat_cols, layers: np.ndarray, idx: int) -> np.ndarray:
    """The record of row idx: mat_cols = column-major uint32[width][n] (None: the digest form — the leaf digest leads), layers = the tree.  An index that is no leaf's: all
    0xFFFFFFFF."""
    layers = np.asarray(layers, dtype=np.uint32)
    n = (len(layers) // 4 + 1) // 2
    lead = 4 if mat_cols is None else np.asarray(mat_cols).shape[0]
    if idx >= n:
        return np.full(lead + 4 * depth_of(n), FILL, np.uint32)
    head = layers[4 * idx:4 * idx + 4] if mat_cols is None else np.asarray(mat_cols, dtype=np.uint32)[:, idx]
    return np.concatenate([head, path_ref(layers, idx)]).astype(np.uint32)


def verify_ref(root, width: int, n_leaves: int, idx: int, record, flags: int = 0) -> int:
    """0 the record hashes to root, 1 it does not, 2 one of its words is >= p (not hashed), 3 idx >= n_leaves; 3 over 2 over 1."""
    record = np.asarray(record, dtype=np.uint32)
    d = depth_of(n_leaves)
    lead = 4 if flags & LEAF_DIGEST else width
    assert len(record) == lead + 4 * d
    if idx >= n_leaves:
        return 3
    if (record >= P).any():
        return 2
    node = record[:4].copy() if flags & LEAF_DIGEST else so.hash_elems(record[:width])
    for lvl in range(d):
        sib = record[lead + 4 * lvl:lead + 4 * lvl + 4]
        node = so.compress(sib, node) if (idx >> lvl) & 1 else so.compress(node, sib)
    return 0 if np.array_equal(node, np.asarray(root, dtype=np.uint32)) else 1


def verify_all_ref(root, width, n_leaves, indices, records, flags=0):
    """(verdicts, summary) over a batch, as the entry points report them"""
    words = record_words(width, n_leaves, flags)
    records = np.asarray(records, dtype=np.uint32).reshape(len(indices), words) if words else np.zeros((len(indices), 0), np.uint32)
    v = np.array([verify_ref(root, width, n_leaves, int(i), r, flags) for i, r in zip(indices, records)], dtype=np.uint32).reshape(-1)
    bad = np.nonzero(v)[0]
    return v, np.array([len(bad), bad[0] if len(bad) else FILL], dtype=np.uint32)


def fri_schedule(log_n: int):
    ks, log_m = [], log_n + 1
    while log_m > LOG_FINAL:
        k = 1 if not ks else min(LOG_ARITY, log_m - LOG_FINAL)
        ks.append(k)
        log_m -= k
    return ks


def proof_queries(proof: np.ndarray, log_n: int, num_queries: int = NUM_QUERIES) -> dict:
    """The query section of a mode-0 proof: its last num_queries * qsize words.  Returns the three roots, N, and per commitment ("trace", "aux", "quotient") the width, the
    indices (q, q + N per query, in proof order) and the records.  Asserts that the section parses exactly and that every record's first word (q) is below N."""
    proof = np.asarray(proof, dtype=np.uint32)
    N, depth0 = 1 << log_n, log_n + 1
    wm, wa = int(proof[3]), so.W_AUX
    lay = so.proof_layout(proof)
    widths = {"trace": wm, "aux": wa, "quotient": 4}
    qsize = 1 + sum(2 * (w + 4 * depth0) for w in widths.values())
    lm = log_n + 1
    for k in fri_schedule(log_n):
        qsize += 4 * (1 << k) + 4 * (lm - k)
        lm -= k
    start = len(proof) - num_queries * qsize
    assert start > lay["openings"], "the query section does not fit behind the openings"
    out = {"N": N, "n_leaves": 2 * N, "roots": {"trace": proof[lay["trace_root"]:lay["trace_root"] + 4].copy(), "aux": proof[lay["aux_root"]:lay["aux_root"] + 4].copy(),
                                                 "quotient": proof[lay["quotient_root"]:lay["quotient_root"] + 4].copy()},
           "widths": widths, "indices": {k: [] for k in widths}, "records": {k: [] for k in widths}, "q": []}
    for t in range(num_queries):
        p = start + t * qsize
        q = int(proof[p]); p += 1
        assert q < N, f"query {t}: first word {q} is not below N = {N}"
        out["q"].append(q)
        for name, w in widths.items():
            for s2 in range(2):
                out["indices"][name].append(q + s2 * N)
                out["records"][name].append(proof[p:p + w + 4 * depth0].copy())
                p += w + 4 * depth0
        lm = log_n + 1
        for k in fri_schedule(log_n):
            p += 4 * (1 << k) + 4 * (lm - k)
            lm -= k
        assert p == start + (t + 1) * qsize
    assert start + num_queries * qsize == len(proof)
    for name in widths:
        out["indices"][name] = np.array(out["indices"][name], dtype=np.uint64)
        out["records"][name] = np.stack(out["records"][name])
    return out


def mutations(width: int, n_leaves: int, indices, records, flags: int = 0, seed: int = 0):
    """The mutation set of the tests over a batch of CORRECT records: returns (indices', records') with, round-robin over the positions, a word set to p, p + 1, 0xFFFFFFFF
    (in the row, in the path, in a digest-form leaf: wherever the record has words), an index of n_leaves or 2^63 (also over a non-canonical record), and a correct record
    presented for index j ^ 1.  Position k keeps kind k % 8 (kind 0: untouched)."""
    rng = np.random.default_rng(seed)
    words = record_words(width, n_leaves, flags)
    idx = np.array(indices, dtype=np.uint64).copy()
    rec = np.array(records, dtype=np.uint32).reshape(len(idx), words).copy()
    lead = 4 if flags & LEAF_DIGEST else width
    for k in range(len(idx)):
        kind = k % 8
        if kind in (1, 2, 3) and words:
            where = [int(rng.integers(0, lead))] if lead and (k // 8) % 2 == 0 else []
            if not where:
                where = [int(rng.integers(lead, words))] if words > lead else [int(rng.integers(0, lead))]
            rec[k, where[0]] = (P, P + 1, FILL)[kind - 1]
        elif kind == 4:
            idx[k] = n_leaves
        elif kind == 5:
            idx[k] = 1 << 63
            if words:
                rec[k, int(rng.integers(0, words))] = P
        elif kind == 6 and n_leaves > 1:
            idx[k] = int(idx[k]) ^ 1
    return idx, rec

"""zkir_merkle_verify_host / zkir_merkle_opening_words without a GPU: the query records of the oracle's own proofs are opening records (a bit-for-bit anchor of the
record format), the host verifier against tests/merkle_open_ref.verify_ref over every shape class and mutation, the digest form and the sharded composition, and
the argument errors."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import merkle_open_ref as mref
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec

P = mref.P
FILL = 0xFFFFFFFF


@functools.lru_cache(maxsize=None)
def _proof(name: str, n: int):
    blob = (spec.fib_endless_program() if name == "endless" else spec.fib_program(12)).to_bytes()
    res = oracle.run(blob, max_cycles=n, enable_execution_trace=True)
    pub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code))
    pr = so.prove(res.rows, pub)
    assert so.verify(pr, pub) == 0
    return pr, so.padded_log_n(len(res.rows))


@pytest.mark.parametrize("name,n", [("endless", 50), ("endless", 300), ("fib12", 100000)])
def test_proof_query_records_are_openings(name, n):
    pr, log_n = _proof(name, n)
    if name == "endless":
        assert log_n == {50: 6, 300: 9}[n]
    q = mref.proof_queries(pr, log_n)
    assert q["widths"]["trace"] == int(pr[3]) and q["widths"]["aux"] == 40 and q["widths"]["quotient"] == 4
    for c in ("trace", "aux", "quotient"):
        w, idx, rec = q["widths"][c], q["indices"][c], q["records"][c]
        assert rec.shape == (100, rt.opening_words(w, q["n_leaves"]))
        assert np.array_equal(idx[0::2], np.array(q["q"], dtype=np.uint64)) and np.array_equal(idx[1::2], idx[0::2] + np.uint64(q["N"]))
        v, s = rt.merkle_verify_host(q["roots"][c], w, q["n_leaves"], idx, rec)
        assert not v.any() and list(s) == [0, FILL], (c, v, s)


def test_corruptions_of_proof_records_are_named():
    pr, log_n = _proof("endless", 300)
    q = mref.proof_queries(pr, log_n)
    w, idx, rec, root, n = q["widths"]["trace"], q["indices"]["trace"], q["records"]["trace"], q["roots"]["trace"], q["n_leaves"]
    d = log_n + 1

    def run(i2, r2):
        v, s = rt.merkle_verify_host(root, w, n, i2, r2)
        return list(np.nonzero(v)[0]), [int(x) for x in v[np.nonzero(v)[0]]], [int(x) for x in s]

    r2 = rec.copy(); r2[7, 3] = (int(r2[7, 3]) + 1) % P                                    # one row word of record 7
    assert run(idx, r2) == ([7], [1], [1, 7])
    r2 = rec.copy(); r2[31, w + 2] ^= 1                                                    # a sibling word at the leaf level
    assert run(idx, r2) == ([31], [1], [1, 31])
    r2 = rec.copy(); r2[31, w + 4 * (d - 1) + 1] ^= 1                                      # .. at the top level
    assert run(idx, r2) == ([31], [1], [1, 31])
    a, b = 12, 57
    assert idx[a] != idx[b]
    i2 = idx.copy(); i2[a], i2[b] = idx[b], idx[a]                                         # the indices of two records swapped
    assert run(i2, rec) == ([a, b], [1, 1], [2, a])


def _tree(n, width, seed):
    mat = np.random.default_rng(seed).integers(0, P, (width, n), dtype=np.uint32)
    root, layers = so.merkle(mat, want_layers=True)
    return mat, root, layers


@pytest.mark.parametrize("n", [1, 2, 8, 64])
@pytest.mark.parametrize("width", [0, 1, 4, 5, 8, 9, 40, 152])
def test_host_verifier_equals_reference(n, width):
    mat, root, layers = _tree(n, width, 100 * n + width)
    idx = np.arange(n, dtype=np.uint64)
    rec = np.stack([mref.open_ref(mat, layers, int(j)) for j in idx])
    assert rec.shape == (n, rt.opening_words(width, n)) and mref.record_words(width, n) == rec.shape[1]
    v, s = rt.merkle_verify_host(root, width, n, idx, rec)
    assert not v.any() and list(s) == [0, FILL]                                           # every index; depth 0 (n = 1): a record with no path
    assert not mref.verify_all_ref(root, width, n, idx, rec)[0].any()
    if rec.shape[1] == 0:
        v, s = rt.merkle_verify_host(root, width, n, [1, 1 << 63], np.zeros(0, np.uint32))
        assert list(v) == [3, 3] and list(s) == [2, 0]
        return
    reps = max(1, 32 // n)                                                               # at least four rounds of the eight kinds
    i2, r2 = mref.mutations(width, n, np.tile(idx, reps), np.tile(rec, (reps, 1)), seed=n + width)
    want_v, want_s = mref.verify_all_ref(root, width, n, i2, r2)
    v, s = rt.merkle_verify_host(root, width, n, i2, r2)
    assert np.array_equal(v, want_v) and np.array_equal(s, want_s), (n, width, v, want_v)
    kinds = np.arange(len(i2)) % 8
    assert (v[np.isin(kinds, (1, 2, 3))] == 2).all() and (v[np.isin(kinds, (4, 5))] == 3).all() and (v[kinds == 0] == 0).all() and (v[kinds == 7] == 0).all()
    assert (v[kinds == 6] == (1 if n > 1 and width else 0)).all()                          # (no columns: every leaf is the same digest and the tree is symmetric — the neighbour's record is the leaf's own)


@pytest.mark.parametrize("n", [1, 2, 8, 64])
def test_digest_form_equals_reference(n):
    _, root, layers = _tree(n, 5, 7 + n)
    idx = np.arange(n, dtype=np.uint64)
    rec = np.stack([mref.open_ref(None, layers, int(j)) for j in idx])
    assert rec.shape[1] == rt.opening_words(0, n, rt.OPEN_LEAF_DIGEST) == 4 + 4 * mref.depth_of(n)
    v, s = rt.merkle_verify_host(root, 0, n, idx, rec, rt.OPEN_LEAF_DIGEST)
    assert not v.any() and list(s) == [0, FILL]
    reps = max(1, 32 // n)
    i2, r2 = mref.mutations(0, n, np.tile(idx, reps), np.tile(rec, (reps, 1)), flags=mref.LEAF_DIGEST, seed=n)
    want_v, want_s = mref.verify_all_ref(root, 0, n, i2, r2, mref.LEAF_DIGEST)
    v, s = rt.merkle_verify_host(root, 0, n, i2, r2, rt.OPEN_LEAF_DIGEST)
    assert np.array_equal(v, want_v) and np.array_equal(s, want_s)
    assert set(int(x) for x in v) >= {0, 2, 3}


def test_sharded_record_composes_with_the_cap_path():
    G, nl, width = 4, 16, 19
    shards = [_tree(nl, width, 500 + g) for g in range(G)]
    cap = np.concatenate([s[1] for s in shards])                                          # the cap tree: the shard roots, then the levels above them by so.compress
    level = [s[1] for s in shards]
    while len(level) > 1:
        level = [so.compress(level[2 * k], level[2 * k + 1]) for k in range(len(level) // 2)]
        cap = np.concatenate([cap] + level)
    capped = level[0]
    whole = np.concatenate([s[0] for s in shards], axis=1)
    root_whole, layers_whole = so.merkle(whole, want_layers=True)
    assert np.array_equal(root_whole, capped)                                             # subtree roots capped with compress = the root over the concatenated rows
    idx, rec = [], []
    for g in range(G):
        cap_rec = mref.open_ref(None, cap, g)
        assert np.array_equal(cap_rec[:4], shards[g][1])
        for j in range(nl):
            r = np.concatenate([mref.open_ref(shards[g][0], shards[g][2], j), cap_rec[4:]])
            assert np.array_equal(r, mref.open_ref(whole, layers_whole, g * nl + j))
            idx.append(g * nl + j); rec.append(r)
    v, s = rt.merkle_verify_host(capped, width, G * nl, idx, np.stack(rec))
    assert not v.any() and list(s) == [0, FILL]
    v, _ = rt.merkle_verify_host(capped, 0, G, np.arange(G), np.stack([mref.open_ref(None, cap, g) for g in range(G)]), rt.OPEN_LEAF_DIGEST)
    assert not v.any()


def test_argument_errors():
    L = rt.lib()
    assert rt.opening_words(152, 0) == 0 and rt.opening_words(152, 3) == 0
    assert rt.opening_words(152, 1 << 21) == 152 + 4 * 21 and rt.opening_words(0, 8, rt.OPEN_LEAF_DIGEST) == 4 + 4 * 3
    root, idx, rec, v, s = (np.zeros(k, t) for k, t in ((4, np.uint32), (1, np.uint64), (16, np.uint32), (1, np.uint32), (2, np.uint32)))
    for args in [(None, 4, 8, idx.ctypes.data, 1, rec.ctypes.data, 0, v.ctypes.data, s.ctypes.data),                       # null root
                 (root.ctypes.data, 4, 3, idx.ctypes.data, 1, rec.ctypes.data, 0, v.ctypes.data, s.ctypes.data),          # n_leaves no power of two
                 (root.ctypes.data, 4, 0, idx.ctypes.data, 1, rec.ctypes.data, 0, v.ctypes.data, s.ctypes.data)]:
        assert L.zkir_merkle_verify_host(*args) == rt.ERR_ARGUMENT
        assert "zkir_merkle_verify_host" in L.zkir_last_error().decode()
    with pytest.raises(rt.RuntimeError) as e:
        rt.merkle_verify_host(root, 4, 3, idx, rec)
    assert e.value.code == rt.ERR_ARGUMENT and e.value.message
    assert L.zkir_merkle_verify_host(root.ctypes.data, 4, 8, idx.ctypes.data, 1, rec.ctypes.data, 0, v.ctypes.data, None) == rt.ZKIR_OK     # no summary asked for

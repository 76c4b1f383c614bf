"""Reference verifiers of a run proven in 'ZKSR' segments (zkir_prove_rate_segment / zkir_verify_rate_segment / zkir_verify_rate_chain), modes 0 and 1, for the
rate-chain tests.  Nothing here imports the product: plain Python over prove_rate_ref (the 'ZKSR' prover and verifier), batch_eval_ref (the embedded proof) and the oracle.

A segment proof is pr.prove_ref(rows[a:e], pub) with pub.n_real = e - a and the RUN's digests: the format does not know whether its first row is the VM's initial state.

verify_segment_ref: pr.verify_ref's rules, in its order, without check 7 (the first state is not the VM's initial state).
verify_chain_ref, first failing check:
    40  an empty chain
    per segment i, in order: 1000 (i + 1) + c where verify_segment_ref (no expectation) answers c; then 43 where its header words 9 .. 20 (mode, entry point, program
        digest, io digest) or 4 .. 6 (num_queries, log_blowup, pow_bits) are not segment 0's
    41  segment 0's first state is not the VM's initial state at the header's entry point
    42  a segment's first state is not its predecessor's last state
    43  `expect` names another mode, entry point or digests;  44  expect.n_real != sum (n_i - 1) + 1 (neighbouring segments share a row)
Check 10 is decided against the HONEST proof of the same segment (prove_rate_ref's module text says why), so both take `honest` / one honest proof per segment."""
from __future__ import annotations

import numpy as np

import batch_eval_ref as bev
import lowdeg_ref as ld
import prove_rate_ref as pr
from oracle import stark_api as so

P, U64 = ld.P, ld.U64
HEADER = pr.HEADER


def segment_pub(run_pub, a: int, e: int):
    """the public inputs of rows [a, e) of the run `run_pub` describes: its digests, the segment's own row count"""
    q = run_pub.clone()
    q.n_real = e - a
    return q


def n_real_of(w) -> int:
    return int(w[7]) | (int(w[8]) << 30)


def verify_segment_ref(proof, expect, min_queries: int, min_pow_bits: int, honest) -> int:
    """zkir_verify_rate_segment's verdict on `proof` (modes 0 and 1)"""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    n = len(w)
    if n < HEADER or int(w[0]) != pr.MAGIC or int(w[9]) > 4 or int(w[1]) != pr.VERSION:
        return 1
    log_n, mode, b = int(w[2]), int(w[9]), int(w[5])
    if mode > 2:
        return 2
    if mode == 2 and n < HEADER + 4:
        return 1
    if int(w[4]) > 128 or int(w[6]) > 24:
        return 2
    if int(w[4]) < 1 or not 1 <= b <= 3 or log_n + b > 27 or int(w[4]) < min_queries or int(w[6]) < min_pow_bits:
        return 2
    if int(w[3]) != so.committed_width(mode) or log_n < 3 or log_n > 26:
        return 2
    assert mode < 2, "the reference covers modes 0 and 1"
    if int(w[7]) >= 1 << 30 or int(w[10]) >= 1 << 20 or int(w[11]) >= 1 << 20 or int(w[12]) >= 1 << 24:
        return 2
    n_real = n_real_of(w)
    entry = int(w[10]) | (int(w[11]) << 20) | (int(w[12]) << 40)
    if (w[21:HEADER] >= P).any():
        return 3
    if n_real == 0 or n_real > 1 << 26 or so.padded_log_n(n_real) != log_n:
        return 2
    if expect is not None and (expect.n_real != n_real or expect.deferred != mode or expect.entry != entry or [int(x) for x in expect.prog] != [int(x) for x in w[13:17]] or
                               [int(x) for x in expect.io] != [int(x) for x in w[17:21]]):
        return 6
    # (no check 7: a segment starts wherever its predecessor stopped)
    if (w[2:] >= P).any():
        return 3
    p = HEADER
    if n < p + 1:
        return 4
    blob_len = int(w[p]); p += 1
    blob_words = (blob_len + 1) // 2
    if blob_len > 1 << 30 or n < p + blob_words:
        return 4
    half = w[p:p + blob_words]
    if (half > 0xFFFF).any() or (blob_len & 1 and int(half[-1]) > 0xFF):
        return 8
    blob = np.stack([half & 0xFF, half >> 8], axis=1).astype(np.uint8).reshape(-1)[:blob_len].tobytes()
    p += blob_words
    if not np.array_equal(so.digest_bytes(blob), w[13:17]) or blob_len < 32:
        return 8
    code_size = int.from_bytes(blob[16:20], "little")
    if code_size % 4 or 32 + code_size > blob_len or int.from_bytes(blob[12:16], "little") != entry:
        return 8
    n_code = code_size // 4
    if n < p + n_code + so.RC_TABLE:
        return 4
    at_mult = p
    p += n_code + so.RC_TABLE
    if n < p + 12:
        return 4
    roots = w[p:p + 12]
    p += 12
    ch = ld.Challenger()
    ch.observe_n(w[2:HEADER])
    ch.observe_n(roots[0:4])
    ch.observe_n(w[at_mult:at_mult + n_code + so.RC_TABLE])
    ch.sample_ext(); ch.sample_ext()
    ch.observe_n(roots[4:8])
    ch.sample_ext()
    ch.observe_n(roots[8:12])
    zeta = ch.sample_ext()
    zeta_w = (zeta.astype(U64) * U64(ld.root_of_unity(log_n)) % U64(P)).astype(np.uint32)
    WM, WT = int(w[3]), int(w[3]) + pr.W_AUX
    e = w[p:]
    at_ev, n_ev = 15 + 12 + 8, 2 * WT + 4
    if len(e) < at_ev + 4 * n_ev:
        return 4
    shape = [bev.MAGIC, 1, log_n, b, 3, 2, int(w[4]), int(w[6]), int(e[8]), WM, 3, pr.W_AUX, 3, 4, 1]
    if [int(x) for x in e[:15]] != shape:
        return 5
    h = np.asarray(honest, np.uint32)
    used = np.repeat(pr.used_openings(mode), 4)
    if len(h) < p + at_ev + 4 * n_ev or not np.array_equal(w[2:p], h[2:p]) or not np.array_equal(e[at_ev:at_ev + 4 * n_ev][used], h[p + at_ev:p + at_ev + 4 * n_ev][used]):
        return 10
    c = bev.verify_ref(e, roots=roots, points=np.stack([zeta, zeta_w]))
    return 100 + c if c else 0


_seen = {}


def _segment_code(proof, min_queries, min_pow_bits, honest) -> int:
    """verify_segment_ref without an expectation, remembered by the words (a chain with one damaged segment checks the others once)"""
    key = (np.asarray(proof, np.uint32).tobytes(), np.asarray(honest, np.uint32).tobytes(), int(min_queries), int(min_pow_bits))
    if key not in _seen:
        _seen[key] = verify_segment_ref(proof, None, min_queries, min_pow_bits, honest)
    return _seen[key]


def verify_chain_ref(proofs, expect, min_queries: int, min_pow_bits: int, honests) -> int:
    """zkir_verify_rate_chain's verdict (modes 0 and 1); honests[i]: the honest proof segment i is (a damaged copy of)"""
    if len(proofs) < 1:
        return 40
    ws = [np.ascontiguousarray(p, dtype=np.uint32).reshape(-1) for p in proofs]
    total = 1
    for i, w in enumerate(ws):
        c = _segment_code(w, min_queries, min_pow_bits, honests[i])
        if c:
            return 1000 * (i + 1) + c
        total += n_real_of(w) - 1
        if not np.array_equal(w[9:21], ws[0][9:21]) or not np.array_equal(w[4:7], ws[0][4:7]):
            return 43
    w0 = ws[0]
    init = np.zeros(68, np.uint32)
    init[1:4] = w0[10:13]
    if not np.array_equal(init, w0[21:21 + 68]):
        return 41
    for i in range(1, len(ws)):
        if not np.array_equal(ws[i][21:21 + 68], ws[i - 1][21 + 68:21 + 136]):
            return 42
    if expect is not None:
        entry = int(w0[10]) | (int(w0[11]) << 20) | (int(w0[12]) << 40)
        if expect.deferred != int(w0[9]) or expect.entry != entry or [int(x) for x in expect.prog] != [int(x) for x in w0[13:17]] or [int(x) for x in expect.io] != [int(x) for x in w0[17:21]]:
            return 43
        if expect.n_real != total:
            return 44
    return 0

"""Reference prover and verifier of ZKIR-STARK proofs at blow-up 2, 4 and 8 ('ZKSR', version 1: zkir_prove_rate / zkir_verify_rate), modes 0 and 1, for the prove-rate
tests.  Nothing here imports the product.  It is assembled from what the other tests already use: lowdeg_ref.Challenger (the transcript), oracle.stark_api (main_trace,
to_committed, lookup_setup, lde, merkle, constraints_eval_states, and so.prove for the header, program and multiplicity words, which do not depend on the rate) and
batch_eval_ref.prove_ref / verify_ref (the embedded evaluation proof).

Proof words (all canonical), M = N << b:
    the STARK part: the words of a blow-up-2 proof from the header to the quotient root — header (157 words) | program | ROM multiplicities | range multiplicities |
        trace root | aux root | quotient root — with header word 0 = 'ZKSR', 1 = 1, 4 = num_queries, 5 = b (log_blowup), 6 = pow_bits; the roots are those of the M-row matrices
    the embedded proof: batch_eval_ref.prove_ref([main (152 / 168), aux (40), quotient (4)], b, masks [3, 3, 1], [zeta, w_N zeta], num_queries, pow_bits)
Transcript: header words 2 .., the trace root, the multiplicities, (alpha_l, lambda), the aux root, alpha, the quotient root, zeta.  The embedded proof has its own.
Quotient, row j of the coset x_j = 31 w_M^j: Q(x_j) = sum_c alpha^c C_c(row j, row j + 2^b) / Z_H(x_j), the constraint sum taken by so.constraints_eval_states with the
selector VALUES is_first = Z_H / (x - 1), is_last = Z_H / (x - w_N^last), is_trans = x - w_N^-1.

Codes of verify_ref, first failing check, in zkir_verify_rate's order: 1 too short for a header, magic, version, a mode above 4; 2 a mode above 2, a header range, fewer
queries / bits than asked, n_real against log_n; 3 a word >= p (the boundary states first); 6 not the expected run; 7 the first state is not the VM's initial state;
4 truncated; 8 the program; 5 the embedded header is not the outer shape; 10 the constraints at zeta; 100 + c the embedded proof's code c (batch_eval_ref.verify_ref,
told the outer roots and [zeta, w_N zeta]).
CHECK 10 HERE: the oracle evaluates the constraint list on base-field rows only, not on extension-field openings, and it forms the table side from a trace, not from a
proof's multiplicities.  So this verifier decides check 10 against the HONEST proof of the same run (`honest`): the identity holds for the honest words, and since every
challenge is a hash of the words before it, it fails (up to 2^-100) as soon as a word the transcript observes before zeta, or an evaluation, differs from them."""
from __future__ import annotations

import numpy as np

import batch_eval_ref as bev
import lowdeg_ref as ld
from oracle import stark_api as so

P, GEN, U64 = ld.P, ld.GEN, ld.U64
MAGIC, VERSION = 0x52534B5A, 1
HEADER = 157
W_AUX = 40
MASKS = [3, 3, 1]
DEFAULT_QUERIES = {1: 50, 2: 25, 3: 17}
VIRTUAL = {0: [9, 10, 11] + list(range(57, 73)) + [161], 1: [9, 10, 11, 57]}       # logical columns the AIR reads as zero (not committed)


def f_inv(a: int) -> int:
    return pow(int(a), P - 2, P)


class Built:
    """what prove_ref computed on the way: the three matrices (uint32[width][M]), the roots, the challenges, the points"""


def stark_part(rows, pub, b: int, num_queries: int, pow_bits: int):
    """(the words up to the multiplicities' end with the 'ZKSR' header, the transcript after the multiplicities are NOT yet observed, logical matrix)"""
    base = so.prove(rows, pub)                                       # header, program and multiplicities do not depend on the rate
    at = so.proof_layout(base)
    head = base[:at["trace_root"]].copy()
    head[0], head[1], head[4], head[5], head[6] = MAGIC, VERSION, num_queries, b, pow_bits
    return head, at


def quotient(LL, AL, lk, pub, first, last, alpha, log_n: int, b: int) -> np.ndarray:
    """uint32[4][M]: Q on the coset, one so.constraints_eval_states call per row.  LL: the LOGICAL main columns over the coset (virtual columns zero), AL: the aux columns."""
    N, M = 1 << log_n, 1 << (log_n + b)
    w_n = ld.root_of_unity(log_n)
    x = ld.powers(ld.root_of_unity(log_n + b), M) * U64(GEN) % U64(P)
    w_last, w_inv = pow(w_n, pub.n_real - 1, P), f_inv(w_n)
    Q = np.zeros((4, M), np.uint32)
    for j in range(M):
        xj, jn = int(x[j]), (j + (1 << b)) % M
        zh = (pow(xj, N, P) - 1) % P
        is_first, is_last, is_trans = zh * f_inv(xj - 1) % P, zh * f_inv(xj - w_last) % P, (xj - w_inv) % P
        s = so.constraints_eval_states(LL[:, j], LL[:, jn], AL[:, j], AL[:, jn], lk, is_first, is_last, is_trans, pub, first, last, alpha)
        Q[:, j] = s.astype(U64) * U64(f_inv(zh)) % U64(P)
    return Q


def prove_ref(rows, pub, b: int, num_queries=None, pow_bits: int = 12, want_built: bool = False, challenges=None):
    """The 'ZKSR' proof of the executed `rows` (oracle.run's) under the oracle's public inputs `pub` (mode 0 or 1).  `challenges` = (alpha_l, lambda, alpha) replaces the
    transcript's draws (tests that compare quotients of different rates built with the same challenges); such a proof does not verify."""
    mode = int(pub.deferred)
    assert mode in (0, 1) and b in (1, 2, 3)
    nq = DEFAULT_QUERIES[b] if num_queries is None else int(num_queries)
    log_n = so.padded_log_n(pub.n_real)
    N = 1 << log_n
    head, at = stark_part(rows, pub, b, nq, pow_bits)
    matrix = so.main_trace(rows, pub)
    committed = so.to_committed(matrix, mode)
    L = np.stack([so.lde(c, b)[1] for c in committed])
    troot = so.merkle(L)
    ch = ld.Challenger()
    ch.observe_n(head[2:HEADER])
    ch.observe_n(troot)
    ch.observe_n(head[at["rom_mult"]:])
    alpha_l, lam = ch.sample_ext(), ch.sample_ext()
    if challenges is not None:
        alpha_l, lam = (np.asarray(c, np.uint32) for c in challenges[:2])
    aux, lk, rom, rc = so.lookup_setup(matrix, pub, alpha_l, lam)
    assert np.array_equal(np.concatenate([rom, rc]), head[at["rom_mult"]:])
    AL = np.stack([so.lde(c, b)[1] for c in aux])
    aroot = so.merkle(AL)
    ch.observe_n(aroot)
    alpha = ch.sample_ext()
    if challenges is not None:
        alpha = np.asarray(challenges[2], np.uint32)
    kept = [c for c in range(matrix.shape[0]) if c not in VIRTUAL[mode]]
    assert np.array_equal(committed, matrix[kept])
    LL = np.zeros((matrix.shape[0], N << b), np.uint32)
    LL[kept] = L
    first, last = matrix[so.STATE_COLS, 0], matrix[so.STATE_COLS, pub.n_real - 1]
    assert np.array_equal(np.concatenate([first, last]), head[21:HEADER])
    Q = quotient(LL, AL, lk, pub, first, last, alpha, log_n, b)
    qroot = so.merkle(Q)
    ch.observe_n(qroot)
    zeta = ch.sample_ext()
    zeta_w = (zeta.astype(U64) * U64(ld.root_of_unity(log_n)) % U64(P)).astype(np.uint32)
    points = np.stack([zeta, zeta_w])
    inner = bev.prove_ref([L, AL, Q], b, MASKS, points, nq, pow_bits)
    proof = np.concatenate([head, troot, aroot, qroot, inner]).astype(np.uint32)
    if not want_built:
        return proof
    bt = Built()
    bt.L, bt.AL, bt.Q, bt.roots, bt.points, bt.alpha_l, bt.lam, bt.alpha, bt.at_eval = L, AL, Q, np.concatenate([troot, aroot, qroot]), points, alpha_l, lam, alpha, len(head) + 12
    return proof, bt


_used = {}


def used_openings(mode: int) -> np.ndarray:
    """bool[2 WT + 4] over the embedded proof's evaluations (main | aux | quotient at zeta, main | aux at zeta w): does the constraint list read this opening?  Found with the
    oracle: so.constraints_eval_states on a random row pair, one column changed at a time (a column whose next-row value no constraint reads does not enter check 10)."""
    if mode in _used:
        return _used[mode]
    rng = np.random.default_rng(4242 + mode)
    blob = bytes(32)
    pub = so.public_inputs(64, blob, deferred=bool(mode))
    wl = so.logical_width(mode)
    kept = [c for c in range(wl) if c not in VIRTUAL[mode]]
    rows = [rng.integers(0, P, wl).astype(np.uint32), rng.integers(0, P, wl).astype(np.uint32), rng.integers(0, P, W_AUX).astype(np.uint32), rng.integers(0, P, W_AUX).astype(np.uint32)]
    rows[0][VIRTUAL[mode]] = 0; rows[1][VIRTUAL[mode]] = 0
    lk, first, last, alpha, sel = (rng.integers(1, P, k).astype(np.uint32) for k in (so.N_LK, 68, 68, 4, 3))

    def value(r):
        return so.constraints_eval_states(r[0], r[1], r[2], r[3], lk, sel[0], sel[1], sel[2], pub, first, last, alpha)
    base = value(rows)

    def reads(which, col):
        r = [x.copy() for x in rows]
        r[which][col] = (int(r[which][col]) + 1) % P
        return not np.array_equal(value(r), base)
    used = [reads(0, c) for c in kept] + [reads(2, c) for c in range(W_AUX)] + [True] * 4 + [reads(1, c) for c in kept] + [reads(3, c) for c in range(W_AUX)]
    _used[mode] = np.array(used)
    return _used[mode]


def layout(proof) -> dict:
    """word offsets of a well-formed proof: program, rom_mult, rc_mult, trace_root, aux_root, quotient_root, eval_proof; widths"""
    w = np.asarray(proof, np.uint32)
    blob_len = int(w[HEADER])
    blob_words = (blob_len + 1) // 2
    half = w[HEADER + 1:HEADER + 1 + blob_words]
    blob = np.stack([half & 0xFF, half >> 8], axis=1).astype(np.uint8).reshape(-1)[:blob_len].tobytes()
    n_rom = int.from_bytes(blob[16:20], "little") // 4
    rom = HEADER + 1 + blob_words
    troot = rom + n_rom + so.RC_TABLE
    return {"program": HEADER, "blob": blob, "rom_mult": rom, "rc_mult": rom + n_rom, "trace_root": troot, "aux_root": troot + 4, "quotient_root": troot + 8,
            "eval_proof": troot + 12, "widths": [int(w[3]), W_AUX, 4]}


def verify_ref(proof, expect, min_queries: int, min_pow_bits: int, honest) -> int:
    """zkir_verify_rate's verdict on `proof` (modes 0 and 1); `honest`: the honest proof of the same run at the same parameters (the module text: check 10)."""
    w = np.ascontiguousarray(proof, dtype=np.uint32).reshape(-1)
    n = len(w)
    if n < HEADER or int(w[0]) != MAGIC or int(w[9]) > 4 or int(w[1]) != VERSION:
        return 1
    log_n, mode, b = int(w[2]), int(w[9]), int(w[5])
    if mode > 2:
        return 2
    if mode == 2 and n < HEADER + 4:                                 # (a mode-2 header has four counter words more)
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
    n_real = int(w[7]) | (int(w[8]) << 30)
    entry = int(w[10]) | (int(w[11]) << 20) | (int(w[12]) << 40)
    if (w[21:HEADER] >= P).any():
        return 3
    if n_real == 0 or n_real > 1 << 26 or so.padded_log_n(n_real) != log_n:
        return 2
    if expect is not None and (expect.n_real != n_real or expect.deferred != mode or expect.entry != entry or [int(x) for x in expect.prog] != [int(x) for x in w[13:17]] or
                               [int(x) for x in expect.io] != [int(x) for x in w[17:21]]):
        return 6
    init = np.zeros(68, np.uint32)
    init[1:4] = w[10:13]
    if not np.array_equal(init, w[21:21 + 68]):
        return 7
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
    WM, WT = int(w[3]), int(w[3]) + W_AUX
    e = w[p:]
    at_ev, n_ev = 15 + 12 + 8, 2 * WT + 4
    if len(e) < at_ev + 4 * n_ev:
        return 4
    shape = [bev.MAGIC, 1, log_n, b, 3, 2, int(w[4]), int(w[6]), int(e[8]), WM, 3, W_AUX, 3, 4, 1]
    if [int(x) for x in e[:15]] != shape:
        return 5
    h = np.asarray(honest, np.uint32)
    used = np.repeat(used_openings(mode), 4)                            # (an opening no constraint reads does not enter the identity: the embedded proof answers for it)
    if len(h) < p + at_ev + 4 * n_ev or not np.array_equal(w[2:p], h[2:p]) or not np.array_equal(e[at_ev:at_ev + 4 * n_ev][used], h[p + at_ev:p + at_ev + 4 * n_ev][used]):
        return 10
    c = bev.verify_ref(e, roots=roots, points=np.stack([zeta, zeta_w]))
    return 100 + c if c else 0

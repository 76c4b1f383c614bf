"""Shared inputs of tests/test_verify_query_stage.py (host) and tests/test_gpu_verify_queries_device.py (device): small oracle proofs of every mode at padded log_n 3 .. 7,
where a query sits in a proof, and the mutation lists whose verdicts both files compare.  Not a test module."""
import functools

import numpy as np

from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec, stark

P = so.P
ROWS = {3: 8, 4: 16, 5: 30, 6: 60, 7: 100}                       # executed rows of fib_endless -> padded log_n (asserted in oracle_proof)
SCHEDULES = {3: [1], 4: [1, 1], 5: [1, 2], 6: [1, 3], 7: [1, 3, 1]}      # fri_shape.h's fri_schedule(log_n, 1): one layer only, every last-step width, a middle 8-to-1 layer
MODE_ARGS = {0: {}, 1: {"deferred": True}, 2: {"io_mode": True}, 3: {"mem_mode": True}, 4: {"wide_mode": True}}


def pub_c_of(pub, num_queries=0, pow_bits=0):
    """the oracle's public inputs in the product's form"""
    c = rt.PublicInputsC(pub.n_real, pub.entry, pub.deferred, (int(num_queries) & 0xFFFF) | (int(pow_bits) << 16))
    c.program_digest[:] = list(pub.prog); c.io_digest[:] = list(pub.io)
    return c


@functools.lru_cache(maxsize=None)
def oracle_proof(mode, log_n, num_queries=0, pow_bits=0):
    """(proof, its public inputs): a fib_endless run of ROWS[log_n] rows proven by the oracle in `mode`"""
    blob = spec.fib_endless_program().to_bytes()
    res = oracle.run(blob, max_cycles=ROWS[log_n], enable_execution_trace=True, enable_deferred_model=(mode == 1))
    pub = so.public_inputs(len(res.rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code), num_queries=num_queries, pow_bits=pow_bits, **MODE_ARGS[mode])
    proof = so.prove(res.rows, pub)
    assert int(proof[9]) == mode and int(proof[2]) == log_n == stark.padded_log_n(len(res.rows)), (mode, log_n, int(proof[2]))
    return proof, pub_c_of(pub, num_queries, pow_bits)


def query_layout(proof):
    """Where the queries of an HONEST proof sit.  The aux width is not a header word: it is the one value that makes the proof's length come out (checked: the layer-count
    word then stands where it must).  records: the offsets inside a query at which a record starts — the index word, main / aux / quotient at q and q + N, the layers — and
    the query's end."""
    lay = stark.proof_layout(proof)
    log_n, WM, nq = int(proof[2]), int(proof[3]), int(proof[4])
    ks, d = SCHEDULES[log_n], log_n + 1
    fri, log_m = 0, d
    for k in ks:
        fri += 4 * (1 << k) + 4 * (log_m - k); log_m -= k
    fixed = lay["openings"] + 8 * WM + 16 + 1 + 4 * len(ks) + 32 + 1 + nq * (1 + 2 * WM + 8 + 24 * d + fri)
    WA, rem = divmod(len(proof) - fixed, 8 + 2 * nq)
    assert rem == 0 and WA > 0
    at_layers = lay["openings"] + 4 * (2 * (WM + WA) + 4)
    assert int(proof[at_layers]) == len(ks)
    at_queries = at_layers + 1 + 4 * len(ks) + 32 + 1
    qsize = 1 + 2 * (WM + 4 * d) + 2 * (WA + 4 * d) + 2 * (4 + 4 * d) + fri
    assert at_queries + nq * qsize == len(proof)
    records, off = [0], 1
    for width in (WM, WM, WA, WA, 4, 4):
        records.append(off); off += width + 4 * d
    log_m = d
    for k in ks:
        records.append(off); off += 4 * (1 << k) + 4 * (log_m - k); log_m -= k
    records.append(off)
    assert off == qsize
    return {"trace_root": lay["trace_root"], "layer_roots": at_layers + 1, "n_layers": len(ks), "at_queries": at_queries, "qsize": qsize, "num_queries": nq, "WM": WM, "WA": WA,
            "depth": d, "records": records, "tables_words": nq + 4 * (2 * (WM + WA) + 4) + 4 * len(ks) + 12 * len(ks)}


def bump(proof, pos):
    t = proof.copy(); t[pos] = (int(t[pos]) + 1) % P
    return t


BUMP_CHUNKS = 16                                                 # a host verification of these proofs is 7 - 10 ms (the table side): a query's ~600 - 1000 words go in 16 cases


def query_bumps(proof, t, chunk=None):
    """every word of query t (-1: the last one) bumped by one (mod p); chunk c of BUMP_CHUNKS: words c, c + BUMP_CHUNKS, .. (every chunk crosses every record)"""
    q = query_layout(proof)
    a = q["at_queries"] + (t % q["num_queries"]) * q["qsize"]
    words = range(q["qsize"]) if chunk is None else range(chunk, q["qsize"], BUMP_CHUNKS)
    return [(f"query {t} word {k}", bump(proof, a + k)) for k in words]


def record_bumps(proof, t):
    """the first word of every record of query t bumped: a part of query_bumps(proof, t) that already meets every check a query word can fail"""
    q = query_layout(proof)
    a = q["at_queries"] + (t % q["num_queries"]) * q["qsize"]
    return [(f"query {t} record {r}", bump(proof, a + r)) for r in q["records"][:-1]]


def other_mutants(proof):
    """the three roots and every layer root bumped (every word), one trailing word, cuts at every record boundary of the last query, in the middle of a record, inside a
    middle query"""
    q = query_layout(proof)
    out = [(f"root word {k}", bump(proof, q["trace_root"] + k)) for k in range(12)]
    out += [(f"layer root word {k}", bump(proof, q["layer_roots"] + k)) for k in range(4 * q["n_layers"])]
    out.append(("trailing word", np.concatenate([proof, np.zeros(1, np.uint32)])))
    last = q["at_queries"] + (q["num_queries"] - 1) * q["qsize"]
    for r in q["records"][:-1]:
        out.append((f"cut at record {r} of the last query", proof[:last + r]))
    out.append(("cut inside a main record", proof[:last + q["records"][1] + 3]))
    out.append(("cut inside a path", proof[:last + q["records"][4] - 2]))
    out.append(("cut inside a layer", proof[:last + q["records"][7] + 5]))
    out.append(("cut in a middle query", proof[:q["at_queries"] + (q["num_queries"] // 2) * q["qsize"] + q["records"][3] + 1]))
    out.append(("cut before query 0's first record", proof[:q["at_queries"] + 1]))
    out.append(("cut at query 0", proof[:q["at_queries"]]))
    return out


MUTANT_PROOFS = [(0, 5), (4, 4)]                                 # (mode, log_n) of the two proofs the mutation lists are made of
WANTED_CODES = {4, 20, 21, 22, 23, 27, 30}                       # check_query's: an index word, a word of each matrix's row, a layer value, a cut, a trailing word


@functools.lru_cache(maxsize=None)
def segments(n_total, seg_rows, mode=0):
    """tests/test_stark_oracle.py::_segments: a fib_endless run cut into segments that overlap by one row -> (the run's public inputs, [proofs])"""
    blob = spec.fib_endless_program().to_bytes()
    res = oracle.run(blob, max_cycles=n_total, enable_execution_trace=True)
    rows = res.rows
    cuts, a = [], 0
    while a < len(rows) - 1:
        b = min(a + seg_rows, len(rows))
        cuts.append((a, b)); a = b - 1
    args = MODE_ARGS[mode]
    full = so.public_inputs(len(rows), blob, [], list(res.outputs), (res.halt_kind, res.halt_code), **args)
    proofs = []
    for a, b in cuts:
        pub = so.public_inputs(b - a, blob, [], list(res.outputs), (res.halt_kind, res.halt_code), **args)
        pub.io[:] = full.io[:]                                   # every segment carries the RUN's io digest
        proofs.append(so.prove(rows[a:b], pub))
    return pub_c_of(full), proofs


def chain_cases(n_total, seg_rows):
    """[(what, proofs, expect)] around one honest chain: honest with and without expect, first segment dropped, two swapped, wrong expectations, a bumped row word in each
    segment's last query, a bumped header word in segment 1 beside a bumped query word in segment 0"""
    full, proofs = segments(n_total, seg_rows)
    out = [("honest", proofs, full), ("honest, no expect", proofs, None), ("first dropped", proofs[1:], None), ("swapped", [proofs[1], proofs[0]] + proofs[2:], None)]
    wrong = rt.PublicInputsC.from_buffer_copy(full); wrong.n_real = full.n_real + 1
    other = rt.PublicInputsC.from_buffer_copy(full); other.program_digest[0] ^= 1
    out += [("wrong row count", proofs, wrong), ("wrong program", proofs, other)]
    for i, p in enumerate(proofs):
        q = query_layout(p)
        t = bump(p, q["at_queries"] + (q["num_queries"] - 1) * q["qsize"] + q["records"][1] + 2)
        out.append((f"row word of segment {i}", proofs[:i] + [t] + proofs[i + 1:], None))
    q0 = query_layout(proofs[0])
    out.append(("header of segment 1, query of segment 0", [bump(proofs[0], q0["at_queries"] + q0["records"][3]), bump(proofs[1], 7)] + proofs[2:], None))
    return out

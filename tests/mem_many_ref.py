"""The reference and the corpus for the memory stages over a LIST of proofs (zkir_mem_sections_stage_*, zkir_verify_many_memory_*, zkir_verify_rate_many_memory_*):
per section the verdict, chunk digests and sum are tests/mem_stage_ref.py's, and a batch's answer is the list of its sections' answers — nothing of one section may
reach another.  The proofs are the oracle prover's (and the two frozen 'ZKSR' proofs); the expected verdict of every proof is the single-proof host verifier's."""
import functools

import numpy as np

import mem_stage_ref as M
import programs as pg
import test_gpu_verify_memory_device as tm
import test_prove_rate_modes_verify as RM
from oracle import api as oracle, stark_api as so
from zkir_amd import stark

P = so.P


# ---- the list stage ------------------------------------------------------------------------------------------------------------------------------------------------------
def stage_ref(secs, modes, code_words, blobs, alphas, lams):
    """(verdicts, digests per section [chunks][4], sums [n][4]) — digests and sum are zero where the verdict is not 0, as the entries return them"""
    verdicts, digests, sums = [], [], []
    for sec, mode, nc, blob, a, l in zip(secs, modes, code_words, blobs, alphas, lams):
        v = M.section_verdict(sec, mode, nc)
        verdicts.append(v)
        n_chunks = (len(sec) + 511) // 512
        digests.append(M.chunk_digests(sec) if v == 0 else [[0, 0, 0, 0]] * n_chunks)
        sums.append([int(x) for x in M.table_side(sec, blob, a, l)] if v == 0 else [0, 0, 0, 0])
    return verdicts, digests, sums


def challenge(seed):
    """a canonical E4 nobody derived from the data, another one per seed"""
    rng = np.random.default_rng(1000 + seed)
    return [int(x) for x in rng.integers(0, P, 4)]


def batch(sections, seed=0):
    """a batch over the given sections with a DIFFERENT mode, code size, alpha, lambda and blob per section: (secs, modes, code_words, blobs, alphas, lams).  Every blob has at most
    7 code words and at least 64 data bytes: cells from 0x1000 + 64 on lie behind the code, the first ones inside the image."""
    rng = np.random.default_rng(seed)
    secs, modes, code_words, blobs, alphas, lams = [], [], [], [], [], []
    for i, sec in enumerate(sections):
        n_code = 3 + (i % 5)
        code = bytes(rng.integers(1, 256, 4 * n_code, dtype=np.uint8))
        data = bytes(rng.integers(1, 256, 64 + 3 * i, dtype=np.uint8))
        secs.append(np.ascontiguousarray(sec, dtype=np.uint32)); modes.append(3 + (i & 1)); code_words.append(n_code); blobs.append(M.make_blob(code, data))
        alphas.append(challenge(2 * i + 100 * seed)); lams.append(challenge(2 * i + 1 + 100 * seed))
    return secs, modes, code_words, blobs, alphas, lams


def sizes_sections(order):
    """one well-formed section per entry of M.SIZES, in the given order of indices; the cells start at 0x1000 + 64 (inside the blobs' data, behind their code)"""
    return [M.section(M.increasing(M.SIZES[k], seed=40 + k, start=0x1000 + 64)) for k in order]


SIZES_ORDERS = [list(range(len(M.SIZES))), list(reversed(range(len(M.SIZES)))), [3, 0, 7, 1, 6, 2, 5, 4]]


def assert_stage(got, want, what=""):
    gv, gd, gs = got
    wv, wd, ws = want
    assert list(gv) == list(wv), (what, gv, wv)
    for i, (a, b) in enumerate(zip(gd, wd)):
        assert np.asarray(a, dtype=np.int64).tolist() == np.asarray(b, dtype=np.int64).tolist(), (what, "digests of section", i)
    assert np.asarray(gs, dtype=np.int64).tolist() == np.asarray(ws, dtype=np.int64).tolist(), (what, "sums")


# ---- the corpus of proofs ------------------------------------------------------------------------------------------------------------------------------------------------
def count_word(proof, rate=False):
    """the count word of a proof's touched-cell section (0: the proof has none)"""
    if int(proof[9]) < 3:
        return 0
    lay = stark.rate_proof_layout(proof) if rate else stark.proof_layout(proof)
    return int(proof[lay["mem_section"]])


@functools.lru_cache(maxsize=None)
def honest_corpus():
    """[(what, proof, public inputs)]: the honest oracle proofs of loads_stores, pc_carry_mem and edge_bc_alias_ok in modes 3 and 4 (mode-3 edge_bc_alias_ok is refused with
    55), sha256_hello in mode 4, fib30 in mode 0 and in mode 3 with no touched cell"""
    out = []
    for mode in (3, 4):
        for name in ("loads_stores", "pc_carry_mem", "edge_bc_alias_ok"):
            proof, pub = tm._oracle_case(name, mode)
            out.append((f"{name} mode {mode}", proof, pub))
    proof, pub = tm._oracle_case("sha256_hello", 4)
    out.append(("sha256_hello mode 4", proof, pub))
    blob, ins, cfg = pg.off_code("fib30")
    ores = oracle.run(blob, list(ins), enable_execution_trace=True)
    for mem_mode in (False, True):
        pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=mem_mode)
        out.append((f"fib30 mode {3 if mem_mode else 0}", so.prove(ores.rows, pub), RM.pub_c(pub)))
    return out


def located_cells(proof, at):
    """the cells of the section at word `at` as a list entry takes them: the count word, where it is 1 .. 2^28 and 1 + 7 n words lie behind it"""
    n = int(proof[at])
    return n if 1 <= n <= 1 << 28 and at + 1 + 7 * n <= len(proof) else 0


@functools.lru_cache(maxsize=None)
def mutants():
    """test_gpu_verify_memory_device.mutations(): [(what, proof)] with the honest proof first"""
    return tm.mutations()


RATE_MUTATION_SEED = 0      # chosen with the host verifier alone (rt.verify_rate on a CPU, seeds 0, 1, ..: the first whose codes over both proofs include 10 and 54)
RATE_MUTATION_CODES = {4, 5, 10, 54, 56}      # the host's codes on it.  A 'ZKSR' front has no grinding before check 10: a changed time or byte of a cell reaches the check
                                              # itself; a changed COUNT word moves everything behind the section (4, 5, 56) — and the front's section is not the located one


@functools.lru_cache(maxsize=None)
def rate_corpus(seed=None):
    """[(what, proof, public inputs, min_queries, min_pow_bits, the section's offset)]: the two frozen 'ZKSR' proofs and ~20 single-word mutants of each one's memory
    section (the count word among them)"""
    out = []
    rng = np.random.default_rng(RATE_MUTATION_SEED if seed is None else seed)
    for key in RM.KEYS:
        proof, opub, rows, b, nq, bits = RM.golden(key)
        pub = RM.pub_c(opub)
        at = stark.rate_proof_layout(proof)["mem_section"]
        n = int(proof[at])
        out.append((f"{key} honest", proof, pub, nq, bits, at))
        for trial in range(20):
            pos = at + int(rng.integers(0, 1 + 7 * n))
            old = int(proof[pos])
            new = [0, 1, 8, 0x1000, 1 << 16, 1 << 20, P - 1, (old + 1) % P, (old + 8) % P][int(rng.integers(0, 9))]
            if new == old:
                continue
            t = proof.copy(); t[pos] = new
            out.append((f"{key} word {pos}: {old} -> {new}", t, pub, nq, bits, at))
    return out

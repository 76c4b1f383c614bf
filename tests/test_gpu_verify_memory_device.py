"""zkir_verify_memory_device / zkir_verify_rate_memory_device: the verifier with the touched-cell section's three stages (cell checks, chunk digests, the cells' share of
the table side — csrc/mem_stage.inl) on the GPU gives zkir_verify's / zkir_verify_rate's verdict on honest mode-3 and mode-4 proofs and on mutated ones, reports what it
ran, and leaves every existing entry as it was.  The chunk digests have no entry of their own: an accepted proof shows them right (a wrong digest changes every challenge
behind it), and mutated section words show them following the words."""
import functools

import numpy as np
import pytest

import mem_stage_ref as M
import programs as pg
import test_prove_rate_modes_verify as RM
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec, stark

pytestmark = pytest.mark.gpu

NONE = {"cells": 0, "launches": 0, "uploaded_words": 0}


@pytest.fixture(autouse=True)
def _every_section_on_the_device(monkeypatch):
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", "0")       # (whatever the default routing of small sections is: these tests are about the device stages)
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")


@functools.lru_cache(maxsize=None)
def _oracle_case(name, mode):
    blob, ins, cfg = pg.off_code(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **{k: v for k, v in cfg.items() if k == "max_cycles"})
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=mode == 3, wide_mode=mode == 4)
    return so.prove(ores.rows, pub), RM.pub_c(pub)


def _both_ways(proof, pub=None):
    """the new entry with and without the query stage; returns the verdict both gave and what the second reported"""
    a = rt.verify(proof, pub, device=True, memory=True)
    last_a, stages_a = rt.verify_memory_last(), rt.verify_last_stages()["device_stages"]
    b = rt.verify(proof, pub, device=True, memory=True, queries=True)
    assert a == b, (a, b)
    assert rt.verify_memory_last() == last_a and rt.verify_last_stages()["device_stages"] == stages_a
    return a, last_a, stages_a


@pytest.mark.parametrize("name,mode", [(n, m) for m in (3, 4) for n in ("loads_stores", "pc_carry_mem", "sha256_hello", "edge_bc_alias_ok") if (n, m) != ("sha256_hello", 3)])
def test_honest_oracle_proofs_are_accepted(name, mode):      # (a hash call has no mode-3 proof)
    proof, pub = _oracle_case(name, mode)
    lay = stark.proof_layout(proof)
    n = int(proof[lay["mem_section"]])
    assert lay["mode"] == mode and n > 0
    if (name, mode) == ("edge_bc_alias_ok", 3):                 # the run touches the boundary cell, which only mode 4 admits: the honest proof is refused by the cell checks
        assert rt.verify(proof, pub) == 55
        code, last, stages = _both_ways(proof, pub)
        assert code == 55 and last["cells"] == n and last["launches"] == 1 and stages == 1
        return
    assert rt.verify(proof, pub) == 0
    code, last, stages = _both_ways(proof, pub)
    assert code == 0
    assert last["cells"] == n and last["launches"] == 3 and last["uploaded_words"] >= 1 + 7 * n and stages >= 3
    # the stage's digests are the section's: the reference sponge over the proof's own words
    sec = proof[lay["mem_section"]:lay["mem_section"] + 1 + 7 * n]
    assert M.section_verdict(sec, mode, lay["n_rom"]) == 0 and len(M.chunk_digests(sec)) == (len(sec) + 511) // 512
    # existing entries: a mode-3 proof's front stays on the host
    if mode == 3:
        assert rt.verify(proof, pub, device=True) == 0
        assert rt.verify_last_stages()["device_stages"] == 0 and rt.verify_memory_last() == NONE
        assert rt.verify(proof, pub, device=True, queries=True) == 0
        assert rt.verify_last_stages()["device_stages"] == 0 and rt.verify_memory_last() == NONE


def test_a_proof_without_a_memory_section_takes_the_existing_entry():
    blob, ins, cfg = pg.off_code("fib30")
    ores = oracle.run(blob, list(ins), enable_execution_trace=True)
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code))
    proof = so.prove(ores.rows, pub)
    assert int(proof[9]) == 0
    code, last, stages = _both_ways(proof, RM.pub_c(pub))
    assert code == 0 and last == NONE and stages == 0
    # a mode-3 proof with NO touched cell: the host stage, no device memory
    pub3 = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=True)
    p3 = so.prove(ores.rows, pub3)
    assert int(p3[9]) == 3 and int(p3[stark.proof_layout(p3)["mem_section"]]) == 0
    code, last, stages = _both_ways(p3, RM.pub_c(pub3))
    assert code == 0 and last == NONE and stages == 0


def test_the_threshold_leaves_small_sections_to_the_host(monkeypatch):
    proof, pub = _oracle_case("loads_stores", 3)
    n = int(proof[stark.proof_layout(proof)["mem_section"]])
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", str(n + 1))
    assert rt.verify(proof, pub, device=True, memory=True) == 0 and rt.verify_memory_last() == NONE and rt.verify_last_stages()["device_stages"] == 0
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", str(n))
    assert rt.verify(proof, pub, device=True, memory=True) == 0 and rt.verify_memory_last()["cells"] == n
    monkeypatch.delenv("ZKIR_VERIFY_DEVICE_MIN_CELLS")              # .. and with the default routing
    assert rt.verify(proof, pub, device=True, memory=True) == 0


def test_the_gpu_provers_array_loop():
    """the GPU prover's mode-3 proof of spec.memory_loop_program: 300 cells, ~3900 rows, a section of five chunks"""
    from zkir_amd import pipeline as pl
    blob = spec.memory_loop_program(300).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="device")
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    lay = stark.proof_layout(proof)
    assert int(proof[9]) == 3 and int(proof[lay["mem_section"]]) == 300 and log.n_rows > 3000
    assert rt.verify(proof, pub) == 0
    code, last, stages = _both_ways(proof, pub)
    assert code == 0 and last["cells"] == 300 and stages == 3
    t = proof.copy(); t[lay["mem_section"] + 1 + 7 * 299 + 2] ^= 1      # the last cell's time: the digests change, so every challenge does
    assert _both_ways(t, pub)[0] == rt.verify(t, pub) != 0
    log.close()


MUTATION_SEED = 12                                              # chosen with the host verifier alone (rt.verify on a CPU, seeds 0, 1, ..: the first whose codes include 4, 54, 55 and
MUTATION_CODES = {3, 4, 8, 12, 21, 22, 23, 27, 54, 55}          # 12 — a changed section word changes the transcript, and the grinding check fails first); the host's codes on it


def mutations(seed=None):
    """[(what, proof words)]: the random mode-4 program of tests/test_gpu_verify_device.py (seed 3, hashes on), ~150 single-word mutations with edge values — half inside
    the touched-cell section [mem_section, hash_section) — and cuts at the section's start, inside its first cell, behind it and at its end"""
    blob, ins = pg.random_program(3, n_instr=200, hashes=True, wide_safe=True)
    ores = oracle.run(blob, ins, max_cycles=600, enable_execution_trace=True)
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    proof = so.prove(ores.rows, pub)
    lay = stark.proof_layout(proof)
    assert lay["mode"] == 4 and lay["hash_section"] - lay["mem_section"] > 7 * 8
    rng = np.random.default_rng(MUTATION_SEED if seed is None else seed)
    out = [("honest", proof)]
    for trial in range(150):
        pos = int(rng.integers(lay["mem_section"], lay["hash_section"])) if trial % 2 == 0 else int(rng.integers(0, len(proof)))
        old = int(proof[pos])
        new = [0, 1, 8, 0x1000, 0x1008, 1 << 16, 1 << 20, so.P - 1, 0xFFFFFFFF, (old + 1) % so.P, (old + 8) % so.P, int(rng.integers(0, so.P))][int(rng.integers(0, 12))]
        if new == old:
            continue
        t = proof.copy(); t[pos] = new
        out.append((f"word {pos}: {old} -> {new}", t))
    for cut in (lay["mem_section"], lay["mem_section"] + 1, lay["mem_section"] + 7, lay["mem_section"] + 8, lay["hash_section"] - 1, lay["hash_section"]):
        out.append((f"cut at {cut}", proof[:cut]))
    return out


def test_mutated_proofs_get_the_host_verdict():
    muts = mutations()
    assert muts[0][0] == "honest" and rt.verify(muts[0][1]) == 0 == _both_ways(muts[0][1])[0]
    codes = set()
    for what, t in muts[1:]:
        host = rt.verify(t)
        assert host != 0, ("a mutated proof was accepted", what)
        dev = _both_ways(t)[0]
        assert dev == host, ("the device form disagrees", what, dev, host)
        codes.add(host)
    assert codes == MUTATION_CODES and {4, 54, 55, 12} <= codes, codes


@pytest.mark.parametrize("key", RM.KEYS)
def test_rate_proofs_get_the_host_verdict(key):
    """the two frozen 'ZKSR' proofs (modes 3 and 4) and single-word mutants of their memory sections"""
    proof, opub, rows, b, nq, bits = RM.golden(key)
    pub = RM.pub_c(opub)
    at = stark.rate_proof_layout(proof)
    n = int(proof[at["mem_section"]])
    assert n > 0
    assert rt.verify_rate(proof, pub, nq, bits) == 0
    assert rt.verify_rate(proof, pub, nq, bits, device=True, memory=True) == 0
    assert rt.verify_memory_last()["cells"] == n and rt.verify_memory_last()["launches"] == 3 and rt.verify_last_stages()["device_stages"] >= 3
    assert rt.verify_rate(proof, pub, nq + 1, bits, device=True, memory=True) == 2
    if key == "mode3":                                          # the existing entry: the front on the host
        assert rt.verify_rate(proof, pub, nq, bits, device=True) == 0 and rt.verify_last_stages()["device_stages"] == 0 and rt.verify_memory_last() == NONE
    rng = np.random.default_rng(5)
    codes = set()
    for trial in range(40):
        pos = at["mem_section"] + int(rng.integers(0, 1 + 7 * n))
        old = int(proof[pos])
        new = [0, 1, 8, 0x1000, 0x1008, 1 << 16, 1 << 20, so.P - 1, (old + 1) % so.P, (old + 8) % so.P][int(rng.integers(0, 10))]
        if new == old:
            continue
        t = proof.copy(); t[pos] = new
        host = rt.verify_rate(t, pub, nq, bits)
        assert host != 0 and rt.verify_rate(t, pub, nq, bits, device=True, memory=True) == host, (pos, old, new, host)
        codes.add(host)
    assert 54 in codes, codes

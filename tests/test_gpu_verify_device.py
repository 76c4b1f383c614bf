"""zkir_verify_device: zkir_verify with a mode-4 proof's tape stages — the record checks, the sections' chunk digests, the tapes' share of the lookup table side with
every hash call's digest recomputed (hash_tape_new_bytes_kernel) — on the GPU.  The verdict is the host verifier's for every input: accepted proofs, single-word
mutations (half of them inside the tapes), truncations at the section boundaries, forged tapes.  No test here provokes a device fault: a malformed tape is stopped by
the record checks before any kernel that trusts it runs, which is what equal verdicts on the mutations show."""
import functools

import numpy as np
import pytest

import programs as pg
import tape_side_ref as R
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt, spec, stark

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def _every_tape_on_the_device(monkeypatch):
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")      # (whatever the default routing of short tapes is: these tests are about the device stages)


@functools.lru_cache(maxsize=None)
def _mode4_proof(name):
    """(proof, public inputs) from the GPU prover, the witness and the tape built on the device"""
    from zkir_amd import pipeline as pl
    blob, ins, cfg = R.real_program(name)
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob, list(ins), wide_mode=True, hash_witness="device")
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    return proof, pub


@functools.lru_cache(maxsize=None)
def _oracle_case(name, **mode):
    """(proof, the oracle's public inputs in the product's form)"""
    blob, ins, cfg = pg.off_code(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **{k: v for k, v in cfg.items() if k == "max_cycles"})
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), **mode)
    pub_c = rt.PublicInputsC(pub.n_real, pub.entry, pub.deferred, 0)
    pub_c.program_digest[:] = list(pub.prog); pub_c.io_digest[:] = list(pub.io)
    return so.prove(ores.rows, pub), pub_c


def _oracle_proof(name, **mode):
    return _oracle_case(name, **mode)[0]


@pytest.mark.parametrize("name", ["sha256_hello", "hashes_all", "hash_edge_calls", "signed_division_loop", "wide_and_hash", "sha_chain_2p12"])
def test_honest_mode4_proofs_are_accepted_by_both(name, monkeypatch):
    proof, pub = _mode4_proof(name)
    lay = stark.proof_layout(proof)
    assert lay["mode"] == 4 and int(proof[lay["hash_section"]]) + int(proof[lay["wide_section"]]) > 0
    assert rt.verify(proof, pub, device=True) == rt.verify(proof, pub) == 0
    assert rt.verify(proof, device=True) == rt.verify(proof) == 0
    assert rt.verify_last_stages()["device_stages"] == 0                               # (the last call was the host's)
    assert rt.verify(proof, device=True) == 0 and rt.verify_last_stages()["device_stages"] >= 3
    monkeypatch.delenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS")                               # .. and with the default routing
    assert rt.verify(proof, pub, device=True) == 0


@pytest.mark.parametrize("mode", [0, 3])
def test_modes_without_tapes_are_the_host_verifier(mode):
    proof, pub = _oracle_case("fib30", **({"mem_mode": True} if mode == 3 else {}))
    assert int(proof[9]) == mode
    assert rt.verify(proof, pub, device=True) == rt.verify(proof, pub) == 0
    assert rt.verify(proof, device=True) == rt.verify(proof) == 0
    other = rt.PublicInputsC(pub.n_real + 1, pub.entry_point, pub.deferred, 0)               # public inputs of another run: refused alike
    other.program_digest[:] = list(pub.program_digest); other.io_digest[:] = list(pub.io_digest)
    assert rt.verify(proof, other, device=True) == rt.verify(proof, other) != 0
    t = proof.copy(); t[len(t) // 2] = (int(t[len(t) // 2]) + 1) % so.P
    assert rt.verify(t, device=True) == rt.verify(t) != 0


def test_the_host_path_stays_host_only():
    """a mode-4 proof with both tapes empty, and a mode-0 proof: accepted, and no stage ran on the device"""
    p4 = _oracle_proof("fib30", wide_mode=True)
    lay = stark.proof_layout(p4)
    assert lay["mode"] == 4 and int(p4[lay["hash_section"]]) == 0 and int(p4[lay["wide_section"]]) == 0
    for proof in (p4, _oracle_proof("fib30")):
        assert rt.verify(proof, device=True) == 0
        assert rt.verify_last_stages()["device_stages"] == 0
    proof, _ = _mode4_proof("sha256_hello")                                            # (the counter does count: a proof with a tape)
    assert rt.verify(proof, device=True) == 0 and rt.verify_last_stages()["device_stages"] > 0


MUTATION_SEED = 36                                              # chosen with the host verifier alone: its codes on these mutations include 4, 10, 56 and 57 (a mutated tape
                                                                # word changes the transcript and fails the grinding check, 12, first: 10 needs the draw that passes it)


def mutations():
    """[(what, proof words)]: the random program of test_mutated_mode4_proofs_are_rejected_by_both_verifiers_alike (seed 3, hashes on), ~150 single-word mutations with that
    test's edge values — half inside the hash and wide sections — and its truncations at the section boundaries"""
    blob, ins = pg.random_program(3, n_instr=200, hashes=True, wide_safe=True)
    ores = oracle.run(blob, ins, max_cycles=600, enable_execution_trace=True)
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    proof = so.prove(ores.rows, pub)
    lay = stark.proof_layout(proof)
    assert lay["mode"] == 4 and lay["rom_mult"] - lay["hash_section"] > 100
    rng = np.random.default_rng(MUTATION_SEED)
    out = [("honest", proof)]
    for trial in range(150):
        pos = int(rng.integers(lay["hash_section"], lay["rom_mult"])) if trial % 2 == 0 else int(rng.integers(0, len(proof)))
        old = int(proof[pos])
        new = [0, 1, 1 << 16, 1 << 20, so.P - 1, 0xFFFFFFFF, (old + 1) % so.P, int(rng.integers(0, so.P))][int(rng.integers(0, 8))]
        if new == old:
            continue
        t = proof.copy(); t[pos] = new
        out.append((f"word {pos}: {old} -> {new}", t))
    t = proof.copy(); t[lay["wide_section"]] = so.P - 1                                 # the wide tape's count word above the row count
    out.append(("wide count", t))
    for cut in (lay["mem_section"] + 1, lay["hash_section"], lay["hash_section"] + 1, lay["hash_section"] + 9, lay["wide_section"], lay["wide_section"] + 1, lay["rom_mult"] - 1, len(proof) - 1):
        out.append((f"cut at {cut}", proof[:cut]))
    return out


def test_mutated_proofs_get_the_host_verdict():
    muts = mutations()
    assert muts[0][0] == "honest" and rt.verify(muts[0][1]) == 0 == rt.verify(muts[0][1], device=True)
    codes = {}
    for what, t in muts[1:]:
        host = rt.verify(t)
        assert host != 0, ("a mutated proof was accepted", what)
        dev = rt.verify(t, device=True)
        assert dev == host, ("the device form disagrees", what, dev, host)
        codes[host] = codes.get(host, 0) + 1
    assert {4, 10, 56, 57} <= set(codes), codes


@functools.lru_cache(maxsize=None)
def _chain():
    """the SHA chain's matrix, touched cells and honest tape (a short run: the cases need its fourth record only), computed once for the forged-tape cases"""
    blob = spec.sha256_chain_program().to_bytes()
    ores = oracle.run(blob, [], max_cycles=200, enable_execution_trace=True)
    pub = so.public_inputs(len(ores.rows), blob, [], list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    hs = so.hash_section(ores.rows, pub)
    rec = 1 + 3 * (8 + 5 * int(hs[1 + 7]))                                              # the fourth record (every record of the chain is 8 + 5 x 8 words)
    assert int(hs[0]) > 8 and int(hs[rec + 6]) == 3 and int(hs[rec + 7]) == 8
    return so.main_trace(ores.rows, pub), pub, so.mem_cells(ores.rows, pub), hs, rec


FORGED = {"honest": 0, "message bit": 10, "length": 10, "kind": 10, "future time": 56, "earlier time": 10, "dropped record": 10, "order": 56}


@pytest.mark.parametrize("case", list(FORGED))
def test_forged_hash_tapes_get_the_oracles_verdicts(case):
    """test_a_forged_hash_tape_is_rejected's cases, rebuilt as that test does (set_hash_calls + prove_matrix_mem): both product verifiers give the oracle's verdict."""
    M, pub, cells, hs, rec = _chain()
    t = hs.copy()
    if case == "message bit":
        t[rec + 8 + 5 * 1 + 1] ^= 1
    elif case == "length":
        t[rec + 3] = int(t[rec + 3]) - 1
    elif case == "kind":
        t[rec + 6] = 5
    elif case == "future time":
        t[rec + 8] = int(t[rec]) + 1
    elif case == "earlier time":
        t[rec + 8] = int(t[rec + 8]) - 1
    elif case == "dropped record":
        t = np.concatenate([[int(hs[0]) - 1], hs[1:rec], hs[rec + 48:]]).astype(np.uint32)
    elif case == "order":
        t[rec] = int(t[rec - 48])
    so.set_hash_calls(t)
    try:
        pr = so.prove_matrix_mem(M, pub, cells)
    finally:
        so.set_hash_calls(None)
    want = FORGED[case]
    assert so.verify(pr, None) == want
    assert rt.verify(pr) == want and rt.verify(pr, device=True) == want

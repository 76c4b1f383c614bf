"""zkir_mem_sections_stage_launch, zkir_verify_many_memory_device and zkir_verify_rate_many_memory_device (csrc/mem_stage_many.inl): the memory sections of MANY proofs
as one GPU batch — three kernels that take a per-section record from device memory — against the host list stage, the Python reference and the single-proof host
verifier; what the batch reports; and that the entries from before it are as they were."""
import numpy as np
import pytest

import mem_many_ref as MR
import mem_stage_ref as M
import test_verify_many_memory as TH
from zkir_amd import runtime as rt, spec, stark

pytestmark = pytest.mark.gpu

NONE = {"cells": 0, "launches": 0, "uploaded_words": 0}


@pytest.fixture(autouse=True)
def _every_section_on_the_device(monkeypatch):
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", "0")
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_RECORDS", "0")


def _three_ways(b, what=""):
    """the device stage against the host stage and the reference"""
    want = MR.stage_ref(*b)
    MR.assert_stage(rt.mem_sections_stage(*b, device=False), want, what + " (host)")
    got = rt.mem_sections_stage(*b, device=True)
    MR.assert_stage(got, want, what + " (device)")
    return got


# ---- the kernels' edges --------------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", range(len(MR.SIZES_ORDERS)))
def test_the_sizes_batch(order):
    _three_ways(MR.batch(MR.sizes_sections(MR.SIZES_ORDERS[order]), seed=order))


def test_the_workgroups_edge_and_ragged_last_chunks():
    sec = lambda n, seed: M.section(M.increasing(n, seed=seed, start=0x1000 + 64))  # noqa: E731
    _three_ways(MR.batch([sec(256, 1), sec(257, 2)], seed=1), "256 | 257")
    _three_ways(MR.batch([sec(257, 1), sec(256, 2), sec(1, 3)], seed=2), "257 | 256 | 1")
    for n in (73, 74, 146):                                     # exactly 512, 519 and 1023 words: a ragged last chunk must end at ITS section's end
        _three_ways(MR.batch([sec(n, 4), sec(300, 5)], seed=n), f"{n} | 300")
        _three_ways(MR.batch([sec(n, 4), sec(n, 6), sec(n, 4)], seed=n + 1), f"{n} three times")


def test_sections_are_kept_apart():
    _three_ways(TH.edge_batch(), "the image's edges under three images")
    got = _three_ways(TH.failing_batch(), "failing sections among well-formed ones")
    assert got[0] == [0, 0, 54, 0, 55, 0]                       # (section 1 starts below section 0's last address: cell 0 has no predecessor)


def test_the_lowest_failing_cell_wins_across_workgroups():
    low = M.cells_at([8 * i for i in range(300)] + [0x1000] + [0x1008 + 8 * i for i in range(300)], seed=3)      # cell 300 is ON the code (55 with two code words)
    def bad(at):
        c = [list(x) for x in low]; c[at][4] = 0x10000
        return M.section(c)
    secs = [bad(10), bad(590), M.section(low), M.section(M.increasing(5))]      # 54 in workgroup 0 before 55 in workgroup 1; 55 in workgroup 1 before 54 in workgroup 2
    b = (secs, [3, 3, 3, 3], [2, 2, 2, 2], [M.make_blob(bytes(8), b"")] * 4, [M.ALPHA] * 4, [M.LAM] * 4)
    assert _three_ways(b)[0] == [54, 55, 55, 0]


def test_the_entrys_cap_of_one_cell_sections():
    rng = np.random.default_rng(8)
    secs = [M.section(M.cells_at([0x2000 + 8 * int(rng.integers(0, 1 << 20))], seed=i)) for i in range(1024)]
    blob = M.make_blob(bytes(8), bytes(range(1, 40)))
    b = (secs, [3 + (i & 1) for i in range(1024)], [2] * 1024, [blob] * 1024, [MR.challenge(i % 7) for i in range(1024)], [MR.challenge(7 + i % 5) for i in range(1024)])
    host = rt.mem_sections_stage(*b, device=False)
    MR.assert_stage(rt.mem_sections_stage(*b, device=True), host)
    k = 1000                                                    # (the reference on one of them)
    one = tuple(x[k:k + 1] for x in b)
    MR.assert_stage(tuple(x[k:k + 1] for x in host), MR.stage_ref(*one))
    with pytest.raises(rt.RuntimeError):
        rt.mem_sections_stage(*(x + x[:1] for x in b), device=True)


def test_one_cell_past_the_grid_cap_among_small_sections():
    """a section of MEM_MAX_BLOCKS * NT + 1 cells: its workgroups stride, the first lane takes two cells; against the host form only (as tests/test_gpu_mem_stage.py does)"""
    n = M.SIDE_GRID_CAP * M.NT + 1
    rng = np.random.default_rng(9)
    addr = 0x1000 + 64 + 8 * np.arange(n, dtype=np.int64)       # (the first cells lie in the image, behind the code)
    big = M.section(np.stack([addr & 0xFFFFF, addr >> 20, rng.integers(0, M.P, n), *rng.integers(0, 1 << 16, (4, n))], axis=1))
    small = lambda n, seed: M.section(M.increasing(n, seed=seed, start=0x1000 + 64))  # noqa: E731
    b = MR.batch([small(3, 1), big, small(74, 2)], seed=4)
    host = rt.mem_sections_stage(*b, device=False)
    assert host[0] == [0, 0, 0] and any(host[2][1])
    MR.assert_stage(rt.mem_sections_stage(*b, device=True), host)


# ---- the entries ---------------------------------------------------------------------------------------------------------------------------------------------------------
def test_the_honest_mixed_batch_is_one_batch(monkeypatch):
    corpus = MR.honest_corpus()
    proofs, pubs = [p for _, p, _ in corpus], [e for _, _, e in corpus]
    want = [rt.verify(p, e) for p, e in zip(proofs, pubs)]
    cells = sum(MR.count_word(p) for p in proofs)
    assert rt.verify_many(proofs, pubs, memory=True) == want
    last = rt.verify_memory_last()
    assert last["cells"] == cells and last["launches"] == 3 and last["uploaded_words"] >= sum(1 + 7 * MR.count_word(p) for p in proofs)
    assert rt.verify_queries_last()["launches"] == 2
    for sub in (proofs[:2], proofs[3:7], proofs[::-1]):         # whatever n is: three launches
        host = [rt.verify(p) for p in sub]
        assert rt.verify_many(sub, memory=True) == host
        assert rt.verify_memory_last()["launches"] == 3 and rt.verify_memory_last()["cells"] == sum(MR.count_word(p) for p in sub)
    # only the refused proof: its section went up, no front deferred
    assert rt.verify_many(proofs[2:3], pubs[2:3], memory=True) == [55] and rt.verify_memory_last()["launches"] == 2
    # the entries from before: no memory stage
    assert rt.verify_many(proofs, pubs) == want and rt.verify_memory_last() == NONE
    # the threshold applies to the TOTAL: one cell more keeps the whole batch on the host
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", str(cells + 1))
    assert rt.verify_many(proofs, pubs, memory=True) == want and rt.verify_memory_last() == NONE
    monkeypatch.setenv("ZKIR_VERIFY_DEVICE_MIN_CELLS", str(cells))
    assert rt.verify_many(proofs, pubs, memory=True) == want and rt.verify_memory_last()["cells"] == cells


def test_mutated_proofs_get_the_host_verdict():
    muts = MR.mutants()
    proofs = [t for _, t in muts]
    want = [rt.verify(t) for t in proofs]
    assert rt.verify_many(proofs, memory=True) == want
    assert rt.verify_memory_last()["launches"] == 3
    rng = np.random.default_rng(2)
    perm = [int(i) for i in rng.permutation(len(proofs))][:40]
    assert rt.verify_many([proofs[i] for i in perm], memory=True) == [want[i] for i in perm]


def test_rate_proofs_and_their_mutants():
    corpus = MR.rate_corpus()
    proofs, pubs = [c[1] for c in corpus], [c[2] for c in corpus]
    mq, mb = [c[3] for c in corpus], [c[4] for c in corpus]
    want = [rt.verify_rate(p, e, q, b) for p, e, q, b in zip(proofs, pubs, mq, mb)]
    assert set(want) - {0} == MR.RATE_MUTATION_CODES
    assert rt.verify_rate_many(proofs, pubs, mq, mb, memory=True) == want
    last = rt.verify_memory_last()
    assert last["launches"] == 3 and last["cells"] == sum(MR.located_cells(c[1], c[5]) for c in corpus)
    rev = list(reversed(range(len(proofs))))
    assert rt.verify_rate_many([proofs[i] for i in rev], [pubs[i] for i in rev], [mq[i] for i in rev], [mb[i] for i in rev], memory=True) == [want[i] for i in rev]
    assert rt.verify_rate_many(proofs, pubs, mq, mb) == want and rt.verify_memory_last() == NONE


def test_the_gpu_provers_array_loop_beside_a_mode4_proof():
    """spec.memory_loop_program(300)'s mode-3 proof (300 cells, five chunks) twice with a mode-4 proof between them: the mode-4 proof's tape stages run BEHIND the batch
    region, which must survive them for phase B"""
    from zkir_amd import pipeline as pl
    blob = spec.memory_loop_program(300).to_bytes()
    log = rt.interpret(blob, [], rt.VMConfig(enable_execution_trace=True))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    pub = rt.public_inputs(log, blob, [], mem_mode=True, mem_witness="device")
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    proof = stark.prove(ctx, tr, pub)
    ctx.close()
    log.close()
    assert int(proof[9]) == 3 and MR.count_word(proof) == 300
    m4 = {w: (p, e) for w, p, e in MR.honest_corpus()}["sha256_hello mode 4"]
    proofs, pubs = [proof, m4[0], proof], [pub, m4[1], pub]
    assert rt.verify_many(proofs, pubs, memory=True) == [0, 0, 0]
    assert rt.verify_memory_last()["cells"] == 600 + MR.count_word(m4[0]) and rt.verify_memory_last()["launches"] == 3
    assert rt.verify_last_stages()["device_stages"] > 3        # (the mode-4 proof's tape stages ran on the device too)
    t = proof.copy(); t[stark.proof_layout(proof)["mem_section"] + 1 + 7 * 299 + 2] ^= 1      # the last cell's time of the LAST proof
    want = rt.verify(t, pub)
    assert want != 0 and rt.verify_many([proof, m4[0], t], pubs, memory=True) == [0, 0, want]


def test_the_probe_on_the_device():
    TH._probe_checks(device=True)

"""The device witness of proof mode 4 for runs WITH hash syscalls (memcheck.hip: a row has 0, 1 or many accesses; the written digests come from the log's zkir_hash_out
records): the memory witness and the hash tape built on the GPU equal the host's sequential replay entry for entry, the proofs made from them equal the oracle's word for
word, and the drop-in call zkir_prove_result proves such runs."""
import ctypes as C

import numpy as np
import pytest

import programs as pg
from oracle import api as oracle, stark_api as so
from test_hash_outs import NAMED, SEEDS, hash_case
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu
P = 0x78000001
A, E, O, EC, EB = pg.A, spec.encode, spec.Opcode, pg.EC, pg.EB


# ---- designed edges: small programs, each one shape of overlap between a call's buffers and the rest of memory ---------------------------------------------------------
def _hc(num, in_ptr, length, out_ptr):
    return [A(11, 0, in_ptr), A(12, 0, length), A(13, 0, out_ptr), A(10, 0, num), EC]


def edge_in_place():
    """in == out: Keccak-256 and BLAKE3 over their own 32 output bytes, SHA-256 over 64 bytes whose first 32 it overwrites; then the digests are hashed again in place."""
    code = [A(5, 0, 0x3000)] + pg._store_bytes(5, bytes(range(1, 41)))
    code += _hc(5, 0x3000, 32, 0x3000) + _hc(6, 0x3000, 32, 0x3000) + _hc(3, 0x3000, 64, 0x3000) + _hc(5, 0x3003, 32, 0x3003) + _hc(3, 0x3004, 9, 0x3004)
    return pg._p(code + [EB]), [], {}


def edge_out_inside_input():
    """The output inside [in, in + len): at offsets that are no multiple of 4 (Keccak-256, BLAKE3) and at 4 modulo 8 (SHA-256) — the message is read before the digest is written."""
    code = [A(5, 0, 0x3300)] + pg._store_bytes(5, bytes((7 * i + 1) & 0xFF for i in range(48)))
    code += _hc(5, 0x3300, 80, 0x3311) + _hc(6, 0x3300, 80, 0x3326) + _hc(3, 0x3300, 80, 0x330C) + _hc(6, 0x3301, 47, 0x3303) + _hc(3, 0x3300, 80, 0x3334)
    return pg._p(code + [EB]), [], {}


def edge_sha_half_cells():
    """SHA-256 at out = 4 (mod 8): five cells, the first and the last half written — next to bytes an earlier SB put into the other halves; LD reads both cells after the call."""
    code = [A(5, 0, 0x3500), A(9, 0, 0xA1), E(O.SB, rs1=5, rs2=9, imm=0), A(9, 0, 0xB2), E(O.SB, rs1=5, rs2=9, imm=3), A(9, 0, 0xC3), E(O.SB, rs1=5, rs2=9, imm=0x26),
            A(9, 0, 0xD4), E(O.SB, rs1=5, rs2=9, imm=0x21), A(6, 0, 0x2000)] + pg._store_bytes(6, b"hello")
    code += _hc(3, 0x2000, 5, 0x3504) + [E(O.LD, 1, 5, imm=0), E(O.LD, 2, 5, imm=0x20), E(O.LD, 3, 5, imm=8), E(O.LW, 4, 5, imm=0x24)]
    return pg._p(code + [EB]), [], {}


def edge_store_between_calls():
    """A store into an input cell between two calls that hash it (and one into an output cell, read back by the second call's neighbour)."""
    code = [A(5, 0, 0x2000)] + pg._store_bytes(5, b"0123456789abcdef")
    code += _hc(5, 0x2000, 16, 0x3600) + [A(9, 0, 0x5A), E(O.SB, rs1=5, rs2=9, imm=3), E(O.SH, rs1=5, rs2=9, imm=10)] + _hc(5, 0x2000, 16, 0x3620)
    code += [A(7, 0, 0x3600), E(O.SW, rs1=7, rs2=9, imm=4), E(O.LD, 1, 7, imm=0)] + _hc(3, 0x3600, 64, 0x3640) + [E(O.LD, 2, 7, imm=0x40)]
    return pg._p(code + [EB]), [], {}


def edge_len_zero():
    """len == 0 for all three kinds (the input pointer is anything: no cell of it is touched), outputs at every alignment the kind admits."""
    code = _hc(3, 0x2001, 0, 0x3000) + _hc(5, 0x2002, 0, 0x3021) + _hc(6, 0, 0, 0x3047) + _hc(3, 0x3000, 0, 0x3004) + _hc(5, 0x3021, 0, 0x3020) + _hc(6, 0x3047, 0, 0x3046)
    return pg._p(code + [EB]), [], {}


def edge_len_2p17():
    """ONE call over 2^17 bytes of mostly-zero memory: 16 385 + 4 cells in a run of a few rows — one row expands to far more accesses than the run has rows, and the witness's
    buffers are far larger than anything sized by the row count."""
    code = pg.li40(5, 0x100000 + 54321) + [A(9, 0, 0xAB), E(O.SB, rs1=5, rs2=9, imm=0)] + pg._call(6, 0x100003, 1 << 17, 0x300000) + pg.li40(7, 0x300000) + [E(O.LD, 1, 7, imm=8)]
    return pg._p(code + [EB]), [], {}


def edge_chain_first_call():
    """The chain program up to its first call: the copy loop that sets the seed up reads the boundary cell (the last code word and the first seed bytes)."""
    return spec.sha256_chain_program().to_bytes(), [], {"max_cycles": 54}


EDGES = {f.__name__: f for f in (edge_in_place, edge_out_inside_input, edge_sha_half_cells, edge_store_between_calls, edge_len_zero, edge_len_2p17, edge_chain_first_call)}
UNSAFE_SEEDS = [4, 8, 12]                                   # random programs without `wide_safe`: the wide opcodes go through the wide tape


def _program(which):
    if isinstance(which, str) and which in EDGES:
        blob, ins, cfg = EDGES[which]()
        return blob, list(ins), cfg
    if isinstance(which, str) and which.startswith("unsafe"):
        blob, ins = pg.random_program(int(which[6:]), n_instr=200, hashes=True)
        return blob, list(ins), {"max_cycles": 600}
    return hash_case(which)


PROVEN = NAMED + SEEDS + ["unsafe%d" % s for s in UNSAFE_SEEDS]


def _device_trace(blob, ins, cfg):
    from zkir_amd import pipeline as pl
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    return log, tr


def _host_witness(log, blob):
    hw = rt.MemcheckWitness(log, blob, 4)
    pub = rt.PublicInputsC(); pub.with_memory(hw)
    n, nc = int(log.n_rows), hw.n_cells
    arr = lambda p, t, m: np.ctypeslib.as_array(C.cast(p, C.POINTER(t)), (m,)).copy() if m and p else np.zeros(0, np.dtype(t))  # noqa: E731
    w = {"mem_old": arr(pub.mem_old, C.c_uint64, n), "mem_told": arr(pub.mem_told, C.c_uint32, n), "cell_addr": arr(pub.cell_addr, C.c_uint64, nc),
         "cell_bytes": arr(pub.cell_bytes, C.c_uint64, nc), "cell_time": arr(pub.cell_time, C.c_uint32, nc),
         "hash_section": arr(pub.hash_section, C.c_uint32, int(pub.hash_section_words)) if pub.hash_section_words else np.zeros(1, np.uint32)}
    return w, hw.n_hash_calls


def _assert_witness_parity(which, min_calls=1, oracle_section=True):
    blob, ins, cfg = _program(which)
    log, tr = _device_trace(blob, ins, cfg)
    want, n_calls = _host_witness(log, blob)
    got = rt.memcheck_witness_device(tr, log, blob, mode=4)
    for name in ("mem_old", "mem_told", "cell_addr", "cell_bytes", "cell_time", "hash_section"):
        assert len(got[name]) == len(want[name]), (name, len(got[name]), len(want[name]))
        if not np.array_equal(got[name], want[name]):
            raise AssertionError(f"{name}: first difference at {int(np.nonzero(got[name] != want[name])[0][0])} of {len(want[name])}")
    assert int(got["hash_section"][0]) == n_calls >= min_calls
    if oracle_section:
        ores = oracle.run(blob, ins, enable_execution_trace=True, **cfg)
        opub = so.public_inputs(len(ores.rows), blob, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
        assert np.array_equal(got["hash_section"], so.hash_section(ores.rows, opub))
    log.close()


@pytest.mark.parametrize("which", PROVEN + list(EDGES))
def test_device_witness_equals_host_replay(which):
    """mem_old / mem_told of every row, the touched cells (address, final bytes, time of the last access) and the hash section word for word: the device's equal the host
    replay's, and the section equals the oracle's so::hash_section."""
    _assert_witness_parity(which)


@pytest.mark.parametrize("seed", range(100, 140))
def test_device_witness_equals_host_replay_on_random_programs(seed):
    _assert_witness_parity(seed, min_calls=0, oracle_section=False)


def _prove_device(which):
    from zkir_amd import stark
    blob, ins, cfg = _program(which)
    ores = oracle.run(blob, ins, enable_execution_trace=True, **cfg)
    log, tr = _device_trace(blob, ins, cfg)
    assert log.n_rows == len(ores.rows)
    opub = so.public_inputs(len(ores.rows), blob, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    pub = rt.public_inputs(log, blob, ins, wide_mode=True, hash_witness="device")
    assert pub.deferred == 4 and not pub.mem_old and not pub.hash_section and pub.n_hash_outs >= 1
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    return blob, ins, cfg, ores, log, tr, opub, pub, ctx, proof


@pytest.mark.parametrize("which", PROVEN + list(EDGES))
def test_device_witness_proof_equals_the_oracles(which):
    """zkir_prove with no witness in the public inputs (mem_old == NULL) proves a run that makes hash calls: the proof equals the oracle's word for word, both verifiers and
    verify_io accept it, tampered copies are rejected alike.  (The parent commit refused such a run: ZKIR_ERR_ARGUMENT.)"""
    blob, ins, cfg, ores, log, tr, opub, pub, ctx, proof = _prove_device(which)
    want = so.prove(ores.rows, opub)
    assert proof[1] == 12 and proof[3] == 288 and proof[9] == 4 and len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"mode-4 proof differs at word {bad[0]} of {len(want)} ({len(bad)} words differ)")
    assert so.verify(proof, opub) == 0 and rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    assert rt.verify_io(proof, pub, ins, list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    for pos in (8, 30, 158, 160, len(proof) // 2, len(proof) - 1):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1) % P
        assert so.verify(t) != 0 and rt.verify(t) == so.verify(t), pos
    ctx.close(); log.close()


@pytest.mark.parametrize("which", ["sha256_hello", "hashes_all"])
def test_drop_in_call_proves_hash_runs(which):
    """VM.run (zkir_exec, execution trace on) + ExecutionResult.prove(mode=4) (zkir_prove_result): the same bytes as zkir_prove from the device witness; mode 0 through the same
    method still equals zkir_prove's mode-0 proof.  (The parent commit: ZKIR_ERR_ARGUMENT in mode 4.)"""
    from zkir_amd import stark
    blob, ins, cfg, ores, log, tr, opub, pub, ctx, proof = _prove_device(which)
    res = rt.VM(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg)).run()
    got = res.prove(mode=4)
    assert np.array_equal(got, proof) and rt.verify(got, pub) == 0 and so.verify(got, opub) == 0
    got0 = res.prove()
    want0 = stark.prove(ctx, tr, rt.public_inputs(log, blob, ins))
    assert got0[9] == 0 and np.array_equal(got0, want0) and rt.verify(got0) == 0
    res.close(); ctx.close(); log.close()


def test_witness_at_the_length_cap():
    """One Keccak-256 call over 2^20 bytes of zero memory (131 072 + 4 cells from one row): device witness == host replay.  2^20 + 1 bytes: both refuse, the same way."""
    blob = pg._p(pg._call(5, 0x100000, 1 << 20, 0x300000) + [EB])
    log, tr = _device_trace(blob, [], {})
    want, n_calls = _host_witness(log, blob)
    got = rt.memcheck_witness_device(tr, log, blob, mode=4)
    assert n_calls == 1 and len(want["cell_addr"]) == (1 << 17) + 4
    for name in want:
        assert np.array_equal(got[name], want[name]), name
    log.close()
    blob, ins, cfg = pg.hash_edge_len_over()
    log, tr = _device_trace(blob, ins, {})
    with pytest.raises(rt.RuntimeError, match="outside what a proof states") as e1:
        rt.MemcheckWitness(log, blob, 4)
    with pytest.raises(rt.RuntimeError, match="outside what a proof states") as e2:
        rt.memcheck_witness_device(tr, log, blob, mode=4)
    assert e1.value.code == e2.value.code == rt.ERR_ARGUMENT
    log.close()


def test_refusals_that_stay():
    from zkir_amd import stark
    blob, ins, cfg = _program("hashes_all")
    log, tr = _device_trace(blob, ins, cfg)
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows))
    # mode 3 states no hash call, from either witness
    with pytest.raises(rt.RuntimeError, match="hash syscall") as e:
        stark.prove(ctx, tr, rt.public_inputs(log, blob, ins, mem_mode=True, mem_witness="device"))
    assert e.value.code == rt.ERR_ARGUMENT
    with pytest.raises(rt.RuntimeError, match="hash syscall"):
        rt.memcheck_witness_device(tr, log, blob, mode=3)
    # a record count that is not the trace's number of hash rows
    pub = rt.public_inputs(log, blob, ins, wide_mode=True, hash_witness="device")
    q = pub.copy(); q.n_hash_outs = pub.n_hash_outs - 1
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, q)
    assert e.value.code == rt.ERR_ARGUMENT
    q = pub.copy(); q.n_hash_outs = 0; q.hash_outs = None                      # no records at all: the witness of loads and stores refuses the run, as before
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, q)
    assert e.value.code == rt.ERR_ARGUMENT
    # records moved to other rows
    outs = log.hash_outs.copy(); outs["row"][3] += 1
    q = pub.copy(); q.hash_outs = outs.ctypes.data
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove(ctx, tr, q)
    assert e.value.code == rt.ERR_ARGUMENT
    # one digest byte flipped: refused, or a proof that BOTH verifiers reject with the same code — never an accepted proof
    for k, byte in ((0, 0), (4, 31), (len(log.hash_outs) - 1, 17)):
        outs = log.hash_outs.copy(); outs["bytes"][k][byte] ^= 0x40
        q = pub.copy(); q.hash_outs = outs.ctypes.data
        try:
            t = stark.prove(ctx, tr, q)
        except rt.RuntimeError as err:
            assert err.code == rt.ERR_ARGUMENT
        else:
            assert so.verify(t) != 0 and rt.verify(t) == so.verify(t)
    assert rt.verify(stark.prove(ctx, tr, pub), pub) == 0                       # the context is fine after the refusals
    ctx.close(); log.close()


def test_sha_chain_at_2p20_device_witness_proof_equals_the_host_witness_proof():
    """BASELINE configs[4]'s program at 2^20 cycles (175 k SHA-256 calls): the proof from the device witness equals the proof from the host replay byte for byte (the oracle's
    golden stops at 2^16; the host path is itself held to the oracle below that), and it verifies."""
    from zkir_amd import stark
    k = 20
    n = 1 << k
    blob = spec.sha256_chain_program().to_bytes()
    log, tr = _device_trace(blob, [], {"max_cycles": n})
    ctx = stark.StarkContext(k)
    pub_d = rt.public_inputs(log, blob, [], wide_mode=True, hash_witness="device")
    assert not pub_d.mem_old and pub_d.n_hash_outs == len(log.hash_outs)
    got = stark.prove(ctx, tr, pub_d)
    pub_h = rt.public_inputs(log, blob, [], wide_mode=True, mem_witness="host")
    want = stark.prove(ctx, tr, pub_h)
    assert got.tobytes() == want.tobytes()
    assert rt.verify(got, pub_d) == 0
    n_calls = int(got[stark.proof_layout(got)["hash_section"]])
    assert n // 6 - 16 <= n_calls <= n // 6 and n_calls == pub_h._mem_ref.n_hash_calls
    ctx.close(); log.close()

"""stark.prove_rate_modes / rt.verify_rate on the GPU in modes 3 and 4: 'ZKSR' proofs of runs with the memory argument, the wide-arithmetic class and the hash tapes at
blow-up 2, 4 and 8.  The oracle has no word-for-word reference in these modes (its lookup set-up and constraint evaluation are fixed to the base widths), so the parts are
checked on their own, as test_gpu_prove_rate.py does in mode 2: the oracle's trace root at the rate, a quotient of low degree, the embedded proof = stark.batch_eval_prove
on the same matrices, both verifiers, host and device verdicts equal on mutants.  Then: both witness routes, modes 0 - 2 through the new entry, forged memory and wrong
executions, named rejections, refusals, the proof's size by rate, the drop-in call, a context shared with stark.prove."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import test_gpu_prove_rate as gr
import test_gpu_stark as gs
from oracle import stark_api as so
from zkir_amd import runtime as rt, spec

pytestmark = pytest.mark.gpu
P = so.P


@functools.lru_cache(maxsize=None)
def case(which, witness, wide):
    return gs._mode3_case(which, witness, wide)


def own_case(blob, ins=(), wide=False, hash_witness="host", **cfg):
    """a run of `blob` on the device without the oracle: (log, trace, public inputs with no witness: the prover makes it)"""
    from zkir_amd import pipeline as pl
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    return log, tr, rt.public_inputs(log, blob, list(ins), mem_mode=not wide, wide_mode=wide, hash_witness=hash_witness)


def both(t, pub, nq, bits) -> int:
    host, device = rt.verify_rate(t, pub, nq, bits), rt.verify_rate(t, pub, nq, bits, device=True)
    assert host == device, f"host {host}, device {device}"
    return host


def parts_hold(ctx, tr, pub, rows, opub, b, nq, bits, n_mut=200):
    """test_gpu_prove_rate._independent_checks through the entry of every mode"""
    import torch
    from zkir_amd import stark
    mode = int(pub.deferred)
    proof = stark.prove_rate_modes(ctx, tr, pub, nq, bits)
    at = stark.rate_proof_layout(proof)
    assert int(proof[0]) == 0x52534B5A and int(proof[1]) == 1
    assert int(proof[3]) == (264 if mode == 3 else 288) == so.committed_width(mode) and int(proof[9]) == mode == at["mode"]
    assert at["log_blowup"] == b and at["num_queries"] == nq and at["pow_bits"] == bits and at["log_n"] == ctx.log_n
    assert np.array_equal(proof[at["trace_root"]:at["trace_root"] + 4], so.commit_trace_blocked(rows, b, pub=opub, threads=8))
    mats = stark.rate_last_matrices(ctx)
    widths = [int(proof[3]), so.aux_width(mode), 4]
    assert widths[1] == (96 if mode == 3 else 128) and [m.shape[0] * 8 for m in mats] == [widths[0], widths[1], 8] and mats[0].shape[1] == 1 << (ctx.log_n + b)
    assert gr.low_degree(gr.b8_to_cols(mats[2], 4), 1 << ctx.log_n)
    inner = proof[at["eval_proof"]:]
    ia = stark.batch_eval_layout(inner)
    assert ia["widths"] == widths and ia["masks"] == [3, 3, 1]
    points = inner[ia["points"]:ia["evals"]].reshape(2, 4)
    roots = proof[at["trace_root"]:at["eval_proof"]].reshape(3, 4)
    dev = [torch.from_numpy(m.view(np.int32)).cuda() for m in mats]
    trees = [stark.merkle_commit(ctx, d, w) for d, w in zip(dev, widths)]
    for t, r in zip(trees, roots):
        assert np.array_equal(t[-4:].cpu().numpy().view(np.uint32), r)
    again = stark.batch_eval_prove(ctx, dev, trees, widths, [3, 3, 1], points, nq, bits)
    assert np.array_equal(again, inner)
    assert rt.batch_eval_verify(inner, roots, points) == 0
    assert both(proof, pub, nq, bits) == 0 and both(proof, None, nq, bits) == 0
    rng = np.random.default_rng(len(proof))
    codes = set()
    for pos in rng.integers(0, len(proof), n_mut):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1 + int(rng.integers(0, 5))) % P
        code = both(t, pub, nq, bits)
        assert code != 0, f"word {pos}: accepted"
        codes.add(code)
    assert any(c > 100 for c in codes), sorted(codes)
    return proof


# small programs: M = N 2^b below one workgroup (timestamps: 8 rows) and above it; every rate
@pytest.mark.parametrize("b,nq,bits", [(1, 3, 0), (2, 5, 4), (3, 9, 6)])
@pytest.mark.parametrize("which,wide", [("loads_stores", False), ("timestamps", False), ("wide_grid", True), ("sha256_hello", True)])
def test_parts_hold_on_their_own(which, wide, b, nq, bits):
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case(which, "device", wide)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), b)
    proof = parts_hold(ctx, tr, pub, ores.rows, opub, b, nq, bits)
    at = stark.rate_proof_layout(proof)
    if which == "sha256_hello":                                            # a hash tape, and the boundary cell among the touched ones
        assert int(proof[at["hash_section"]]) == 1 and int(proof[at["mem_section"]]) >= 1
    ctx.close()


# padded log_n >= 9 with n_real no power of two: `last` lies far from N - 1 (the selector read at j - 2^b last, the wrap of j + 2^b)
@pytest.mark.parametrize("which,wide,b", [("memloop", False, 2), ("signed_division_loop", True, 3)])
def test_parts_hold_on_a_padded_run(which, wide, b):
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case(which, "device", wide)
    n = len(ores.rows)
    log_n = stark.padded_log_n(n)
    assert log_n >= 9 and n & (n - 1) and n < (1 << log_n) - 16
    ctx = stark.StarkContext(log_n, b)
    parts_hold(ctx, tr, pub, ores.rows, opub, b, 7, 4)
    ctx.close()


@pytest.mark.parametrize("which,wide", [("loads_stores", False), ("sha256_hello", True)])
def test_both_witness_routes_give_the_same_proof(which, wide):
    """the memory witness (mode 4 on a hash run: and the tape) made on the device, or brought from the host's replay"""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, hpub = case(which, "host", wide)
    assert hpub.mem_old
    dpub = rt.public_inputs(log, blob, ins, mem_mode=not wide, wide_mode=wide, hash_witness="device")
    assert not dpub.mem_old and not dpub.hash_section
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    from_host, from_device = stark.prove_rate_modes(ctx, tr, hpub, 5, 4), stark.prove_rate_modes(ctx, tr, dpub, 5, 4)
    assert np.array_equal(from_host, from_device) and int(from_host[9]) == (4 if wide else 3)
    assert both(from_device, hpub, 5, 4) == 0
    ctx.close()


def test_modes_0_to_2_give_prove_rates_words():
    from zkir_amd import stark
    for name in ("fib", "deferred"):
        blob, log, tr, rows, opub, pub = gr.case(name, 64)
        ctx = stark.StarkContext(6, 2)
        assert np.array_equal(stark.prove_rate_modes(ctx, tr, pub, 7, 4), stark.prove_rate(ctx, tr, pub, 7, 4))
        ctx.close()
    blob, ins, ores, log, tr, opub, pub = gs._mode2_case("io")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    got = stark.prove_rate_modes(ctx, tr, pub, 7, 4)
    assert int(got[9]) == 2 and np.array_equal(got, stark.prove_rate(ctx, tr, pub, 7, 4))
    ctx.close(); log.close()


def refused_or_rejected(ctx, tr, pub, expect, nq=6, bits=4):
    """the prover refuses, or both verifiers refuse its proof with the same code"""
    from zkir_amd import stark
    try:
        bad = stark.prove_rate_modes(ctx, tr, pub, nq, bits)
    except rt.RuntimeError:
        return None
    code = both(bad, expect, nq, bits)
    assert code != 0
    return code


@pytest.mark.parametrize("b", [2, 3])
def test_forged_memory_is_rejected(b):
    """test_gpu_stark.test_mode3_forged_memory_is_rejected_on_the_gpu_path's edits: a load that reads a STALE cell; a forged final cell"""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = gs._mode3_case("timestamps", "host")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), b)
    assert both(stark.prove_rate_modes(ctx, tr, pub, 6, 4), pub, 6, 4) == 0
    n = len(ores.rows)
    old = np.ctypeslib.as_array(C.cast(pub.mem_old, C.POINTER(C.c_uint64)), (n,)).copy()
    told = np.ctypeslib.as_array(C.cast(pub.mem_told, C.POINTER(C.c_uint32)), (n,)).copy()
    assert told[5] == 5 and old[5] == 0x0000020000000100
    old[5], told[5] = old[4], told[4]
    f = pub.copy(); f._old, f._told = old, told
    f.mem_old, f.mem_told = old.ctypes.data, told.ctypes.data
    refused_or_rejected(ctx, tr, f, pub)
    g = pub.copy()
    cb = np.ctypeslib.as_array(C.cast(pub.cell_bytes, C.POINTER(C.c_uint64)), (pub.n_cells,)).copy()
    cb[0] ^= 1
    g._cb = cb; g.cell_bytes = cb.ctypes.data
    assert refused_or_rejected(ctx, tr, g, None) in (None, 10)              # every row is locally consistent; the multiset equation does not close
    ctx.close(); log.close()


@pytest.mark.parametrize("b", [2, 3])
def test_wrong_execution_is_rejected(b):
    """test_gpu_stark.test_mode3_wrong_execution_is_rejected_on_the_gpu_path's edits, patched in HBM: loads, XOR, ANDI, OR on the ring program; the shifts and MUL on alu_all"""
    from oracle import api as oracle
    from zkir_amd import stark
    import programs as pg
    for blob, ins, cfg, edits in ((spec.memory_ring_program(4).to_bytes(), [], dict(max_cycles=700), [(0x34, 8), (0x12, 2), (0x13, 5), (0x11, 12), (0x33, 9), (0x30, 10)]),
                                  (pg.alu_all()[0], list(pg.alu_all()[1]), {}, [(op, None) for op in (0x18, 0x19, 0x1A, 0x1B, 0x1C, 0x1D, 0x02)])):
        rows = oracle.run(blob, ins, enable_execution_trace=True, **cfg).rows
        n = len(rows)
        ops, rds = rows["instruction"] & 0x7F, (rows["instruction"] >> 7) & 0xF
        log, tr, pub = own_case(blob, ins, **cfg)
        ctx = stark.StarkContext(stark.padded_log_n(n), b)
        assert both(stark.prove_rate_modes(ctx, tr, pub, 6, 4), pub, 6, 4) == 0
        for op, rd in edits:
            ks = np.nonzero((ops == op) & ((rds == rd) if rd is not None else (rds != 0)))[0]
            k = int(ks[3] if rd is not None else ks[len(ks) // 2])
            r = int(rds[k])
            later = np.nonzero(rds[k + 1:] == r)[0]
            hi = k + 1 + (int(later[0]) if len(later) else n - k - 2)
            saved = tr.registers[r, k + 1:hi + 1].clone()
            tr.registers[r, k + 1:hi + 1] = saved ^ (2 if rd is not None else 1)
            refused_or_rejected(ctx, tr, pub, pub)
            tr.registers[r, k + 1:hi + 1] = saved
        assert both(stark.prove_rate_modes(ctx, tr, pub, 6, 4), pub, 6, 4) == 0
        ctx.close(); log.close()


def test_named_rejections_on_honest_mode4_proofs():
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case("sha256_hello", "host", True)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    proof = stark.prove_rate_modes(ctx, tr, pub, 6, 4)
    ctx.close()
    at = stark.rate_proof_layout(proof)
    assert both(proof, pub, 6, 4) == 0
    # the device entry runs the hash tape's record checks, digests and table side on the GPU and says so; the host entry runs none there
    assert rt.verify_rate(proof, pub, 6, 4, device=True) == 0 and rt.verify_last_stages()["device_stages"] >= 3
    assert rt.verify_rate(proof, pub, 6, 4) == 0 and rt.verify_last_stages()["device_stages"] == 0
    m0 = at["mem_section"]
    assert int(proof[m0]) >= 2
    t = proof.copy(); t[m0 + 1:m0 + 8], t[m0 + 8:m0 + 15] = proof[m0 + 8:m0 + 15], proof[m0 + 1:m0 + 8]      # the first two touched cells swapped
    assert both(t, pub, 6, 4) == 54
    h0 = at["hash_section"]
    assert int(proof[h0]) == 1
    for word in (1, 2, 9):                                                   # the record's header, its first cell
        t = proof.copy(); t[h0 + word] = (int(t[h0 + word]) + 1) % P
        assert both(t, pub, 6, 4) in (56, 10), word
    assert both(proof, pub, 7, 4) == 2 and both(proof, pub, 6, 5) == 2
    assert rt.verify(proof, pub) != 0 and rt.verify(proof) != 0            # zkir_verify does not take the 'ZKSR' words
    # the wide tape: a run whose divisions and high products take raw 64-bit operands
    blob, ins, ores, log, tr, opub, pub = case("signed_division_loop", "device", True)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    proof = stark.prove_rate_modes(ctx, tr, pub, 6, 4)
    ctx.close()
    at = stark.rate_proof_layout(proof)
    w0 = at["wide_section"]
    n = int(proof[w0])
    assert n >= 2 and both(proof, pub, 6, 4) == 0
    for word in (0, 2, 7):                                                   # a record's cycle, an operand limb, its opcode
        t = proof.copy(); t[w0 + 1 + 8 * (n // 2) + word] = (int(t[w0 + 1 + 8 * (n // 2) + word]) + 1) % P
        assert both(t, pub, 6, 4) in (57, 10), word


def test_refusals_name_the_entry():
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case("loads_stores", "device", False)
    log_n = stark.padded_log_n(len(ores.rows))
    ctx = stark.StarkContext(log_n, 2)

    def refused(fn, *words):
        with pytest.raises(rt.RuntimeError) as e:
            fn()
        assert e.value.code == rt.ERR_ARGUMENT and all(w in e.value.message for w in ("zkir_prove_rate_modes",) + words), e.value.message
    seg = rt.PublicInputsC.from_buffer_copy(pub); seg.writes_before = 1
    refused(lambda: stark.prove_rate_modes(ctx, tr, seg, 5, 4), "segment")
    refused(lambda: stark.prove_rate_modes(ctx, tr, pub, 0, 4), "num_queries")
    refused(lambda: stark.prove_rate_modes(ctx, tr, pub, 129, 4), "num_queries")
    refused(lambda: stark.prove_rate_modes(ctx, tr, pub, 5, 25), "pow_bits")
    five = rt.PublicInputsC.from_buffer_copy(pub); five.deferred = 5
    refused(lambda: stark.prove_rate_modes(ctx, tr, five, 5, 4), "mode")
    other = stark.StarkContext(log_n + 1, 2)
    refused(lambda: stark.prove_rate_modes(other, tr, pub, 5, 4), "log_n")
    other.close()
    out, n = C.POINTER(C.c_uint32)(), C.c_uint64()
    L = rt.lib()
    assert L.zkir_prove_rate_modes(ctx.handle, None, C.byref(pub), 5, 4, C.byref(out), C.byref(n), None, None) == rt.ERR_ARGUMENT
    assert b"null" in L.zkir_last_error() and b"zkir_prove_rate_modes" in L.zkir_last_error()
    assert L.zkir_prove_rate_modes(None, C.byref(tr.c), C.byref(pub), 5, 4, C.byref(out), C.byref(n), None, None) == rt.ERR_ARGUMENT
    assert L.zkir_prove_rate_modes(ctx.handle, C.byref(tr.c), None, 5, 4, C.byref(out), C.byref(n), None, None) == rt.ERR_ARGUMENT
    assert L.zkir_prove_rate_modes(ctx.handle, C.byref(tr.c), C.byref(pub), 5, 4, None, C.byref(n), None, None) == rt.ERR_ARGUMENT
    # zkir_prove_rate keeps its scope on the same context, and zkir_prove its rate; the entry of every mode serves both
    for p in (pub, case("loads_stores", "device", True)[6]):
        with pytest.raises(rt.RuntimeError) as e:
            stark.prove_rate(ctx, tr, p, 5, 4)
        assert e.value.code == rt.ERR_ARGUMENT and "zkir_prove_rate:" in e.value.message and "mode" in e.value.message
    with pytest.raises(rt.RuntimeError):
        stark.prove(ctx, tr, pub)
    assert rt.verify_rate(stark.prove_rate_modes(ctx, tr, pub, 5, 4), pub, 5, 4) == 0
    ctx.close()
    # a run that stores into its own code segment has no proof in these modes, from either witness
    for witness in ("device", "host"):
        blob, ins, ores, log, tr, opub, pub = gs._mode3_case("timestamps_on_code", witness)
        ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
        refused(lambda: stark.prove_rate_modes(ctx, tr, pub, 5, 4), "overlaps the code segment")
        ctx.close(); log.close()


@pytest.mark.parametrize("which,mode,needle", [("edge_at_2p40", 3, "2^40"), ("edge_bc_alias_low_1", 4, "B + 8 p j"), ("hash_edge_len_over", 4, "is outside what a proof states")])
def test_zkir_proves_refusals_of_the_public_inputs_stay(which, mode, needle):
    """an address at 2^40, a store into a boundary-cell alias, a hash call no proof states: refused from the device witness, under this entry's name"""
    from zkir_amd import stark
    import programs
    blob, ins, cfg = getattr(programs, which)()
    log, tr, pub = own_case(blob, ins, wide=mode == 4, hash_witness="device")
    assert not pub.mem_old
    ctx = stark.StarkContext(stark.padded_log_n(log.n_rows), 2)
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove_rate_modes(ctx, tr, pub, 5, 4)
    assert e.value.code == rt.ERR_ARGUMENT and "zkir_prove_rate_modes" in e.value.message and needle in e.value.message, e.value.message
    ctx.close(); log.close()


def test_an_incomplete_witness_is_refused():
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case("loads_stores", "host", False)
    cut = pub.copy(); cut.mem_told = None
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    with pytest.raises(rt.RuntimeError) as e:
        stark.prove_rate_modes(ctx, tr, cut, 5, 4)
    assert e.value.code == rt.ERR_ARGUMENT and "zkir_prove_rate_modes" in e.value.message and "complete" in e.value.message
    ctx.close()


def test_proof_shrinks_as_the_rate_falls():
    """mode 3 at log_n 10 with the defaults 50 / 25 / 17 queries + 12 bits: a query opens 364 words of rows and three paths, so fewer queries are worth more than in mode 0"""
    from zkir_amd import stark
    log, tr, pub = own_case(spec.memory_loop_program(60).to_bytes())
    assert stark.padded_log_n(log.n_rows) == 10
    sizes = []
    for b, nq in ((1, 50), (2, 25), (3, 17)):
        ctx = stark.StarkContext(10, b)
        proof = stark.prove_rate_modes(ctx, tr, pub)
        assert (int(proof[4]), int(proof[5]), int(proof[6]), int(proof[9])) == (nq, b, 12, 3)
        assert both(proof, pub, nq, 12) == 0 and both(proof, pub, nq + 1, 12) == 2
        sizes.append(len(proof))
        ctx.close()
    assert sizes[0] > sizes[1] > sizes[2], sizes
    log.close()


def test_drop_in_call_proves_a_hash_run_at_blowup_4():
    """VM.run + ExecutionResult.prove_rate(4, 2) (zkir_prove_result_rate): the context of that rate, the witness and the tape are made inside the call"""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case("sha256_hello", "host", True)
    res = rt.VM(blob, ins, rt.VMConfig(enable_execution_trace=True)).run()
    got = res.prove_rate(4, 2)
    assert (int(got[0]), int(got[4]), int(got[5]), int(got[6]), int(got[9])) == (0x52534B5A, 25, 2, 12, 4)
    assert both(got, pub, 25, 12) == 0
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    assert np.array_equal(got, stark.prove_rate_modes(ctx, tr, pub))        # the same words as the entry on a context of the caller's
    small = res.prove_rate(4, 3, 4, 3)                                      # explicit parameters below zkir_prove's ranges: the rate entry's hold
    assert (int(small[4]), int(small[5]), int(small[6])) == (4, 3, 3) and both(small, pub, 4, 3) == 0
    with pytest.raises(rt.RuntimeError):
        res.prove_rate(4, 4)
    with pytest.raises(rt.RuntimeError):
        res.prove_rate(4, 2, 129)
    res.close(); ctx.close()


def test_a_blowup2_context_serves_both_provers_in_turn():
    """stark.prove (mode 3), stark.prove_rate_modes, stark.prove on ONE log_blowup 1 context: zkir_prove's bytes stay the oracle's"""
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = case("loads_stores", "device", False)
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    first = stark.prove(ctx, tr, pub)
    rate = stark.prove_rate_modes(ctx, tr, pub, 7, 4)
    third = stark.prove(ctx, tr, pub)
    assert np.array_equal(first, third) and np.array_equal(first, so.prove(ores.rows, opub))
    assert int(rate[5]) == 1 and both(rate, pub, 7, 4) == 0 and rt.verify(first, pub) == 0
    ctx.close()

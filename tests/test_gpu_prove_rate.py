"""stark.prove_rate / rt.verify_rate on the GPU: ZKIR-STARK proofs at blow-up 2, 4 and 8 ('ZKSR').  Word for word against tests/prove_rate_ref.py on small runs; on larger
ones and in mode 2 the parts are checked on their own (the oracle's trace root at the rate, a quotient of low degree, the embedded proof = stark.batch_eval_prove on the same
matrices, both verifiers, host and device verdicts equal on mutants); the defaults; wrong executions; refusals before any launch; a context shared with stark.prove."""
from __future__ import annotations

import ctypes as C
import functools

import numpy as np
import pytest

import prove_rate_ref as pr
import test_gpu_stark as gs
from oracle import stark_api as so
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu
P = so.P


@functools.lru_cache(maxsize=None)
def case(name, n):
    return gs._case(name, n)


def b8_to_cols(mat: np.ndarray, width: int) -> np.ndarray:
    """B8 uint32[nb][M][8] -> uint32[width][M]"""
    nb, m, _ = mat.shape
    return np.ascontiguousarray(mat.transpose(0, 2, 1).reshape(nb * 8, m)[:width])


def low_degree(q_cols: np.ndarray, n: int) -> bool:
    return all(not so.ntt(q_cols[i], inverse=True)[n:].any() for i in range(4))


# fib 5 (log_n 3) and 64 (log_n 6) at every rate in both modes; fib 300 (log_n 9: padded rows, `last` far from N - 1) once
@pytest.mark.parametrize("name,n,b,nq,bits", [("fib", 5, 1, 3, 0), ("deferred", 5, 2, 4, 4), ("fib", 5, 3, 5, 0), ("deferred", 64, 1, 6, 4), ("fib", 64, 2, 7, 0),
                                              ("deferred", 64, 3, 8, 4), ("fib", 5, 2, 3, 4), ("deferred", 5, 1, 3, 0), ("deferred", 5, 3, 3, 0), ("fib", 64, 1, 3, 0),
                                              ("deferred", 64, 2, 3, 4), ("fib", 64, 3, 3, 0), ("fib", 300, 2, 3, 4)])
def test_proof_equals_the_reference_word_for_word(name, n, b, nq, bits):
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = case(name, n)
    ctx = stark.StarkContext(stark.padded_log_n(n), b)
    proof = stark.prove_rate(ctx, tr, pub, nq, bits)
    want = pr.prove_ref(rows, opub, b, nq, bits)
    assert len(proof) == len(want)
    if not np.array_equal(proof, want):
        bad = np.nonzero(proof != want)[0]
        raise AssertionError(f"the proof differs from the reference at word {bad[0]} of {len(want)} ({len(bad)} words differ; layout {pr.layout(want)})")
    assert rt.verify_rate(proof, pub, nq, bits) == 0 and rt.verify_rate(proof, pub, nq, bits, device=True) == 0
    ctx.close()


def _independent_checks(ctx, tr, pub, rows, opub, b, nq, bits, n_mut=200):
    import torch
    from zkir_amd import stark
    proof = stark.prove_rate(ctx, tr, pub, nq, bits)
    at = stark.rate_proof_layout(proof)
    assert at["log_blowup"] == b and at["num_queries"] == nq and at["pow_bits"] == bits
    assert np.array_equal(proof[at["trace_root"]:at["trace_root"] + 4], so.commit_trace(rows, b, pub=opub))
    mats = stark.rate_last_matrices(ctx)
    widths = [int(proof[3]), so.aux_width(int(pub.deferred)), 4]
    n = 1 << ctx.log_n
    assert low_degree(b8_to_cols(mats[2], 4), n)
    # the embedded proof is stark.batch_eval_prove's on the same matrices and points, and stands alone
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
    assert rt.verify_rate(proof, pub, nq, bits) == 0 and rt.verify_rate(proof, pub, nq, bits, device=True) == 0
    rng = np.random.default_rng(len(proof))
    codes = set()
    for pos in rng.integers(0, len(proof), n_mut):
        t = proof.copy()
        t[pos] = (int(t[pos]) + 1 + int(rng.integers(0, 5))) % P
        host, device = rt.verify_rate(t, pub, nq, bits), rt.verify_rate(t, pub, nq, bits, device=True)
        assert host == device != 0, f"word {pos}: host {host}, device {device}"
        codes.add(host)
    assert any(c > 100 for c in codes)
    return proof


@pytest.mark.parametrize("b", [2, 3])
def test_fib_1000_parts_hold_on_their_own(b):
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = case("fib", 1000)
    ctx = stark.StarkContext(10, b)
    _independent_checks(ctx, tr, pub, rows, opub, b, 9, 6)
    ctx.close()


def test_mode2_parts_hold_and_a_forged_output_is_refused():
    from zkir_amd import stark
    blob, ins, ores, log, tr, opub, pub = gs._mode2_case("io")
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)), 2)
    proof = _independent_checks(ctx, tr, pub, ores.rows, opub, 2, 9, 6)
    assert proof[9] == 2 and proof[3] == 160
    # a forged output tape in the proof: both verifiers refuse it with the same code
    at = stark.rate_proof_layout(proof)
    n_in = int(proof[at["io_section"]])
    out0 = at["io_section"] + 1 + 4 * n_in + 1
    t = proof.copy(); t[out0] ^= 1
    host, device = rt.verify_rate(t, pub, 9, 6), rt.verify_rate(t, pub, 9, 6, device=True)
    assert host == device and host in (50, 51, 10)
    ctx.close()


def test_default_parameters_by_rate():
    """50 / 25 / 17 queries + 12 bits at log_n 10: both verifiers accept, and the proof shrinks as the rate falls"""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = case("fib", 1000)
    sizes = []
    for b, nq in ((1, 50), (2, 25), (3, 17)):
        ctx = stark.StarkContext(10, b)
        proof = stark.prove_rate(ctx, tr, pub)
        assert (int(proof[4]), int(proof[5]), int(proof[6])) == (nq, b, 12)
        assert rt.verify_rate(proof, pub, nq, 12) == 0 and rt.verify_rate(proof, pub, nq, 12, device=True) == 0
        assert rt.verify_rate(proof, pub, nq + 1, 12) == 2 and rt.verify(proof, pub) != 0
        sizes.append(len(proof))
        ctx.close()
    assert sizes[0] > sizes[1] > sizes[2], sizes


def test_wrong_execution_is_refused():
    """one ADD result off by one in HBM (test_gpu_stark's edit): the prover refuses, or both verifiers refuse its proof with the same code"""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = gs._case("fib", 256)
    ops = rows["instruction"] & 0x7F
    k = int(np.nonzero(ops == 0x00)[0][5])
    nxt = k + 1 + int(np.nonzero(ops[k + 1:] == 0x00)[0][0])
    tr.registers[4, k + 1:nxt + 1] += 1
    for b in (2, 3):
        ctx = stark.StarkContext(8, b)
        try:
            bad = stark.prove_rate(ctx, tr, pub, 6, 4)
        except rt.RuntimeError:
            ctx.close()
            continue
        host, device = rt.verify_rate(bad, pub, 6, 4), rt.verify_rate(bad, pub, 6, 4, device=True)
        assert host == device != 0
        ctx.close()
    log.close()


def test_refusals_come_before_any_launch_with_a_message():
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = case("fib", 64)
    ctx = stark.StarkContext(6, 2)

    def refused(fn, *words):
        with pytest.raises(rt.RuntimeError) as e:
            fn()
        assert e.value.code == rt.ERR_ARGUMENT and all(w in e.value.message for w in ("zkir_prove_rate",) + words), e.value.message
    for mode in (3, 4):
        p = rt.PublicInputsC.from_buffer_copy(pub); p.deferred = mode
        refused(lambda: stark.prove_rate(ctx, tr, p, 5, 4), "mode")
    refused(lambda: stark.prove_rate(ctx, tr, pub, 0, 4), "num_queries")
    refused(lambda: stark.prove_rate(ctx, tr, pub, 129, 4), "num_queries")
    refused(lambda: stark.prove_rate(ctx, tr, pub, 5, 25), "pow_bits")
    seg = rt.PublicInputsC.from_buffer_copy(pub); seg.writes_before = 1
    refused(lambda: stark.prove_rate(ctx, tr, seg, 5, 4), "segment")
    out, n = C.POINTER(C.c_uint32)(), C.c_uint64()
    L = rt.lib()
    assert L.zkir_prove_rate(ctx.handle, None, C.byref(pub), 5, 4, C.byref(out), C.byref(n), None, None) == rt.ERR_ARGUMENT and b"null" in L.zkir_last_error()
    assert L.zkir_prove_rate(None, C.byref(tr.c), C.byref(pub), 5, 4, C.byref(out), C.byref(n), None, None) == rt.ERR_ARGUMENT
    assert L.zkir_prove_rate(ctx.handle, C.byref(tr.c), C.byref(pub), 5, 4, None, C.byref(n), None, None) == rt.ERR_ARGUMENT
    other = stark.StarkContext(7, 2)
    refused(lambda: stark.prove_rate(other, tr, pub, 5, 4), "log_n")
    # zkir_prove keeps refusing such a context; the rate entry serves it
    with pytest.raises(rt.RuntimeError):
        stark.prove(ctx, tr, pub)
    assert rt.verify_rate(stark.prove_rate(ctx, tr, pub, 5, 4), pub, 5, 4) == 0
    other.close(); ctx.close()


def test_a_blowup2_context_serves_both_provers_in_turn():
    """stark.prove, stark.prove_rate, stark.prove on ONE log_blowup 1 context: the workspace and the selector table are shared; zkir_prove's bytes stay the oracle's"""
    from zkir_amd import stark
    blob, log, tr, rows, opub, pub = case("fib", 1000)
    ctx = stark.StarkContext(10)
    first = stark.prove(ctx, tr, pub)
    rate = stark.prove_rate(ctx, tr, pub, 7, 4)
    third = stark.prove(ctx, tr, pub)
    assert np.array_equal(first, third) and np.array_equal(first, so.prove(rows, opub))
    assert rt.verify_rate(rate, pub, 7, 4) == 0 and rt.verify(first, pub) == 0
    with pytest.raises(rt.RuntimeError):                                  # the workspace no longer holds the rate proof's matrices
        stark.rate_last_matrices(ctx)
    ctx.close()

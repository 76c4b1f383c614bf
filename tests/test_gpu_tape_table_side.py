"""(mode 4) The tapes' share of the lookup table side and the hash tape's record checks ON THE DEVICE (csrc/tape_table.inl: hash_table_side_kernel, wide_table_side_kernel,
hash_tape_check_kernel — what zkir_prove runs on the tape its device witness built) against the host forms and the Python-integer reference (tests/tape_side_ref.py), and
the whole-proof guard: proofs made through them equal the oracle's word for word."""
import numpy as np
import pytest

import tape_side_ref as R
from oracle import api as oracle, stark_api as so
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("name", R.SYNTHETIC)
def test_device_table_side_equals_host_and_reference_on_designed_tapes(name):
    """(a) the empty tape (sum zero, nothing launched), (b) len = 0, (c) one span and two spans, (d) a 2^17-byte call (16 388 cells) between two 8-cell calls — the cell's
    search for its call crosses workgroups, many partial sums —, (e) item counts of exactly the workgroup size and +- 1, (f) the five wide opcodes at their edges and more
    records than a workgroup, (g) both sections at once."""
    hs, nb, ws = R.synthetic(name)
    dev = rt.tape_table_side(hs, nb, ws, R.ALPHA, R.LAM, device=True)
    host = rt.tape_table_side(hs, nb, ws, R.ALPHA, R.LAM, device=False)
    for k in ("sum", "hh", "ww"):
        assert np.array_equal(dev[k], host[k]), (name, k)
    R.assert_equal(dev, R.synthetic_reference(name), name)
    if name == "empty":
        assert not dev["sum"].any() and dev["hh"].shape == (0, 4) and dev["ww"].shape == (0, 4)
    if name.startswith("items"):
        assert int(hs[0]) + len(nb) == int(name[5:]) and abs(int(name[5:]) - R.NT) <= 1


def test_record_order_of_the_wide_section_permutes_ww_and_keeps_the_sum():
    a = rt.tape_table_side(*R.synthetic("wide_sorted"), R.ALPHA, R.LAM, device=True)
    b = rt.tape_table_side(*R.synthetic("wide_reversed"), R.ALPHA, R.LAM, device=True)
    assert np.array_equal(a["sum"], b["sum"]) and np.array_equal(a["ww"], b["ww"][::-1]) and len(a["ww"]) == len(R.RECORD_OPS)


@pytest.mark.parametrize("name", R.REAL)
def test_device_table_side_and_checks_on_the_sections_of_real_runs(name):
    hs, nb, ws, n_real, code_end = R.real_sections(name)
    alpha, lam = [7, R.P - 1, 0, 123456], [2, 0, 0, 1]
    dev = rt.tape_table_side(hs, nb, ws, alpha, lam, device=True)
    host = rt.tape_table_side(hs, nb, ws, alpha, lam, device=False)
    for k in ("sum", "hh", "ww"):
        assert np.array_equal(dev[k], host[k]), (name, k)
    R.assert_equal(dev, R.reference(hs, nb, ws, alpha, lam), name)
    assert rt.hash_tape_check(hs, n_real, code_end, device=True) == 0


def test_device_check_equals_parse_section():
    """0 on the valid three-call tape; on every single mutation and on tapes with two faults in different records the host's code: the lowest record wins."""
    base, _ = R.check_tape()
    assert rt.hash_tape_check(base, R.CHECK_N_REAL, R.CHECK_CODE_END, device=True) == 0
    seen = set()
    for name, words in R.check_mutations():
        host = rt.hash_tape_check(words, R.CHECK_N_REAL, R.CHECK_CODE_END, device=False)
        assert host == R.expected_check_code(words) != 0, name
        assert rt.hash_tape_check(words, R.CHECK_N_REAL, R.CHECK_CODE_END, device=True) == host, name
        seen.add(host)
    assert seen == {4, 55, 56}
    assert rt.hash_tape_check(np.zeros(0, np.uint32), 10, 0x2000, device=True) == 4 == rt.hash_tape_check(np.zeros(0, np.uint32), 10, 0x2000, device=False)
    assert rt.hash_tape_check(R.EMPTY, 10, 0x2000, device=True) == 0


def test_a_malformed_section_is_refused_alike():
    hs, nb, ws = R.synthetic("both")
    bad = hs.copy(); bad[1 + 8 + 5 + 2] = 0x10000                                       # a piece of the first call's second cell
    for device in (False, True):
        with pytest.raises(rt.RuntimeError) as e:
            rt.tape_table_side(bad, nb, ws, R.ALPHA, R.LAM, device=device)
        assert e.value.code == rt.ERR_ARGUMENT and "56" in e.value.message


def _device_trace(blob, ins, cfg):
    from zkir_amd import pipeline as pl
    log = rt.interpret(blob, ins, rt.VMConfig(enable_execution_trace=True, **cfg))
    ddl = pl.upload(log); tr = pl.DeviceTrace(ddl); pl.trace_fill(pl.trace_fill_args(ddl, tr))
    return log, tr


@pytest.mark.parametrize("name", ["sha256_hello", "signed_division_loop", "wide_and_hash"])
def test_device_witness_proof_equals_the_oracles(name):
    """Hash calls only, wide-tape rows only, both: the proof zkir_prove makes with no witness from the caller — the table side of both tapes formed by the kernels — equals
    so::prove's word for word, and verifies."""
    from zkir_amd import stark
    blob, ins, cfg = R.real_program(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)
    log, tr = _device_trace(blob, list(ins), cfg)
    opub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), wide_mode=True)
    pub = rt.public_inputs(log, blob, list(ins), wide_mode=True, hash_witness="device")
    assert pub.deferred == 4 and not pub.mem_old and not pub.hash_section
    ctx = stark.StarkContext(stark.padded_log_n(len(ores.rows)))
    proof = stark.prove(ctx, tr, pub)
    want = so.prove(ores.rows, opub)
    lay = stark.proof_layout(proof)
    assert (int(proof[lay["hash_section"]]) > 0) == (name != "signed_division_loop") and (int(proof[lay["wide_section"]]) > 0) == (name != "sha256_hello")
    assert len(proof) == len(want) and np.array_equal(proof, want)
    assert rt.verify(proof, pub) == 0 and rt.verify(proof) == 0
    ctx.close(); log.close()


def test_sha_chain_at_2p12_device_witness_proof_equals_the_host_witness_proof():
    """spec.sha256_chain_program() at 2^12 cycles: the same bytes from the device witness (tape checked and table side formed on the device) and from the host witness (parsed
    on the host, the hash calls' table side on host threads)."""
    from zkir_amd import stark
    blob, ins, cfg = R.real_program("sha_chain_2p12")
    log, tr = _device_trace(blob, ins, cfg)
    ctx = stark.StarkContext(12)
    got = stark.prove(ctx, tr, rt.public_inputs(log, blob, [], wide_mode=True, hash_witness="device"))
    pub_h = rt.public_inputs(log, blob, [], wide_mode=True, mem_witness="host")
    want = stark.prove(ctx, tr, pub_h)
    assert got.tobytes() == want.tobytes() and rt.verify(got, pub_h) == 0
    assert int(got[stark.proof_layout(got)["hash_section"]]) >= (1 << 12) // 6 - 16
    ctx.close(); log.close()

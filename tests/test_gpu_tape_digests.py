"""(mode 4) hash_tape_new_bytes_kernel (csrc/tape_digest.inl): what every hash call of a tape wrote, recomputed ON THE DEVICE — a lane per call of at most L_dev = 1024
bytes, the longer calls on host threads — against the host form (hashcall::new_bytes) word for word, and on the designed tape against the oracle's digests
(tests/tape_digest_ref.py)."""
import numpy as np
import pytest

import tape_digest_ref as D
import tape_side_ref as R
from zkir_amd import runtime as rt

pytestmark = pytest.mark.gpu


def _same(words, what):
    dev = rt.hash_tape_new_bytes(words, device=True)
    host = rt.hash_tape_new_bytes(words, device=False)
    assert dev.shape == host.shape, what
    bad = np.nonzero(dev != host)[0]
    assert len(bad) == 0, (what, "first differing cell", int(bad[0]), hex(int(dev[bad[0]])), hex(int(host[bad[0]])))
    return dev


def test_device_equals_host_and_the_oracle_on_the_designed_tape():
    dev = _same(D.tape("designed"), "designed")
    assert np.array_equal(dev, D.designed_expected())


@pytest.mark.parametrize("name", ["l_dev", "calls255", "calls256", "calls257", "len2p17"])
def test_device_equals_host_at_the_path_and_workgroup_edges(name):
    """L_dev - 1, L_dev, L_dev + 1 for each kind (the last lane-hashed lengths and the first host-hashed one); 255 / 256 / 257 calls (the last workgroup partial, full, one
    lane); the 2^17-byte call between two short ones (16 388 cells copied by the cell kernel, the call itself hashed by the host)."""
    words = D.tape(name)
    dev = _same(words, name)
    if name == "l_dev":
        assert sorted({c[2] for c in R.parse_tape(words)}) == [D.L_DEV - 1, D.L_DEV, D.L_DEV + 1]
        assert np.array_equal(dev, D.expected_new_bytes(words))


def test_one_call_of_max_len_per_kind():
    """hashcall::MAX_LEN = 1 MiB itself, SHA-256, Keccak-256 and BLAKE3 (1024 chunks), with a short call between them: 393 240 cells.  Both forms hash these calls with
    hashcall::new_bytes, so the oracle's digests of the three messages are the independent side (D.expected_output_cells)."""
    words = D.tape("max_len")
    assert sorted(c[2] for c in R.parse_tape(words)) == [32, D.MAX_LEN, D.MAX_LEN, D.MAX_LEN]
    dev = _same(words, "max_len")
    at, want = D.expected_output_cells(words)
    assert len(at) == 4 + 4 + 5 + 5 and np.array_equal(dev[at], want)


@pytest.mark.parametrize("name", R.REAL)
def test_device_equals_host_on_the_sections_of_real_runs(name):
    """.. and both equal what the interpreter's hash_outs records say the calls wrote (what the prover's table side is made from)."""
    hs, nb, _, _, _ = R.real_sections(name)
    dev = _same(hs, name)
    assert np.array_equal(dev, nb)


def test_a_malformed_section_is_refused_alike():
    bad = D.tape("designed").copy(); bad[1 + 8 + 5 + 2] = 0x10000
    for device in (False, True):
        with pytest.raises(rt.RuntimeError) as e:
            rt.hash_tape_new_bytes(bad, device=device)
        assert e.value.code == rt.ERR_ARGUMENT and "56" in e.value.message
    assert len(rt.hash_tape_new_bytes(R.EMPTY, device=True)) == 0

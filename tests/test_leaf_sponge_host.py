"""Host builds of what the full-block leaf sponge and the 2-to-1 compression run (poseidon2.h, round 28): no device needed.

* permute_scaled_quad<Q> — permute_scaled with its last linear layer computed for ONE quad, M4(q0 + q1 + q2 + qQ) — must leave, for Q = 0, 1, 2, exactly words
  4Q .. 4Q + 3 of permute_scaled on the same RAW input words, over the whole documented input range (below 1.96 p).
* the sponge over full blocks with the constants derived forwards from the factor the words carry (generate(c, f0), f0 = 1 and f0 = R) gives the oracle's hash_elems."""
import numpy as np
import pytest

from oracle import stark_api as so
from zkir_amd import runtime as rt

P = so.P
R = (1 << 32) % P
LAZY_MAX = P * 196 // 100            # the largest word a linear layer of permute_scaled admits (poseidon2.h: inputs below 1.96 p)


def _quads(states):
    states = np.ascontiguousarray(states, dtype=np.uint32)
    full, quads = np.zeros_like(states), np.zeros_like(states)
    rt.lib().zkir_poseidon2_scaled_quads(states.ctypes.data, len(states), full.ctypes.data, quads.ctypes.data)
    return full, quads


def test_quad_layer_equals_the_full_layer_on_random_states():
    rng = np.random.default_rng(28)
    states = rng.integers(0, LAZY_MAX + 1, (10_000, 12)).astype(np.uint32)
    full, quads = _quads(states)
    assert full.any() and not np.array_equal(full[0], full[1])
    for q in range(3):
        assert np.array_equal(quads[:, 4 * q:4 * q + 4], full[:, 4 * q:4 * q + 4]), f"quad {q}"


def test_quad_layer_equals_the_full_layer_at_the_edges():
    edges = [np.zeros(12, np.uint32), np.full(12, P - 1, np.uint32), np.full(12, LAZY_MAX, np.uint32)]
    for base in (0, P - 1):
        for i in range(12):                                       # the largest admitted lazy word in every position
            s = np.full(12, base, np.uint32)
            s[i] = LAZY_MAX
            edges.append(s)
    full, quads = _quads(np.stack(edges))
    assert np.array_equal(quads, full)
    # the raw words mean what permute_scaled's callers read: canonical states through the documented scale factors give the oracle's permutation
    canon = np.stack([np.zeros(12, np.uint32), np.full(12, P - 1, np.uint32), np.arange(12, dtype=np.uint32)])
    for s in canon:
        got = s.copy()
        rt.lib().zkir_poseidon2_permute_scaled(got.ctypes.data, 1)
        assert np.array_equal(got, so.permute(s))


def _sponge(words, form):
    words = np.ascontiguousarray(words, dtype=np.uint32)
    out = np.zeros(4, np.uint32)
    assert rt.lib().zkir_poseidon2_sponge_full_blocks(words.ctypes.data, len(words), form, out.ctypes.data) == rt.ZKIR_OK
    return out


def _rows(width):
    rng = np.random.default_rng(width)
    rows = [rng.integers(0, P, width).astype(np.uint32) for _ in range(40)]
    rows += [np.zeros(width, np.uint32), np.full(width, P - 1, np.uint32), np.ones(width, np.uint32)]
    mixed = np.zeros(width, np.uint32); mixed[::3] = P - 1; mixed[1::3] = 1
    return rows + [mixed]


@pytest.mark.parametrize("width", [8, 16, 152])
def test_forward_derived_sponge_equals_the_oracle(width):
    """form 0: the constants every kernel uses (words scaled on their way in); 1: derived from the input factor 1, canonical words absorbed as they lie; 2: from the
    input factor R, the same words in Montgomery form."""
    for row in _rows(width):
        want = so.hash_elems(row)
        mont = (row.astype(np.uint64) * R % P).astype(np.uint32)
        assert np.array_equal(_sponge(row, 0), want)
        assert np.array_equal(_sponge(row, 1), want)
        assert np.array_equal(_sponge(mont, 2), want)


def test_sponge_hook_refuses_ragged_rows():
    w = np.zeros(12, np.uint32)
    out = np.zeros(4, np.uint32)
    for n, form in ((0, 0), (7, 0), (12, 1), (8, 3)):
        assert rt.lib().zkir_poseidon2_sponge_full_blocks(w.ctypes.data, n, form, out.ctypes.data) == rt.ERR_ARGUMENT

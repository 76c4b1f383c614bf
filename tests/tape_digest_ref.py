"""What tests/test_tape_digests.py (host) and tests/test_gpu_tape_digests.py (GPU) share: designed hash tapes for zkir_hash_tape_new_bytes_* and the Python reconstruction
of what every call writes — the message read out of the cells' OLD bytes, the digest from the oracle (oracle.api sha256 / keccak256 / blake3: the independent reference),
the 32 bytes laid over the old bytes at out_ptr.  Nothing here is computed by the product."""
import functools

import numpy as np

import tape_side_ref as R

L_DEV = 1024                                                  # csrc/tape_digest.inl TAPE_L_DEV: a lane hashes calls up to this length, the host the longer ones
MAX_LEN = 1 << 20                                             # hashcall::MAX_LEN

SHA_LENS = [0, 1, 55, 56, 63, 64, 65, 119, 120, 128]
KECCAK_LENS = [0, 1, 135, 136, 137, 271, 272, 273]
BLAKE3_LENS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 2048, 2049, 3072]      # (3072: three chunks, a tree that is not a power of two)


def fast_tape(calls, seed=1):
    """R.make_tape's section for calls with many cells (vectorised; random old bytes and previous-access times at most the cycle)"""
    rng = np.random.default_rng(seed)
    parts = [np.array([len(calls)], np.uint32)]
    for cycle, in_ptr, length, out_ptr, kind in calls:
        n = len(R.cells_of(in_ptr, length, out_ptr)) if length < 4096 else None
        if n is None:                                             # (closed form for the long ones: the ranges used here do not overlap)
            n = ((in_ptr + length - 1) >> 3) - (in_ptr >> 3) + 1 + ((out_ptr + 31) >> 3) - (out_ptr >> 3) + 1
        rec = np.zeros((n, 5), np.uint32)
        rec[:, 0] = rng.integers(0, cycle + 1, n)
        rec[:, 1:] = rng.integers(0, 1 << 16, (n, 4))
        parts += [np.array([cycle, in_ptr & 0xFFFFF, in_ptr >> 20, length, out_ptr & 0xFFFFF, out_ptr >> 20, kind, n], np.uint32), rec.reshape(-1)]
    return np.concatenate(parts)


def designed_calls():
    """every length edge of the three functions, in_ptr & 7 over 0..7, out_ptr & 7 over 0..7 (kinds 5 / 6) and over 0 and 4 (kind 3), and the placements of the output
    against the input"""
    calls, cycle = [], 1
    def add(in_ptr, length, out_ptr, kind):
        nonlocal cycle
        calls.append((cycle, in_ptr, length, out_ptr, kind)); cycle += 3
    i = 0
    for kind, lens in ((3, SHA_LENS), (5, KECCAK_LENS), (6, BLAKE3_LENS)):
        for length in lens:
            add(0x10000 + 0x1000 * i + i % 8, length, 0x800000 + 64 * i + (4 * (i % 2) if kind == 3 else (3 * i + 1) % 8), kind)
            i += 1
    for k in range(8):                                            # every in / out alignment against every other, on a message that crosses cells
        add(0x100000 + 64 * k + k, 13, 0x200000 + 64 * k + (7 - k), 5 if k % 2 else 6)
    add(0x40003, 100, 0x40021, 5)                                 # the output inside the input: the message is the OLD bytes
    add(0x40003, 100, 0x40024, 3)
    add(0x50009, 5, 0x50002, 6)                                   # the input inside the output's cells
    add(0x60000, 12, 0x6000C, 3)                                  # input and output share exactly one cell (0x60008)
    add(0x70005, 70, 0x6F000, 6)                                  # two spans, the output's first
    add(0x70005, 70, 0x70400, 6)                                  # two spans, the input's first
    add(0x80003, 0, 0x80003, 5)                                   # len = 0 at an odd pointer the output shares
    add((1 << 40) - 37, 37, (1 << 40) - 32, 5)                    # the top of the address space
    assert {c[1] & 7 for c in calls} == set(range(8)) and {c[3] & 7 for c in calls if c[4] != 3} == set(range(8)) and {c[3] & 7 for c in calls if c[4] == 3} == {0, 4}
    assert len(R.cells_of(0x60000, 12, 0x6000C)) == 2 + 5 - 1
    return calls


@functools.lru_cache(maxsize=None)
def tape(name):
    if name == "designed":
        return R.make_tape(designed_calls(), seed=11)[0]
    if name == "l_dev":                                           # L_dev - 1, L_dev, L_dev + 1 for each kind, odd alignments
        return fast_tape([(5 + 2 * j, 0x10000 + 0x1000 * j + j % 8, L_DEV - 1 + j % 3, 0x800000 + 64 * j + (4 if k == 3 else 5), k) for j, k in enumerate([3, 3, 3, 5, 5, 5, 6, 6, 6])], seed=3)
    if name in ("calls255", "calls256", "calls257"):              # the last workgroup is partial / full / one lane
        n = int(name[5:])
        return fast_tape([(1 + k, 0x2000 + 64 * k + k % 8, 32 + k % 3, 0x400000 + 64 * k + 4 * (k % 2), (3, 5, 6)[k % 3]) for k in range(n)], seed=n)
    if name == "len2p17":
        return R.synthetic("len2p17")[0]
    if name == "max_len":                                         # one call of MAX_LEN per kind (hashed by the host: above L_dev), a short call between them
        return fast_tape([(10, 0x1000003, MAX_LEN, 0x9000001 & ~3, 3), (11, 0x2000, 32, 0x3000, 3), (12, 0x3000005, MAX_LEN, 0x9000101, 5), (13, 0x5000000, MAX_LEN, 0x9000207, 6)], seed=8)
    raise KeyError(name)


def expected_new_bytes(words):
    """per touched cell, in the section's order: old bytes, the call's 32 output bytes over them (kind 3: the eight words little-endian; kinds 5 / 6: the digest in order)"""
    from oracle import api as oracle
    out = []
    for _, in_ptr, length, out_ptr, kind, cells in R.parse_tape(words):
        addrs = R.cells_of(in_ptr, length, out_ptr)
        mem = {}
        for addr, (_, old) in zip(addrs, cells):
            for k in range(8):
                mem[addr + k] = (old >> (8 * k)) & 0xFF
        msg = bytes(mem[in_ptr + k] for k in range(length))      # reads come before writes
        written = oracle.sha256(msg).astype("<u4").tobytes() if kind == 3 else oracle.keccak256(msg) if kind == 5 else oracle.blake3(msg)
        assert len(written) == 32
        for k in range(32):
            mem[out_ptr + k] = written[k]
        out += [sum(mem[a + k] << (8 * k) for k in range(8)) for a in addrs]
    return np.array(out, np.uint64)


def expected_output_cells(words):
    """(indices, values): expected_new_bytes on the cells under every call's OUTPUT alone, for tapes whose calls are long and whose ranges do not overlap (fast_tape):
    the message and the cell arithmetic are vectorised, the digest is the oracle's"""
    from oracle import api as oracle
    w = np.asarray(words, np.uint32)
    at, want, q, base = [], [], 1, 0
    for _ in range(int(w[0])):
        _, in_lo, in_hi, length, out_lo, out_hi, kind, n = (int(x) for x in w[q:q + 8])
        in_ptr, out_ptr = in_lo | (in_hi << 20), out_lo | (out_hi << 20)
        rec = w[q + 8:q + 8 + 5 * n].reshape(n, 5).astype(np.uint64)
        old = rec[:, 1] | (rec[:, 2] << np.uint64(16)) | (rec[:, 3] << np.uint64(32)) | (rec[:, 4] << np.uint64(48))
        n_in, n_out = ((in_ptr + length - 1) >> 3) - (in_ptr >> 3) + 1, ((out_ptr + 31) >> 3) - (out_ptr >> 3) + 1
        assert n == n_in + n_out and (out_ptr >> 3) > ((in_ptr + length - 1) >> 3)      # disjoint, the input's cells first (cells lie in address order)
        msg = old[:n_in].astype("<u8").tobytes()[in_ptr & 7:(in_ptr & 7) + length]
        written = oracle.sha256(msg).astype("<u4").tobytes() if kind == 3 else oracle.keccak256(msg) if kind == 5 else oracle.blake3(msg)
        cells = bytearray(old[n_in:].astype("<u8").tobytes())
        cells[out_ptr & 7:(out_ptr & 7) + 32] = written
        at += list(range(base + n_in, base + n)); want += list(np.frombuffer(bytes(cells), "<u8"))
        q += 8 + 5 * n; base += n
    return np.array(at), np.array(want, np.uint64)


@functools.lru_cache(maxsize=None)
def designed_expected():
    return expected_new_bytes(tape("designed"))

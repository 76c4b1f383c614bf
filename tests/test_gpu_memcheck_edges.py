"""The device memory witness (zkir_amd/csrc/memcheck.hip) on SYNTHETIC traces that put every access where the test wants it in the sorted (cell, row) order — on the edges
of the segmented scan's geometry (8 elements per thread, 512 per wave, 2048 per tile, ceil(n_tiles / 256) tiles per spine thread) and of the mode-4 row pipeline (256 rows
per block, ceil(n_blocks / 256) blocks per spine thread) — bit-exact against the plain replay of tests/memcheck_ref.py, which tests/test_memcheck_ref.py holds to the host
replay on real runs.

The kernels read three things of a trace: `instruction`, `registers` and `reg_stride` (access_of / row_kind / hout_kernel in memcheck.hip read nothing else), so the tests
write those columns directly; the other column pointers point at a small dummy.  Every input stays inside what the VM can emit: naturally aligned accesses, addresses below
2^40 and hash calls a proof can state (but in the refusal cases), rows below 2^26.

Every host output array is a little larger than needed and prefilled with the byte 0xA5: behind the counts the call reports nothing may be written, and mem_old / mem_told
must be 0 on the rows that access nothing (the reference has them 0)."""
import ctypes as C

import numpy as np
import pytest
import torch

from zkir_amd import runtime as rt, spec

import memcheck_ref as mr

pytestmark = pytest.mark.gpu

O, E = spec.Opcode, spec.encode
FILL, SLACK = 0xA5, 64
THREAD, WAVE, TILE = 8, 512, 2048

# the program image: 9 code words and 17 data bytes — 53 bytes, so the last image cell (0x1030) holds 5 image bytes and 3 zero bytes
CODE = [E(O.ADDI, 1, 0, imm=0x7F3), E(O.XORI, 2, 1, imm=-0x55), E(O.ADD, 3, 1, 2), E(O.LD, 4, 5, imm=-8), E(O.SB, rs1=5, rs2=9, imm=77), E(O.MUL, 9, 9, 9),
        E(O.BNE, rs1=1, rs2=2, imm=-12), E(O.JAL, 15, imm=-4), spec.ebreak()]
BLOB = spec.Program.from_code(CODE, data=bytes(range(0xC1, 0xC1 + 17))).to_bytes()
IMAGE_LEN = 4 * len(CODE) + 17
LAST_IMAGE_CELL = 0x1000 + IMAGE_LEN // 8 * 8
assert IMAGE_LEN % 8 == 5 and len(BLOB) == 32 + IMAGE_LEN

# ---- instruction words: a table of spec.encode's words, indexed per row -------------------------------------------------------------------------------------------------
KINDS = (O.LB, O.LBU, O.LH, O.LHU, O.LW, O.LD, O.SB, O.SH, O.SW, O.SD)       # an access's `kind` is its index here: 0..5 loads, 6..9 stores
WIDTH = np.array([1, 1, 2, 2, 4, 8, 1, 2, 4, 8])
LW_, LD_, SB_, SH_, SW_, SD_ = 4, 5, 6, 7, 8, 9
IMMS = (0, 8, -8, 1, -3, 65535, -65536)                                       # rs1 = address - imm mod 2^64: a small address under a positive immediate wraps past 2^64
REGSETS = ((5, 9), (7, 14), (15, 1), (13, 10))                                # (base register, stored / loaded register); the last pair: the hash calls' registers as plain ones
WORDS = np.array([[[E(op, rd=v, rs1=b, imm=imm) if op <= O.LD else E(op, rs1=b, rs2=v, imm=imm) for b, v in REGSETS] for imm in IMMS] for op in KINDS], np.uint32)
IMM_U64 = np.array([imm & mr.M64 for imm in IMMS], np.uint64)
BASE_REG, VALUE_REG = np.array([b for b, _ in REGSETS]), np.array([v for _, v in REGSETS])
# rows that access nothing: ALU / branch / jump words whose opcodes sit next to the load and store ranges, EBREAK, and ECALLs that are no hash call
IDLE = np.array([E(O.ADDI, 3, 4, imm=-1), E(O.CMOVNZ, 1, 2, 3), E(O.BEQ, rs1=5, rs2=9, imm=8), E(O.JAL, 1, imm=8), E(O.SRAI, 2, 2, imm=63), spec.ebreak(), spec.ecall()], np.uint32)
NO_HASH_R10 = np.array([0, 1, 2, 7, (1 << 32) + 3, (1 << 63) + 5, 999], np.uint64)


class Run:
    """The two trace columns of a synthetic run of n rows (cap = n rounded up to 16, plus 16: the rows behind n hold stores that no kernel may read as rows)."""

    def __init__(self, n, seed):
        self.n, self.cap = n, (n + 15) // 16 * 16 + 16
        self.rng = rng = np.random.default_rng(seed)
        self.ins = IDLE[rng.integers(0, len(IDLE), self.cap)]
        self.regs = rng.integers(0, 1 << 64, (16, self.cap), dtype=np.uint64)
        self.regs[10] = NO_HASH_R10[rng.integers(0, len(NO_HASH_R10), self.cap)]
        self.ins[n:] = E(O.SD, rs1=5, rs2=9, imm=0)
        self.regs[5, n:] = 0x10
        self.records, self.wrapped = [], 0

    def access(self, rows, kinds, addrs, values):
        """rows[k] becomes the load / store KINDS[kinds[k]] at addrs[k]; values[k] is the stored register (all 64 bits: the store keeps its low bytes)."""
        rows, kinds = np.asarray(rows, np.int64), np.asarray(kinds, np.int64)
        addrs, values = np.asarray(addrs, np.uint64), np.asarray(values, np.uint64)
        assert not ((addrs % WIDTH[kinds].astype(np.uint64)) != 0).any() and len(np.unique(rows)) == len(rows)
        b, c = self.rng.integers(0, len(IMMS), len(rows)), self.rng.integers(0, len(REGSETS), len(rows))
        self.ins[rows] = WORDS[kinds, b, c]
        with np.errstate(over="ignore"):
            self.regs[BASE_REG[c], rows] = addrs - IMM_U64[b]
        self.wrapped += int(np.count_nonzero((IMM_U64[b] < np.uint64(1 << 63)) & (addrs < IMM_U64[b])))      # rs1 + imm passes 2^64 on these rows
        st = kinds >= SB_
        self.regs[VALUE_REG[c][st], rows[st]] = values[st]

    def call(self, row, kind, in_ptr, length, out_ptr, record=True):
        self.ins[row] = spec.ecall()
        self.regs[10:14, row] = [kind, in_ptr, length, out_ptr]
        if record:
            self.records.append((row, self.rng.integers(0, 256, 32, dtype=np.uint8)))

    def hash_outs(self):
        outs = np.zeros(len(self.records), rt.HASH_OUT_DTYPE)
        for k, (row, data) in enumerate(sorted(self.records, key=lambda r: r[0])):
            outs[k]["row"], outs[k]["bytes"] = row, data
        outs["reserved"] = 0xDEAD
        return outs


# ---- the device call ----------------------------------------------------------------------------------------------------------------------------------------------------
_DUMMY = None


def _filled(count, dtype):
    return np.frombuffer(bytes([FILL]) * ((count + SLACK) * np.dtype(dtype).itemsize), dtype).copy()


def device(run, mode, outs=None, blob=BLOB, cap=None, wcap=None, entry=None):
    """-> (rc, arrays, n_cells, n_hash_words).  mode 3 goes through zkir_memcheck_witness_device unless entry == "mode"; cap / wcap: the capacities TOLD to the call (the
    arrays always hold SLACK items more than the reference needs, and at least n cells)."""
    global _DUMMY
    L = rt.lib()
    U64, V = C.c_uint64, C.c_void_p
    L.zkir_memcheck_witness_device.restype = C.c_int
    L.zkir_memcheck_witness_device.argtypes = [C.POINTER(rt.TraceColumnsC), U64, C.c_char_p, C.c_size_t, V, V, V, V, V, U64, C.POINTER(U64), V]
    if _DUMMY is None:
        _DUMMY = torch.zeros(64, dtype=torch.uint8, device="cuda")
    ins_t = torch.from_numpy(run.ins.view(np.int32)).cuda()
    regs_t = torch.from_numpy(run.regs.view(np.int64)).cuda()
    assert ins_t.shape == (run.cap,) and regs_t.shape == (16, run.cap) and run.cap % 16 == 0 and run.n < 1 << 26
    d = _DUMMY.data_ptr()
    cols = rt.TraceColumnsC(d, d, ins_t.data_ptr(), regs_t.data_ptr(), d, d, d, d, run.cap)
    n = run.n
    cells = max(n, int(getattr(run, "n_cells", 0)))              # (n_cells, hash_cells: set by reference() — a hash call touches more cells than the run has rows)
    a = {"mem_old": _filled(n, "<u8"), "mem_told": _filled(n, "<u4"), "cell_addr": _filled(cells, "<u8"), "cell_bytes": _filled(cells, "<u8"), "cell_time": _filled(cells, "<u4")}
    nc, nw = U64(0xA5A5), U64(0xA5A5)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    if mode == 3 and entry != "mode":
        rc = L.zkir_memcheck_witness_device(C.byref(cols), n, blob, len(blob), a["mem_old"].ctypes.data, a["mem_told"].ctypes.data, a["cell_addr"].ctypes.data,
                                            a["cell_bytes"].ctypes.data, a["cell_time"].ctypes.data, cells if cap is None else cap, C.byref(nc), stream)
        return rc, a, int(nc.value), None
    outs = np.zeros(0, rt.HASH_OUT_DTYPE) if outs is None else np.ascontiguousarray(outs)
    words = 1 + 8 * len(outs) + 5 * int(getattr(run, "hash_cells", 0)) + 8        # (a call the reference refuses needs no room)
    a["hash_section"] = _filled(words, "<u4")
    rc = L.zkir_memcheck_witness_device_mode(C.byref(cols), n, blob, len(blob), mode, outs.ctypes.data if len(outs) else None, len(outs), a["mem_old"].ctypes.data,
                                             a["mem_told"].ctypes.data, a["cell_addr"].ctypes.data, a["cell_bytes"].ctypes.data, a["cell_time"].ctypes.data,
                                             cells if cap is None else cap, C.byref(nc), a["hash_section"].ctypes.data, words if wcap is None else wcap, C.byref(nw), stream)
    return rc, a, int(nc.value), int(nw.value)


def _untouched(x, what):
    assert (x.view(np.uint8) == FILL).all(), f"{what}: written at item {int(np.nonzero(x.view(np.uint8) != FILL)[0][0]) // x.dtype.itemsize}"


def _same(got, want, what):
    assert got.dtype == want.dtype and len(got) == len(want), (what, len(got), len(want))
    if not np.array_equal(got, want):
        k = int(np.nonzero(got != want)[0][0])
        raise AssertionError(f"{what}: {int(np.count_nonzero(got != want))} of {len(want)} differ, first at {k}: {int(got[k]):#x}, the reference says {int(want[k]):#x}")


def reference(run, mode, blob=BLOB, outs=None):
    want = mr.replay(run.ins[:run.n], run.regs[:, :run.n], blob, mode, outs if mode == 4 else None)
    if want.refusal is None:
        run.n_cells = len(want.cell_addr)
    if want.refusal is None and mode == 4:
        run.hash_cells = (len(want.hash_section) - 1 - 8 * int(want.hash_section[0])) // 5
    return want


def check(run, mode, blob=BLOB, outs=None, entry=None, want=None):
    """The device's five arrays (and the hash section in mode 4) equal the reference's; nothing is written behind them; rows without an access hold 0."""
    if mode == 4 and outs is None:
        outs = run.hash_outs()
    want = want or reference(run, mode, blob, outs)
    assert want.refusal is None, want.refusal
    rc, got, nc, nw = device(run, mode, outs, blob, entry=entry)
    assert rc == rt.ZKIR_OK, rt.lib().zkir_last_error().decode()
    n = run.n
    assert nc == len(want.cell_addr), (nc, len(want.cell_addr))
    _same(got["mem_told"][:n], want.mem_told, "mem_told"); _same(got["mem_old"][:n], want.mem_old, "mem_old")
    _same(got["cell_addr"][:nc], want.cell_addr, "cell_addr"); _same(got["cell_time"][:nc], want.cell_time, "cell_time"); _same(got["cell_bytes"][:nc], want.cell_bytes, "cell_bytes")
    _untouched(got["mem_old"][n:], "mem_old behind n_real"); _untouched(got["mem_told"][n:], "mem_told behind n_real")
    for name in ("cell_addr", "cell_bytes", "cell_time"):
        _untouched(got[name][nc:], f"{name} behind n_cells")
    if mode == 4:
        assert nw == len(want.hash_section), (nw, len(want.hash_section))
        _same(got["hash_section"][:nw], want.hash_section, "hash_section")
        _untouched(got["hash_section"][nw:], "hash_section behind n_hash_words")
    return want


def check_refused(run, mode, refusal, outs=None, blob=BLOB):
    if mode == 4 and outs is None:
        outs = run.hash_outs()
    assert reference(run, mode, blob, outs).refusal == refusal
    for entry in (None, "mode") if mode == 3 else ("mode",):
        rc, got, nc, nw = device(run, mode, outs, blob, entry=entry)
        assert rc == rt.ERR_ARGUMENT, (rc, entry)
        for name in ("cell_addr", "cell_bytes", "cell_time"):
            _untouched(got[name], f"{name} of a refused call")


# ---- placing accesses: chains of chosen lengths at chosen positions of the sorted array ---------------------------------------------------------------------------------
KIND_P = np.array([0.09] * 6 + [0.20, 0.13, 0.11, 0.02])


def synth(lengths, n, seed, pairs=None, store_ok=None, cells=None, halt_store=False):
    """A run of n rows whose accesses, in sorted (cell, row) order, are chains of the given lengths: chain k — all the accesses of one cell — starts at sorted position
    sum(lengths[:k]).  Cells ascend (the last third lies above 2^39); the rows of a chain ascend, and which rows a chain gets is drawn at random over the whole run: the sort
    has real work to do.  Every chain mixes data: one of 8 or more accesses starts with SB at offsets 0..7 with distinct bytes, then loads, SB / SH / SW at random offsets
    and a rare SD; at every sorted position p of `pairs` (default: every multiple of 512, and 8 past every multiple of 2048) that falls INSIDE a chain, accesses p - 1 and p
    are SB to the same byte with different values — the later one must win across the boundary — and p + 1 is an LD.  store_ok[p] == False turns access p into a load."""
    lengths = np.asarray(lengths, np.int64)
    A, n_chains = int(lengths.sum()), len(lengths)
    assert A <= n - 1
    run = Run(n, seed)
    rng = run.rng
    start = np.concatenate([[0], np.cumsum(lengths)[:-1]])
    cid = np.repeat(np.arange(n_chains), lengths)
    idx = np.arange(A) - start[cid]
    if cells is None:
        cells = 0x2000 + 8 * np.cumsum(rng.integers(1, 4, n_chains)).astype(np.uint64)
        cells[n_chains * 2 // 3:] += np.uint64(1 << 39)
    cells = np.asarray(cells, np.uint64)
    assert (np.diff(cells.astype(np.int64)) > 0).all() and int(cells[-1]) < 1 << 40
    ok = np.ones(A, bool) if store_ok is None else np.asarray(store_ok, bool)
    kinds = rng.choice(10, A, p=KIND_P / KIND_P.sum())
    offs = rng.integers(0, 8, A) // WIDTH[kinds] * WIDTH[kinds]
    values = rng.integers(0, 1 << 64, A, dtype=np.uint64)
    first = (idx < 8) & (lengths[cid] >= 8)
    kinds[first], offs[first] = SB_, idx[first]
    values[first] = (values[first] & np.uint64(mr.M64 ^ 0xFF)) | (0x11 * (idx[first] + 1)).astype(np.uint64)
    if pairs is None:
        pairs = sorted(set(range(WAVE, A, WAVE)) | set(range(THREAD, A, TILE)))
    pairs = np.array([p for p in pairs if 0 < p < A and cid[p - 1] == cid[p] and ok[p - 1] and ok[p]], np.int64)
    if len(pairs):
        kinds[pairs - 1] = kinds[pairs] = SB_
        offs[pairs - 1] = offs[pairs] = pairs % 8 ^ 5
        values[pairs] = values[pairs - 1] ^ np.uint64(0x5A)
        nxt = pairs + 1
        nxt = nxt[(nxt < A)]
        nxt = nxt[(cid[nxt] == cid[nxt - 1]) & ~np.isin(nxt, pairs - 1)]
        kinds[nxt], offs[nxt] = LD_, 0
    turn = ~ok & (kinds >= SB_)
    kinds[turn] = rng.integers(0, 6, int(turn.sum()))
    offs = offs // WIDTH[kinds] * WIDTH[kinds]
    perm = rng.permutation(n - 1)[:A]
    rows = perm[np.lexsort((perm, cid))]
    run.access(rows, kinds, cells[cid] + offs.astype(np.uint64), values)
    if halt_store:                                              # a store on the halt row, into the first chain's cell: it must be ignored
        run.access([n - 1], [SD_], [int(cells[0])], [0x0123456789ABCDEF])
    run.cid, run.kinds, run.pairs, run.A, run.rows = cid, kinds, pairs, A, rows      # (all in sorted order: rows[p] is the row of sorted position p)
    return run


def straddled(run, p):
    """Sorted position p lies inside a chain that stores a partial width before p: a carry across p has bytes to bring."""
    cid, kinds = run.cid, run.kinds
    if not 0 < p < run.A or cid[p - 1] != cid[p]:
        return False
    lo = p - 1
    while lo > 0 and cid[lo - 1] == cid[p]:
        lo -= 1
    return bool(((kinds[lo:p] >= SB_) & (kinds[lo:p] < SD_)).any())


def chain_at(start, length, tail=(1, 1, 1, 9)):
    """`start` filler cells of one access each, a chain of `length`, and behind it three more cells of one access and a short chain (a head right behind the chain)."""
    return [1] * start + [length] + list(tail)


# ---- 1. thread / wave / tile boundaries ---------------------------------------------------------------------------------------------------------------------------------
LENGTHS = (1, 7, 8, 9, 511, 512, 513, 2047, 2048, 2049)
STARTS = (0, 1, 7, 2047, 2048)


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("start", STARTS)
def test_chain_lengths_at_scan_positions(start, mode):
    """Every chain length of LENGTHS starting at sorted position `start` (one run each): over all starts a head falls on the first and on the last element of a thread, a wave
    and a tile, and every length crosses the next boundary up at least once (start 7: length 9 a thread's, 511 a wave's, 2047 a tile's)."""
    for length in LENGTHS:
        lengths = chain_at(start, length)
        A = sum(lengths)
        run = synth(lengths, A + 1 + A // 5, 1000 * start + length)
        for unit in (THREAD, WAVE, TILE):                       # the run is what it claims to be
            p = (start // unit + 1) * unit
            assert straddled(run, p) or not start < p < start + length, (start, length, p)
        check(run, mode)


def test_both_mode3_entries_give_the_same_witness():
    run = synth(chain_at(7, 513), 700, 5)
    check(run, 3, entry="mode")


# ---- 2. a tile without a head ---------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("stores", ["first_and_last_tile", "everywhere"])
def test_a_chain_over_tiles_without_a_head(stores, mode):
    """One chain of 3 * 2048 + 5 accesses from 5 elements before a tile boundary: the tiles behind it hold no head, the whole-tile carry passes through aggregates with
    head = 0 — through two tiles of loads alone (mask 0) when the partial stores lie in the first and the last tile only."""
    start, length = TILE - 5, 3 * TILE + 5
    lengths = chain_at(start, length)
    A = sum(lengths)
    ok = np.ones(A, bool)
    if stores == "first_and_last_tile":
        ok[TILE:3 * TILE] = False
    run = synth(lengths, A + 300, 77, store_ok=ok, pairs=[TILE, 3 * TILE, 3 * TILE + WAVE, 4 * TILE - 7])
    assert straddled(run, TILE) and straddled(run, 2 * TILE) and straddled(run, 3 * TILE) and run.cid[TILE - 5] == run.cid[4 * TILE - 1] != run.cid[4 * TILE]
    if stores == "first_and_last_tile":
        assert not (run.kinds[TILE:3 * TILE] >= SB_).any() and (run.kinds[TILE - 5:TILE] >= SB_).any() and (run.kinds[3 * TILE:4 * TILE] >= SB_).any()
    check(run, mode)


# ---- 3. the head count across tiles -------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
def test_cell_index_behind_tiles_of_single_access_cells(mode):
    """3 * 2048 + 1 cells of one access each, then a chain: every element is a head, the cell index (count - 1) must carry over the tile boundaries."""
    run = synth([1] * (3 * TILE + 1) + [40, 1, 1], 3 * TILE + 1 + 42 + 500, 31)
    want = check(run, mode)
    assert len(want.cell_addr) == 3 * TILE + 4


# ---- 4. / 5. the spine ---------------------------------------------------------------------------------------------------------------------------------------------------
def _long_run(n, A, seed, placed):
    """Chains of random lengths (1 .. 5000, a share of single cells) filling A sorted positions, with a chain of placed[p] accesses starting at every position p of `placed`."""
    rng = np.random.default_rng(seed)
    lengths, pos = [], 0
    for p, length in sorted(placed.items()):
        while pos < p:
            k = min(p - pos, int(rng.integers(1, 5000)) if rng.random() < 0.5 else 1)
            lengths.append(k); pos += k
        lengths.append(length); pos += length
    while pos < A:
        k = min(A - pos, int(rng.integers(1, 5000)) if rng.random() < 0.5 else 1)
        lengths.append(k); pos += k
    return synth(lengths, n, seed)


@pytest.mark.parametrize("mode", [3, 4])
def test_spine_wave_boundary(mode):
    """n_real just above 64 * 2048: a data-mixing chain crosses sorted element 131 072 — tile 63 -> 64, spine lane 63 -> 64."""
    edge = 64 * TILE
    run = _long_run(edge + 900, edge + 800, 64, {edge - 700: 1400})
    assert straddled(run, edge) and edge in run.pairs
    check(run, mode)


def test_spine_with_two_tiles_per_thread_mode3():
    """n_real = 524 288 + 2048 + 3: 258 tiles, two per spine thread.  A chain over tiles 1 to 4 (spine threads 0 -> 2) and one across element 262 144 (spine lane 63 -> 64);
    chains of random lengths everywhere else, so most tile boundaries — the one between the two tiles of one thread among them — carry bytes."""
    n = 524288 + TILE + 3
    mid = 262144
    run = _long_run(n, mid + 9000, 258, {TILE + 100: 3 * TILE + 200, mid - 1500: 3000})
    assert run.cid[TILE + 100] == run.cid[4 * TILE + 299] and all(straddled(run, t * TILE) for t in (2, 3, 4)) and straddled(run, mid)
    assert sum(straddled(run, t * TILE) for t in range(1, run.A // TILE, 2)) >= 40          # even -> odd tile: inside one spine thread
    check(run, 3)


def test_spine_with_two_tiles_per_thread_mode4_megabyte_calls():
    """Fewer than 1000 rows, five Keccak-256 calls of 2^20 bytes over one region (outputs inside it, at its end, behind it, before it, unaligned in it) and a store into a
    cell of the region at most tile boundaries of the sorted array, between two of the calls: about 655 k accesses, 321 tiles, two per spine thread; every tape entry, every
    cell's final bytes."""
    rng = np.random.default_rng(321)
    REG, LEN = 0x100000, 1 << 20
    outs_at = [REG + 0x40, REG + LEN - 32, REG + LEN, REG - 13, REG + 0x80003]
    events = [[] for _ in range(6)]                              # events[g]: the cells stored into before call g (g = 5: behind the last call)
    for g in (0, 1, 2, 5):                                       # stores into the calls' output cells, before the first call and behind the last one too
        events[g] += [(outs_at[0] - REG) // 8, (outs_at[1] - REG) // 8 + 3, (outs_at[4] - REG) // 8 + 1, 7 + g]
    fixed = sorted(c for ev in events for c in ev)
    placed = 0
    for t in range(1, 321):
        # cell c's chain of five hash accesses starts at sorted position 2 + 5 c + (the stores into cells below c): two cells under the region come first
        guess = (t * TILE - 2 - placed) // 5
        c, r = divmod(t * TILE - 2 - placed - sum(f < guess - 8 for f in fixed), 5)
        if c >= LEN // 8:
            break
        if r == 0:                                               # the tile starts with c's chain: lengthen the chain of c - 1 instead, over the boundary
            c, g = c - 1, int(rng.integers(1, 5))
        else:                                                    # r accesses of the chain lie before the boundary: the store goes among them when there is room
            g = int(rng.integers(1, r)) if r >= 2 else int(rng.integers(1, 5))
        events[g].append(c)
        placed += 1
    rows, row = [], 3
    for g in range(6):
        for c in events[g]:
            rows.append((row, c)); row += 1 + int(rng.random() < 0.25)
        if g < 5:
            rows.append((row, None)); row += 2
    n = row + 3
    assert n < 1000
    run = Run(n, 321)
    st = [(r, c) for r, c in rows if c is not None]
    kinds = rng.choice([SB_, SW_, SH_], len(st), p=[0.5, 0.4, 0.1])
    offs = rng.integers(0, 8, len(st)) // WIDTH[kinds] * WIDTH[kinds]
    run.access([r for r, _ in st], kinds, np.array([REG + 8 * c for _, c in st], np.uint64) + offs.astype(np.uint64), rng.integers(0, 1 << 64, len(st), dtype=np.uint64))
    for k, r in enumerate(r for r, c in rows if c is None):
        run.call(r, 5, REG, LEN, outs_at[k])
    outs = run.hash_outs()
    want = reference(run, 4, outs=outs)
    assert want.n_accesses == 5 * (LEN // 8) + 4 + 2 + len(st) and (want.n_accesses + TILE - 1) // TILE == 321
    # the layout the stores were placed for: the sorted (cell, row) list, and how many tile boundaries fall inside a chain with a store or a written output before them
    cell = np.concatenate([np.repeat(np.arange(LEN // 8), 5), np.array([c for _, c in st]), [-2, -1, LEN // 8, LEN // 8 + 1, LEN // 8 + 2, LEN // 8 + 3]])
    arow = np.concatenate([np.tile([r for r, c in rows if c is None], LEN // 8), np.array([r for r, _ in st]), [0] * 6])
    is_store = np.concatenate([np.zeros(5 * (LEN // 8), bool), np.ones(len(st), bool), np.zeros(6, bool)])
    order = np.lexsort((arow, cell))
    cell, is_store = cell[order], is_store[order]
    carried = 0
    for t in range(1, 321):
        p = t * TILE
        lo = p - 1
        while cell[lo - 1] == cell[p]:
            lo -= 1
        carried += bool(cell[p - 1] == cell[p] and is_store[lo:p].any())
    assert carried >= 150, carried
    check(run, 4, outs=outs, want=want)


# ---- 6. small and ragged sizes ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 2049])
def test_small_and_ragged_sizes(n, mode):
    """n_real around the block size; at each size a run with accesses on about half its rows, one where EVERY row before the halt row is an access, and both again with a
    store on the halt row (ignored: it executes nothing)."""
    for dense in (False, True):
        for halt_store in (False, True):
            A = (n - 1) if dense else (n - 1) // 2
            rng = np.random.default_rng(n + dense)
            lengths = []
            while sum(lengths) < A:
                lengths.append(min(A - sum(lengths), int(rng.integers(1, 12))))
            if A == 0:
                run = Run(n, n)
                if halt_store:
                    run.access([n - 1], [SD_], [0x2000], [5])
                run.A = 0
            else:
                run = synth(lengths, n, 10 * n + dense, halt_store=halt_store)
            want = check(run, mode)
            assert want.n_accesses == A and (A > 0) == (len(want.cell_addr) > 0)


@pytest.mark.parametrize("mode", [3, 4])
def test_a_run_without_any_access(mode):
    run = Run(700, 9)
    rc, got, nc, nw = device(run, mode)
    assert rc == rt.ZKIR_OK and nc == 0
    assert not got["mem_old"][:700].any() and not got["mem_told"][:700].any()
    for name in ("cell_addr", "cell_bytes", "cell_time"):
        _untouched(got[name], name)
    check(run, mode)


# ---- 7. address and image edges ---------------------------------------------------------------------------------------------------------------------------------------------
EDGE_CELLS = [0, 8, 0x0FF8, 0x1000, 0x1008, LAST_IMAGE_CELL - 8, LAST_IMAGE_CELL, LAST_IMAGE_CELL + 8, 0x2000, (1 << 20) - 8, 1 << 20, (1 << 39) + 0x1000, (1 << 40) - 16, (1 << 40) - 8]


def _edge_run(seed):
    """Per cell of EDGE_CELLS: an LD first (the image's bytes, or zero), then partial stores and loads of every width."""
    lengths = [12] * len(EDGE_CELLS)
    A = sum(lengths)
    ok = np.ones(A, bool)
    ok[::12] = False                                            # a chain's first access becomes a load ...
    run = synth(lengths, A + 40, seed, cells=EDGE_CELLS, store_ok=ok, pairs=[])
    return run


@pytest.mark.parametrize("mode", [3, 4])
def test_address_and_image_edges(mode):
    """Cell 0, the cell at 0x1000, the last image cell (five image bytes, three zero), the first cell behind the image, the cell at 2^40 - 8; rs1 + imm wraps past 2^64
    wherever the address is below the immediate."""
    run = _edge_run(40)
    assert run.wrapped >= 5                                     # base registers near 2^64 are there
    want = check(run, mode)
    assert [int(a) for a in want.cell_addr] == EDGE_CELLS
    image = BLOB[32:]
    for k, cell in enumerate(EDGE_CELLS):                       # the reference's own first reads, against the image laid out by hand
        first = int(run.rows[12 * k])
        fresh = sum(image[a - 0x1000] << (8 * (a - cell)) for a in range(cell, cell + 8) if 0 <= a - 0x1000 < IMAGE_LEN)
        assert int(want.mem_told[first]) == 0 and int(want.mem_old[first]) == fresh, hex(cell)
        assert (fresh != 0) == (0x1000 <= cell <= LAST_IMAGE_CELL) and (cell != LAST_IMAGE_CELL or 0 < fresh < 1 << 40)
    short = check(run, mode, blob=BLOB[:-1])                    # a blob shorter than its header says: the image counts as empty
    assert not any(int(short.mem_old[int(run.rows[12 * k])]) for k in range(len(EDGE_CELLS)))


@pytest.mark.parametrize("mode", [3, 4])
@pytest.mark.parametrize("addr", [1 << 40, (1 << 40) + 8, (1 << 64) - 8])
def test_an_access_at_2p40_or_above_is_refused(addr, mode):
    run = _edge_run(41)
    idle = [r for r in range(run.n - 1) if (int(run.ins[r]) & 0x7F) not in range(0x30, 0x3C)]
    run.access([idle[3]], [LD_], [addr], [0])
    check_refused(run, mode, "address")


def test_a_hash_row_is_refused_in_mode_3():
    run = _edge_run(42)
    idle = [r for r in range(run.n - 1) if (int(run.ins[r]) & 0x7F) not in range(0x30, 0x3C)]
    run.call(idle[2], 5, 0x3000, 16, 0x3100)
    check_refused(run, 3, "hash")
    check(run, 4)                                               # (mode 4 states the call)


# ---- 8. hash-call row geometry (mode 4, synthetic records) ------------------------------------------------------------------------------------------------------------------
def hash_run(n, calls, regions, seed, density=0.5):
    """n rows: the hash calls `calls` = {row: (kind, in, len, out)} and, on `density` of the other rows before the halt row, loads and stores of every width into the cells
    of `regions` = [(base, n_cells), ..] (a region is drawn per access: a small one next to a large one still gets its share)."""
    run = Run(n, seed)
    rng = run.rng
    free = np.array([r for r in range(n - 1) if r not in calls], np.int64)
    rows = free[rng.random(len(free)) < density]
    kinds = rng.choice(10, len(rows), p=KIND_P / KIND_P.sum())
    offs = rng.integers(0, 8, len(rows)) // WIDTH[kinds] * WIDTH[kinds]
    which = rng.integers(0, len(regions), len(rows))
    base, size = np.array([b for b, _ in regions], np.uint64)[which], np.array([s for _, s in regions])[which]
    cell = (rng.random(len(rows)) * size).astype(np.uint64)
    run.access(rows, kinds, base + np.uint64(8) * cell + offs.astype(np.uint64), rng.integers(0, 1 << 64, len(rows), dtype=np.uint64))
    for row, (kind, in_ptr, length, out_ptr) in sorted(calls.items()):
        run.call(row, kind, in_ptr, length, out_ptr)
    return run


R = 0x3000                                                       # the region the small hash runs work in: 64 cells


def test_hash_rows_on_the_row_block_boundary():
    """Calls on rows 255, 256 and 257 (the last thread of one block of hcount / hrows, the first two of the next), loads and stores all around them into the cells they touch."""
    calls = {255: (5, R + 3, 70, R + 0x101), 256: (3, R + 0x100, 64, R + 0x44), 257: (6, R + 0x40, 9, R + 0x1E0), 100: (6, R, 8, R + 8), 511: (5, R + 1, 1, R + 2), 512: (3, R, 0, R + 4)}
    run = hash_run(700, calls, [(R, 64)], 255, density=0.8)
    want = check(run, 4)
    assert int(want.hash_section[0]) == 6


def test_hash_rows_with_two_row_blocks_per_spine_thread():
    """65 536 + 300 rows: 258 row blocks, two per thread of hcount_spine_kernel; calls on both sides of row 65 536 and in the second block of a thread."""
    n = 65536 + 300
    calls = {100: (5, R, 100, R + 0x80), 300: (6, R + 9, 33, R + 0x21), 65535: (3, R + 0x10, 64, R + 0x14), 65536: (5, R + 0x1F0, 16, R + 0x1D5), 65537: (6, R, 512, R + 0x1E0),
             65800: (3, R + 0x100, 0, R + 0x100)}
    for row in range(2000, 65000, 1777):
        calls[row] = (5, R + row % 200, row % 90, R + 0x100 + row % 64)
    run = hash_run(n, calls, [(R, 64), (0x8000, 3000)], 65536, density=0.5)
    want = check(run, 4)
    assert int(want.hash_section[0]) == len(calls)


def test_hash_call_shapes():
    """len == 0; input and output sharing cells (one span); the two spans in either order; consecutive calls over the same cells with a partial store into an output cell
    between them (hash_run fills every other row with loads and stores into the same 64 cells)."""
    calls = {10: (5, R + 0x55, 0, R + 0x100), 11: (6, 0, 0, R + 0x107), 20: (3, R + 0x80, 40, R + 0x90), 21: (5, R + 0x80, 17, R + 0x90), 22: (6, R + 0xA1, 40, R + 0x83),
             30: (5, R, 24, R + 0x180), 31: (5, R + 0x180, 24, R), 40: (3, R + 0x40, 32, R + 0x60), 42: (3, R + 0x40, 32, R + 0x60), 43: (3, R + 0x40, 64, R + 0x60),
             44: (6, R + 0x60, 32, R + 0x60)}
    run = hash_run(60, calls, [(R, 64)], 8, density=0.0)
    run.access([41], [SH_], [R + 0x66], [0xBEEF])               # the partial store into an output cell, between two calls over the same cells
    run.access([5, 12, 23, 32, 45, 50], [SD_, SW_, SB_, LD_, LW_, LD_], [R + 0x100, R + 0x104, R + 0x91, R + 0x180, R + 0x64, R + 0x60], [1, 2, 3, 4, 5, 6])
    want = check(run, 4)
    assert int(want.hash_section[0]) == len(calls)
    dense = hash_run(300, {5 * k + 7: v for k, v in enumerate(calls.values())}, [(R, 64)], 9, density=0.9)
    check(dense, 4)


def test_a_huge_call_between_tiny_neighbours():
    """A call touching 16 389 cells between neighbours touching 4 and 5 (hcells_kernel finds a hash access's call by bisection over the calls' offsets), with loads and
    stores into the same cells before, between and behind the calls."""
    BIG = 0x40000
    calls = {50: (5, 0, 0, BIG + 0x100), 51: (6, BIG, 16385 * 8, BIG + 0x30000), 52: (5, 0, 0, BIG + 0x203), 53: (3, BIG + 0x100, 32, BIG + 0x30000), 120: (6, BIG + 8, 16385 * 8 - 8, BIG + 0x1001)}
    run = hash_run(200, calls, [(BIG, 16385), (BIG + 0x30000, 4), (BIG + 0x100, 4), (BIG + 0x200, 5)], 16389, density=0.9)
    want = check(run, 4)
    s = want.hash_section
    assert [int(s[8]), int(s[8 + 8 + 5 * 4]), int(s[8 + 2 * 8 + 5 * (4 + 16389)])] == [4, 16389, 5]


@pytest.mark.parametrize("record", [False, True])
def test_a_hash_row_on_the_halt_row(record):
    """The halt row executes nothing: a hash row there makes no call, and a record the log holds for it is ignored."""
    n = 300
    calls = {40: (5, R, 20, R + 0x40), n - 1: (3, R + 0x40, 32, R + 0x80)}
    run = hash_run(n, calls, [(R, 64)], 300 + record, density=0.7)
    if not record:
        run.records = [r for r in run.records if r[0] != n - 1]
    outs = run.hash_outs()
    assert len(outs) == 1 + record
    want = check(run, 4, outs=outs)
    assert int(want.hash_section[0]) == 1
    only = Run(5, 1)                                            # the run's ONLY hash row is the halt row: an empty tape
    only.call(4, 5, R, 8, R + 8, record=record)
    only.access([1, 2], [SW_, LD_], [R + 8, R + 8], [7, 0])
    want = check(only, 4)
    assert len(want.hash_section) == 1


def test_records_that_are_not_the_runs_are_refused():
    calls = {40: (5, R, 20, R + 0x40), 41: (6, R, 20, R + 0x60), 200: (3, R + 0x40, 32, R + 0x80)}
    run = hash_run(300, calls, [(R, 64)], 12, density=0.7)
    outs = run.hash_outs()
    check(run, 4, outs=outs)
    moved = outs.copy(); moved["row"][1] = 42                   # a record whose row is not its call's
    check_refused(run, 4, "records", outs=moved)
    moved = outs.copy(); moved["row"][2] = 199
    check_refused(run, 4, "records", outs=moved)
    check_refused(run, 4, "records", outs=outs[:2])             # fewer records than calls
    check_refused(run, 4, "records", outs=outs[1:])
    check_refused(run, 4, "records", outs=outs[:0])
    more = np.concatenate([outs, outs[-1:]]); more["row"][-1] = 250
    check_refused(run, 4, "records", outs=more)                 # more records than calls
    check(run, 4, outs=outs)                                    # and the call is fine behind the refusals


@pytest.mark.parametrize("case", ["len_over", "out_past_2p40", "in_past_2p40", "sha_out_misaligned", "kind_4"])
def test_a_call_outside_what_a_proof_states_is_refused(case):
    call = {"len_over": (5, R, (1 << 20) + 1, R + 0x100000), "out_past_2p40": (6, R, 8, (1 << 40) - 31), "in_past_2p40": (5, (1 << 40) - 4, 5, R),
            "sha_out_misaligned": (3, R, 8, R + 0x42), "kind_4": (4, R, 8, R + 0x40)}[case]
    run = hash_run(100, {30: (5, R, 8, R + 0x40), 60: call}, [(R, 64)], 13, density=0.5)
    check_refused(run, 4, "hash_range")


# ---- 9. capacity -----------------------------------------------------------------------------------------------------------------------------------------------------------
def test_cell_capacity_one_below_the_count():
    run = synth([3, 1, 9, 1, 1, 20, 2], 60, 90)
    want = reference(run, 3)
    nc = len(want.cell_addr)
    assert nc == 7
    for mode, entry in ((3, None), (3, "mode"), (4, "mode")):
        rc, got, got_nc, _ = device(run, mode, entry=entry, cap=nc - 1)
        assert rc == rt.ERR_ARGUMENT and got_nc == nc, (mode, entry, rc, got_nc)
        for name in ("cell_addr", "cell_bytes", "cell_time"):
            _untouched(got[name], name)
        rc, got, got_nc, _ = device(run, mode, entry=entry, cap=nc)
        assert rc == rt.ZKIR_OK and got_nc == nc


def test_hash_word_capacity_one_below_the_count():
    run = hash_run(100, {30: (5, R, 8, R + 0x40), 60: (6, R + 3, 70, R + 0x100)}, [(R, 64)], 91, density=0.5)
    outs = run.hash_outs()
    want = reference(run, 4, outs=outs)
    nw = len(want.hash_section)
    rc, got, got_nc, got_nw = device(run, 4, outs, wcap=nw - 1)
    assert rc == rt.ERR_ARGUMENT and got_nw == nw and got_nc == len(want.cell_addr)
    for name in ("cell_addr", "cell_bytes", "cell_time", "hash_section"):
        _untouched(got[name], name)
    rc, got, got_nc, got_nw = device(run, 4, outs, wcap=nw)
    assert rc == rt.ZKIR_OK and got_nw == nw and np.array_equal(got["hash_section"][:nw], want.hash_section)

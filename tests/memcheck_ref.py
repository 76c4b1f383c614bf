"""A plain reference of the memory witness of proof modes 3 and 4 (what zkir_amd/csrc/memcheck.hip builds on the device): a sequential replay over a dictionary of 8-byte
cells, walked in row order.  It shares nothing with the library: its inputs are the two trace columns the kernels read (the instruction words and the registers BEFORE each
row), the program blob and — for mode 4 — the records of what every hash syscall wrote (rt.HASH_OUT_DTYPE); it computes no digest.

The rules (memcheck.hip's header, csrc/hashcall.h):
  * the last row executes nothing;
  * a load (opcodes 0x30..0x35: widths 1, 1, 2, 2, 4, 8) reads at register (w >> 11) & 15 plus the sign-extended 17-bit immediate w >> 15, wrapping mod 2^64; a store
    (0x38..0x3B: widths 1, 2, 4, 8) writes the low `width` bytes of register (w >> 11) & 15 at register (w >> 7) & 15 plus the immediate.  The row's mem_old is its cell's
    bytes before the access, its mem_told the time of the cell's previous access (that access's row + 1, 0 when there is none);
  * a row with opcode 0x50 and R10 in {3, 5, 6} is a hash call over R11 (input), R12 (length), R13 (output): it touches the cells under [in, in + len) and [out, out + 32),
    ascending, each once; every touched cell gets a tape entry [time of its previous access][its bytes before the call in four 16-bit pieces], then the record's 32 bytes are
    written at out; the row's own mem_old / mem_told stay 0;
  * memory starts as the program image (code_size + data_size bytes from blob offset 32, at 0x1000; empty when the blob is shorter than that) and zero elsewhere;
  * refused: an address of 2^40 or more ("address"); in mode 3 a hash syscall ("hash"); in mode 4 a call outside what a proof states ("hash_range"); records that are not
    those of the run's hash rows, row for row ("records").

Only the decoding of the rows is vectorised (numpy); the replay itself is a Python loop over the rows that access memory."""
from dataclasses import dataclass

import numpy as np

M64 = (1 << 64) - 1
LIMIT = 1 << 40
MAX_LEN = 1 << 20
IMAGE_BASE = 0x1000
LOAD_WIDTH = {0x30: 1, 0x31: 1, 0x32: 2, 0x33: 2, 0x34: 4, 0x35: 8}
STORE_WIDTH = {0x38: 1, 0x39: 2, 0x3A: 4, 0x3B: 8}
HASH_KINDS = (3, 5, 6)


@dataclass
class Witness:
    refusal: str | None            # None, "address", "hash", "hash_range" or "records"; everything below is None when refused
    mem_old: np.ndarray = None     # u64[n]
    mem_told: np.ndarray = None    # u32[n]
    cell_addr: np.ndarray = None   # u64[n_cells], increasing
    cell_bytes: np.ndarray = None  # u64[n_cells]
    cell_time: np.ndarray = None   # u32[n_cells]
    hash_section: np.ndarray = None  # u32 (mode 4; None in mode 3): hashcall::put_section's layout
    n_accesses: int = 0            # cell accesses: one per load / store row, one per touched cell of a call


def image_of(blob):
    code_size, data_size = int.from_bytes(blob[16:20], "little"), int.from_bytes(blob[20:24], "little")
    n = code_size + data_size
    return bytes(blob[32:32 + n]) if len(blob) >= 32 + n else b""


def hash_call_in_range(kind, in_ptr, length, out_ptr):
    return (kind in HASH_KINDS and (kind != 3 or out_ptr % 4 == 0) and length <= MAX_LEN and in_ptr < LIMIT and in_ptr + length <= LIMIT
            and out_ptr < LIMIT and out_ptr + 32 <= LIMIT)


def hash_call_cells(in_ptr, length, out_ptr):
    cells = set(range(out_ptr & ~7, out_ptr + 32, 8))
    if length:
        cells.update(range(in_ptr & ~7, in_ptr + length, 8))
    return sorted(cells)


def replay(instruction, registers, blob, mode, hash_outs=None):
    """instruction: u32[n]; registers: u64[16][n] (column k = the registers before row k); hash_outs: rt.HASH_OUT_DTYPE records (mode 4)."""
    assert mode in (3, 4)
    ins = np.ascontiguousarray(instruction).view(np.uint32).astype(np.uint64)
    regs = np.ascontiguousarray(registers).view(np.uint64)
    n = len(ins)
    assert regs.shape == (16, n) and n >= 1
    image = image_of(blob)
    padded = bytes(8) + image + bytes(8)

    def fresh(cell):                                           # the cell's bytes before the run
        k = cell - IMAGE_BASE
        return int.from_bytes(padded[k + 8:k + 16], "little") if -8 < k < len(image) else 0

    # ---- decoding, vectorised: which rows touch memory, and where ----
    op = ins & np.uint64(0x7F)
    is_load, is_store = (op >= 0x30) & (op <= 0x35), (op >= 0x38) & (op <= 0x3B)
    is_hash = (op == 0x50) & (regs[10] >= 3) & (regs[10] <= 6)
    active = is_load | is_store | is_hash
    active[n - 1] = False                                      # the last row executes nothing
    rows = np.nonzero(active)[0]
    imm17 = (ins[rows] >> np.uint64(15)) & np.uint64(0x1FFFF)
    imm = np.where(imm17 & np.uint64(0x10000), imm17 | np.uint64(M64 ^ 0x1FFFF), imm17)
    base_reg = np.where(is_load[rows], (ins[rows] >> np.uint64(11)) & np.uint64(15), (ins[rows] >> np.uint64(7)) & np.uint64(15)).astype(np.int64)
    with np.errstate(over="ignore"):
        ea_v = regs[base_reg, rows] + imm                      # u64: wraps mod 2^64
    value_v = regs[((ins[rows] >> np.uint64(11)) & np.uint64(15)).astype(np.int64), rows]
    rows_l, op_l, ea_l, value_l = rows.tolist(), op[rows].tolist(), ea_v.tolist(), value_v.tolist()

    outs = [] if hash_outs is None else [(int(r["row"]), bytes(r["bytes"])) for r in hash_outs]
    if outs and outs[-1][0] + 1 >= n:                          # a record of the last row: the row executes nothing, its record is ignored
        outs.pop()
    next_out = 0

    mem = {}                                                   # cell address -> [bytes, time of the last access]
    mem_old, mem_told = np.zeros(n, np.uint64), np.zeros(n, np.uint32)
    old_l, told_l = [], []
    section, n_calls, n_accesses = [], 0, 0
    for i, o, ea, value in zip(rows_l, op_l, ea_l, value_l):
        if o == 0x50:
            if mode == 3:
                return Witness("hash")
            kind, in_ptr, length, out_ptr = (int(regs[k, i]) for k in (10, 11, 12, 13))
            if not hash_call_in_range(kind, in_ptr, length, out_ptr):
                return Witness("hash_range")
            if next_out >= len(outs) or outs[next_out][0] != i:
                return Witness("records")
            written = outs[next_out][1]
            next_out += 1
            cells = hash_call_cells(in_ptr, length, out_ptr)
            slots = []
            for c in cells:
                s = mem.get(c)
                if s is None:
                    s = mem[c] = [fresh(c), 0]
                slots.append(s)
            before = np.array([s[0] for s in slots], np.uint64)
            entry = np.empty((len(cells), 5), np.uint32)
            entry[:, 0] = [s[1] for s in slots]
            for k in range(4):
                entry[:, 1 + k] = (before >> np.uint64(16 * k)) & np.uint64(0xFFFF)
            section.append(np.array([i, in_ptr & 0xFFFFF, in_ptr >> 20, length, out_ptr & 0xFFFFF, out_ptr >> 20, kind, len(cells)], np.uint32))
            section.append(entry.reshape(-1))
            for k in range(32):
                a = out_ptr + k
                s, sh = mem[a & ~7], 8 * (a & 7)
                s[0] = (s[0] & ~(0xFF << sh)) | (written[k] << sh)
            for s in slots:
                s[1] = i + 1
            n_calls += 1
            n_accesses += len(cells)
            old_l.append(0); told_l.append(0)
            continue
        if ea >= LIMIT:
            return Witness("address")
        cell, off = ea & ~7, ea & 7
        s = mem.get(cell)
        if s is None:
            s = mem[cell] = [fresh(cell), 0]
        old_l.append(s[0]); told_l.append(s[1])
        if o >= 0x38:
            width = STORE_WIDTH[o]
            assert off % width == 0, "the VM emits naturally aligned accesses only"
            mask = ((1 << (8 * width)) - 1) << (8 * off)
            s[0] = (s[0] & ~mask) | ((value << (8 * off)) & mask)
        else:
            assert off % LOAD_WIDTH[o] == 0, "the VM emits naturally aligned accesses only"
        s[1] = i + 1
        n_accesses += 1
    if next_out != len(outs):
        return Witness("records")
    mem_old[rows] = np.array(old_l, np.uint64)
    mem_told[rows] = np.array(told_l, np.uint32)
    addrs = sorted(mem)
    w = Witness(None, mem_old, mem_told, np.array(addrs, np.uint64), np.array([mem[a][0] for a in addrs], np.uint64), np.array([mem[a][1] for a in addrs], np.uint32),
                n_accesses=n_accesses)
    if mode == 4:
        w.hash_section = np.concatenate([np.array([n_calls], np.uint32)] + section)
    return w

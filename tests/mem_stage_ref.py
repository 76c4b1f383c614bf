"""What tests/test_mem_stage_ref.py (host), tests/test_gpu_mem_stage.py and tests/test_gpu_verify_memory_device.py (GPU) and tests/test_mem_stage_sanitized.py share: a
Python reference of the verifier's three stages over the touched-cell section of a mode-3 / mode-4 proof, builders of synthetic sections, and the named cases.  Nothing here
is computed by the product: extension-field products and inverses are the oracle's (so.emul / so.einv), chunk digests the oracle's sponge (so.hash_elems).

The section is [n] + 7 n words; a cell is [address limb 0 (20 bits, a multiple of 8)] [limb 1 (20 bits)] [time of the last access] [final bytes: four 16-bit pieces].
  check    4 where the words end inside the section (or n > 2^28); else the code of the LOWEST failing cell, and within a cell the first of: limb ranges, byte pieces, an
           address not above its predecessor's (54), an overlap with the code words at 0x1000 (55; mode 4 admits the boundary cell of an odd code size in words)
  digests  the sponge digest of every chunk of 512 words (so::observe_section)
  side     sum over the cells of 1 / (alpha - fp(cell, 0, image bytes)) - 1 / (alpha - fp(cell, t_last, final bytes)),
           fp = 7 lambda^11 + limb0 + limb1 lambda + t lambda^2 + sum_k byte_k lambda^(3 + k)"""
import functools

import numpy as np

from oracle import api as oracle, stark_api as so

P = so.P
TAG_MEM, N_TUPLE, CODE_BASE = 7, 11, 0x1000
ALPHA, LAM = [1234567891, 987654321, 5, P - 2], [P - 1, 2, 1357911, 1 << 30]      # canonical challenges nobody derived from the data
SIZES = [0, 1, 73, 74, 146, 255, 256, 257]                    # 73 cells: exactly 512 words; 146: 1023 words; 255 / 256 / 257: the workgroup's edge
SIDE_GRID_CAP, NT = 512, 256                                  # mem_stage.inl: MEM_MAX_BLOCKS workgroups of NT lanes — one cell more and a lane takes two


# ---- the reference ------------------------------------------------------------------------------------------------------------------------------------------------------
def cell_code(c, prev, mode, n_code):
    if c[0] >= 1 << 20 or c[0] & 7 or c[1] >= 1 << 20:
        return 54
    if any(x > 0xFFFF for x in c[3:7]):
        return 54
    addr = c[0] | (c[1] << 20)
    if prev is not None and addr <= (prev[0] | (prev[1] << 20)):
        return 54
    boundary = CODE_BASE + 4 * n_code - 4 if (4 * n_code) % 8 == 4 else CODE_BASE
    if addr + 8 > CODE_BASE and addr < CODE_BASE + 4 * n_code and not (mode == 4 and n_code & 1 and addr == boundary):
        return 55
    return 0


def section_verdict(words, mode, n_code):
    w = [int(x) for x in words]
    if len(w) < 1 or w[0] > 1 << 28 or len(w) < 1 + 7 * w[0]:
        return 4
    for k in range(w[0]):
        code = cell_code(w[1 + 7 * k:8 + 7 * k], w[7 * k - 6:7 * k + 1] if k else None, mode, n_code)
        if code:
            return code
    return 0


def image_cell(blob, addr):
    """the eight bytes of cell `addr` in the VM's initial memory: all zero where the blob is shorter than its header, or than the code + data its header claims"""
    if len(blob) < 32:
        return 0
    code_size, data_size = int.from_bytes(blob[16:20], "little"), int.from_bytes(blob[20:24], "little")
    if 32 + code_size + data_size > len(blob):
        return 0
    v = 0
    for k in range(8):
        a = addr + k
        if a >= CODE_BASE and a - CODE_BASE < code_size + data_size:
            v |= blob[32 + a - CODE_BASE] << (8 * k)
    return v


def _lam_pows(lam):
    out = [[1, 0, 0, 0]]
    for _ in range(N_TUPLE):
        out.append([int(x) for x in so.emul(out[-1], lam)])
    return out


def _den(alpha, pows, c, t, by):
    e = [c[0], c[1], t] + [(by >> (8 * k)) & 0xFF for k in range(8)]
    fp = [TAG_MEM * x % P for x in pows[N_TUPLE]]
    for j, v in enumerate(e):
        fp = [(a + (v % P) * x) % P for a, x in zip(fp, pows[j])]
    return [(a - f) % P for a, f in zip(alpha, fp)]


def table_side(words, blob, alpha=ALPHA, lam=LAM):
    """canonical E4 words; the section must pass check 54"""
    w = [int(x) for x in words]
    assert len(w) == 1 + 7 * w[0]
    pows, T = _lam_pows(lam), [0, 0, 0, 0]
    for k in range(w[0]):
        c = w[1 + 7 * k:8 + 7 * k]
        addr, fin = c[0] | (c[1] << 20), c[3] | (c[4] << 16) | (c[5] << 32) | (c[6] << 48)
        plus, minus = so.einv(_den(alpha, pows, c, 0, image_cell(blob, addr))), so.einv(_den(alpha, pows, c, c[2], fin))
        T = [(a + int(x) - int(y)) % P for a, x, y in zip(T, plus, minus)]
    return T


def chunk_digests(words):
    w = np.ascontiguousarray(words, dtype=np.uint32)
    return [[int(x) for x in so.hash_elems(w[at:at + 512])] for at in range(0, len(w), 512)]


# ---- sections -----------------------------------------------------------------------------------------------------------------------------------------------------------
def section(cells):
    """[n] + 7 n words from rows of (limb 0, limb 1, time, four pieces)"""
    c = np.asarray(cells, dtype=np.int64).reshape(-1, 7)
    return np.concatenate([[len(c)], c.reshape(-1)]).astype(np.uint32)


def cells_at(addrs, seed=1):
    """well-formed cells at the given cell addresses, with times and bytes drawn from `seed`"""
    rng = np.random.default_rng(seed)
    return [[a & 0xFFFFF, a >> 20, int(rng.integers(0, P)), *(int(x) for x in rng.integers(0, 1 << 16, 4))] for a in addrs]


def increasing(n, seed=1, start=0x2000):
    """n well-formed cells at strictly increasing addresses behind `start` (steps of 8 .. 2^24: both limbs move, and limb 0 falls where limb 1 rises)"""
    rng = np.random.default_rng(seed)
    steps = 8 * rng.integers(1, 1 << 21, n, dtype=np.int64)
    return cells_at([int(a) for a in start + np.cumsum(steps) - 8], seed)


@functools.lru_cache(maxsize=None)
def honest(name):
    """(the cells of a real run as the oracle's proof carries them, the program blob)"""
    import programs as pg
    blob, ins, cfg = pg.off_code(name)
    ores = oracle.run(blob, list(ins), enable_execution_trace=True, **{k: v for k, v in cfg.items() if k == "max_cycles"})
    pub = so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), mem_mode=True)
    return so.mem_cells(ores.rows, pub), bytes(blob)


def check_cases():
    """[(what, section words, mode, code size in words, the verdict the case is built to have)] — the reference must agree with the last entry"""
    out = []
    for n in SIZES:
        out.append((f"{n} cells", section(increasing(n, seed=n)), 3, 5, 0))
    for name in ("loads_stores", "pc_carry_mem"):
        cells, blob = honest(name)
        out.append((f"{name}'s cells", section(cells), 3, int.from_bytes(blob[16:20], "little") // 4, 0))
    base = increasing(300, seed=7)
    def bad(at, field, value, cells=base):
        c = [list(x) for x in cells]; c[at][field] = value
        return c
    for at in (0, 299, 255, 256):
        out.append((f"a byte piece of cell {at} = 0x10000", section(bad(at, 3 + at % 4, 0x10000)), 3, 5, 54))
    # two bad cells with different codes: 20 cells below the code, then cell 20 ON the code (55 with two code words), then cells behind it
    low = cells_at([8 * i for i in range(20)] + [0x1000] + [0x1008 + 8 * i for i in range(20)], seed=3)
    out.append(("54 at cell 10 before 55 at cell 20", section(bad(10, 4, 0x10000, low)), 3, 2, 54))
    out.append(("55 at cell 20 before 54 at cell 30", section(bad(30, 4, 0x10000, low)), 3, 2, 55))
    out.append(("54 and 55 in ONE cell: the piece comes first", section(bad(20, 6, 0x10000, low)), 3, 2, 54))
    out.append(("limb 0 = 2^20", section(bad(17, 0, 1 << 20)), 3, 5, 54))
    out.append(("limb 0 not a multiple of 8", section(bad(17, 0, base[17][0] + 4)), 3, 5, 54))
    out.append(("limb 1 = 2^20", section(bad(17, 1, 1 << 20)), 3, 5, 54))
    out.append(("a byte piece = 0x10000", section(bad(17, 6, 0x10000)), 3, 5, 54))
    eq = [list(x) for x in base]; eq[18][0], eq[18][1] = eq[17][0], eq[17][1]
    out.append(("equal addresses", section(eq), 3, 5, 54))
    out.append(("limb 0 falls where limb 1 rises", section(cells_at([0x2000, (1 << 20) | 0xFFF8, (2 << 20) | 0x10, (3 << 20) | 0x8])), 3, 5, 0))
    out.append(("a cell at 0xFF8 ends at the code base", section(cells_at([0xFF8, 0x2000])), 3, 5, 0))
    out.append(("a cell at 0x1000", section(cells_at([0xFF8, 0x1000, 0x2000])), 3, 5, 55))
    out.append(("the last code cell (even code size)", section(cells_at([0x1010, 0x2000])), 3, 6, 55))
    out.append(("the first cell behind an even code size", section(cells_at([0x1018, 0x2000])), 3, 6, 0))
    out.append(("the boundary cell of an odd code size, mode 3", section(cells_at([0x1010, 0x2000])), 3, 5, 55))
    out.append(("the boundary cell of an odd code size, mode 4", section(cells_at([0x1010, 0x2000])), 4, 5, 0))
    out.append(("a code cell below the boundary cell, mode 4", section(cells_at([0x1008, 0x1010])), 4, 5, 55))
    out.append(("no code at all", section(cells_at([0xFF8, 0x1000, 0x1008])), 3, 0, 0))
    full = section(base)
    out.append(("one word short", full[:-1], 3, 5, 4))
    out.append(("the count word alone", full[:1], 3, 5, 4))
    out.append(("no words", full[:0], 3, 5, 4))
    out.append(("a bad cell in a section that is cut: 4 first", section(bad(0, 0, 1 << 20))[:-1], 3, 5, 4))
    return out


def make_blob(code, data, claim_data=None):
    """a program blob as far as the image goes: a 32-byte header with the code size at 16 and the data size at 20, then code and data"""
    h = bytearray(32)
    h[16:20] = len(code).to_bytes(4, "little"); h[20:24] = (len(data) if claim_data is None else claim_data).to_bytes(4, "little")
    return bytes(h) + bytes(code) + bytes(data)


def side_cases():
    """[(what, section words, blob, alpha, lambda)]"""
    rng = np.random.default_rng(11)
    code, data = bytes(rng.integers(1, 256, 20, dtype=np.uint8)), bytes(rng.integers(1, 256, 13, dtype=np.uint8))      # the image ends at 0x1021: inside the cell at 0x1020
    blob = make_blob(code, data)
    edge = cells_at([0xFF8, 0x1000, 0x1008, 0x1010, 0x1018, 0x1020, 0x1028, 0x2000, (5 << 20) | 0x1000])      # before the code, in it, code | data, data, across the data's end, beyond
    edge[2][2] = P - 1; edge[3][3:7] = [0xFFFF] * 4; edge[5][2] = 0; edge[6][3:7] = [0] * 4
    out = [("the image's edges", section(edge), blob, ALPHA, LAM),
           ("a blob shorter than its header", section(edge), blob[:31], ALPHA, LAM),
           ("a blob that claims more data than it holds", section(edge), make_blob(code, data, claim_data=14), ALPHA, LAM),
           ("no blob", section(edge), b"", ALPHA, LAM),
           ("alpha and lambda with a zero component", section(edge), blob, [0, 77, P - 1, 3], [5, 0, 0, P - 1]),
           ("alpha and lambda = p - 1 throughout", section(edge), blob, [P - 1] * 4, [P - 1] * 4)]
    for n in SIZES:
        out.append((f"{n} cells", section(increasing(n, seed=100 + n, start=0x1000 + 16)), blob, ALPHA, LAM))
    for name in ("loads_stores", "pc_carry_mem"):
        cells, b = honest(name)
        out.append((f"{name}'s cells", section(cells), b, ALPHA, LAM))
    return out

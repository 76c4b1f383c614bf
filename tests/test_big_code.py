"""Programs larger than the prover's LDS window over the instruction ROM (ROM_LDS = 4096 code words) and pcs past 2^20 — the host half, no GPU.

Every other program of the suite has at most 410 code words, so every pc stays below 0x1668: pc limbs 1 and 2 are zero in every trace, the pc + 4 carry out of limb 0 never
fires, no branch or jump delta borrows across a limb, no link value has a second limb, and no ROM index reaches 4096.  The builders of tests/programs.py (BIG_CODE) cross
both edges; here the host interpreter, the host's main-trace row code (the function main_trace_kernel runs per lane), the host memory witness and the host verifier are
held against oracle/stark_oracle.cpp, which shares no code with the product.  tests/test_gpu_big_code.py holds the device kernels against the same expected values
(tests/big_code_ref.py computes them once).

COVERED: pc limbs 0 and 1 (pcs up to 0x100048, the carry and the borrow between the two limbs, links and ROM tuples with a non-zero pc1), ROM indices on both sides of 4096,
n_code up to 261 185 (1 MiB of code: n_code > N by a factor of 8000, the boundary cell above 2^20 with LK_B1 != 0, the code-segment bound above 2^20).
NOT COVERED: pc limb 2 (pc >= 2^40).  The code segment is loaded at 0x1000 and a pc outside it has no ROM row, so a run with pc2 != 0 needs a code section of 1 TiB, which no
program blob can carry (the header's code_size is 32 bits): there is no such case, here or on the GPU."""
import ctypes as C

import numpy as np
import pytest

import big_code_ref as ref
import programs as pg
from oracle import stark_api as so
from zkir_amd import runtime as rt, stark

P = so.P
C_PC1 = 2                                             # committed column of pc limb 1 (cycle, pc0, pc1, pc2 open block 0 in every mode)


def _pub_c(p):
    out = rt.PublicInputsC(p.n_real, p.entry, p.deferred, 0)
    out.program_digest[:] = list(p.prog); out.io_digest[:] = list(p.io)
    return out


# ---- the builders reach the edges they are named for: otherwise everything below could pass without touching them ------------------------------------------------------------
def test_rom_builders_reach_both_sides_of_the_split():
    u = ref.rom_index(ref.run("rom_straddle").rows)
    for w in range(pg.ROM_LDS - 3, pg.ROM_LDS + 4):                                   # straight-line code through words 4093 .. 4099
        assert (u == w).any(), w
    assert int((u == pg.ROM_LDS - 1).sum()) == 300 and int((u == pg.ROM_LDS).sum()) == 300
    first, last = int(np.nonzero(u >= pg.ROM_LDS - 2)[0][0]), int(np.nonzero(u == pg.ROM_LDS + 1)[0][-1])
    assert (u[:first] == 10).any() and (u[last:] == 10).any()                         # the low block: before and after the loop
    assert len(u) < len(pg.rom_straddle()[0]) // 4 - 8                                # more ROM rows than trace rows, padded
    lay = so.proof_layout(ref.proof("rom_straddle", 0))
    mult = ref.proof("rom_straddle", 0)[lay["rom_mult"]:lay["rom_mult"] + lay["n_rom"]]
    assert lay["n_rom"] == 4200 and int(mult[pg.ROM_LDS]) > 255 and int(mult[pg.ROM_LDS - 1]) > 255          # the oracle's multiplicities, as its proof carries them
    assert np.array_equal(mult[:pg.ROM_LDS + 2], np.bincount(u, minlength=4200)[:pg.ROM_LDS + 2])           # (the halt row's padding copies sit on the exit's ECALL, further up)
    u = ref.rom_index(ref.run("rom_far_hot").rows)
    assert len(u) == 1 << 12 and int((u < pg.ROM_LDS).sum()) == 2 and 6 <= len(np.unique(u[2:])) <= 8
    for name, n in (("rom_exact_4096", 4096), ("rom_exact_4097", 4097)):
        blob = ref.program(name)[0]
        u = ref.rom_index(ref.run(name).rows)
        assert int.from_bytes(blob[16:20], "little") == 4 * n and int(u[-1]) == n - 1 and int((u == n - 1).sum()) == 1


def test_pc_builders_cross_2p20():
    rows = ref.run("pc_carry").rows
    pc = rows["pc"].astype(np.int64)
    ops = rows["instruction"] & 0x7F
    assert (pc >= 1 << 20).any() and (pc < 1 << 20).any()
    assert [int(i) for i in np.nonzero(pc == 0xFFFFC)[0]] == [5, 10] and ops[5] == 0x48       # the JAL whose link is 2^20
    assert int(rows["registers"][6][5]) == 1 << 20 and int(pc[6]) == 1 << 20
    bne = np.nonzero(ops == 0x41)[0]
    assert [int(pc[i]) for i in bne] == [0x100008, 0x100008] and [int(pc[i + 1]) for i in bne] == [0xFFFF8, 0x10000C]     # taken (a borrow out of limb 1), not taken
    jalr = int(np.nonzero(ops == 0x49)[0][0])
    assert int(pc[jalr]) == 0x10000C and int(pc[jalr + 1]) == 0xFFFE8 and int(rows["registers"][jalr + 1][6]) == 0x100010
    assert list(ref.run("pc_carry").outputs) == [0x100001] and ref.run("pc_carry").halt_kind == 1
    for name in ("pc_carry_mem", "pc_carry_mem_wide"):
        rows = ref.run(name).rows
        pc = rows["pc"].astype(np.int64)
        i = int(np.nonzero(pc == 0xFFFFC)[0][0])
        assert (rows["instruction"][i] & 0x7F) == 0x08 and int(pc[i + 1]) == 1 << 20          # a sequential row: the pc + 4 carry itself
        assert int(ref.run(name).halt_kind) == 1 and len(ref.program(name)[0]) > (1 << 20) - 0x1000
    assert pg.PC_CARRY_MEM_WORDS % 2 == 1 and pg.PC_CARRY_MEM_BC % 8 == 0 and (pg.PC_CARRY_MEM_BC >> 20) & 0xFFFFF == 1       # LK_B1 = 1
    for name, mode in (("pc_carry_mem", 3), ("pc_carry_mem_wide", 4)):
        cells = so.mem_cells(ref.run(name).rows, ref.public(name, mode))
        assert len(cells) >= 3 and (cells[:, 1] == 1).all()                                   # every touched cell's second address limb
        assert (mode == 4) == bool(((cells[:, 0] == (pg.PC_CARRY_MEM_BC & 0xFFFFF)) & (cells[:, 1] == 1)).any())      # mode 4 touches the boundary cell
    hs = so.hash_section(ref.run("pc_carry_mem_wide").rows, ref.public("pc_carry_mem_wide", 4))
    assert int(hs[0]) == 1                                                                    # one hash call, next to the large code bound
    for name, mode in ref.PROOF_CASES:
        if name in ref.PC_PROGRAMS:
            M = so.to_committed(so.main_trace(ref.run(name).rows, ref.public(name, mode)), mode)
            assert set(np.unique(M[C_PC1])) == {0, 1} and not M[C_PC1 + 1].any(), (name, mode)        # pc limb 1 takes both values; limb 2 cannot


# ---- the host interpreter -------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(ref.MODES) + list(ref.REFUSED))
def test_interpreter_rows_equal_the_oracles(name):
    """rt.interpret (interp.cpp) against oracle.run: rows, memory ops, outputs, halt reason — pcs past 2^20, links of 2^20 and above, a 1 MiB program image."""
    from test_host_vs_oracle import compare
    blob, ins, cfg = ref.program(name)
    log, want = compare(blob, ins, cfg)
    assert log.n_rows == len(ref.run(name).rows) and log.n_rows < cfg["max_cycles"] + (name == "rom_far_hot")
    log.close()


# ---- the host's main-trace row code (stark.hip: main_trace_row<mode>, what main_trace_kernel runs per lane) ---------------------------------------------------------------
class _IoArgs(C.Structure):
    _fields_ = [("inputs", C.c_void_p), ("n_inputs", C.c_uint64), ("writes_before", C.c_uint64), ("reads_before", C.c_uint64)]


@pytest.mark.parametrize("name,mode", ref.PROOF_CASES)
def test_host_main_trace_equals_the_oracles(name, mode):
    """Every committed column of every row, the three pc limbs among them; the failure names the column and the first row."""
    blob, ins, cfg = ref.program(name)
    ores = ref.run(name)
    rows, nr = ores.rows, len(ores.rows)
    opub = ref.public(name, mode)
    cyc, pc, ins_c = (np.ascontiguousarray(rows[f]) for f in ("cycle", "pc", "instruction"))
    regs, bb_, bt, bp, st = (np.ascontiguousarray(rows[f].T) for f in ("registers", "bound_bits", "bound_tag", "bound_payload", "reg_state"))
    tc = rt.TraceColumnsC(cyc.ctypes.data, pc.ctypes.data, ins_c.ctypes.data, regs.ctypes.data, bb_.ctypes.data, bt.ctypes.data, bp.ctypes.data, st.ctypes.data, nr)
    N, wm = 1 << so.padded_log_n(nr), so.committed_width(mode)
    out = np.zeros((wm // 8, N, 8), np.uint32)
    tape = np.asarray([0], dtype=np.uint64)
    io = _IoArgs(tape.ctypes.data, 0, 0, 0)
    L = rt.lib()
    V, U64 = C.c_void_p, C.c_uint64
    if mode == 0:
        L.zkir_main_trace_host.restype = C.c_int; L.zkir_main_trace_host.argtypes = [V, U64, C.c_uint32, V]
        rc = L.zkir_main_trace_host(C.byref(tc), nr, 0, out.ctypes.data)
    elif mode == 2:
        L.zkir_main_trace_io_host.restype = C.c_int; L.zkir_main_trace_io_host.argtypes = [V, U64, V, V]
        rc = L.zkir_main_trace_io_host(C.byref(tc), nr, C.byref(io), out.ctypes.data)
    else:
        log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
        pub = rt.public_inputs(log, blob, list(ins), mem_mode=mode == 3, wide_mode=mode == 4, mem_witness="host")
        assert pub.deferred == mode and list(pub.io_digest) == list(opub.io) and list(pub.program_digest) == list(opub.prog)
        if mode == 3:
            L.zkir_main_trace_mem_host.restype = C.c_int; L.zkir_main_trace_mem_host.argtypes = [V, U64, V, V, V, V]
            rc = L.zkir_main_trace_mem_host(C.byref(tc), nr, C.byref(io), pub.mem_old, pub.mem_told, out.ctypes.data)
        else:
            L.zkir_main_trace_wide_host.restype = C.c_int; L.zkir_main_trace_wide_host.argtypes = [V, U64, V, V, V, U64, V]
            rc = L.zkir_main_trace_wide_host(C.byref(tc), nr, C.byref(io), pub.mem_old, pub.mem_told, int.from_bytes(blob[16:20], "little"), out.ctypes.data)
        log.close()
    assert rc == 0
    got = out.transpose(0, 2, 1).reshape(wm, N)
    want = so.to_committed(so.main_trace(rows, opub), mode)
    for k in range(wm):
        assert np.array_equal(got[k], want[k]), f"committed column {k}: first difference at row {int(np.nonzero(got[k] != want[k])[0][0])}"


# ---- the host memory witness ----------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("pc_carry_mem", 3), ("pc_carry_mem_wide", 4)])
def test_host_memory_witness_equals_the_oracles_cells(name, mode):
    """zkir_memcheck_witness_of on cells above 2^20, next to a code bound above 2^20: the oracle's touched cells entry for entry; in mode 4 its hash tape word for word."""
    blob, ins, cfg = ref.program(name)
    opub = ref.public(name, mode)
    log = rt.interpret(blob, list(ins), rt.VMConfig(enable_execution_trace=True, **cfg))
    pub = rt.public_inputs(log, blob, list(ins), mem_mode=mode == 3, wide_mode=mode == 4, mem_witness="host")
    want = so.mem_cells(ref.run(name).rows, opub)
    assert pub.n_cells == len(want) > 0
    ca = np.ctypeslib.as_array(C.cast(pub.cell_addr, C.POINTER(C.c_uint64)), (pub.n_cells,))
    cb = np.ctypeslib.as_array(C.cast(pub.cell_bytes, C.POINTER(C.c_uint64)), (pub.n_cells,))
    ct = np.ctypeslib.as_array(C.cast(pub.cell_time, C.POINTER(C.c_uint32)), (pub.n_cells,))
    for k in range(pub.n_cells):
        w = [int(x) for x in want[k]]
        assert (int(ca[k]) & 0xFFFFF, int(ca[k]) >> 20, int(ct[k]), [(int(cb[k]) >> (16 * i)) & 0xFFFF for i in range(4)]) == (w[0], w[1], w[2], w[3:]), k
    if mode == 4:
        got_hash = np.ctypeslib.as_array(C.cast(pub.hash_section, C.POINTER(C.c_uint32)), (pub.hash_section_words,))
        assert np.array_equal(got_hash, so.hash_section(ref.run(name).rows, opub))
    log.close()


# ---- the host verifier ----------------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", ref.PROOF_CASES)
def test_host_verifier_accepts_the_oracles_proof(name, mode):
    """zkir_verify (verify.cpp + air.h) on the oracle's proof: accepted with and without expected public inputs, and with the claim in the clear."""
    blob, ins, cfg = ref.program(name)
    ores, opub, pr = ref.run(name), ref.public(name, mode), ref.proof(name, mode)
    assert int(pr[9]) == mode and so.verify(pr, opub) == 0 and so.verify(pr) == 0
    assert rt.verify(pr) == 0 and rt.verify(pr, _pub_c(opub)) == 0
    if mode >= 2:
        assert rt.verify_io(pr, _pub_c(opub), list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code)) == 0
    other = ref.public(name, mode); other.entry += 4
    assert rt.verify(pr, _pub_c(other)) == so.verify(pr, other) != 0


def _tamper_positions(name, mode, pr):
    """test_mode3_proof_bytes_match_oracle_and_verify's positions, a halfword of an executed code word inside the carried program (the bulk of these proofs), and the
    opening of pc limb 1 at the out-of-domain point."""
    u = ref.rom_index(ref.run(name).rows)
    word = pg.W20 - 1 if name in ref.PC_PROGRAMS else int(u.max())                          # the JAL / ADDI at pc 0xFFFFC; the highest executed ROM row
    assert (u == word).any() and (name == "rom_exact_4096" or word >= pg.ROM_LDS)
    return {"8": 8, "30": 30, "158": 158, "160": 160, "middle": len(pr) // 2, "last": len(pr) - 1, "code word": ref.blob_at(mode) + 16 + 2 * word,
            "pc1 opening": stark.proof_layout(pr)["openings"] + 4 * C_PC1}


@pytest.mark.parametrize("where", ["8", "30", "158", "160", "middle", "last", "code word", "pc1 opening"])
@pytest.mark.parametrize("name,mode", ref.PROOF_CASES)
def test_host_verifier_gives_the_oracles_verdict_on_tampered_proofs(name, mode, where):
    pr = ref.proof(name, mode)
    pos = _tamper_positions(name, mode, pr)[where]
    t = pr.copy()
    t[pos] = (int(t[pos]) ^ 0x80) if where == "code word" else (int(t[pos]) + 1) % P
    want = so.verify(t)
    assert want != 0 and rt.verify(t) == want, (pos, want)
    if where == "code word":                                                                  # the changed word is part of the program the header's digest names
        lay = stark.proof_layout(t)
        assert lay["blob"] != ref.program(name)[0] and len(lay["blob"]) == len(ref.program(name)[0])


# ---- what a mode-3 proof cannot state: an access to the code segment, with the segment's end above 2^20 ----------------------------------------------------------------------
@pytest.mark.parametrize("name", ref.REFUSED)
def test_accesses_to_the_last_code_word_have_no_mode3_proof(name):
    """A store to / a load from the last word of a 1 MiB code segment (0x1000FC): the VM runs it; both verifiers reject the oracle's proof with check 55 (the touched cell
    overlaps [0x1000, 0x100100)).  The GPU prover's refusal of the same runs is pinned in tests/test_gpu_big_code.py."""
    ores = ref.run(name)
    opub = ref.public(name, 3)
    cells = so.mem_cells(ores.rows, opub)
    assert len(cells) == 1 and (int(cells[0][0]), int(cells[0][1])) == (0x000F8, 1) and ores.halt_kind == 0
    pr = ref.proof(name, 3)
    assert so.verify(pr, opub) == 55 and rt.verify(pr) == 55 and rt.verify(pr, _pub_c(opub)) == 55

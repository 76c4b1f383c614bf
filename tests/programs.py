"""Test programs: the reference's own test programs re-typed with the v3.4 encoder, targeted quirk probes
 and a seeded random-program generator.  Each entry returns (blob, inputs, cfg_kwargs)."""
from __future__ import annotations

import functools

import numpy as np

from zkir_amd import spec
from zkir_amd.spec import Opcode as O, encode as E, Program

A = lambda rd, rs1, imm: E(O.ADDI, rd, rs1, imm=imm)  # noqa: E731
EB = spec.ebreak()
EC = spec.ecall()


def _p(code, data=b"", config=None):
    return Program.from_code(code, data, config).to_bytes()


def _exit0():
    return [A(10, 0, 0), A(11, 0, 0), EC]


def li40(rd, value, tmp=None):
    """Load an arbitrary 40-bit constant with 16-bit pieces (17-bit signed immediates, Q11)."""
    v = value & ((1 << 40) - 1)
    out = [A(rd, 0, (v >> 32) & 0xFF)]
    for sh in (16, 0):
        out += [E(O.SLLI, rd, rd, imm=16), E(O.ORI, rd, rd, imm=(v >> sh) & 0xFFFF)]
    return out


# ---- the reference's own programs ---------------------------------------------------------------
def exit_42():                      # vm.rs:464-486
    return _p([A(10, 0, 0), A(11, 0, 42), EC]), [], {}


def io_echo():                      # vm.rs:489-533
    return _p([A(10, 0, 1), EC, A(11, 10, 0), A(10, 0, 2), EC, A(11, 0, 0), A(10, 0, 0), EC]), [123], {}


def echo5():                        # stress_tests.rs:397-430 (five values, exhausted tape reads 0)
    code = []
    for _ in range(6):
        code += [A(10, 0, 1), EC, A(11, 10, 0), A(10, 0, 2), EC]
    return _p(code + _exit0()), [1, 2, 3, 4, 5], {}


def jal_self_cycle_limit():         # vm.rs:536-552
    return _p([spec.jal(0, 0)]), [], {"max_cycles": 100}


def basic_add_ebreak():             # vm.rs:434-461
    return _p([A(1, 0, 10), A(2, 0, 20), spec.add(3, 1, 2), EB]), [], {}


# The reference's own memory tests store at 0x1000 — the FIRST CODE WORD (strict protection is off, vm.rs:175; the word has been executed by then).  `base` moves the data
# off the code segment: what a mode-3 proof needs (format v11: no touched cell may overlap the code, check 55) — OFF_CODE below.
OFF_CODE = 0x2000


def mem_sw_lw(base=0x1000):         # vm.rs:996-1070
    return _p([A(1, 0, 0x42), A(3, 0, base), spec.sw(3, 1, 0), spec.lw(4, 3, 0), EB]), [], {}


def timestamps(base=0x1000):        # vm.rs:1073-1200
    return _p([A(1, 0, 0x100), A(2, 0, base), spec.sw(2, 1, 0), A(3, 0, 0x200), spec.sw(2, 3, 4), spec.lw(4, 2, 0),
               spec.lw(5, 2, 4), EB]), [], {}


def beq_skip():                     # vm.rs:594-632
    return _p([A(1, 0, 10), A(2, 0, 10), spec.beq(1, 2, 8), A(3, 0, 99), EB]), [], {}


def sum_1_to_5():                   # cross_module.rs:406-437
    return _p([A(1, 0, 0), A(2, 0, 1), A(3, 0, 6), spec.add(1, 1, 2), A(2, 2, 1), spec.bne(2, 3, -8), A(11, 1, 0), A(10, 0, 2), EC]
              + _exit0()), [], {}


def fib30():
    return spec.fib_program(30).to_bytes(), [], {}


def rc_doubling(base=0x1000):       # vm.rs:698-752: 30 doublings then SW -> deferred range checks flushed
    code = [A(1, 0, (1 << 15) - 1)] + [spec.add(1, 1, 1)] * 30 + [A(2, 0, base), spec.sw(2, 1, 0), EB]
    return _p(code), [], {"enable_range_checking": True}


def rc_small_consts():              # vm.rs:755-806: no witnesses
    return _p([A(1, 0, 100), A(2, 0, 200), spec.add(3, 1, 2), A(4, 0, 0x2000), spec.sw(4, 3, 0), EB]), [], {"enable_range_checking": True}


def rc_many_pending():              # >= 16 pending checks force a checkpoint without an observation opcode (range_check.rs:122-135)
    code = [A(1, 0, 3)] + li40(2, 0xFFFFFFFFFF)
    code += [spec.mul(3, 2, 2)] * 3 + [spec.add(4, 3, 3)] * 40 + [spec.mul(5, 4, 2)] * 5 + [spec.bne(0, 0, 8), EB]
    return _p(code), [], {"enable_range_checking": True}


def rc_config_30bit():              # header limb_bits=30 -> chunk_bits=15, data_bits=60 (vm.rs:185, range_check.rs:29)
    code = li40(2, 0xABCDE12345) + [spec.mul(3, 2, 2), spec.mul(4, 3, 3), spec.mul(5, 4, 4), A(6, 0, 0x2000), spec.sw(6, 5, 0), EB]
    return _p(code, config=spec.Config(30, 2, 2)), [], {"enable_range_checking": True}


# ---- ALU / bound-algebra coverage ---------------------------------------------------------------
def alu_all():
    code = li40(1, 0xFEDCBA9876) + li40(2, 0x0123456789) + [A(3, 0, -5), A(4, 0, 37), A(5, 0, 1)]
    for op in (O.ADD, O.SUB, O.MUL, O.MULH, O.DIVU, O.REMU, O.DIV, O.REM, O.AND, O.OR, O.XOR, O.SLL, O.SRL, O.SRA, O.SLTU, O.SGEU,
               O.SLT, O.SGE, O.SEQ, O.SNE, O.CMOV, O.CMOVZ, O.CMOVNZ):
        for (a, b) in ((1, 2), (2, 1), (3, 4), (1, 3), (3, 3), (4, 5), (0, 1), (1, 0) if op not in (O.DIVU, O.REMU, O.DIV, O.REM) else (1, 5)):
            code.append(E(op, 6 + (len(code) % 4), a, b))
    for op in (O.ADDI, O.ANDI, O.ORI, O.XORI):
        for imm in (0, 1, -1, 65535, -65536, 0x7FFF, -12345):
            code.append(E(op, 6 + (len(code) % 4), 1 + (len(code) % 3), imm=imm))
    for op in (O.SLLI, O.SRLI, O.SRAI):
        for sh in (0, 1, 19, 20, 39, 40, 41, 63, 64, 255):
            code.append(E(op, 6 + (len(code) % 4), 1 + (len(code) % 3), imm=sh))
    # shifts by register use rs2 & 0x3F (Q5)
    code += [A(9, 0, 64 + 3), E(O.SLL, 6, 1, 9), E(O.SRL, 7, 1, 9), E(O.SRA, 8, 1, 9), A(9, 0, 45), E(O.SLL, 6, 1, 9), E(O.SRA, 8, 1, 9)]
    return _p(code + [EB]), [], {}


def mul_grid():
    """MUL (execute.rs:79-99) on a grid of 40-bit operands: zero, one, all ones, the sign bit, every chunk at its extremes (the largest carries), a register with bits above 40
    set by LB's sign extension (masked: Value40::from_u64), rs1 = rs2 = rd."""
    vals = [0, 1, 2, 0xFFFFFFFFFF, 0x8000000000, 0xF0F0A5C3E1, 0x0312345678, 1023, 1024, 0xFFFFF, 0x100000, 0x3FF003FF, 0xFFC00FFC00, 0x7FFFFFFFFF]
    code = [A(5, 0, 0x4000), A(6, 0, 0x80), E(O.SB, rs1=5, rs2=6, imm=0), E(O.LB, 7, 5, imm=0)]           # R7 = 0xFFFF...FF80 (Q1)
    for a in vals:
        code += li40(1, a)
        for b in vals:
            code += li40(2, b) + [E(O.MUL, 3, 1, 2), E(O.MUL, 4, 2, 1)]
        code += [E(O.MUL, 8, 1, 7), E(O.MUL, 9, 7, 1), E(O.MUL, 1, 1, 1)]
    code += [E(O.MUL, 7, 7, 7), E(O.MUL, 0, 1, 2)]
    return _p(code + [EB]), [], {}


def wide_grid(vals=None):
    """MULH DIVU REMU DIV REM (execute.rs:101-183) on a grid of operands BELOW 2^40 (AIR mode 4's domain): zero and one, all ones, the sign bit of a 40-bit value (positive as an
    i64: quirk Q2), every chunk at its extremes (the largest carries of the 80-bit product), dividend < divisor, equal operands, powers of two, rs1 = rs2 = rd, rd = r0."""
    vals = vals or [0, 1, 2, 0xFFFFFFFFFF, 0x8000000000, 0xF0F0A5C3E1, 0x0312345678, 1023, 1024, 0xFFFFF, 0x100000, 0x3FF003FF, 0xFFC00FFC00, 0x7FFFFFFFFF]
    code = []
    for a in vals:
        code += li40(1, a)
        for b in vals:
            code += li40(2, b) + [E(O.MULH, 3, 1, 2), E(O.MULH, 4, 2, 1)]
            if b:
                code += [E(O.DIVU, 5, 1, 2), E(O.REMU, 6, 1, 2), E(O.DIV, 7, 1, 2), E(O.REM, 8, 1, 2)]
        code += [E(O.MULH, 9, 1, 1)] + ([E(O.DIVU, 9, 1, 1), E(O.REM, 0, 1, 1)] if a else [])
    code += li40(1, 0xFEDCBA9876) + [E(O.REMU, 1, 1, 1)] + li40(1, 0xFEDCBA9876) + [E(O.DIV, 1, 1, 1), E(O.MULH, 1, 1, 1)]
    return _p(code + [EB]), [], {}


def loads_stores():
    code = [A(5, 0, 0x4000)] + li40(1, 0x80F1E2D3C4) + [A(2, 0, -1)]
    code += [E(O.SD, rs1=5, rs2=1, imm=0), E(O.SW, rs1=5, rs2=1, imm=8), E(O.SH, rs1=5, rs2=1, imm=12), E(O.SB, rs1=5, rs2=1, imm=14),
             E(O.SD, rs1=5, rs2=2, imm=16), E(O.SB, rs1=5, rs2=2, imm=31)]
    for off in (0, 1, 2, 3, 7, 14, 16, 31, 100):
        code += [E(O.LB, 6, 5, imm=off), E(O.LBU, 7, 5, imm=off)]
    for off in (0, 2, 6, 12, 16, 30):
        code += [E(O.LH, 6, 5, imm=off), E(O.LHU, 7, 5, imm=off)]
    for off in (0, 4, 8, 16, 28):
        code += [E(O.LW, 8, 5, imm=off)]
    code += [E(O.LD, 9, 5, imm=0), E(O.LD, 9, 5, imm=16), E(O.LD, 9, 5, imm=1024)]
    # Q1/Q6: sign-extended 64-bit register values in raw compares, DIV on "negative" raw values, MULH on raw operands
    code += [E(O.LB, 6, 5, imm=31), E(O.LB, 7, 5, imm=31), E(O.SEQ, 8, 6, 7), E(O.ADDI, 7, 7, imm=0), E(O.SEQ, 8, 6, 7), E(O.SNE, 9, 6, 7),
             spec.beq(6, 7, 8), A(12, 0, 1), A(4, 0, 3), E(O.DIV, 13, 6, 4), E(O.REM, 14, 6, 4), E(O.MULH, 15, 6, 6), E(O.CMOVNZ, 12, 6, 6),
             E(O.SD, rs1=5, rs2=6, imm=40), E(O.LD, 3, 5, imm=40), E(O.ADD, 3, 3, 0)]
    return _p(code + [EB]), [], {}


def jumps_and_links():
    code = [spec.jal(1, 8), EB, A(2, 1, 0), E(O.JALR, 3, 1, imm=12 + 1),    # jalr target = (r1 + 13) & ~1
            EB, EB, A(4, 3, 0), spec.jal(0, 8), EB, A(5, 0, 7), E(O.BLT, rs1=0, rs2=5, imm=8), EB, E(O.BGEU, rs1=5, rs2=0, imm=8), EB,
            A(6, 0, -1), E(O.BLT, rs1=6, rs2=0, imm=8), EB, E(O.BLTU, rs1=6, rs2=0, imm=8), E(O.BGE, rs1=0, rs2=6, imm=8), EB, EB]
    return _p(code), [], {}


def q9_access_at_own_pc():
    """Q9: any data op whose address equals the fetching pc is dropped from the row (vm.rs:295)."""
    code = [A(1, 0, 0x1000 + 8), A(2, 0, 0), spec.lw(3, 1, 0), A(1, 0, 0x1000 + 16), spec.sw(1, 3, 0), EB]
    # instr[2] at pc 0x1008 loads from 0x1008; instr[4] at pc 0x1010 stores to 0x1010 (overwrites itself after the fetch)
    return _p(code), [], {}


def self_modifying():
    """strict protection is off at run time (vm.rs:175): a store can rewrite a later instruction."""
    target = 0x1000 + 4 * 6
    new_word = A(7, 0, 1234)
    code = li40(1, new_word) + [A(2, 0, target)]         # 5 + 1 = 6 instrs
    code = li40(1, new_word)[:5] + [A(2, 0, 0x1000 + 4 * 8), spec.sw(2, 1, 0), A(0, 0, 0), EB, EB]
    # word index 8 (an EBREAK) is replaced by `addi r7, r0, 1234` before it is fetched
    return _p(code), [], {}


def cmov_false_keeps_bound():
    code = [A(1, 0, 5), A(2, 0, 9), E(O.CMOV, 2, 1, 0), E(O.CMOVZ, 2, 1, 1), E(O.CMOVNZ, 2, 1, 1), E(O.CMOVZ, 3, 1, 0), EB]
    return _p(code), [], {}


# ---- syscalls --------------------------------------------------------------------------------------
def _store_bytes(base_reg, data: bytes):
    out = []
    for i, b in enumerate(data):
        out += [A(9, 0, b), E(O.SB, rs1=base_reg, rs2=9, imm=i)]
    return out


def sha256_hello():                 # syscall.rs:280-318
    code = [A(5, 0, 0x2000)] + _store_bytes(5, b"hello") + [A(11, 5, 0), A(12, 0, 5), A(13, 0, 0x3000), A(10, 0, 3), EC,
                                                          spec.lw(1, 13, 0), spec.lw(2, 13, 28)] + _exit0()
    return _p(code), [], {}


def hashes_all():
    msg = bytes((i * 7 + 3) & 0xFF for i in range(70))
    code = [A(5, 0, 0x2000)] + _store_bytes(5, msg)
    for num, ln, out in ((3, 0, 0x3000), (3, 55, 0x3020), (3, 56, 0x3040), (3, 70, 0x3060), (5, 0, 0x3080), (5, 70, 0x30A0), (6, 0, 0x30C0), (6, 70, 0x30E0)):
        code += [A(11, 5, 0), A(12, 0, ln), A(13, 0, out), A(10, 0, num), EC, A(1, 14, 0)]
    # unaligned input pointer is fine (byte reads); chain: hash the previous digest
    code += [A(11, 0, 0x3001), A(12, 0, 31), A(13, 0, 0x3100), A(10, 0, 3), EC, A(11, 0, 0x3100), A(12, 0, 32), A(13, 0, 0x3120), A(10, 0, 5), EC]
    return _p(code + _exit0()), [], {}


def blake3_multi_chunk():
    """Input > 1024 bytes exercises BLAKE3's chunk tree; zero-filled memory reads as zeros (memory.rs:301-305)."""
    code = [A(5, 0, 0x4000), A(9, 0, 0xAB), E(O.SB, rs1=5, rs2=9, imm=1500)]
    for ln, out in ((1024, 0x3000), (1025, 0x3020), (2048, 0x3040), (2049, 0x3060), (3073, 0x3080), (5000, 0x30A0)):
        code += [A(11, 5, 0), A(12, 0, ln), A(13, 0, out), A(10, 0, 6), EC]
    code += [A(11, 5, 0), A(12, 0, 137), A(13, 0, 0x3100), A(10, 0, 5), EC, A(11, 5, 0), A(12, 0, 300), A(13, 0, 0x3120), A(10, 0, 5), EC]
    return _p(code + _exit0()), [], {}


def sha_chain_small():
    return spec.sha256_chain_program().to_bytes(), [], {"max_cycles": 600}


# ---- deferred carry model (execute.rs:888-1003) -----------------------------------------------------
def deferred_add_branch():          # deferred_integration_test.rs:21-98
    code = [A(1, 0, 100), A(2, 0, 200), spec.add(3, 1, 2), A(4, 0, 300), spec.beq(3, 4, 8), A(5, 0, 1), A(5, 0, 42)] + _exit0()
    return _p(code), [], {"enable_deferred_model": True}


def deferred_chain_store():         # deferred_integration_test.rs:101-160
    code = [A(1, 0, 10), A(1, 1, 20), A(1, 1, 30), A(1, 1, 40), A(1, 1, 50), E(O.SW, rs1=0, rs2=1, imm=0x10000)] + _exit0()
    return _p(code), [], {"enable_deferred_model": True}


def deferred_add_sub_mix():         # deferred_integration_test.rs:163-224
    code = [A(1, 0, 100), A(2, 0, 50), spec.add(3, 1, 2), A(4, 0, 30), spec.sub(5, 3, 4), E(O.ANDI, 6, 5, imm=0xFFFF)] + _exit0()
    return _p(code), [], {"enable_deferred_model": True}


def deferred_negative_and_overflow():
    """Two's-complement ADDI (normalize.rs:331-360), SUB underflow wrap (deferred.rs:184-187), limb overflow
    forcing source normalization (deferred.rs:100-113), non-deferred writers leaving the Accumulated flag set (Q10)."""
    code = [A(1, 0, 32767), A(1, 1, 1), A(2, 1, -16), A(3, 0, 5), spec.sub(4, 3, 1), spec.sub(4, 4, 1), E(O.XOR, 4, 4, 3), spec.add(4, 4, 4)]
    code += [A(6, 0, 65535), E(O.SLLI, 6, 6, imm=4), A(6, 6, 0)]
    code += [spec.add(6, 6, 6)] * 14                    # limb0 doubles until it would exceed 2^30
    code += [A(7, 6, -1)] + [spec.add(7, 7, 6)] * 3 + [A(8, 0, 1), A(10, 0, 1), EC, spec.add(9, 10, 10), E(O.MUL, 9, 9, 7),
                                                       E(O.SLTU, 11, 7, 6), E(O.SD, rs1=0, rs2=7, imm=0x4000), E(O.SRAI, 12, 7, imm=3), spec.bne(7, 6, 8), EB, EB]
    return _p(code), [777], {"enable_deferred_model": True}


def deferred_fib():
    return spec.fib_program(40).to_bytes(), [], {"enable_deferred_model": True, "enable_range_checking": True}


def fib_rc():
    """fib with range checking: every ADD whose bound exceeds 40 bits defers and is flushed at the next BNE."""
    return spec.fib_program(200).to_bytes(), [], {"enable_range_checking": True}


ALL = {f.__name__: f for f in (fib_rc,
    exit_42, io_echo, echo5, jal_self_cycle_limit, basic_add_ebreak, mem_sw_lw, timestamps, beq_skip, sum_1_to_5, fib30, rc_doubling,
    rc_small_consts, rc_many_pending, rc_config_30bit, alu_all, loads_stores, jumps_and_links, q9_access_at_own_pc, self_modifying,
    cmov_false_keeps_bound, sha256_hello, hashes_all, blake3_multi_chunk, sha_chain_small, deferred_add_branch, deferred_chain_store,
    deferred_add_sub_mix, deferred_negative_and_overflow, deferred_fib)}


# ---- programs that must fail with a specific RuntimeError (error.rs:7-37) ---------------------------
def err_div_zero(): return _p([A(1, 0, 5), E(O.DIV, 2, 1, 0), EB]), [], {}, 3
def err_remu_zero(): return _p([A(1, 0, 5), E(O.REMU, 2, 1, 0), EB]), [], {}, 3
def err_misaligned_lw(): return _p([A(1, 0, 0x2002), spec.lw(2, 1, 0), EB]), [], {}, 1
def err_misaligned_sd(): return _p([A(1, 0, 0x2004), E(O.SD, rs1=1, rs2=0, imm=0), EB]), [], {}, 1
def err_misaligned_sha_out(): return _p([A(11, 0, 0x2000), A(12, 0, 0), A(13, 0, 0x3002), A(10, 0, 3), EC, EB]), [], {}, 1
def err_invalid_syscall(): return _p([A(10, 0, 999), EC]), [], {}, 4
def err_poseidon2(): return _p([A(10, 0, 4), EC]), [], {}, 6          # crypto.rs:306-315
def err_unknown_opcode(): return _p([A(1, 0, 1), 0x0000007F]), [], {}, 5
def err_misaligned_pc(): return _p([A(1, 0, 0x1000 + 10), E(O.JALR, 0, 1, imm=0), EB]), [], {}, 6    # target & ~1 = 0x100a
def err_debug_format():
    p = Program.from_code([EB]); p.header.entry_point = 32
    return p.to_bytes(), [], {}, 7
def err_bad_magic(): return b"\x00" * 40, [], {}, 7
def err_truncated():
    return _p([EB, EB])[:-3], [], {}, 7


ERRORS = {f.__name__: f for f in (err_div_zero, err_remu_zero, err_misaligned_lw, err_misaligned_sd, err_misaligned_sha_out,
                                  err_invalid_syscall, err_poseidon2, err_unknown_opcode, err_misaligned_pc, err_debug_format,
                                  err_bad_magic, err_truncated)}


# ---- seeded random programs --------------------------------------------------------------------------
_R_OPS = [O.ADD, O.SUB, O.MUL, O.MULH, O.AND, O.OR, O.XOR, O.SLL, O.SRL, O.SRA, O.SLTU, O.SGEU, O.SLT, O.SGE, O.SEQ, O.SNE, O.CMOV, O.CMOVZ, O.CMOVNZ]
_I_OPS = [O.ADDI, O.ANDI, O.ORI, O.XORI]
_GP = [1, 2, 3, 4, 7, 8, 9, 14, 15]       # r5 = memory base, r6 = non-zero divisor, r10-r13 = syscall scratch


def random_program(seed: int, n_instr: int = 300, range_checking: bool = False, hashes: bool = True, wide_safe: bool = False):
    """`wide_safe` (proof mode 4): the five wide opcodes read operands cut below 2^40 first (SRLI by >= 24 into the syscall scratch r12 / r13, or r0 / r6), which is
    what mode 4 states them on; MULH leaves the generic R-type pool for the same reason.  Zero dividends, zero factors and equal operands stay in the draw."""
    rng = np.random.default_rng(seed)
    ri = lambda lo, hi: int(rng.integers(lo, hi))  # noqa: E731
    reg = lambda: _GP[ri(0, len(_GP))]              # noqa: E731
    src = lambda: ([0] + _GP + [5, 6])[ri(0, len(_GP) + 3)]  # noqa: E731
    code = [A(5, 0, 0x8000), E(O.SLLI, 5, 5, imm=1)] + li40(6, int(rng.integers(1, 1 << 40)) | 1)
    for r in _GP:
        code += li40(r, int(rng.integers(0, 1 << 40))) if rng.random() < 0.6 else [A(r, 0, ri(-65536, 65536))]
    body = []
    while len(body) < n_instr:
        k = rng.random()
        if k < 0.40:
            op = _R_OPS[ri(0, len(_R_OPS))]
            if wide_safe and op == O.MULH:
                op = O.MUL
            body.append(E(op, reg(), src(), src()))
        elif k < 0.55:
            body.append(E(_I_OPS[ri(0, len(_I_OPS))], reg(), src(), imm=ri(-65536, 65536)))
        elif k < 0.63:
            body.append(E([O.SLLI, O.SRLI, O.SRAI][ri(0, 3)], reg(), src(), imm=ri(0, 64) if rng.random() < 0.9 else ri(64, 256)))
        elif k < 0.73:
            w = [1, 2, 4, 8][ri(0, 4)]
            off = ri(0, 256) * w
            ops = {1: [O.LB, O.LBU], 2: [O.LH, O.LHU], 4: [O.LW], 8: [O.LD]}[w]
            body.append(E(ops[ri(0, len(ops))], reg(), 5, imm=off))
        elif k < 0.82:
            w = [1, 2, 4, 8][ri(0, 4)]
            body.append(E({1: O.SB, 2: O.SH, 4: O.SW, 8: O.SD}[w], rs1=5, rs2=src(), imm=ri(0, 256) * w))
        elif k < 0.86 and wide_safe:
            body += [E(O.SRLI, 12, src(), imm=ri(24, 64)), E(O.SRLI, 13, src(), imm=ri(24, 64)), E(O.ORI, 13, 13, imm=1)]      # r13 != 0: a zero divisor is a VM error
            op = [O.DIVU, O.REMU, O.DIV, O.REM, O.MULH][ri(0, 5)]
            b = [13, 12, 6, 0][ri(0, 4)] if op == O.MULH else [13, 13, 6][ri(0, 3)]
            body.append(E(op, reg(), [12, 12, 12, 13, 6, 0][ri(0, 6)], b))
        elif k < 0.86:
            body.append(E([O.DIVU, O.REMU, O.DIV, O.REM][ri(0, 4)], reg(), src(), 6 if rng.random() < 0.97 else src()))
        elif k < 0.93:
            body.append(E([O.BEQ, O.BNE, O.BLT, O.BGE, O.BLTU, O.BGEU][ri(0, 6)], rs1=src(), rs2=src(), imm=4 * ri(1, 5)))
        elif k < 0.94:
            body.append(spec.jal(reg() if rng.random() < 0.5 else 0, 4 * ri(1, 4)))
        elif k < 0.95:                                               # a computed jump: link the next address, then JALR past 1..3 instructions (even and odd sums)
            body += [spec.jal(7, 4), E(O.JALR, reg() if rng.random() < 0.5 else 0, 7, imm=4 * ri(1, 5) + ri(0, 2))]
        elif k < 0.97:
            body += [A(11, src(), 0), A(10, 0, 2), EC] if rng.random() < 0.5 else [A(10, 0, 1), EC, A(reg(), 10, 0)]
        elif hashes:
            num = [3, 5, 6][ri(0, 3)]
            body += [A(11, 5, ri(0, 512)), A(12, 0, ri(0, 200)), A(13, 5, 1024 + 4 * ri(0, 128)), A(10, 0, num), EC, A(reg(), 14, 0)]
    code += body + [EB] * 6
    inputs = [int(x) for x in rng.integers(0, 1 << 62, size=5)]
    return _p(code), inputs


def off_code(name):
    """The program `name` with its data moved off the code segment (mem_sw_lw, timestamps, rc_doubling: the reference's tests store at 0x1000); every other program as it is."""
    f = globals()[name]
    import inspect
    return f(base=OFF_CODE) if "base" in inspect.signature(f).parameters else f()


# ---- memory edges of proof modes 3 / 4: addresses whose limbs carry, wrap or sit at the top of the 40-bit space (tests/test_memory_edges.py) --------------------
P8 = 8 * 0x78000001                  # 8 p: two cells this far apart are the same Baby Bear element (0x3C0000008, ~15 GiB)
TOP = (1 << 40) - 8                  # the last cell below 2^40
_LOADS = {1: (O.LB, O.LBU), 2: (O.LH, O.LHU), 4: (O.LW,), 8: (O.LD,)}
_STORES = {1: O.SB, 2: O.SH, 4: O.SW, 8: O.SD}


def _widths_at(base_reg, imm):
    """SD a pattern at base + imm, read it back at every width (signed and unsigned), overwrite a byte, a halfword and a word, read the doubleword again."""
    code = [E(O.SD, rs1=base_reg, rs2=1, imm=imm), E(O.LD, 2, base_reg, imm=imm), E(O.LW, 3, base_reg, imm=imm + 4), E(O.LH, 4, base_reg, imm=imm + 6),
            E(O.LHU, 4, base_reg, imm=imm + 6), E(O.LB, 7, base_reg, imm=imm + 7), E(O.LBU, 7, base_reg, imm=imm + 3)]
    code += [E(O.SB, rs1=base_reg, rs2=2, imm=imm + 1), E(O.SH, rs1=base_reg, rs2=3, imm=imm + 2), E(O.SW, rs1=base_reg, rs2=4, imm=imm + 4), E(O.LD, 8, base_reg, imm=imm)]
    return code


def _pattern():
    return li40(1, 0x80F1E2D3C4)          # every byte distinct, the top bit of bytes 4 (0x80) / 3 (0xF1) / 7 set once the stores have run


def edge_limb_carries():
    """base[0] + imm carries into limb 1 (and a negative imm17 borrows through it): bases whose limb 0 sits just below 2^20, immediates 8 .. 65528 and -8 .. -65536,
    every width; a byte access at imm = +65535.  The cells stay far above the code and below 2^40."""
    code = _pattern()
    for base in (0x3_FFFF8, 0x5_FFFC0, 0x7_F8000, 0xABCDE_FFFF8):
        code += li40(5, base)
        for imm in (8, 0x40, 0x8000, 65528):
            code += _widths_at(5, imm)
        code += [E(O.SB, rs1=5, rs2=1, imm=65535), E(O.LB, 9, 5, imm=65535), E(O.LBU, 9, 5, imm=65535)]
    for base in (0x3_00010, 0x6_10000, 0x8_00008, 0xFFFFF_00000):
        code += li40(5, base)
        for imm in (-8, -16, -0x8000, -65536):
            code += _widths_at(5, imm)
    return _p(code + [EB]), [], {}


def edge_high_limbs():
    """Cells whose limb 1 is 0xFFFFF, 0x80000, 0x55555 (every width), and the top cell 2^40 - 8: an SD / LD pair, a byte stored into each of its eight bytes, read back."""
    code = _pattern()
    for hi in (0xFFFFF, 0x80000, 0x55555):
        code += li40(5, (hi << 20) | 0xABCD0) + _widths_at(5, 0) + _widths_at(5, -0x10)
    code += li40(5, TOP) + [E(O.SD, rs1=5, rs2=1, imm=0), E(O.LD, 2, 5, imm=0)]
    for k in range(8):
        code += [A(9, 0, 0x81 + 0x11 * k), E(O.SB, rs1=5, rs2=9, imm=k), E(O.LB, 3, 5, imm=k), E(O.LBU, 4, 5, imm=k)]
    code += [E(O.LD, 2, 5, imm=0), E(O.LW, 3, 5, imm=4), E(O.LH, 4, 5, imm=6)]
    code += li40(5, TOP - 0x10000 + 8) + _widths_at(5, 65528 - 8)                  # the top cell again, reached through limb-0 carry
    return _p(code + [EB]), [], {}


def edge_wrap64():
    """A raw 64-bit base plus imm wrapping past 2^64 or landing below 2^40 (column C_CM2): an LB sign-extended base 0xFFFF_FFFF_FFFF_FF80 + 0x2080 = 0x2000; bases that arrive by
    READ (raw 64 bits) — 2^64 - 8 + 0x3008, 2^64 - 0x8000 + 0xA000, and 2^40 + 8 with negative immediates (2^40 - 8: the top cell, 2^40 - 65528)."""
    code = _pattern() + [A(5, 0, 0x4000), A(9, 0, 0x80), E(O.SB, rs1=5, rs2=9, imm=0), E(O.LB, 6, 5, imm=0)]      # r6 = 0xFFFF_FFFF_FFFF_FF80 (Q1)
    code += _widths_at(6, 0x2080)
    for imm in (0x3008, 0xA000, -16, -65536):
        code += [A(10, 0, 1), EC] + _widths_at(10, imm)                               # READ: r10 = the next input, raw
    return _p(code + [EB]), [(1 << 64) - 8, (1 << 64) - 0x8000, (1 << 40) + 8, (1 << 40) + 8], {}


def edge_aliases():
    """Two (three) distinct cells whose addresses differ by a multiple of 8 p — the same value as ONE field element — written and read back alternately."""
    code = _pattern() + li40(5, 0x20000) + li40(6, 0x20000 + P8) + li40(7, 0x20000 + 68 * P8)
    for r in range(3):
        code += [A(9, 0, 0x111 * (r + 1)), E(O.SD, rs1=5, rs2=9, imm=0), A(9, 0, 0x222 * (r + 1)), E(O.SD, rs1=6, rs2=9, imm=0),
                 E(O.LD, 2, 5, imm=0), E(O.LD, 3, 6, imm=0), A(9, 0, 0x333 * (r + 1)), E(O.SW, rs1=7, rs2=9, imm=4), E(O.LD, 4, 7, imm=0), E(O.LD, 2, 5, imm=0),
                 E(O.SB, rs1=6, rs2=1, imm=r), E(O.LD, 3, 6, imm=0), E(O.LD, 4, 5, imm=0)]
    return _p(code + [EB]), [], {}


_BC_WORDS = 41                       # an odd number of code words: the boundary cell B = 0x1000 + 4 * 41 - 4 holds the last code word and the first data word
BC = 0x1000 + 4 * _BC_WORDS - 4


def _bc_program(stores):
    """Code of _BC_WORDS words (an EBREAK, then padding that is never executed) + 8 data bytes; `stores` = [(address, opcode)] with r1 the stored value."""
    code = _pattern()
    for addr, op in stores:
        code += li40(5, addr) + [E(op, rs1=5, rs2=1, imm=0), E(O.LD, 2, 5, imm=-(addr & 7))]
    code += [EB]
    assert len(code) <= _BC_WORDS
    code += [A(7, 0, 2)] * (_BC_WORDS - len(code))
    return _p(code, data=bytes(range(0x41, 0x49)))


def edge_bc_alias_ok():
    """Next to the boundary cell's aliases, what proves: a store into the HIGH half of B + 8 p, into the low half of B + 8 p + 8, a byte into B's data half."""
    return _bc_program([(BC + P8 + 4, O.SW), (BC + P8 + 8, O.SW), (BC + P8 + 8 + 3, O.SB), (BC + 5, O.SB)]), [], {}


def edge_bc_alias_low_1():
    """A store into the low half of B + 8 p: the boundary-cell constraint sees delta = cell - B = 0 — no proof in format v12 (the prover refuses)."""
    return _bc_program([(BC + P8, O.SW)]), [], {}


def edge_bc_alias_low_68():
    """The same at B + 68 * 8 p, the last alias below 2^40 (a byte store)."""
    assert BC + 68 * P8 < (1 << 40) <= BC + 69 * P8
    return _bc_program([(BC + 68 * P8 + 2, O.SB)]), [], {}


def edge_at_2p40():
    """An access at exactly 2^40 (the top cell's register + 8: the address add is a wrapping u64 add, not a 40-bit one): the VM runs it, no proof exists."""
    return _p(_pattern() + li40(5, TOP) + [E(O.SD, rs1=5, rs2=1, imm=0), E(O.LD, 2, 5, imm=8), EB]), [], {}


def edge_above_2p40():
    """A store above 2^40 (2^40 - 8 + 65528) after accesses that have a proof: the VM runs it, no proof exists."""
    return _p(_pattern() + li40(5, TOP) + [E(O.SD, rs1=5, rs2=1, imm=0), E(O.SB, rs1=5, rs2=1, imm=65528), E(O.LD, 2, 5, imm=0), EB]), [], {}


MEM_EDGES = {f.__name__: f for f in (edge_limb_carries, edge_high_limbs, edge_wrap64, edge_aliases, edge_bc_alias_ok)}      # these have a mode-3 / mode-4 proof
MEM_EDGES_NO_PROOF = {f.__name__: f for f in (edge_bc_alias_low_1, edge_bc_alias_low_68, edge_at_2p40, edge_above_2p40)}     # the VM runs them; no proof exists
ALL.update(MEM_EDGES)
ALL.update(MEM_EDGES_NO_PROOF)


# ---- hash-call edges of proof mode 4 (tests/test_memory_edges.py) -----------------------------------------------------------------------------------------------
HASH_MAX_LEN = 1 << 20               # a mode-4 proof states hash calls of up to 1 MiB of input


def _call(num, in_ptr, length, out_ptr):
    """r11 = in, r12 = len, r13 = out (any 40-bit value), r10 = the syscall; ECALL."""
    return li40(11, in_ptr) + li40(12, length) + li40(13, out_ptr) + [A(10, 0, num), EC]


def hash_edge_calls():
    """Keccak-256 and BLAKE3 digests written at out = 1, 3, 5 (mod 8) — 5 cells instead of 4, byte writes — SHA-256 at out = 4 (mod 8), zero-length inputs, inputs that overlap
    their own output.  The hashed messages are the reference's KAT messages ("" and "hello" at 0x2000)."""
    code = [A(5, 0, 0x2000)] + _store_bytes(5, b"hello")
    for num, ln, out in ((5, 5, 0x3001), (5, 0, 0x3043), (5, 5, 0x3085), (6, 0, 0x3101), (6, 0, 0x3143), (6, 5, 0x3185), (3, 5, 0x3204), (3, 0, 0x324C)):
        code += [A(11, 5, 0), A(12, 0, ln), A(13, 0, out), A(10, 0, num), EC]
    code += [A(11, 0, 0x3300), A(12, 0, 40), A(13, 0, 0x3311), A(10, 0, 5), EC]     # the output inside the input: the message is read before the digest is written
    code += [A(11, 0, 0x3404), A(12, 0, 64), A(13, 0, 0x3404), A(10, 0, 3), EC]     # the same first byte
    code += [A(11, 0, 0x3001), A(12, 0, 75), A(13, 0, 0x3003), A(10, 0, 6), EC]     # re-hash the digests above, the output over them
    return _p(code + [EB]), [], {}


def hash_edge_top():
    """An input that ends exactly at 2^40 and an output at 2^40 - 32 (the top cell holds its last 8 bytes)."""
    code = li40(5, (1 << 40) - 40) + _store_bytes(5, bytes(range(0xC0, 0xC8)))
    code += _call(5, (1 << 40) - 37, 37, (1 << 40) - 32) + _call(3, (1 << 40) - 32, 32, (1 << 40) - 64) + _call(6, (1 << 40) - 64, 64, (1 << 40) - 33)
    return _p(code + [EB]), [], {}


def hash_edge_boundary():
    """A digest written over the boundary cell's data half (out = B + 4) and one that starts inside it (out = B + 6); the first message is read from B itself (the last code
    word and the first data word) and the data word behind it."""
    code = _call(6, BC, 12, BC + 4) + _call(5, BC + 4, 32, BC + 6) + [EB]
    assert len(code) <= _BC_WORDS
    code += [A(7, 0, 2)] * (_BC_WORDS - len(code))
    return _p(code, data=bytes(range(0x41, 0x49))), [], {}


def hash_edge_max_len():
    """A SHA-256 call over exactly MAX_LEN = 1 MiB (memory that is zero but for one byte)."""
    code = li40(5, 0x100000 + 12345) + [A(9, 0, 0xAB), E(O.SB, rs1=5, rs2=9, imm=0)] + _call(3, 0x100000, HASH_MAX_LEN, 0x300000)
    return _p(code + [EB]), [], {}


def hash_edge_len_over():
    """MAX_LEN + 1 bytes of input: the VM hashes them, a mode-4 proof cannot state the call."""
    return _p(_call(5, 0x100000, HASH_MAX_LEN + 1, 0x300000) + [EB]), [], {}


def hash_edge_out_over_2p40():
    """A digest whose last 16 bytes land above 2^40 (byte writes: the VM runs it)."""
    return _p(_call(6, 0x2000, 8, (1 << 40) - 16) + [EB]), [], {}


def hash_edge_in_over_code():
    """A message read from the code segment (the VM reads it; the AIR states no code cell)."""
    return _p(_call(5, 0x1000, 16, 0x3000) + [EB]), [], {}


def hash_edge_out_over_code():
    """A digest written over the first eight code words, already executed (strict protection is off, vm.rs:175)."""
    return _p([A(0, 0, 0)] * 8 + _call(6, 0x2000, 8, 0x1000) + [EB]), [], {}


def hash_misaligned_sha_shape():
    """err_misaligned_sha_out with its SHA-256 output pointer moved to 0x3000: the run the VM completes, whose rows a forger starts from."""
    return _p([A(11, 0, 0x2000), A(12, 0, 0), A(13, 0, 0x3000), A(10, 0, 3), EC, EB]), [], {}


HASH_EDGES = {f.__name__: f for f in (hash_edge_calls, hash_edge_top, hash_edge_boundary, hash_edge_max_len)}                      # these have a mode-4 proof
HASH_EDGES_NO_PROOF = {f.__name__: f for f in (hash_edge_len_over, hash_edge_out_over_2p40, hash_edge_in_over_code, hash_edge_out_over_code)}


# ---- programs larger than the prover's LDS window over the instruction ROM (4096 words) and pcs past 2^20 (tests/test_big_code.py, tests/test_gpu_big_code.py) -------------
# Built at run time and cached: the largest blob is about 1 MiB.  Every word that is not placed is an EBREAK, so a run that strays halts; every run is capped with max_cycles a
# little above its intended row count, so a builder mistake costs rows and not minutes.
ROM_LDS = 4096                                   # the first ROM rows the prover counts in LDS; rows from here on are counted with global atomics
W20 = (0x100000 - 0x1000) // 4                   # the code word whose pc is 2^20 (261120): JAL's 21-bit offset reaches it from the first words
PC = lambda word: 0x1000 + 4 * word              # noqa: E731


def _big(n_words, placed, data=b""):
    """A blob of n_words code words: `placed` = {first word index: [words]}, EBREAK everywhere else."""
    code = [EB] * n_words
    for at, words in placed.items():
        assert 0 <= at and at + len(words) <= n_words and all(w == EB for w in code[at:at + len(words)]), at
        code[at:at + len(words)] = words
    return _p(code, data)


def _jal_to(rd, frm, to):
    """JAL at word `frm` to word `to`."""
    assert -(1 << 20) <= 4 * (to - frm) < (1 << 20)
    return spec.jal(rd, 4 * (to - frm))


@functools.lru_cache(maxsize=None)
def _rom_straddle():
    n, body = 4200, ROM_LDS - 2
    return _big(n, {
        0: [A(3, 0, 300), A(1, 0, 0), _jal_to(14, 2, 10), _jal_to(0, 3, body - 4)],
        10: [A(2, 2, 7), A(1, 1, 1), E(O.JALR, 0, 14, imm=0)],                               # a block below the window's end, called before and after the loop
        body - 4: [A(4, 0, 1), A(4, 4, 1), A(4, 4, 1), A(4, 4, 1),                          # words 4090 .. 4093: straight-line code that runs on through 4099
                   spec.add(4, 4, 2), A(1, 1, 3), A(3, 3, -1), spec.bne(3, 0, -12),          # words 4094 .. 4097: the loop body, 300 times, two words on each side of the split
                   A(4, 4, 1), A(4, 4, 1), _jal_to(14, body + 6, 10),                        # words 4098 .. 4100
                   A(11, 1, 0), A(10, 0, 2), EC] + _exit0()})


def rom_straddle():
    """4200 code words; straight-line code through words 4093 .. 4099, a counted loop over words 4094 .. 4097 run 300 times (multiplicities above 255 on both sides of the
    split), a block at words 10 .. 12 called before and after the loop.  1223 rows: more ROM rows than trace rows (N = 2048)."""
    return _rom_straddle(), [], {"max_cycles": 1240}


@functools.lru_cache(maxsize=None)
def _rom_far_hot():
    hot = 4300
    return _big(4400, {0: [A(1, 0, 1), _jal_to(0, 1, hot)],
                       hot: [spec.add(2, 2, 1), A(3, 2, 5), E(O.XOR, 4, 3, 2), spec.sub(5, 4, 1), E(O.SLTU, 6, 5, 4), A(1, 1, 1), _jal_to(0, hot + 6, hot)]})


def rom_far_hot():
    """About 4400 code words, the whole hot loop (7 words) above word 4096, run to exactly 2^12 rows: every lane of every block adds to the same few global counters."""
    return _rom_far_hot(), [], {"max_cycles": 1 << 12}


@functools.lru_cache(maxsize=None)
def _rom_exact(n):
    return _big(n, {0: [A(3, 0, 3), _jal_to(0, 1, n - 6)], n - 6: [A(1, 1, 1), A(3, 3, -1), spec.bne(3, 0, -8), A(10, 0, 0), A(11, 0, 0), EC]})


def rom_exact_4096():
    """Exactly 4096 code words (the LDS window is the whole ROM), the last one executed."""
    return _rom_exact(ROM_LDS), [], {"max_cycles": 24}


def rom_exact_4097():
    """Exactly 4097 code words: the global path holds a single ROM row, executed once (the exit's ECALL)."""
    return _rom_exact(ROM_LDS + 1), [], {"max_cycles": 24}


PC_CARRY_WORDS = W20 + 64


@functools.lru_cache(maxsize=None)
def _pc_carry():
    return _big(PC_CARRY_WORDS, {
        0: [A(1, 0, 0), A(7, 0, 2), _jal_to(0, 2, W20 - 3)],                                  # the delta is 0xFEFEC: below 2^20
        W20 - 6: [A(8, 6, 0), _jal_to(9, W20 - 5, W20 + 4)],                                  # 0xFFFE8: where the JALR lands; forward over the boundary again (link 0xFFFF0)
        W20 - 3: [A(3, 3, 5), A(1, 1, 1),                                                     # 0xFFFF4, 0xFFFF8 (the BNE's target: the pass counter)
                  spec.jal(5, 4),                                                             # 0xFFFFC: the link is 0x100000, and so is the next pc
                  A(4, 5, 0), E(O.SRLI, 12, 5, imm=20),                                       # 0x100000, 0x100004: the link's second limb, read
                  spec.bne(1, 7, -16),                                                        # 0x100008 -> 0xFFFF8: taken on the first pass, not on the second
                  E(O.JALR, 6, 5, imm=-24),                                                   # 0x10000C -> 0xFFFE8 through the linked register; link 0x100010
                  spec.add(11, 4, 12), A(10, 0, 2), EC] + _exit0()})                          # 0x100010: WRITE 0x100001, exit


def pc_carry():
    """W20 + 64 code words (1 MiB).  A JAL from word 2 to pc 0xFFFF4; a JAL at pc 0xFFFFC whose link and target are 0x100000; a BNE at 0x100008 back to 0xFFFF8 (a negative
    imm17 borrowing out of pc limb 1), taken once and not taken once; a JALR through the linked register from 0x10000C back to 0xFFFE8; a JAL forward again; WRITE, exit.
    23 rows; rows 5 and 10 sit at pc 0xFFFFC."""
    return _pc_carry(), [], {"max_cycles": 32}


PC_CARRY_MEM_WORDS = W20 + 65                                         # odd: the boundary cell 0x100100 holds the last code word and the first data word
PC_CARRY_MEM_DATA = PC(PC_CARRY_MEM_WORDS)                            # 0x100104
PC_CARRY_MEM_BC = PC_CARRY_MEM_DATA - 4


@functools.lru_cache(maxsize=None)
def _pc_carry_mem(wide):
    base = PC_CARRY_MEM_DATA + 4                                      # 0x100108: the first whole data cell
    head = li40(5, base) + [A(1, 0, 0x1234)]
    body = [A(3, 3, 5), A(3, 3, 1), A(3, 3, 1),                       # 0xFFFF4 .. 0xFFFFC: the pc + 4 carry of a sequential row
            spec.sw(5, 1, 40), spec.lw(2, 5, 40), E(O.LB, 4, 5, imm=1), spec.lw(6, 5, 0), E(O.SB, rs1=5, rs2=1, imm=33), E(O.LD, 7, 5, imm=32)]
    if wide:
        body += [spec.lw(8, 5, -4),                                   # the data half of the boundary cell
                 A(11, 5, 0), A(12, 0, 32), A(13, 5, 32), A(10, 0, 3), EC, spec.lw(9, 13, 0)]       # SHA-256 of the data's first 32 bytes, the digest right behind them
    body += [A(11, 2, 0), A(10, 0, 2), EC] + _exit0()
    return _big(PC_CARRY_MEM_WORDS, {0: head + [_jal_to(0, len(head), W20 - 3)], W20 - 3: body}, data=bytes(range(0x41, 0x41 + 36)))


def pc_carry_mem(wide=False):
    """pc_carry's jump to 0xFFFF4 and straight-line code over pc 0x100000 (the sequential pc + 4 carry), an odd word count and 36 data bytes at 0x100104 — above 2^20, so
    every address limb 1 and every touched cell's second limb is non-zero: SW / LW / LB / SB / LD there.  `wide` (mode 4) adds a load of the boundary cell's data half and
    one SHA-256 call whose input is that data and whose output lies right behind it."""
    return _pc_carry_mem(bool(wide)), [], {"max_cycles": 48}


def _on_last_code_word(store):
    last = PC(PC_CARRY_WORDS - 1)
    return _big(PC_CARRY_WORDS, {0: li40(5, last) + [A(1, 0, 7), spec.sw(5, 1, 0) if store else spec.lw(2, 5, 0), A(3, 0, 1), EB]})


@functools.lru_cache(maxsize=None)
def _big_store_on_code():
    return _on_last_code_word(True)


@functools.lru_cache(maxsize=None)
def _big_load_on_code():
    return _on_last_code_word(False)


def big_store_on_code():
    """A store to the last code word of a 1 MiB code segment (0x1000FC): the VM runs it, a mode-3 proof is refused (the overlap rule, with a bound above 2^20)."""
    return _big_store_on_code(), [], {"max_cycles": 16}


def big_load_on_code():
    """A load from the last code word of a 1 MiB code segment: likewise."""
    return _big_load_on_code(), [], {"max_cycles": 16}


BIG_CODE = {f.__name__: f for f in (rom_straddle, rom_far_hot, rom_exact_4096, rom_exact_4097, pc_carry, pc_carry_mem)}
BIG_CODE_REFUSED = {f.__name__: f for f in (big_store_on_code, big_load_on_code)}

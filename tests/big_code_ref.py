"""Shared by tests/test_big_code.py (CPU) and tests/test_gpu_big_code.py (GPU): the big-code programs of tests/programs.py run through the oracle ONCE per process — its rows,
public inputs and proofs are the expected values of both modules and are never changed (tampered copies are copies)."""
from __future__ import annotations

import functools

import numpy as np

import programs as pg
from oracle import api as oracle, stark_api as so

HEADER_WORDS = 157
MODE_KW = {0: {}, 2: {"io_mode": True}, 3: {"mem_mode": True}, 4: {"wide_mode": True}}

# program -> the proof modes it is proven in.  pc_carry_mem is two programs: a mode-3 proof states neither a hash call nor the boundary cell, so the mode-4 variant adds both.
MODES = {"rom_straddle": (0, 3), "rom_far_hot": (0, 3), "rom_exact_4096": (0, 3), "rom_exact_4097": (0, 3), "pc_carry": (0, 2, 3), "pc_carry_mem": (0, 3), "pc_carry_mem_wide": (4,)}
PROOF_CASES = [(name, mode) for name, modes in MODES.items() for mode in modes]
PC_PROGRAMS = ("pc_carry", "pc_carry_mem", "pc_carry_mem_wide")
REFUSED = tuple(sorted(pg.BIG_CODE_REFUSED))


def program(name):
    """(blob, inputs, cfg) of a big-code program by its case name."""
    if name == "pc_carry_mem_wide":
        return pg.pc_carry_mem(wide=True)
    return (pg.BIG_CODE.get(name) or pg.BIG_CODE_REFUSED[name])()


@functools.lru_cache(maxsize=None)
def run(name):
    """The oracle's run of a program (rows, outputs, halt reason)."""
    blob, ins, cfg = program(name)
    return oracle.run(blob, list(ins), enable_execution_trace=True, **cfg)


def public(name, mode):
    """The oracle's public inputs of a program's run in a proof mode (a fresh struct: callers may edit it)."""
    blob, ins, cfg = program(name)
    ores = run(name)
    return so.public_inputs(len(ores.rows), blob, list(ins), list(ores.outputs), (ores.halt_kind, ores.halt_code), **MODE_KW[mode])


@functools.lru_cache(maxsize=None)
def proof(name, mode):
    """The oracle's proof (read-only)."""
    pr = so.prove(run(name).rows, public(name, mode))
    pr.setflags(write=False)
    return pr


def blob_at(mode):
    """The proof word that holds the first 16-bit halfword of the carried program (oracle/stark_oracle.cpp so::prove: header, modes 2+ four counter words, the byte length)."""
    return HEADER_WORDS + (4 if mode >= 2 else 0) + 1


def rom_index(rows):
    """The instruction-ROM row of every executed row."""
    return (rows["pc"].astype(np.int64) - 0x1000) >> 2

"""Driver for the self-defined prover stages (stark.hip) — Baby Bear LDE + Poseidon2-12 Merkle commitment.

NOT in the reference (parity unpinned); spec = oracle/stark_oracle.cpp, DESIGN.md §8.
PyTorch is plumbing (device buffers, streams); all arithmetic happens in the HIP kernels behind the C ABI.
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional, Sequence

import numpy as np
import torch

from . import pipeline as pl
from . import runtime as rt

P = 2013265921
W_MAIN = 152                 # COMMITTED main-trace columns of a default-mode run (zkir_main_trace_width); the AIR has 172 logical columns (air.h: W)
W_MAIN_DEFERRED = 168        # deferred mode: the storage states are committed too
W_AUX = 40                  # aux trace of the lookup argument (air.h): H0..H7, HR, S as four base columns each
RC_TABLE = 1024
HEADER_WORDS = 157


MEM_MULT = RC_TABLE + 256 + 16 + 3 * 256 + RC_TABLE     # (mode 3) LOW3 | BYTE | NIBBLE | AND | OR | XOR | LOW6 multiplicities (air.h MEM_MULT)


def proof_layout(proof) -> dict:
    """Word offsets inside a proof of ANY mode (word 9): header (157 words; modes 2 / 3: + the four counter words) | program (byte length, 16-bit halfwords) | modes 2 / 3: the
    I/O section (n_in, inputs as four 16-bit pieces each, n_out, outputs, halt kind, halt code) | mode 3: the touched cells (n, 7 words a cell) | mode 4: the hash tape, the wide tape | ROM multiplicities | range
    multiplicities | mode 3: the LOW3 .. LOW6 multiplicities | trace root | aux root | quotient root | openings ...  (oracle/stark_oracle.cpp so::prove is the layout's definition)."""
    mode = int(proof[9])
    at = HEADER_WORDS + (4 if mode >= 2 else 0)
    blob_len = int(proof[at])
    at += 1
    half = np.asarray(proof[at:at + (blob_len + 1) // 2], dtype=np.uint32)
    blob = np.stack([half & 0xFF, half >> 8], axis=1).astype(np.uint8).reshape(-1)[:blob_len].tobytes()
    n_rom = int.from_bytes(blob[16:20], "little") // 4 if blob_len >= 32 else 0
    at += (blob_len + 1) // 2
    io_at = mem_at = None
    if mode >= 2:
        io_at = at
        n_in = int(proof[at]); at += 1 + 4 * n_in
        n_out = int(proof[at]); at += 1 + 4 * n_out
        at += 5
    hash_at = wide_at = None
    if mode >= 3:
        mem_at = at
        at += 1 + 7 * int(proof[at])
    if mode == 4:                                             # (mode 4) the hash calls: [n] then per call 8 words + 5 per touched cell
        hash_at = at
        n_calls = int(proof[at]); at += 1
        for _ in range(n_calls):
            at += 8 + 5 * int(proof[at + 7])
        wide_at = at                                          # .. then the wide tape: [n] then per record [cycle] [rs1: three limbs] [rs2: three limbs] [opcode]
        at += 1 + 8 * int(proof[at])
    rom_mult = at
    troot = rom_mult + n_rom + RC_TABLE + (MEM_MULT if mode >= 3 else 0)
    return {"mode": mode, "num_queries": int(proof[4]), "pow_bits": int(proof[6]), "blob": blob, "n_rom": n_rom, "io_section": io_at, "mem_section": mem_at, "hash_section": hash_at, "wide_section": wide_at, "rom_mult": rom_mult,
            "rc_mult": rom_mult + n_rom, "trace_root": troot, "aux_root": troot + 4, "quotient_root": troot + 8, "openings": troot + 12}


def trace_root(proof) -> list:
    t0 = proof_layout(proof)["trace_root"]
    return [int(x) for x in proof[t0:t0 + 4]]


class StarkContext:
    """zkir_stark_ctx: device tables for traces of 2^log_n rows, extended to 2^(log_n + log_blowup) (log_blowup 1, 2, 3: blow-up 2, 4, 8; log_n + log_blowup <= 27).
    Contexts of log_blowup 2 / 3 serve the commitment (lde, merkle_commit, commit_trace); and lowdeg_prove (a low-degree proof of such a
    commitment, at the context's rate); zkir_prove's proofs are blow-up 2: prove() raises on them, prove_rate() (modes 0 - 2) and prove_rate_modes() (every mode) prove a run at the context's own rate."""

    def __init__(self, log_n: int, log_blowup: int = 1):
        pl._require_gpu()
        self.log_n, self.log_blowup = log_n, log_blowup
        h = C.c_void_p()
        rc = rt.lib().zkir_stark_ctx_create(log_n, log_blowup, C.byref(h))
        if rc != rt.ZKIR_OK:
            rt._raise(rc)
        self._h = h
        if hasattr(rt.lib(), "zkir_stark_ctx_log_blowup"):
            self.log_blowup = int(rt.lib().zkir_stark_ctx_log_blowup(h))     # what the library holds

    @property
    def handle(self):
        return self._h

    def close(self):
        if self._h:
            rt.lib().zkir_stark_ctx_free(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _sp(stream):
    return C.c_void_p((stream or torch.cuda.current_stream()).cuda_stream)


def padded_log_n(n_real: int) -> int:
    return int(rt.lib().zkir_padded_log_n(n_real))


# ---- the B8 matrix layout of the C ABI (include/zkir_amd.h): blocks of 8 columns, block b = [rows][8] -----------------------------
def to_b8(cols: torch.Tensor) -> torch.Tensor:
    """Column-major int32[width][n] -> B8 int32[ceil(width/8)][n][8] (missing columns of the last block are zero)."""
    width, n = cols.shape
    nb = (width + 7) // 8
    out = torch.zeros((nb * 8, n), dtype=cols.dtype, device=cols.device)
    out[:width] = cols
    return out.view(nb, 8, n).permute(0, 2, 1).contiguous()


def main_width(deferred: bool = False) -> int:
    """Committed main-trace columns of a run (zkir_main_trace_width_for): 152 in the default VM mode, 168 with the deferred model."""
    return W_MAIN_DEFERRED if deferred else W_MAIN


def from_b8(mat: torch.Tensor, width: int) -> torch.Tensor:
    """B8 int32[nb][n][8] -> column-major int32[width][n]."""
    nb, n, _ = mat.shape
    return mat.permute(0, 2, 1).reshape(nb * 8, n)[:width].contiguous()


def main_trace(trace: pl.DeviceTrace, stream=None, deferred: bool = False) -> torch.Tensor:
    """K4: SoA execution trace (n_rows executed rows) -> the COMMITTED main-trace matrix in the B8 layout, int32[main_width(deferred) / 8][N][8],
    N = the padded power of two."""
    n = trace.n_rows
    out = torch.empty((main_width(deferred) // 8, 1 << padded_log_n(n), 8), dtype=torch.int32, device=trace.cycle.device)
    pl._check(rt.lib().zkir_main_trace_launch(C.byref(trace.c), n, int(deferred), out.data_ptr(), _sp(stream)))
    return out


def lde(ctx: StarkContext, mat: torch.Tensor, stream=None, clobber: bool = False) -> torch.Tensor:
    """Per-column LDE of a B8 matrix int32[nb][N][8] to int32[nb][M][8], M = N << ctx.log_blowup, on the coset 31*<w_M> (natural order)."""
    nb, n, eight = mat.shape
    assert eight == 8 and n == 1 << ctx.log_n and mat.dtype == torch.int32 and mat.is_contiguous()
    src = mat if clobber else mat.clone()
    out = torch.empty((nb, n << ctx.log_blowup, 8), dtype=torch.int32, device=mat.device)
    pl._check(rt.lib().zkir_lde_launch(ctx.handle, src.data_ptr(), nb * 8, out.data_ptr(), _sp(stream)))
    return out


def merkle_commit(ctx: StarkContext, mat: torch.Tensor, width: Optional[int] = None, stream=None) -> torch.Tensor:
    """Poseidon2-12 Merkle tree over the rows (positions) of a B8 matrix int32[nb][n][8] with `width` real columns (default all);
    returns the tree int32[4*(2n-1)], root = last 4."""
    nb, n, eight = mat.shape
    assert eight == 8 and mat.dtype == torch.int32 and mat.is_contiguous()
    width = nb * 8 if width is None else width
    tree = torch.empty(4 * (2 * n - 1), dtype=torch.int32, device=mat.device)
    pl._check(rt.lib().zkir_merkle_commit_launch(ctx.handle, mat.data_ptr(), width, n, tree.data_ptr(), _sp(stream)))
    return tree


def merkle_cap(ctx: StarkContext, digests: torch.Tensor, stream=None) -> torch.Tensor:
    """Root over n (power of two) digests int32[n][4] — the all-gathered per-GPU subtree roots of a row-sharded commitment."""
    n = digests.shape[0]
    tree = torch.empty(4 * (2 * n - 1), dtype=torch.int32, device=digests.device)
    tree[:4 * n] = digests.reshape(-1)
    pl._check(rt.lib().zkir_merkle_cap_launch(ctx.handle, tree.data_ptr(), n, _sp(stream)))
    return tree[-4:]


opening_words = rt.opening_words
OPEN_LEAF_DIGEST, VERIFY_FORM_LANE, VERIFY_FORM_ROW16 = rt.OPEN_LEAF_DIGEST, rt.VERIFY_FORM_LANE, rt.VERIFY_FORM_ROW16


def _indices(indices, device) -> torch.Tensor:
    """Row indices as the C ABI takes them: uint64 words on the device (torch has no arithmetic on uint64: they travel as int64 bit patterns)."""
    if isinstance(indices, torch.Tensor):
        assert indices.dtype == torch.int64
        return indices.to(device).contiguous().reshape(-1)
    return torch.from_numpy(np.asarray(indices, dtype=np.uint64).reshape(-1).view(np.int64).copy()).to(device)


def merkle_open(ctx: StarkContext, mat: Optional[torch.Tensor], tree: torch.Tensor, indices, width: Optional[int] = None, stream=None) -> torch.Tensor:
    """zkir_merkle_open_launch: the opening records int32[n_idx][width + 4 d] of the rows `indices` of the committed B8 matrix `mat` (`width` real columns, default all)
    under `tree` (merkle_commit's); mat=None: the digest form int32[n_idx][4 + 4 d] of a tree over digests (merkle_cap's full buffer).  An index >= n_leaves gives a record
    of 0xFFFFFFFF words."""
    assert tree.dtype == torch.int32 and tree.is_contiguous() and tree.numel() % 4 == 0
    n = (tree.numel() // 4 + 1) // 2
    if mat is None:
        assert width in (None, 0)
        width, flags = 0, OPEN_LEAF_DIGEST
    else:
        nb, rows, eight = mat.shape
        assert eight == 8 and rows == n and mat.dtype == torch.int32 and mat.is_contiguous()
        width, flags = (nb * 8 if width is None else width), 0
    idx = _indices(indices, tree.device)
    words = opening_words(width, n, flags)
    out = torch.empty((idx.numel(), words), dtype=torch.int32, device=tree.device)
    pl._check(rt.lib().zkir_merkle_open_launch(ctx.handle, mat.data_ptr() if mat is not None else None, width, n, tree.data_ptr(), idx.data_ptr(), idx.numel(), out.data_ptr(), _sp(stream)))
    return out


def merkle_verify(ctx: StarkContext, root: torch.Tensor, width: int, n_leaves: int, indices, openings: torch.Tensor, flags: int = 0, stream=None):
    """zkir_merkle_verify_launch: (verdicts int32[n_idx], summary int32[2]) of the opening records against `root` (a device tensor of four words, e.g. tree[-4:]):
    0 ok, 1 wrong, 2 a word >= p, 3 index >= n_leaves; summary = (failures, smallest failing position or -1 = 0xFFFFFFFF)."""
    assert root.dtype == torch.int32 and root.numel() == 4 and openings.dtype == torch.int32 and openings.is_contiguous()
    root = root.contiguous()
    idx = _indices(indices, openings.device)
    assert openings.numel() == idx.numel() * opening_words(width, n_leaves, flags)
    verdicts = torch.empty(idx.numel(), dtype=torch.int32, device=openings.device)
    summary = torch.empty(2, dtype=torch.int32, device=openings.device)
    pl._check(rt.lib().zkir_merkle_verify_launch(ctx.handle, root.data_ptr(), width, n_leaves, idx.data_ptr(), idx.numel(), openings.data_ptr(), flags, verdicts.data_ptr(), summary.data_ptr(), _sp(stream)))
    return verdicts, summary


lowdeg_proof_words = rt.lowdeg_proof_words


def _matrix_width(name: str, ctx: StarkContext, lde_mat: torch.Tensor, width: Optional[int]) -> int:
    """the real columns of a B8 matrix (default all); ValueError for a matrix that is not of the context's size or does not have them"""
    m = 1 << (ctx.log_n + ctx.log_blowup)
    if lde_mat.dim() != 3 or lde_mat.shape[1] != m or lde_mat.shape[2] != 8 or lde_mat.dtype != torch.int32 or not lde_mat.is_contiguous():
        raise ValueError(f"{name}: the matrix must be contiguous int32[blocks][{m}][8], the context's extension size")
    width = lde_mat.shape[0] * 8 if width is None else int(width)
    if width > lde_mat.shape[0] * 8:
        raise ValueError(f"{name}: width exceeds the matrix's columns")
    return width


def _check_tree(name: str, ctx: StarkContext, tree: torch.Tensor, the: str = "the") -> None:
    """ValueError unless the tree is merkle_commit's over the context's leaves"""
    m = 1 << (ctx.log_n + ctx.log_blowup)
    if tree.dtype != torch.int32 or not tree.is_contiguous() or tree.numel() != 4 * (2 * m - 1):
        raise ValueError(f"{name}: {the} tree must be contiguous int32[{4 * (2 * m - 1)}], merkle_commit's over {m} leaves")


def _prove_call(entry: str, n_stages: int, args: tuple, cap: int, stream, want_stage_ms: bool):
    """the tail of a prove call: a buffer of `cap` words, the entry or its _stages variant (n_stages device ms), the proof cut to the words written"""
    out = np.zeros(max(cap, 1), np.uint32)
    n_words = C.c_uint64()
    args = (*args, out.ctypes.data, cap, C.byref(n_words))
    if want_stage_ms:
        ms = (C.c_float * n_stages)()
        pl._check(getattr(rt.lib(), entry + "_stages")(*args, ms, _sp(stream)))
        return out[:n_words.value], [float(x) for x in ms]
    pl._check(getattr(rt.lib(), entry)(*args, _sp(stream)))
    return out[:n_words.value]


def lowdeg_prove(ctx: StarkContext, lde_mat: torch.Tensor, tree: torch.Tensor, width: Optional[int] = None, num_queries: int = 50, pow_bits: int = 12, stream=None,
                 want_stage_ms: bool = False):
    """zkir_lowdeg_prove: the low-degree proof (np.uint32 words) of the commitment `tree` (merkle_commit's) to the B8 matrix `lde_mat` (lde's output on `ctx`, `width` real
    columns, default all): every column is close to a polynomial of degree < 2^ctx.log_n — no constraint, no opening at a point.  Works at every rate a context serves.
    A matrix or tree that is not of the context's size raises ValueError; the library refuses bad parameters with ERR_ARGUMENT before any launch.
    want_stage_ms: also the device ms of (combine, FRI commit phase, grinding, query section)."""
    width = _matrix_width("lowdeg_prove", ctx, lde_mat, width)
    _check_tree("lowdeg_prove", ctx, tree)
    cap = lowdeg_proof_words(ctx.log_n, ctx.log_blowup, width, num_queries)
    return _prove_call("zkir_lowdeg_prove", 4, (ctx.handle, lde_mat.data_ptr(), width, tree.data_ptr(), int(num_queries), int(pow_bits)), cap, stream, want_stage_ms)


def _verify_stream(device: bool, stream):
    """the stream a *_verify(device=True) call runs on (a torch stream, default the current one); None for the host form, which touches no GPU"""
    return _sp(stream) if device else None


def lowdeg_verify(proof, root=None, device: bool = False, stream=None) -> int:
    """rt.lowdeg_verify; device=True checks the queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.lowdeg_verify(proof, root, device=device, stream=_verify_stream(device, stream))


pcs_verify_last_jobs = rt.pcs_verify_last_jobs


def lowdeg_combine(ctx: StarkContext, lde_mat: torch.Tensor, gamma, width: Optional[int] = None, stream=None) -> torch.Tensor:
    """(tests, measurements) zkir_lowdeg_combine_launch: the codeword int32[4][M] of lowdeg_prove's first stage for a GIVEN canonical gamma (four words):
    row t = coordinate t of sum_k gamma^k col_k."""
    nb, m, eight = lde_mat.shape
    assert eight == 8 and m == 1 << (ctx.log_n + ctx.log_blowup) and lde_mat.dtype == torch.int32 and lde_mat.is_contiguous()
    width = nb * 8 if width is None else int(width)
    assert 1 <= width <= nb * 8
    g = np.ascontiguousarray(gamma, dtype=np.uint32).reshape(4)
    scratch = torch.empty(32 * ((width + 7) // 8), dtype=torch.int32, device=lde_mat.device)
    cw = torch.empty((4, m), dtype=torch.int32, device=lde_mat.device)
    pl._check(rt.lib().zkir_lowdeg_combine_launch(ctx.handle, lde_mat.data_ptr(), width, g.ctypes.data, scratch.data_ptr(), cw.data_ptr(), _sp(stream)))
    return cw


eval_proof_words = rt.eval_proof_words


def eval_verify(proof, root=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """rt.eval_verify; device=True checks the queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.eval_verify(proof, root, points, evals, device=device, stream=_verify_stream(device, stream))


def _eval_args(name: str, ctx: StarkContext, lde_mat: torch.Tensor, width: Optional[int], points):
    """(width, points uint32[n_points][4]) of an evaluation call; ValueError for a matrix that is not of the context's size or points that are not rows of four words"""
    width = _matrix_width(name, ctx, lde_mat, width)
    pts = np.ascontiguousarray(points, dtype=np.uint32)
    if pts.ndim != 2 or pts.shape[1] != 4:
        raise ValueError(f"{name}: points must be [n_points][4] canonical words")
    return width, pts


def eval_prove(ctx: StarkContext, lde_mat: torch.Tensor, tree: torch.Tensor, width: Optional[int], points, num_queries: int = 50, pow_bits: int = 12, stream=None,
               want_stage_ms: bool = False):
    """zkir_eval_prove: the evaluation proof (np.uint32 words) of the commitment `tree` (merkle_commit's) to the B8 matrix `lde_mat` (lde's output on `ctx`, `width` real
    columns, default all) at `points` ([1 or 2][4] canonical words, E4 elements outside the base field, CHOSEN AFTER THE ROOT): every column is close to a polynomial of
    degree < 2^ctx.log_n with the proof's evaluations at the points (eval_layout finds them).  Works at every rate a context serves.  A matrix or tree that is not of the
    context's size raises ValueError; the library refuses bad parameters and points with ERR_ARGUMENT before any launch.
    want_stage_ms: also the device ms of (weights, evaluations, quotient, FRI commit phase, grinding, query section)."""
    width, pts = _eval_args("eval_prove", ctx, lde_mat, width, points)
    _check_tree("eval_prove", ctx, tree)
    cap = eval_proof_words(ctx.log_n, ctx.log_blowup, width, len(pts), num_queries)
    return _prove_call("zkir_eval_prove", 6, (ctx.handle, lde_mat.data_ptr(), width, tree.data_ptr(), pts.ctypes.data, len(pts), int(num_queries), int(pow_bits)), cap, stream, want_stage_ms)


def eval_at(ctx: StarkContext, lde_mat: torch.Tensor, points, width: Optional[int] = None, stream=None) -> torch.Tensor:
    """(tests, measurements) zkir_eval_at_launch: the evaluations int32[n_points][width][4] of eval_prove's first stages alone, for GIVEN points."""
    width, pts = _eval_args("eval_at", ctx, lde_mat, width, points)
    scratch = torch.empty(max(1, int(rt.lib().zkir_eval_at_scratch_words(ctx.log_n, width, len(pts)))), dtype=torch.int32, device=lde_mat.device)
    out = torch.empty((len(pts), width, 4), dtype=torch.int32, device=lde_mat.device)
    pl._check(rt.lib().zkir_eval_at_launch(ctx.handle, lde_mat.data_ptr(), width, pts.ctypes.data, len(pts), scratch.data_ptr(), out.data_ptr(), _sp(stream)))
    return out


def eval_quotient(ctx: StarkContext, lde_mat: torch.Tensor, gamma, points, evals, width: Optional[int] = None, stream=None) -> torch.Tensor:
    """(tests, measurements) zkir_eval_quotient_launch: the codeword int32[4][M] of eval_prove's quotient stage for GIVEN canonical gamma (four words), points and
    evaluations ([n_points][width][4]): row t = coordinate t of F."""
    width, pts = _eval_args("eval_quotient", ctx, lde_mat, width, points)
    g = np.ascontiguousarray(gamma, dtype=np.uint32).reshape(4)
    y = np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
    if len(y) != 4 * len(pts) * width:
        raise ValueError("eval_quotient: evals must be [n_points][width][4] words")
    m = 1 << (ctx.log_n + ctx.log_blowup)
    scratch = torch.empty(max(1, int(rt.lib().zkir_eval_quotient_scratch_words(ctx.log_n + ctx.log_blowup, width, len(pts)))), dtype=torch.int32, device=lde_mat.device)
    cw = torch.empty((4, m), dtype=torch.int32, device=lde_mat.device)
    pl._check(rt.lib().zkir_eval_quotient_launch(ctx.handle, lde_mat.data_ptr(), width, g.ctypes.data, pts.ctypes.data, len(pts), y.ctypes.data, scratch.data_ptr(), cw.data_ptr(), _sp(stream)))
    return cw


def eval_layout(proof) -> dict:
    """Word offsets of a well-formed evaluation proof: the header's fields, root, points, evals ([n_points][width][4] from there), layer_roots, final, nonce, queries, and the
    words of one query (qsize)."""
    log_n, b, width, n_points, nq, _, n_layers = (int(x) for x in proof[2:9])
    at = {"log_n": log_n, "log_blowup": b, "width": width, "n_points": n_points, "num_queries": nq, "n_layers": n_layers, "root": 9, "points": 13, "evals": 13 + 4 * n_points}
    at["layer_roots"] = at["evals"] + 4 * n_points * width
    at["final"] = at["layer_roots"] + 4 * n_layers
    at["nonce"] = at["final"] + 4 * (4 << b)
    at["queries"] = at["nonce"] + 1
    at["qsize"] = (len(proof) - at["queries"]) // nq if nq else 0
    return at


batch_eval_proof_words = rt.batch_eval_proof_words


def batch_eval_verify(proof, roots=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """rt.batch_eval_verify; device=True checks the queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.batch_eval_verify(proof, roots, points, evals, device=device, stream=_verify_stream(device, stream))


def _batch_args(name: str, ctx: StarkContext, mats, widths, masks, points):
    """(widths uint32[n], masks uint32[n], points uint32[n_points][4], the matrices' device pointers as a C array) of a batched call; ValueError for lists of different
    lengths, a matrix that is not of the context's size, a width its matrix does not have, or points that are not rows of four words"""
    mats = list(mats)
    widths = [m.shape[0] * 8 for m in mats] if widths is None else [int(w) for w in widths]
    masks = [int(k) for k in masks]
    if not (len(mats) == len(widths) == len(masks)):
        raise ValueError(f"{name}: mats, widths and masks must have one entry per matrix")
    if not mats or any(w < 0 for w in widths) or any(k < 0 for k in masks):
        raise ValueError(f"{name}: at least one matrix, and no negative width or mask")
    for m, w in zip(mats, widths):
        _, pts = _eval_args(name, ctx, m, w, points)
    ptrs = (C.c_void_p * max(len(mats), 1))(*[m.data_ptr() for m in mats])
    return np.array(widths, np.uint32), np.array(masks, np.uint32), pts, ptrs


def batch_eval_prove(ctx: StarkContext, mats, trees, widths, masks, points, num_queries: int = 50, pow_bits: int = 12, stream=None, want_stage_ms: bool = False):
    """zkir_batch_eval_prove: ONE evaluation proof (np.uint32 words) opening the 1 .. 4 commitments `trees` (merkle_commit's) to the B8 matrices `mats` (lde's outputs on
    `ctx`; `widths` real columns each, None: all) at the shared `points` ([1 or 2][4] canonical words, E4 elements outside the base field, CHOSEN AFTER THE ROOTS);
    masks[m] bit i: matrix m is opened at point i.  One inverse table, one FRI commit phase, one grind and one set of query rows for all the matrices
    (batch_eval_layout finds the sections).  Tensors of the wrong size raise ValueError; the library refuses bad parameters with ERR_ARGUMENT before any launch.
    want_stage_ms: also the device ms of (weights, evaluations, quotient, FRI commit phase, grinding, query section)."""
    ws, ks, pts, mat_ptrs = _batch_args("batch_eval_prove", ctx, mats, widths, masks, points)
    trees = list(trees)
    if len(trees) != len(ws):
        raise ValueError("batch_eval_prove: trees must have one entry per matrix")
    for tree in trees:
        _check_tree("batch_eval_prove", ctx, tree, "a")
    tree_ptrs = (C.c_void_p * max(len(trees), 1))(*[t.data_ptr() for t in trees])
    cap = batch_eval_proof_words(ctx.log_n, ctx.log_blowup, ws, ks, len(pts), num_queries)
    return _prove_call("zkir_batch_eval_prove", 6, (ctx.handle, len(ws), mat_ptrs, ws.ctypes.data, tree_ptrs, ks.ctypes.data, pts.ctypes.data, len(pts), int(num_queries), int(pow_bits)), cap,
                       stream, want_stage_ms)


def batch_eval_quotient(ctx: StarkContext, mats, gamma, points, evals, widths, masks, stream=None) -> torch.Tensor:
    """(tests, measurements) zkir_batch_eval_quotient_launch: the codeword int32[4][M] of batch_eval_prove's quotient stage for GIVEN canonical gamma (four words), points and
    evaluations (4 words each, in the proof's exponent order: for each point, for each matrix opened at it, for each column): row t = coordinate t of F."""
    ws, ks, pts, mat_ptrs = _batch_args("batch_eval_quotient", ctx, mats, widths, masks, points)
    g = np.ascontiguousarray(gamma, dtype=np.uint32).reshape(4)
    y = np.ascontiguousarray(evals, dtype=np.uint32).reshape(-1)
    if len(y) != 4 * sum(int(w) * bin(int(k) & ((1 << len(pts)) - 1)).count("1") for w, k in zip(ws, ks)):
        raise ValueError("batch_eval_quotient: evals must hold 4 words per selected (point, matrix, column)")
    m = 1 << (ctx.log_n + ctx.log_blowup)
    dev = mats[0].device
    scratch = torch.empty(max(1, int(rt.lib().zkir_batch_eval_quotient_scratch_words(ctx.log_n + ctx.log_blowup, len(ws), ws.ctypes.data, len(pts)))), dtype=torch.int32, device=dev)
    cw = torch.empty((4, m), dtype=torch.int32, device=dev)
    pl._check(rt.lib().zkir_batch_eval_quotient_launch(ctx.handle, len(ws), mat_ptrs, ws.ctypes.data, ks.ctypes.data, g.ctypes.data, pts.ctypes.data, len(pts), y.ctypes.data,
                                                       scratch.data_ptr(), cw.data_ptr(), _sp(stream)))
    return cw


def batch_eval_layout(proof) -> dict:
    """Word offsets of a well-formed batched evaluation proof: the header's fields, widths, masks, shape, roots, points, evals (in the exponent order; evals_of[(i, m)] is where
    y[i][m][0] stands), layer_roots, final, nonce, queries, the words of one query (qsize) and, relative to a query's start, records[m] = (record_m(q), record_m(q + M/2))."""
    log_n, b, n_mats, n_points, nq, _, n_layers = (int(x) for x in proof[2:9])
    widths, masks = [int(x) for x in proof[9:9 + 2 * n_mats:2]], [int(x) for x in proof[10:10 + 2 * n_mats:2]]
    at = {"log_n": log_n, "log_blowup": b, "n_mats": n_mats, "n_points": n_points, "num_queries": nq, "n_layers": n_layers, "widths": widths, "masks": masks, "shape": 9,
          "roots": 9 + 2 * n_mats, "points": 9 + 6 * n_mats, "evals": 9 + 6 * n_mats + 4 * n_points, "evals_of": {}}
    e = 0
    for i in range(n_points):
        for m in range(n_mats):
            if (masks[m] >> i) & 1:
                at["evals_of"][(i, m)] = at["evals"] + 4 * e
                e += widths[m]
    at["n_evals"] = e
    at["layer_roots"] = at["evals"] + 4 * e
    at["final"] = at["layer_roots"] + 4 * n_layers
    at["nonce"] = at["final"] + 4 * (4 << b)
    at["queries"] = at["nonce"] + 1
    at["qsize"] = (len(proof) - at["queries"]) // nq if nq else 0
    rel, at["records"] = 1, []
    for w in widths:
        rec = w + 4 * (log_n + b)
        at["records"].append((rel, rel + rec))
        rel += 2 * rec
    return at


class EvalGroup(NamedTuple):
    """One group of mixed_eval_prove: what batch_eval_prove takes at one height — the group's context, its 1 .. 4 B8 matrices and their trees, widths (None: all columns),
    masks, and its own points ([1 or 2][4] canonical words)."""
    ctx: StarkContext
    mats: Sequence
    trees: Sequence
    widths: Optional[Sequence]
    masks: Sequence
    points: object


mixed_eval_proof_words = rt.mixed_eval_proof_words


def mixed_eval_verify(proof, roots=None, points=None, evals=None, device: bool = False, stream=None) -> int:
    """rt.mixed_eval_verify; device=True checks the queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.mixed_eval_verify(proof, roots, points, evals, device=device, stream=_verify_stream(device, stream))


def mixed_eval_prove(groups, num_queries: int = 50, pow_bits: int = 12, stream=None, want_stage_ms: bool = False):
    """zkir_mixed_eval_prove: ONE evaluation proof (np.uint32 words) opening commitments of DIFFERENT heights: `groups` are 2 or 3 EvalGroups whose contexts share one
    log_blowup and have strictly decreasing log_n; each group is opened as batch_eval_prove opens it, at its own points.  One gamma, one FRI commit phase (a lower group's
    quotient is added to the layer of its size), one grind, one set of query rows (mixed_eval_layout finds the sections).  The workspace is the first group's context's.
    Tensors of the wrong size — a matrix or tree that is not of ITS group's context's size — raise ValueError; the library refuses bad parameters (one group, four groups,
    equal or rising heights, a context of another log_blowup, a group's shape, its points) with ERR_ARGUMENT before any launch.
    want_stage_ms: also the device ms of (weights, evaluations, quotients, FRI commit phase, grinding, query section)."""
    groups = [EvalGroup(*g) for g in groups]
    if not groups:
        raise ValueError("mixed_eval_prove: no group")
    ws, ks, pts, mat_ptrs, tree_ptrs = [], [], [], [], []
    for g in groups:
        w, k, p, _ = _batch_args("mixed_eval_prove", g.ctx, g.mats, g.widths, g.masks, g.points)
        trees = list(g.trees)
        if len(trees) != len(w):
            raise ValueError("mixed_eval_prove: trees must have one entry per matrix")
        for tree in trees:
            _check_tree("mixed_eval_prove", g.ctx, tree, "a")
        ws.append(w); ks.append(k); pts.append(p.reshape(-1))
        mat_ptrs += [m.data_ptr() for m in g.mats]; tree_ptrs += [t.data_ptr() for t in trees]
    shapes = [(w, k, len(p) // 4) for w, k, p in zip(ws, ks, pts)]
    cap = mixed_eval_proof_words([g.ctx.log_n for g in groups], groups[0].ctx.log_blowup, shapes, num_queries)
    ctxs = (C.c_void_p * len(groups))(*[g.ctx.handle for g in groups])
    n_mats, n_points = np.array([len(w) for w in ws], np.uint32), np.array([n for _, _, n in shapes], np.uint32)
    w_all, k_all, p_all = np.concatenate(ws), np.concatenate(ks), np.concatenate(pts)
    mp, tp = (C.c_void_p * len(mat_ptrs))(*mat_ptrs), (C.c_void_p * len(tree_ptrs))(*tree_ptrs)
    return _prove_call("zkir_mixed_eval_prove", 6, (ctxs, len(groups), n_mats.ctypes.data, mp, w_all.ctypes.data, tp, k_all.ctypes.data, p_all.ctypes.data, n_points.ctypes.data,
                                                    int(num_queries), int(pow_bits)), cap, stream, want_stage_ms)


def mixed_eval_layout(proof) -> dict:
    """Word offsets of a well-formed 'ZKMH' proof: log_blowup, n_groups, num_queries, n_layers; groups[h] = {log_n, widths, masks, n_points, roots, points, evals, n_evals,
    evals_of[(i, m)], records[m] (relative to a query's start: (record(q), record(q + M_0/2)) for group 0, (record(q mod M_h),) below)}; roots, points, evals, layer_roots,
    final, nonce, queries and the words of one query (qsize)."""
    b, n_groups, nq, _, n_layers = (int(x) for x in proof[2:7])
    parsed = rt.mixed_eval_groups(proof)
    if parsed is None:
        raise ValueError("mixed_eval_layout: the header is one no 'ZKMH' proof can have")
    at = {"log_blowup": b, "n_groups": n_groups, "num_queries": nq, "n_layers": n_layers, "groups": parsed[0]}
    at["roots"] = parsed[1]
    at["points"] = at["roots"] + 4 * sum(len(g["widths"]) for g in at["groups"])
    at["evals"] = at["points"] + 4 * sum(g["n_points"] for g in at["groups"])
    r_at, p_at, e, rel = at["roots"], at["points"], 0, 1
    for h, g in enumerate(at["groups"]):
        g["roots"], g["points"], g["evals"], g["evals_of"], g["records"] = r_at, p_at, at["evals"] + 4 * e, {}, []
        first = e
        for i in range(g["n_points"]):
            for m, (w, k) in enumerate(zip(g["widths"], g["masks"])):
                if (k >> i) & 1:
                    g["evals_of"][(i, m)] = at["evals"] + 4 * e
                    e += w
        g["n_evals"] = e - first
        for w in g["widths"]:
            rec = w + 4 * (g["log_n"] + b)
            g["records"].append((rel, rel + rec) if h == 0 else (rel,))
            rel += (2 if h == 0 else 1) * rec
        r_at += 4 * len(g["widths"]); p_at += 4 * g["n_points"]
    at["n_evals"] = e
    at["layer_roots"] = at["evals"] + 4 * e
    at["final"] = at["layer_roots"] + 4 * n_layers
    at["nonce"] = at["final"] + 4 * (4 << b)
    at["queries"] = at["nonce"] + 1
    at["qsize"] = (len(proof) - at["queries"]) // nq if nq else 0
    return at


def fri_fold(ctx: StarkContext, layer: torch.Tensor, k: int, beta, addend: Optional[torch.Tensor] = None, stream=None) -> torch.Tensor:
    """(tests, measurements) zkir_fri_fold_launch: the FRI fold kernel alone.  `layer` int32[4][m] (row t = coordinate t, canonical) is a layer of m = 2^log_m values of the
    context's FRI (log_m <= log_n + log_blowup; its coset shift is 31^(2^(log_n + log_blowup - log_m))); it is folded k (1 .. 3) times with the canonical E4 `beta`,
    beta^2, beta^4 into int32[4][m >> k].  addend (int32[4][m >> k] or None) is added by index: the add form mixed_eval_prove uses.  Wrong sizes raise ValueError."""
    if layer.dim() != 2 or layer.shape[0] != 4 or layer.dtype != torch.int32 or not layer.is_contiguous():
        raise ValueError("fri_fold: layer must be contiguous int32[4][m]")
    m = layer.shape[1]
    if m < 2 or m & (m - 1):
        raise ValueError("fri_fold: the layer's size must be a power of two")
    if not 1 <= int(k) <= 3 or m >> int(k) == 0:
        raise ValueError("fri_fold: k must be 1 .. 3 and at most log2 of the layer's size")
    g = m >> int(k)
    if addend is not None and (tuple(addend.shape) != (4, g) or addend.dtype != torch.int32 or not addend.is_contiguous()):
        raise ValueError(f"fri_fold: addend must be contiguous int32[4][{g}]")
    bt = np.ascontiguousarray(beta, dtype=np.uint32).reshape(4)
    out = torch.empty((4, g), dtype=torch.int32, device=layer.device)
    pl._check(rt.lib().zkir_fri_fold_launch(ctx.handle, layer.data_ptr(), m.bit_length() - 1, int(k), bt.ctypes.data, addend.data_ptr() if addend is not None else None, out.data_ptr(),
                                            _sp(stream)))
    return out


def commit_trace(ctx: StarkContext, trace: pl.DeviceTrace, stream=None, deferred: bool = False):
    """main trace -> LDE (at the context's blow-up) -> Merkle.  Returns (root np.uint32[4], lde matrix tensor (B8), tree tensor)."""
    m = main_trace(trace, stream, deferred)
    L = lde(ctx, m, stream, clobber=True)
    tree = merkle_commit(ctx, L, main_width(deferred), stream)
    root = tree[-4:].cpu().numpy().view(np.uint32)
    return root, L, tree


def prove(ctx: StarkContext, trace, pub: rt.PublicInputsC, stream=None, want_stage_ms: bool = False):
    """zkir_prove: full ZKIR-STARK v1 proof of a device trace (`trace`: pl.DeviceTrace or zkir_trace_columns) bound to the public
    inputs `pub` (rt.public_inputs / ExecutionResult.public_inputs).  Returns np.uint32 proof words (and stage ms).  Proofs are blow-up 2: a context of
    log_blowup != 1 is refused by the library (rt.RuntimeError, ERR_ARGUMENT)."""
    cols = trace.c if hasattr(trace, "c") else trace
    out = C.POINTER(C.c_uint32)()
    n_words = C.c_uint64()
    ms = (C.c_float * 9)()
    pl._check(rt.lib().zkir_prove(ctx.handle, C.byref(cols), C.byref(pub), C.byref(out), C.byref(n_words), ms if want_stage_ms else None, _sp(stream)))
    proof = np.ctypeslib.as_array(out, shape=(n_words.value,)).copy()
    rt.lib().zkir_proof_free(out)
    return (proof, list(ms)) if want_stage_ms else proof


verify = rt.verify


def prove_rate(ctx: StarkContext, trace, pub: rt.PublicInputsC, num_queries: Optional[int] = None, pow_bits: int = 12, stream=None, want_stage_ms: bool = False):
    """zkir_prove_rate: a ZKIR-STARK proof of a whole run in mode 0, 1 or 2 at the CONTEXT's rate (log_blowup 1, 2 or 3), in the 'ZKSR' format: the sections of a prove()
    proof through the quotient root, then one batch evaluation proof ('ZKBE') of the main, aux and quotient commitments at [zeta, zeta w] (rate_proof_layout finds both).
    num_queries None: 50 / 25 / 17 by log_blowup; `pub.fri_params` is not consulted.  Returns np.uint32 proof words (and the device ms of its eleven stages: prove()'s first
    five, then batch_eval_prove's six)."""
    cols = trace.c if hasattr(trace, "c") else trace
    nq = rt.RATE_DEFAULT_QUERIES.get(ctx.log_blowup, 50) if num_queries is None else int(num_queries)
    out = C.POINTER(C.c_uint32)()
    n_words = C.c_uint64()
    ms = (C.c_float * 11)()
    pl._check(rt.lib().zkir_prove_rate(ctx.handle, C.byref(cols), C.byref(pub), nq, int(pow_bits), C.byref(out), C.byref(n_words), ms if want_stage_ms else None, _sp(stream)))
    proof = np.ctypeslib.as_array(out, shape=(n_words.value,)).copy()
    rt.lib().zkir_proof_free(out)
    return (proof, list(ms)) if want_stage_ms else proof


def prove_rate_modes(ctx: StarkContext, trace, pub: rt.PublicInputsC, num_queries: Optional[int] = None, pow_bits: int = 12, stream=None, want_stage_ms: bool = False):
    """zkir_prove_rate_modes: prove_rate with modes 0 - 4 admitted.  Modes 0 - 2 give prove_rate's words; in modes 3 / 4 `pub` is what prove() takes there (no witness: the
    memory witness, and a hash run's tape, are made on the device; or the host witness of rt.memcheck_witness; mode 4: the tapes), with prove()'s refusals.  The proof is a
    'ZKSR' proof with the mode in word 9; rt.verify_rate checks it, rate_proof_layout and rate_last_matrices read it."""
    cols = trace.c if hasattr(trace, "c") else trace
    nq = rt.RATE_DEFAULT_QUERIES.get(ctx.log_blowup, 50) if num_queries is None else int(num_queries)
    out = C.POINTER(C.c_uint32)()
    n_words = C.c_uint64()
    ms = (C.c_float * 11)()
    pl._check(rt.lib().zkir_prove_rate_modes(ctx.handle, C.byref(cols), C.byref(pub), nq, int(pow_bits), C.byref(out), C.byref(n_words), ms if want_stage_ms else None, _sp(stream)))
    proof = np.ctypeslib.as_array(out, shape=(n_words.value,)).copy()
    rt.lib().zkir_proof_free(out)
    return (proof, list(ms)) if want_stage_ms else proof


def prove_rate_segment(ctx: StarkContext, trace, pub: rt.PublicInputsC, num_queries: Optional[int] = None, pow_bits: int = 12, stream=None, want_stage_ms: bool = False):
    """zkir_prove_rate_segment: prove_rate for a SEGMENT of a run — `trace` is the device trace of a row shard (rt.exec_shard on log.shard(a, e)), `pub` the shard's public
    inputs (n_real = its rows; mode 2: the whole run's tapes with writes_before / reads_before) — or for a whole run, whose words are prove_rate's.  Modes 0, 1, 2; the
    'ZKSR' format; rt.verify_rate_segment / rt.verify_rate_chain check such proofs."""
    cols = trace.c if hasattr(trace, "c") else trace
    nq = rt.RATE_DEFAULT_QUERIES.get(ctx.log_blowup, 50) if num_queries is None else int(num_queries)
    out = C.POINTER(C.c_uint32)()
    n_words = C.c_uint64()
    ms = (C.c_float * 11)()
    pl._check(rt.lib().zkir_prove_rate_segment(ctx.handle, C.byref(cols), C.byref(pub), nq, int(pow_bits), C.byref(out), C.byref(n_words), ms if want_stage_ms else None, _sp(stream)))
    proof = np.ctypeslib.as_array(out, shape=(n_words.value,)).copy()
    rt.lib().zkir_proof_free(out)
    return (proof, list(ms)) if want_stage_ms else proof


def rate_proof_layout(proof) -> dict:
    """Word offsets inside a 'ZKSR' proof of any mode: proof_layout's sections of the STARK part (header .. quotient_root; modes 3 / 4: the touched cells, the tapes), the header's log_blowup, num_queries and pow_bits, and
    `eval_proof`: where the embedded 'ZKBE' proof starts (it runs to the end; batch_eval_layout reads it)."""
    at = proof_layout(proof)
    at["log_n"], at["log_blowup"] = int(proof[2]), int(proof[5])
    at["eval_proof"] = at.pop("openings")
    return at


def rate_last_matrices(ctx: StarkContext):
    """(tests, measurements) zkir_prove_rate_last_matrices: the main, aux and quotient LDE matrices (np.uint32 [blocks][M][8], canonical words) of the context's last
    prove_rate proof, copied out of its workspace; raises once another proof has used the context."""
    widths = (C.c_uint32 * 3)()
    rows = C.c_uint64()
    pl._check(rt.lib().zkir_prove_rate_last_matrices(ctx.handle, None, None, None, widths, C.byref(rows)))
    mats = [np.empty(((int(w) + 7) // 8, rows.value, 8), dtype=np.uint32) for w in widths]
    pl._check(rt.lib().zkir_prove_rate_last_matrices(ctx.handle, mats[0].ctypes.data, mats[1].ctypes.data, mats[2].ctypes.data, widths, C.byref(rows)))
    return mats


def verify_rate(proof, expect=None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None) -> int:
    """rt.verify_rate; device=True checks the embedded proof's queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.verify_rate(proof, expect, min_queries, min_pow_bits, device=device, stream=_verify_stream(device, stream))


def verify_rate_segment(proof, expect=None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None):
    """rt.verify_rate_segment; device=True checks the embedded proof's queries on the GPU, on the torch stream `stream` (default: the current one) — the same verdict."""
    return rt.verify_rate_segment(proof, expect, min_queries, min_pow_bits, device=device, stream=_verify_stream(device, stream))


def verify_rate_chain(proofs, expect=None, min_queries: int = 1, min_pow_bits: int = 0, device: bool = False, stream=None) -> int:
    """rt.verify_rate_chain; device=True checks all the segments' queries as one batch on the GPU, on the torch stream `stream` (default: the current one)."""
    return rt.verify_rate_chain(proofs, expect, min_queries, min_pow_bits, device=device, stream=_verify_stream(device, stream))


def verify_rate_many(proofs, expects=None, min_queries=None, min_pow_bits=None, stream=None):
    """rt.verify_rate_many on the torch stream `stream` (default: the current one)."""
    return rt.verify_rate_many(proofs, expects, min_queries, min_pow_bits, stream=_verify_stream(True, stream))


def pcs_verify_many(kinds, proofs, roots=None, points=None, evals=None, stream=None):
    """rt.pcs_verify_many on the torch stream `stream` (default: the current one)."""
    return rt.pcs_verify_many(kinds, proofs, roots, points, evals, stream=_verify_stream(True, stream))

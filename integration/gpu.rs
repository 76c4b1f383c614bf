//! zkir-runtime/src/gpu.rs — `VM::new(program, inputs, config).run()` on an MI355X through the C ABI of include/zkir_amd.h.
//!
//! NOT COMPILED IN THIS REPOSITORY: the build image has no Rust toolchain (no rustc / cargo; the workspace's crates.io dependencies cannot be fetched).
//! It is the module a maintainer of seceq/zkir adds (`#[cfg(feature = "gpu")] pub mod gpu;` in zkir-runtime/src/lib.rs, build.rs next to it); every call
//! below is exercised from C++ by tests/cpp/reference_tests.cpp and from Python by zkir_amd/runtime.py.  Reference seam: zkir-runtime/src/vm.rs:138 (VM::new),
//! :208 (VM::run), :54-103 (ExecutionResult); error kinds zkir-runtime/src/error.rs:7-37.
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};

use zkir_spec::Program;

use crate::error::RuntimeError;
use crate::vm::{HaltReason, VMConfig};

#[repr(C)]
pub struct ZkirVmConfig {
    pub max_cycles: u64,
    pub trace: u8,
    pub enable_range_checking: u8,
    pub enable_execution_trace: u8,
    pub enable_deferred_model: u8,
}

/// Device pointers (HBM), struct of arrays, 372 B per row (include/zkir_amd.h: zkir_trace_columns).
#[repr(C)]
pub struct ZkirTraceColumns {
    pub cycle: *mut u64,
    pub pc: *mut u64,
    pub instruction: *mut u32,
    pub registers: *mut u64,
    pub bound_bits: *mut u32,
    pub bound_tag: *mut u8,
    pub bound_payload: *mut u64,
    pub reg_state: *mut u8,
    pub reg_stride: u64,
}

#[repr(C)]
pub struct ZkirPublicInputs {
    pub n_real: u64,
    pub entry_point: u64,
    pub deferred: u32,
    pub fri_params: u32,   // num_queries | pow_bits << 16, 0 = the defaults (zkir_public_inputs_set_params)
    pub program_digest: [u32; 4],
    pub io_digest: [u32; 4],
    pub program_blob: *const u8, // borrowed: must outlive zkir_prove
    pub program_blob_len: u64,
    // mode 2 (deferred == 2: + the I/O argument): the tapes and the halt reason in the clear (borrowed; zkir_public_inputs_of fills them)
    pub inputs: *const u64,
    pub n_inputs: u64,
    pub outputs: *const u64,
    pub n_outputs: u64,
    pub halt_kind: u32,
    pub reserved2: u32,
    pub halt_code: u64,
    pub writes_before: u64,
    pub reads_before: u64,
    // mode 3 (deferred == 3: + the memory argument): the run's memory witness (borrowed; zkir_public_inputs_set_memory points them at a ZkirMemcheckWitness)
    pub mem_old: *const u64,
    pub mem_told: *const u32,
    pub cell_addr: *const u64,
    pub cell_bytes: *const u64,
    pub cell_time: *const u32,
    pub n_cells: u64,
    // mode 4 (round 6): the hash calls of the run as the proof's hash section — borrowed from a zkir_memcheck_witness made with zkir_memcheck_witness_of_mode(.., 4, ..)
    pub hash_section: *const u32,
    pub hash_section_words: u64,
    // (ABI 7) what the run's hash syscalls wrote: 40-byte records (row u32, reserved u32, 32 bytes) borrowed from the run's delta log — zkir_public_inputs_of sets them;
    // with no witness set, zkir_prove builds the mode-4 memory witness and the hash tape on the device from them
    pub hash_outs: *const u8,
    pub n_hash_outs: u64,
}
pub enum ZkirMemcheckWitness {}

pub enum ZkirResult {}
pub enum ZkirDeltaLog {}
pub enum ZkirStarkCtx {}

extern "C" {
    fn zkir_exec(blob: *const u8, len: usize, inputs: *const u64, n_inputs: usize, cfg: *const ZkirVmConfig, out: *mut *mut ZkirResult) -> c_int;
    fn zkir_result_free(r: *mut ZkirResult);
    fn zkir_result_delta_log(r: *const ZkirResult) -> *const ZkirDeltaLog;
    fn zkir_result_trace(r: *const ZkirResult) -> *const ZkirTraceColumns;
    fn zkir_result_copy_column(r: *const ZkirResult, field: c_int, reg: c_int, dst: *mut c_void) -> c_int;
    fn zkir_delta_log_cycles(l: *const ZkirDeltaLog) -> u64;
    fn zkir_delta_log_halt_kind(l: *const ZkirDeltaLog) -> c_int;
    fn zkir_delta_log_halt_code(l: *const ZkirDeltaLog) -> u64;
    fn zkir_delta_log_n_outputs(l: *const ZkirDeltaLog) -> usize;
    fn zkir_delta_log_outputs(l: *const ZkirDeltaLog) -> *const u64;
    fn zkir_last_error() -> *const c_char;
    // proving (self-defined stages: the reference has none — DESIGN.md §8)
    fn zkir_stark_ctx_create(log_n: u32, log_blowup: u32, out: *mut *mut ZkirStarkCtx) -> c_int;
    fn zkir_stark_ctx_log_blowup(ctx: *const ZkirStarkCtx) -> u32;
    fn zkir_stark_ctx_free(ctx: *mut ZkirStarkCtx);
    fn zkir_padded_log_n(n_real: u64) -> u32;
    fn zkir_public_inputs_of(log: *const ZkirDeltaLog, blob: *const u8, len: usize, inputs: *const u64, n_inputs: usize, deferred: u32, out: *mut ZkirPublicInputs) -> c_int;
    fn zkir_memcheck_witness_of(log: *const ZkirDeltaLog, blob: *const u8, len: usize, out: *mut *mut ZkirMemcheckWitness) -> c_int;   // mode 3: the host's sequential memory replay
    fn zkir_memcheck_witness_free(w: *mut ZkirMemcheckWitness);
    fn zkir_public_inputs_set_memory(public: *mut ZkirPublicInputs, w: *const ZkirMemcheckWitness);                                      // sets deferred = 3
    fn zkir_prove(ctx: *const ZkirStarkCtx, trace: *const ZkirTraceColumns, public: *const ZkirPublicInputs, proof: *mut *mut u32, words: *mut u64, stage_ms: *mut f32,
                  stream: *mut c_void) -> c_int;
    fn zkir_verify(proof: *const u32, words: u64, expect: *const ZkirPublicInputs) -> c_int;
    fn zkir_proof_free(proof: *mut u32);
    // prove(result, params) -> proof bytes (the handle of zkir_exec keeps the program and the input tape)
    fn zkir_prove_result(result: *const ZkirResult, params: *const ZkirProverParams, proof: *mut *mut u8, len: *mut usize) -> c_int;
    fn zkir_proof_bytes_free(proof: *mut u8);
    // proofs at the context's own rate ('ZKSR': log_blowup 1, 2, 3), every mode; the drop-in call makes its own context of that rate
    pub fn zkir_prove_rate_modes(ctx: *mut ZkirStarkCtx, trace: *const ZkirTraceColumns, public: *const ZkirPublicInputs, num_queries: u32, pow_bits: u32, proof: *mut *mut u32,
                                 words: *mut u64, stage_ms: *mut f32, stream: *mut c_void) -> c_int;
    pub fn zkir_prove_result_rate(result: *const ZkirResult, params: *const ZkirProverParams, log_blowup: u32, proof: *mut *mut u8, len: *mut usize) -> c_int;
    pub fn zkir_verify_rate(proof: *const u32, words: u64, expect: *const ZkirPublicInputs, min_queries: u32, min_pow_bits: u32) -> c_int;
    pub fn zkir_verify_rate_device(proof: *const u32, words: u64, expect: *const ZkirPublicInputs, min_queries: u32, min_pow_bits: u32, stream: *mut c_void) -> c_int;
    fn zkir_abi_version() -> u32;
    // openings of a commitment (rows of a committed B8 matrix + their Merkle paths) and their check: device pointers throughout, _host takes host pointers and needs no device
    pub fn zkir_merkle_opening_words(width: u32, n_leaves: u64, flags: u32) -> u64;
    pub fn zkir_merkle_open_launch(ctx: *const ZkirStarkCtx, mat: *const u32, width: u32, n_leaves: u64, tree: *const u32, indices: *const u64, n_idx: u64, out: *mut u32,
                                   stream: *mut c_void) -> c_int;
    pub fn zkir_merkle_verify_launch(ctx: *const ZkirStarkCtx, root: *const u32, width: u32, n_leaves: u64, indices: *const u64, n_idx: u64, openings: *const u32, flags: u32,
                                     verdicts: *mut u32, summary: *mut u32, stream: *mut c_void) -> c_int;
    pub fn zkir_merkle_verify_host(root: *const u32, width: u32, n_leaves: u64, indices: *const u64, n_idx: u64, openings: *const u32, flags: u32, verdicts: *mut u32,
                                   summary: *mut u32) -> c_int;
    // a low-degree proof of a commitment at the context's rate (log_blowup 1, 2, 3), and its host verifier
    pub fn zkir_lowdeg_proof_words(log_n: u32, log_blowup: u32, width: u32, num_queries: u32) -> u64;
    pub fn zkir_lowdeg_prove(ctx: *mut ZkirStarkCtx, lde_mat: *const u32, width: u32, tree: *const u32, num_queries: u32, pow_bits: u32, proof_host: *mut u32, cap_words: u64,
                             n_words: *mut u64, stream: *mut c_void) -> c_int;
    pub fn zkir_lowdeg_verify(proof: *const u32, n_words: u64, expect_root: *const u32) -> c_int;
    // an evaluation proof of a commitment at 1 or 2 points of E4 chosen AFTER the root (points: 4 n_points canonical words, host), and its host verifier
    // (expect_* null = any; expect_points holds 4 proof[5] words, expect_evals 4 proof[5] proof[4] words)
    pub fn zkir_eval_proof_words(log_n: u32, log_blowup: u32, width: u32, n_points: u32, num_queries: u32) -> u64;
    pub fn zkir_eval_prove(ctx: *mut ZkirStarkCtx, lde_mat: *const u32, width: u32, tree: *const u32, points: *const u32, n_points: u32, num_queries: u32, pow_bits: u32,
                           proof_host: *mut u32, cap_words: u64, n_words: *mut u64, stream: *mut c_void) -> c_int;
    pub fn zkir_eval_verify(proof: *const u32, n_words: u64, expect_root: *const u32, expect_points: *const u32, expect_evals: *const u32) -> c_int;
    // a batched evaluation proof: 1 .. 4 commitments of ONE context opened in one proof at a shared list of 1 or 2 points; masks[m] bit i = matrix m is opened at point i.
    // lde_mats / trees / widths / masks are host arrays of n_mats entries (the matrices and trees they name: device pointers); the verifier is host only, zkir_eval_verify's codes
    // (expect_* null = any; read at the sizes the proof's header states: 4 n_mats root words, 4 n_points point words, the proof's evaluation words)
    pub fn zkir_batch_eval_proof_words(log_n: u32, log_blowup: u32, n_mats: u32, widths: *const u32, masks: *const u32, n_points: u32, num_queries: u32) -> u64;
    pub fn zkir_batch_eval_prove(ctx: *mut ZkirStarkCtx, n_mats: u32, lde_mats: *const *const u32, widths: *const u32, trees: *const *const u32, masks: *const u32, points: *const u32,
                                 n_points: u32, num_queries: u32, pow_bits: u32, proof_host: *mut u32, cap_words: u64, n_words: *mut u64, stream: *mut c_void) -> c_int;
    pub fn zkir_batch_eval_verify(proof: *const u32, n_words: u64, expect_roots: *const u32, expect_points: *const u32, expect_evals: *const u32) -> c_int;
    // an evaluation proof over SEVERAL HEIGHTS at one log_blowup ('ZKMH'): n_groups (2 or 3) groups of strictly decreasing log_n, each what zkir_batch_eval_prove takes at its
    // own height with its own points.  Flat host arrays, groups concatenated: ctxs / n_mats / n_points / log_ns have n_groups entries, lde_mats / trees / widths / masks one per
    // matrix, points 4 words per point.  The workspace and the lock are ctxs[0]'s.  The verifier is host only (no device form): zkir_batch_eval_verify's codes, expect_* read at
    // the sizes the proof's header states (all roots, all points, all evaluations, in the proof's order)
    pub fn zkir_mixed_eval_proof_words(log_blowup: u32, n_groups: u32, log_ns: *const u32, n_mats: *const u32, n_points: *const u32, widths: *const u32, masks: *const u32,
                                       num_queries: u32) -> u64;
    pub fn zkir_mixed_eval_prove(ctxs: *const *mut ZkirStarkCtx, n_groups: u32, n_mats: *const u32, lde_mats: *const *const u32, widths: *const u32, trees: *const *const u32,
                                 masks: *const u32, points: *const u32, n_points: *const u32, num_queries: u32, pow_bits: u32, proof_host: *mut u32, cap_words: u64,
                                 n_words: *mut u64, stream: *mut c_void) -> c_int;
    pub fn zkir_mixed_eval_verify(proof: *const u32, n_words: u64, expect_roots: *const u32, expect_points: *const u32, expect_evals: *const u32) -> c_int;
    // the four verifiers above with checks 7 - 11 of all queries on the current HIP device (proof and expectations: host memory; no context): the host entry's verdict for
    // every input; a negative result is a device failure (-ZKIR_ERR_DEVICE) or no host memory (-ZKIR_ERR_OTHER), not a verdict
    pub fn zkir_lowdeg_verify_device(proof: *const u32, n_words: u64, expect_root: *const u32, stream: *mut c_void) -> c_int;
    pub fn zkir_eval_verify_device(proof: *const u32, n_words: u64, expect_root: *const u32, expect_points: *const u32, expect_evals: *const u32, stream: *mut c_void) -> c_int;
    pub fn zkir_batch_eval_verify_device(proof: *const u32, n_words: u64, expect_roots: *const u32, expect_points: *const u32, expect_evals: *const u32, stream: *mut c_void) -> c_int;
    pub fn zkir_mixed_eval_verify_device(proof: *const u32, n_words: u64, expect_roots: *const u32, expect_points: *const u32, expect_evals: *const u32, stream: *mut c_void) -> c_int;
    // (mode 4) the tapes' share of the lookup table side and the hash tape's record checks as calls of their own (host arrays in, host arrays out)
    pub fn zkir_tape_table_side_launch(hash_words: *const u32, n_hash_words: u64, new_bytes: *const u64, wide_words: *const u32, n_wide_words: u64, alpha: *const u32, lambda: *const u32,
                                       sum: *mut u32, hh: *mut u32, ww: *mut u32, stream: *mut c_void) -> c_int;
    pub fn zkir_tape_table_side_host(hash_words: *const u32, n_hash_words: u64, new_bytes: *const u64, wide_words: *const u32, n_wide_words: u64, alpha: *const u32, lambda: *const u32,
                                     sum: *mut u32, hh: *mut u32, ww: *mut u32) -> c_int;
    pub fn zkir_hash_tape_check_launch(hash_words: *const u32, n_hash_words: u64, n_real: u64, code_end: u64, code: *mut c_int, stream: *mut c_void) -> c_int;
    pub fn zkir_hash_tape_check_host(hash_words: *const u32, n_hash_words: u64, n_real: u64, code_end: u64, code: *mut c_int) -> c_int;
    // (mode 4) what every hash call of a section wrote, recomputed from the tape alone (new_bytes: one entry per touched cell), and the verifier that runs its tape stages on the GPU:
    // the same verdict as zkir_verify; a negative result is a device failure, not a verdict
    pub fn zkir_hash_tape_new_bytes_launch(hash_words: *const u32, n_hash_words: u64, new_bytes: *mut u64, stream: *mut c_void) -> c_int;
    pub fn zkir_hash_tape_new_bytes_host(hash_words: *const u32, n_hash_words: u64, new_bytes: *mut u64) -> c_int;
    pub fn zkir_verify_device(proof: *const u32, words: u64, expect: *const ZkirPublicInputs, stream: *mut c_void) -> c_int;
    // diagnostics: the host clocks (ms: parsing, section digests, hash table side, wide table side, rest) of this thread's last zkir_verify* call and how many stages ran on the GPU
    pub fn zkir_verify_last_stages(ms: *mut f64, device_stages: *mut u32) -> c_int;
}

/// zkir_prover_params: the proof's mode (0 default VM mode, 1 deferred model, 2 + the I/O argument, 3 + the memory argument) and its FRI parameters
/// (0 = the defaults: 50 queries, 12 grinding bits; accepted 50..128 / 12..24).  They are header words of the proof: a verifier's `expect` must name the same.
#[repr(C)]
#[derive(Clone, Copy, Default)]
pub struct ZkirProverParams { pub mode: u32, pub num_queries: u32, pub pow_bits: u32 }
pub const ZKIR_AMD_ABI_VERSION: u32 = 7;

/// include/zkir_amd.h return codes <-> RuntimeError (error.rs:7-37); the message text is the reference's own.
fn map_error(code: c_int) -> RuntimeError {
    let msg = unsafe { CStr::from_ptr(zkir_last_error()) }.to_string_lossy().into_owned();
    match code {
        // 1 MisalignedAccess / 2 InvalidMemoryAccess / 3 DivisionByZero / 4 InvalidSyscall carry their fields in the message; a maintainer who wants the
        // structured variants parses them back or extends the ABI with zkir_last_error_fields() — the kinds are distinct codes already
        5 | 6 | 7 | 8 => RuntimeError::Other(msg),
        _ => RuntimeError::Other(format!("zkir_amd error {code}: {msg}")),
    }
}

/// `ExecutionResult` with the execution trace left in HBM (vm.rs:54-103).
pub struct GpuExecutionResult {
    handle: *mut ZkirResult,
    blob: Vec<u8>,
    inputs: Vec<u64>,
    deferred: bool,
}

impl GpuExecutionResult {
    fn log(&self) -> *const ZkirDeltaLog { unsafe { zkir_result_delta_log(self.handle) } }
    pub fn cycles(&self) -> u64 { unsafe { zkir_delta_log_cycles(self.log()) } }
    pub fn outputs(&self) -> Vec<u64> {
        unsafe { std::slice::from_raw_parts(zkir_delta_log_outputs(self.log()), zkir_delta_log_n_outputs(self.log())) }.to_vec()
    }
    pub fn halt_reason(&self) -> HaltReason {
        match unsafe { zkir_delta_log_halt_kind(self.log()) } {
            0 => HaltReason::Ebreak,
            1 => HaltReason::Exit(unsafe { zkir_delta_log_halt_code(self.log()) }),
            _ => HaltReason::CycleLimit,
        }
    }
    /// Device-resident columns for a prover that links HIP itself.
    pub fn trace_columns(&self) -> &ZkirTraceColumns { unsafe { &*zkir_result_trace(self.handle) } }
    /// One column copied to the host (field ids: include/zkir_amd.h ZKIR_FIELD_*): rebuilding `Vec<TraceRow>` for tests.
    pub fn copy_column_u64(&self, field: c_int, reg: c_int) -> Result<Vec<u64>, RuntimeError> {
        let mut v = vec![0u64; self.cycles() as usize];
        let rc = unsafe { zkir_result_copy_column(self.handle, field, reg, v.as_mut_ptr() as *mut c_void) };
        if rc != 0 { Err(map_error(rc)) } else { Ok(v) }
    }
    /// `zkir_runtime::prove(&result, &params)` as SURVEY 8(b) writes it: the proof bytes of the whole run behind this handle.
    pub fn prove_with(&self, params: &ZkirProverParams) -> Result<Vec<u8>, RuntimeError> {
        assert_eq!(unsafe { zkir_abi_version() }, ZKIR_AMD_ABI_VERSION, "libzkir_amd.so was built from another revision of include/zkir_amd.h");
        let (mut proof, mut len) = (std::ptr::null_mut::<u8>(), 0usize);
        let rc = unsafe { zkir_prove_result(self.handle, params, &mut proof, &mut len) };
        if rc != 0 { return Err(map_error(rc)); }
        let out = unsafe { std::slice::from_raw_parts(proof, len) }.to_vec();
        unsafe { zkir_proof_bytes_free(proof) };
        Ok(out)
    }
    /// `prove()` of north_star: the proof words (u32 little-endian, format zkir_proof_version()) and the public inputs it is bound to.
    /// Mode 0 (default VM mode) or 1 (the deferred model), as the run was configured.
    pub fn prove(&self) -> Result<(Vec<u32>, ZkirPublicInputs), RuntimeError> { self.prove_mode(self.deferred as u32) }
    /// mode 2 = the default VM mode + the I/O argument (the proof says what was read and written), 3 = mode 2 + the memory argument (loads / stores constrained,
    /// memory consistent; whole runs only; refused for runs that execute a hash syscall or touch an address of 2^40 or more)
    pub fn prove_mode(&self, mode: u32) -> Result<(Vec<u32>, ZkirPublicInputs), RuntimeError> {
        let mut public = std::mem::MaybeUninit::<ZkirPublicInputs>::uninit();
        let rc = unsafe { zkir_public_inputs_of(self.log(), self.blob.as_ptr(), self.blob.len(), self.inputs.as_ptr(), self.inputs.len(), mode, public.as_mut_ptr()) };
        if rc != 0 { return Err(map_error(rc)); }
        let mut public = unsafe { public.assume_init() };
        let mut witness: *mut ZkirMemcheckWitness = std::ptr::null_mut();
        if mode == 3 {
            let rc = unsafe { zkir_memcheck_witness_of(self.log(), self.blob.as_ptr(), self.blob.len(), &mut witness) };
            if rc != 0 { return Err(map_error(rc)); }
            unsafe { zkir_public_inputs_set_memory(&mut public, witness) };
        }
        struct FreeWitness(*mut ZkirMemcheckWitness);
        impl Drop for FreeWitness { fn drop(&mut self) { if !self.0.is_null() { unsafe { zkir_memcheck_witness_free(self.0) } } } }
        let _free = FreeWitness(witness);                     // the borrowed mode-3 pointers are only read by zkir_prove below
        let mut ctx: *mut ZkirStarkCtx = std::ptr::null_mut();
        let rc = unsafe { zkir_stark_ctx_create(zkir_padded_log_n(public.n_real), 1, &mut ctx) };
        if rc != 0 { return Err(map_error(rc)); }
        let (mut proof, mut words) = (std::ptr::null_mut::<u32>(), 0u64);
        let rc = unsafe { zkir_prove(ctx, zkir_result_trace(self.handle), &public, &mut proof, &mut words, std::ptr::null_mut(), std::ptr::null_mut()) };
        unsafe { zkir_stark_ctx_free(ctx) };
        if rc != 0 { return Err(map_error(rc)); }
        let out = unsafe { std::slice::from_raw_parts(proof, words as usize) }.to_vec();
        unsafe { zkir_proof_free(proof) };
        // the returned struct is what a verifier's `expect` needs (row count, mode, entry point, digests); the prover-side borrowed pointers end with this call
        public.mem_old = std::ptr::null(); public.mem_told = std::ptr::null(); public.cell_addr = std::ptr::null(); public.cell_bytes = std::ptr::null();
        public.cell_time = std::ptr::null(); public.n_cells = 0; public.hash_section = std::ptr::null(); public.hash_section_words = 0;
        Ok((out, public))
    }
}

impl Drop for GpuExecutionResult {
    fn drop(&mut self) { unsafe { zkir_result_free(self.handle) } }
}

/// Host-only check of a proof against the public inputs the caller expects (0 = accepted).
pub fn verify(proof: &[u32], expect: &ZkirPublicInputs) -> bool { unsafe { zkir_verify(proof.as_ptr(), proof.len() as u64, expect) == 0 } }

/// Drop-in for `VM::new(program, inputs, config).run()` (vm.rs:138, :208).  A debug-format program is reported as an error (code 7), not a panic (vm.rs:141-147).
pub fn run_on_gpu(program: &Program, inputs: &[u64], config: &VMConfig) -> Result<GpuExecutionResult, RuntimeError> {
    let blob = program.to_bytes(); // zkir-spec/src/program.rs:300-315
    let cfg = ZkirVmConfig {
        max_cycles: config.max_cycles,
        trace: 0,
        enable_range_checking: config.enable_range_checking as u8,
        enable_execution_trace: config.enable_execution_trace as u8,
        enable_deferred_model: config.enable_deferred_model as u8,
    };
    let mut res: *mut ZkirResult = std::ptr::null_mut();
    let rc = unsafe { zkir_exec(blob.as_ptr(), blob.len(), inputs.as_ptr(), inputs.len(), &cfg, &mut res) };
    if rc != 0 { return Err(map_error(rc)); }
    Ok(GpuExecutionResult { handle: res, blob, inputs: inputs.to_vec(), deferred: config.enable_deferred_model })
}

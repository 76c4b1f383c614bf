/* zkir_amd.h — C ABI of the MI355X-native ZKIR v3.4 execution-trace path.
 *
 * The reference (seceq/zkir) has NO FFI/plugin boundary: its only seam is the Rust API
 *     VM::new(program, inputs, config) -> VM          zkir-runtime/src/vm.rs:138
 *     VM::run(self) -> Result<ExecutionResult>        zkir-runtime/src/vm.rs:208
 *     ExecutionResult::get_memory_trace()             zkir-runtime/src/vm.rs:85-94
 * so this header defines the boundary a thin Rust shim would bind to replace that
 * path.  Plain pointers and sizes only; no C++ or torch types.
 *
 * Two layers:
 *   1. zkir_exec / zkir_result_*  — drop-in for VM::new + VM::run: host interpreter -> delta log ->
 *      HIP kernels that materialise the wide SoA trace in HBM.
 *   2. zkir_interpret / zkir_*_launch — the same stages individually (host delta log; device kernels
 *      on caller-owned device buffers and a caller-chosen HIP stream), used by bench.py and by
 *      multi-GPU row sharding.
 *
 * Error codes mirror RuntimeError (zkir-runtime/src/error.rs:7-37) + program validation
 * (zkir-spec/src/program.rs:147-167).  The message of the last failure on the calling thread is
 * returned by zkir_last_error().
 */
#ifndef ZKIR_AMD_H
#define ZKIR_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes --------------------------------------------------------------------------- */
enum {
  ZKIR_OK = 0,
  ZKIR_ERR_MISALIGNED = 1,      /* RuntimeError::MisalignedAccess      error.rs:15 */
  ZKIR_ERR_INVALID_MEMORY = 2,  /* RuntimeError::InvalidMemoryAccess   error.rs:18 */
  ZKIR_ERR_DIV_ZERO = 3,        /* RuntimeError::DivisionByZero        error.rs:21 */
  ZKIR_ERR_INVALID_SYSCALL = 4, /* RuntimeError::InvalidSyscall        error.rs:24 */
  ZKIR_ERR_DECODE = 5,          /* RuntimeError::Other("Decode error") vm.rs:376   */
  ZKIR_ERR_OTHER = 6,           /* RuntimeError::Other                 error.rs:36 */
  ZKIR_ERR_BAD_PROGRAM = 7,     /* ZkIrError header/size validation program.rs:147-167,318-346; debug-format
                                   programs (vm.rs:141-147 panics) are reported here instead of aborting */
  ZKIR_ERR_DEVICE = 8,          /* HIP failure / no device: the product path never falls back to the CPU */
  ZKIR_ERR_ARGUMENT = 9
};

/* HaltReason, zkir-runtime/src/state.rs:8-15 */
enum { ZKIR_HALT_EBREAK = 0, ZKIR_HALT_EXIT = 1, ZKIR_HALT_CYCLE_LIMIT = 2 };

/* BoundSource tag, zkir-spec/src/bound.rs:82-93 (declaration order); payload meaning per tag */
enum {
  ZKIR_BOUND_PROGRAM_WIDTH = 0, /* payload 0 */
  ZKIR_BOUND_TYPE_WIDTH = 1,    /* payload = bits */
  ZKIR_BOUND_CRYPTO_OUTPUT = 2, /* payload = CryptoType: 0 Sha256, 1 Keccak256, 2 Poseidon2, 3 Blake3 (bound.rs:10-19) */
  ZKIR_BOUND_COMPUTED = 3,      /* payload 0 */
  ZKIR_BOUND_CONSTANT = 4       /* payload = the constant */
};

/* VMConfig, zkir-runtime/src/vm.rs:15-50 (defaults: 1_000_000, false, false, false, false) */
typedef struct zkir_vm_config {
  uint64_t max_cycles;
  uint8_t trace;                  /* per-cycle eprintln; ignored */
  uint8_t enable_range_checking;
  uint8_t enable_execution_trace;
  uint8_t enable_deferred_model;
} zkir_vm_config;

/* ---- delta log (host memory): what the sequential interpreter hands to the GPU ---------------- */

/* One register write: the full (value, bound, storage-state) triple of register `reg`, visible in the
 * pre-state of every row >= vis (TraceRow holds the state BEFORE its instruction, vm.rs:245-253).
 * Events are ordered by vis; there is at most one event per (reg, vis).  The first 16 events are the
 * initial snapshot (event r describes register r, vis = 0), so every register always has a writer. */
typedef struct zkir_reg_event {
  uint64_t value;     /* VMState.regs[reg] raw u64 (un-masked, state.rs:87-91) */
  uint64_t payload;   /* BoundSource payload */
  uint32_t max_bits;  /* ValueBound.max_bits */
  uint32_t vis;       /* shard-relative row index from which the write is visible (= cycle + 1) */
  uint8_t reg;        /* 0..15 */
  uint8_t state;      /* RegisterState: 0 Normalized, 1 Accumulated (trace.rs:11-17) */
  uint8_t tag;        /* ZKIR_BOUND_* */
  uint8_t pad[5];
} zkir_reg_event;     /* 32 bytes */

/* One architectural data-memory access (MemoryOp, trace.rs:149-167); bound is always
 * TypeWidth(8*width) (memory.rs:245) and is re-derived on the device. */
typedef struct zkir_mem_event {
  uint64_t address;
  uint64_t value;
  uint32_t row;       /* = timestamp = cycle */
  uint8_t is_write;
  uint8_t width;      /* 1, 2, 4, 8 */
  uint16_t pad;
} zkir_mem_event;     /* 24 bytes */

/* A deferred range check flushed at a checkpoint (range_check.rs:59-66, 140-168) */
typedef struct zkir_rc_event {
  uint64_t value;     /* Value40::to_u64() */
  uint64_t pc;
} zkir_rc_event;      /* 16 bytes */

/* An observation-point normalization (normalization_witness.rs:19-43), before expansion */
typedef struct zkir_norm_event {
  uint64_t cycle;
  uint64_t pc;
  uint64_t raw_value; /* register value before normalization */
  uint8_t reg;
  uint8_t state;      /* storage state before normalization (selects 20- or 30-bit unpacking, state.rs:202-220) */
  uint8_t opcode;     /* triggering opcode byte */
  uint8_t pad[5];
} zkir_norm_event;    /* 32 bytes */

/* A single-block SHA-256 syscall (input_len < 56): the padded 64-byte message block, big-endian words
 * as parse_message_block produces them (crypto.rs:127-139), and the row it belongs to. */
typedef struct zkir_sha_block {
  uint32_t message_block[16];
  uint64_t timestamp;
} zkir_sha_block;     /* 72 bytes */

/* What an executed SHA-256 / Keccak-256 / BLAKE3 syscall WROTE (only with enable_execution_trace): the row (relative to the log, like zkir_mem_event.row) and the 32 bytes as
 * they lie in memory at out .. out + 32 after the call (SHA-256: the eight big-endian-parsed words stored little-endian, crypto.rs:251-254; the other two: the digest bytes in
 * order).  The device memory witness of mode 4 (memcheck.hip) takes the written bytes from here: a digest depends on what earlier calls wrote, and no trace column holds it. */
typedef struct zkir_hash_out {
  uint32_t row;
  uint32_t reserved;
  uint8_t bytes[32];
} zkir_hash_out;      /* 40 bytes */

typedef struct zkir_delta_log zkir_delta_log;   /* opaque, host memory */

/* Run the program on the host interpreter (bit-exact to VM::run, vm.rs:208-358) and record the delta
 * log.  tile_rows (power of two, 256..2048; 0 = default: 256 when max_cycles <= 2^21, else 512) fixes
 * the granularity of the tile index (one K1 workgroup per tile).
 * Returns ZKIR_OK or an error code (then *out is NULL).  No device WORK is queued; when the process has a device, the log's large
 * arrays (pc, instruction words, register events: >= 8 MiB) live in PINNED host blocks recycled by a process-wide pool, so that
 * zkir_host_to_device / hipMemcpyAsync out of them is plain DMA at link rate (ZKIR_PIN_LOG=0: pageable memory).  A caller that
 * queues asynchronous copies out of a log must let them complete before zkir_delta_log_free hands the blocks back to the pool. */
int zkir_interpret(const uint8_t* program_blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs,
                   const zkir_vm_config* cfg, uint32_t tile_rows, zkir_delta_log** out);
void zkir_delta_log_free(zkir_delta_log* log);

/* Trace WINDOW: the delta log of rows [row_begin, min(row_end, rows of the run)) only (cycle_base = row_begin).  VM::run is a
 * sequential chain (vm.rs:208-358: cycle c + 1 needs the registers, memory and pc of cycle c), so the state at row_begin exists only
 * after rows [0, row_begin) have been executed: this call executes them UNTRACED (no log stores; measured 1.5-2x the traced rate),
 * takes the register snapshot from the live machine, records the window and stops.  Multi-GPU: rank g of G calls it
 * with its own row range on its own host core — every GPU gets its shard after g * n * t_untraced + n * t_traced, sooner than a
 * single traced interpreter reaches those rows, with no inter-process transport.  cfg->enable_execution_trace must be set.
 * zkir_delta_log_cycles / halt / outputs describe the machine where the interpretation stopped; zkir_delta_log_window_open() = 1 if
 * that was the window's end rather than a halt (the run continues past row_end). */
int zkir_interpret_window(const uint8_t* program_blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs, const zkir_vm_config* cfg,
                          uint32_t tile_rows, uint64_t row_begin, uint64_t row_end, zkir_delta_log** out);
int zkir_delta_log_window_open(const zkir_delta_log*);

/* Row sharding (multi-GPU): a self-contained delta log for rows [row_begin, row_end) of `log` (ABSOLUTE row numbers: a source that
 * is itself a window or a shard holds rows [cycle_base, cycle_base + n_rows))
 * (any row range; a row_begin that is not a multiple of tile_rows — segment proofs overlap by one row — gets the shard its own
 * tiling, rebuilt from the events).  Its first 16 events are the register snapshot at row_begin, event
 * `vis`, mem-event rows and the tile index are rebased to the shard, and zkir_delta_log_cycle_base()
 * returns row_begin.  Side logs (range checks, normalizations, SHA blocks) are cut by the same cycle range.
 * Outputs / halt reason / cycles stay those of the whole run. */
int zkir_delta_log_shard(const zkir_delta_log* log, uint64_t row_begin, uint64_t row_end, zkir_delta_log** out);
uint64_t zkir_delta_log_cycle_base(const zkir_delta_log*);

uint64_t zkir_delta_log_cycles(const zkir_delta_log*);        /* ExecutionResult.cycles */
int zkir_delta_log_halt_kind(const zkir_delta_log*);          /* ZKIR_HALT_* */
uint64_t zkir_delta_log_halt_code(const zkir_delta_log*);     /* Exit(code) */
size_t zkir_delta_log_n_outputs(const zkir_delta_log*);
const uint64_t* zkir_delta_log_outputs(const zkir_delta_log*);
uint64_t zkir_delta_log_n_rows(const zkir_delta_log*);        /* 0 unless enable_execution_trace */
uint32_t zkir_delta_log_tile_rows(const zkir_delta_log*);
const uint64_t* zkir_delta_log_pc(const zkir_delta_log*);     /* [n_rows] TraceRow.pc          */
const uint32_t* zkir_delta_log_inst(const zkir_delta_log*);   /* [n_rows] TraceRow.instruction */
size_t zkir_delta_log_n_reg_events(const zkir_delta_log*);    /* includes the 16 snapshot events */
const zkir_reg_event* zkir_delta_log_reg_events(const zkir_delta_log*);
size_t zkir_delta_log_n_tiles(const zkir_delta_log*);
const uint32_t* zkir_delta_log_tile_ev_off(const zkir_delta_log*); /* [n_tiles+1] first event with vis > tile start */
const uint32_t* zkir_delta_log_tile_snap(const zkir_delta_log*);   /* [n_tiles][16] last event per register with vis <= tile start */
size_t zkir_delta_log_n_mem_events(const zkir_delta_log*);
const zkir_mem_event* zkir_delta_log_mem_events(const zkir_delta_log*);
size_t zkir_delta_log_n_rc_events(const zkir_delta_log*);
const zkir_rc_event* zkir_delta_log_rc_events(const zkir_delta_log*);
size_t zkir_delta_log_n_rc_witnesses(const zkir_delta_log*);
const uint64_t* zkir_delta_log_rc_offsets(const zkir_delta_log*);  /* [n_rc_witnesses+1] CSR over rc_events */
const uint64_t* zkir_delta_log_rc_cycles(const zkir_delta_log*);   /* [n_rc_witnesses] cycle of the checkpoint that produced witness k (vm.rs:316-344) */
uint32_t zkir_delta_log_rc_chunk_bits(const zkir_delta_log*);      /* header limb_bits / 2 (range_check.rs:29) */
size_t zkir_delta_log_n_norm_events(const zkir_delta_log*);
const zkir_norm_event* zkir_delta_log_norm_events(const zkir_delta_log*);
size_t zkir_delta_log_n_sha_blocks(const zkir_delta_log*);
const zkir_sha_block* zkir_delta_log_sha_blocks(const zkir_delta_log*);
size_t zkir_delta_log_n_hash_outs(const zkir_delta_log*);     /* one per executed hash syscall of the log's rows, in row order */
const zkir_hash_out* zkir_delta_log_hash_outs(const zkir_delta_log*);

/* ---- device stage: kernels on caller-owned device memory ------------------------------------- */

/* The wide execution trace in HBM, struct-of-arrays (one contiguous column per field per register;
 * TraceRow schema zkir-spec/src/trace.rs:24-50).  Register-indexed arrays are [16][reg_stride]
 * elements, column r starting at base + r*reg_stride. 372 bytes per row in total. */
typedef struct zkir_trace_columns {
  uint64_t* cycle;          /* [n_rows]                                        8 B/row  */
  uint64_t* pc;             /* [n_rows]  (may alias the uploaded delta-log pc)  8 B/row  */
  uint32_t* instruction;    /* [n_rows]  (may alias the uploaded delta-log inst)4 B/row  */
  uint64_t* registers;      /* [16][reg_stride]                               128 B/row */
  uint32_t* bound_bits;     /* [16][reg_stride]                                64 B/row */
  uint8_t* bound_tag;       /* [16][reg_stride]                                16 B/row */
  uint64_t* bound_payload;  /* [16][reg_stride]                               128 B/row */
  uint8_t* reg_state;       /* [16][reg_stride]                                16 B/row */
  uint64_t reg_stride;      /* elements between consecutive register columns (>= n_rows, multiple of 16) */
} zkir_trace_columns;

typedef struct zkir_trace_fill_args {
  const zkir_reg_event* events;   /* device, [n_events] */
  const uint32_t* tile_ev_off;    /* device, [n_tiles+1] */
  const uint32_t* tile_snap;      /* device, [n_tiles][16] */
  uint64_t n_rows;
  uint64_t cycle_base;            /* TraceRow.cycle of row 0 (row-sharding across GPUs) */
  uint32_t tile_rows;
  uint32_t n_events;
  zkir_trace_columns out;         /* device */
} zkir_trace_fill_args;

/* K1: expand the register-write log into the SoA trace columns (cycle, registers, bounds, states).
 * Asynchronous on `hip_stream` (a hipStream_t; NULL = default stream). */
int zkir_trace_fill_launch(const zkir_trace_fill_args* args, void* hip_stream);
/* The same for tiles [tile_begin, tile_end) only (args describe the whole trace): used to fill the tiles whose log has already been
 * uploaded while the host interpreter is still producing the rest (zkir_exec does this internally). */
int zkir_trace_fill_range_launch(const zkir_trace_fill_args* args, uint64_t tile_begin, uint64_t tile_end, void* hip_stream);

/* Algorithmic HBM bytes one zkir_trace_fill_launch moves: 360*n_rows written +
 * 32*n_events + 68*n_tiles read. */
uint64_t zkir_trace_fill_bytes(uint64_t n_rows, uint64_t n_events, uint64_t n_tiles);

/* ---- witness expansion kernels (witness.hip); every pointer is device memory, all launches async ----- */

/* MemoryOp columns (trace.rs:149-167), 39 bytes per op; each array has n_ops elements */
typedef struct zkir_memop_columns {
  uint64_t* address;
  uint64_t* value;
  uint64_t* timestamp;
  uint8_t* is_write;       /* MemOpType: 0 Read, 1 Write */
  uint8_t* width;
  uint32_t* bound_bits;    /* ValueBound::from_type_width(8*width), memory.rs:245 */
  uint8_t* bound_tag;
  uint64_t* bound_payload;
} zkir_memop_columns;

/* TraceRow.memory_ops flattened in row order */
int zkir_memops_expand_launch(const zkir_mem_event* events, uint64_t n_ops, uint64_t cycle_base, const zkir_memop_columns* out, void* hip_stream);
/* TraceRow.memory_ops in row order, the CSR row offsets (n_rows + 1 entries) and the per-row shape flags the sort needs (n_rows bytes;
 * 1 = the row's ops are not [ascending reads][ascending writes]) — all three from ONE pass over the events (24 B read per op) */
int zkir_memops_expand_csr_launch(const zkir_mem_event* events, uint64_t n_ops, uint64_t n_rows, uint64_t cycle_base, const zkir_memop_columns* out,
                                  uint64_t* row_offsets, uint8_t* seg_flags, void* hip_stream);
/* ExecutionResult::get_memory_trace() given the offsets and flags of zkir_memops_expand_csr_launch: one more pass over the events */
int zkir_memops_sort_prepared_launch(const zkir_mem_event* events, uint64_t n_ops, uint64_t cycle_base, const uint64_t* row_offsets, const uint8_t* seg_flags,
                                     const zkir_memop_columns* out, void* hip_stream);
/* CSR alone: offsets[r] = number of ops whose row < r, r = 0..n_rows (n_rows+1 entries); one binary search per row */
int zkir_memops_row_offsets_launch(const zkir_mem_event* events, uint64_t n_ops, uint64_t n_rows, uint64_t* offsets, void* hip_stream);
/* ExecutionResult::get_memory_trace() (vm.rs:85-94): stable order by (timestamp, address, Read<Write).
 * row_offsets from zkir_memops_row_offsets_launch; seg_scratch = n_rows bytes of device scratch. */
int zkir_memops_sort_launch(const zkir_mem_event* events, uint64_t n_ops, uint64_t n_rows, uint64_t cycle_base, const uint64_t* row_offsets,
                            uint8_t* seg_scratch, const zkir_memop_columns* out, void* hip_stream);

/* RangeCheckWitness entries (range_check.rs:175-192,212): value[n], pc[n], chunks[4][chunk_stride] (u16) and, if
 * multiplicity != NULL, the lookup multiplicities of all chunks: multiplicity[2^chunk_bits] (zeroed by the call). */
int zkir_range_check_expand_launch(const zkir_rc_event* events, uint64_t n, uint32_t chunk_bits, uint64_t* value, uint64_t* pc,
                                   uint16_t* chunks, uint64_t chunk_stride, uint32_t* multiplicity, void* hip_stream);

/* NormalizationEvent columns (normalization_witness.rs:19-43; normalized_bits = 20, limb_bits = 30, cause = ObservationPoint) */
typedef struct zkir_norm_columns {
  uint64_t* cycle; uint64_t* pc; uint8_t* reg; uint8_t* opcode;
  uint64_t* accumulated0; uint64_t* accumulated1;
  uint32_t* normalized0; uint32_t* normalized1;
  uint32_t* carry0; uint32_t* carry1;
} zkir_norm_columns;
int zkir_norm_expand_launch(const zkir_norm_event* events, uint64_t n, const zkir_norm_columns* out, void* hip_stream);

/* SHA-256 chip (Sha256Witness, trace.rs:236-256; crypto.rs:142-207): out = 608 word-columns [608][stride] (u32):
 * [0,16) message_block, [16,24) initial_state, [24,88) message_schedule, [88,600) round_states[64][8], [600,608) final_state;
 * timestamps[n] optional. */
int zkir_sha256_chip_launch(const zkir_sha_block* blocks, uint64_t n, uint32_t* out, uint64_t stride, uint64_t* timestamps, void* hip_stream);

/* ---- prover stages over Baby Bear (stark.hip, ntt.hip, verify.cpp) ---------------------------------
 * NOT in the reference (no prove(), no Plonky3: Cargo.toml:67-69) => self-defined
 * ("ZKIR-STARK v1"), parity unpinned; spec = oracle/stark_oracle.cpp, frozen by tests/golden/stark_goldens.json.
 * Field elements are canonical u32 (< p = 2^31 - 2^27 + 1) at rest.
 * Matrix layout "B8": the columns of a matrix with `width` columns and n rows are grouped in ceil(width/8) blocks of 8; block b is
 * the array [n][8] of u32 (32 contiguous bytes per row position: columns 8b..8b+7), blocks follow each other; element (column k,
 * row j) is word ((k/8)*n + j)*8 + k%8.  Columns past `width` in the last block are zero.  Every kernel moves 16-byte vectors and
 * the NTT shares its twiddles across the columns a lane carries; one block is one absorption of the rate-8 Poseidon2 sponge.
 * Demonstrator parameters: blow-up 2, 50 FRI queries + 12 bits of grinding (~62 bits, conjectured), Poseidon2 width 12 with
 * capacity 4 (~62-bit collisions).  What the AIR does and does not constrain is stated in zkir_amd/csrc/air.h. */
typedef struct zkir_stark_ctx zkir_stark_ctx;     /* device tables (twiddles, coset powers, Poseidon2 constants) + workspace for 2^log_n rows.
                                                     One proof at a time per context; different contexts are independent (no process-wide state). */
/* log_blowup in {1, 2, 3} (rate 1/2, 1/4, 1/8) with log_n <= 26 and log_n + log_blowup <= 27, the field's two-adicity; anything else is ZKIR_ERR_ARGUMENT before anything is
 * allocated.  A context of log_blowup 2 / 3 serves the COMMITMENT: zkir_lde_launch and the zkir_merkle_* calls.  The prover (zkir_prove; zkir_prove_result always makes its own
 * context of log_blowup 1) and the experiments built on its LDE (zkir_amd_experimental.h) are defined at blow-up 2 only and refuse such a context with ZKIR_ERR_ARGUMENT
 * before any launch: the proof format, AIR and verifier are blow-up 2. */
int zkir_stark_ctx_create(uint32_t log_n, uint32_t log_blowup, zkir_stark_ctx** out);
uint32_t zkir_stark_ctx_log_blowup(const zkir_stark_ctx* ctx);   /* what the context was created with (0 for NULL) */
void zkir_stark_ctx_free(zkir_stark_ctx* ctx);
uint32_t zkir_main_trace_width(void);             /* 152: COMMITTED main-trace columns of a default-mode run (the AIR's 172 logical columns minus the ones that
                                                     are identically zero there: R0's limbs and the 16 storage states; zkir_amd/csrc/air.h) */
uint32_t zkir_main_trace_width_for(uint32_t deferred);   /* 152 (deferred = 0) / 168 (VMConfig.enable_deferred_model: the storage states are committed) */
uint32_t zkir_padded_log_n(uint64_t n_real);      /* log2 of the padded trace length: max(3, ceil(log2(n_real))) */
/* trace columns (K1 output, n_real executed rows) -> main trace matrix (B8: zkir_main_trace_width_for(deferred) / 8 blocks [N][8]), N = 2^zkir_padded_log_n(n_real): rows past n_real are
 * padding (class "pad": state of the last executed row, cycle keeps counting).  deferred = VMConfig.enable_deferred_model of the run. */
int zkir_main_trace_launch(const zkir_trace_columns* trace, uint64_t n_real, uint32_t deferred, uint32_t* out, void* hip_stream);
/* The main trace of MODE 2 (default VM mode + the I/O argument: 160 committed columns): ECALL rows are dispatched on R10, every row shows the counters of the WRITE ecalls /
 * consumed inputs before it — a prefix count over the rows (scratch: 2 N + 2 (N / 1024 + 2) words of device memory, N = the padded row count).  inputs = the input tape ON
 * THE DEVICE (a live READ row's written value is looked up against it). */
typedef struct zkir_io_args { const uint64_t* inputs; uint64_t n_inputs; uint64_t writes_before, reads_before; } zkir_io_args;
int zkir_main_trace_io_launch(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, uint32_t* scratch, uint32_t* out, void* hip_stream);
/* the same on the HOST (host pointers everywhere; no scratch): a test entry point like zkir_main_trace_host */
int zkir_main_trace_io_host(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, uint32_t* out);
/* The main trace of MODE 3 (mode 2 + the memory argument, the bitwise opcodes, the shifts and MUL: 264 committed columns): load / store rows also show the accessed window, the cell's bytes before the access, the
 * time of its previous access and the pieces of the value moved.  mem_old / mem_told: [n_real] DEVICE arrays (zkir_memcheck_witness_of computes them on the host: memory is a
 * sequential chain); scratch as zkir_main_trace_io_launch.  _host: host pointers everywhere, a test entry point. */
int zkir_main_trace_mem_launch(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, const uint64_t* mem_old, const uint32_t* mem_told, uint32_t* scratch, uint32_t* out,
                               void* hip_stream);
int zkir_main_trace_mem_host(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, const uint64_t* mem_old, const uint32_t* mem_told, uint32_t* out);
/* The main trace of MODE 4 (round 6: mode 3 + the wide-arithmetic class — MULH / DIVU / REMU / DIV / REM, execute.rs:101-183: by a chunk relation on operands below 2^40, through the verifier-recomputed WIDE TAPE on raw 64-bit ones — + hash syscalls as a
 * tape + the code segment's boundary cell: 288 committed columns, six more 10-bit range values per row); arguments as zkir_main_trace_mem_launch / _host, plus the program's
 * code_size (header bytes 16..20): when it is 4 modulo 8 the last code word shares an 8-byte cell with the first data bytes, and stores into that cell's low half have no proof. */
int zkir_main_trace_wide_launch(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, const uint64_t* mem_old, const uint32_t* mem_told, uint64_t code_size,
                                uint32_t* scratch, uint32_t* out, void* hip_stream);
int zkir_main_trace_wide_host(const zkir_trace_columns* trace, uint64_t n_real, const zkir_io_args* io, const uint64_t* mem_old, const uint32_t* mem_told, uint64_t code_size, uint32_t* out);
/* the same rows computed on the HOST (trace = host pointers, out = host buffer, same B8 layout): the kernel's per-row code is one host + device
 * function, so the CPU test suite checks it against the oracle without a GPU.  A test / diagnostic entry point — the product never calls it
 * (there is no CPU fallback). */
int zkir_main_trace_host(const zkir_trace_columns* trace, uint64_t n_real, uint32_t deferred, uint32_t* out);
/* (the measurement probes and kernel experiments the library also exports — ALU / HBM-copy peaks, the fused first blocks, the strided-pass tilings — are declared in
 * zkir_amd_experimental.h: not part of the drop-in boundary) */
/* Test entry points of the AIR evaluation as the quotient kernel runs it (stark_prove.inl: QuotientOps — lazy 32-bit arithmetic, 96-bit sums, one
 * accumulator per row selector), host builds of the same code; nothing in the product calls them.
 * zkir_air_eval_host: sum_c alpha^c C_c (canonical E4 -> out4) of one (row, next row) pair given as LOGICAL columns (172 main, 40 aux; canonical
 * words), lookup parameters lk[56] (alpha, lambda^0..11, T / N), selector values, the two boundary states and alpha.
 * zkir_air_check_bounds: the static soundness check of that arithmetic on the constraint list (air.h: BoundOps): 0 = sound, else the broken rule. */
void zkir_air_eval_host(const uint32_t* loc, const uint32_t* nxt, const uint32_t* aloc, const uint32_t* anxt, const uint32_t* lk, uint32_t is_first, uint32_t is_last, uint32_t is_trans,
                        const uint32_t* first68, const uint32_t* last68, const uint32_t* alpha4, uint32_t mode /* 0 default, 1 deferred, 2 default + I/O: 180 / 48 columns, lk[57] */,
                        const uint32_t* cnt4 /* mode 2: (oc, ic) of the first and of the last row; else NULL */, uint32_t* out4);
int zkir_air_check_bounds(uint32_t deferred, char* why, size_t why_len);
/* per-column low-degree extension: in = B8 matrix with N rows (evaluations over <w_N>, natural order; CLOBBERED as scratch when N >= 1024)
 * -> out = B8 matrix with M = N << log_blowup rows (the context's: 2N, 4N or 8N) = evaluations over the coset 31*<w_M>, natural order, canonical words.  All 8 columns of
 * every block are transformed (zero columns of a ragged last block stay zero).  The extensions nest: row 2j at log_blowup b is row j at b - 1. */
int zkir_lde_launch(const zkir_stark_ctx* ctx, uint32_t* in, uint32_t width, uint32_t* out, void* hip_stream);
/* Poseidon2-12 Merkle tree over the n_leaves rows of the B8 matrix `mat` (leaf j = sponge over the `width` real columns of row j);
 * tree = 4*(2*n_leaves-1) words, leaf digests first, root = last 4 words.  This call, _leaves_ and _cap_ take the leaf count from the caller and use nothing of the
 * context that depends on its rate: n_leaves = N << log_blowup, up to 2^27, needs nothing else (64-bit leaf indices, at most 2^19 workgroups a launch). */
int zkir_merkle_commit_launch(const zkir_stark_ctx* ctx, const uint32_t* mat, uint32_t width, uint64_t n_leaves, uint32_t* tree, void* hip_stream);

/* The two halves of zkir_merkle_commit_launch, for callers that time or schedule them separately: the leaf digests (tree[0..4n), one
 * sponge per row: leaf_hash_kernel, the dominant kernel of the commit step), then zkir_merkle_cap_launch(ctx, tree, n_leaves) for the
 * levels above them. */
int zkir_merkle_leaves_launch(const zkir_stark_ctx* ctx, const uint32_t* mat, uint32_t width, uint64_t n_leaves, uint32_t* digests, void* hip_stream);

/* Top of a row-sharded commitment: tree[0..4n) holds n (power of two) digests — the all-gathered subtree roots of the row
 * shards, in rank order — and the call appends the log2(n) upper levels; root = last 4 words of the 4*(2n-1)-word buffer. */
int zkir_merkle_cap_launch(const zkir_stark_ctx* ctx, uint32_t* tree, uint64_t n_digests, void* hip_stream);

/* ---- openings of a commitment: "row j of what I committed is these words" ----
 * An opening RECORD of a tree with n_leaves = 2^d leaves over a matrix of `width` columns is width + 4 d words: the row's `width` canonical words in column order (the zero
 * padding of a ragged last block dropped), then the sibling digest of every level, leaf level first, four words each — the per-position record a proof's query section carries.
 * With ZKIR_OPEN_LEAF_DIGEST the tree's leaves are digests with no matrix behind them (the cap tree over shard roots): the record is the leaf digest itself, then the path,
 * 4 + 4 d words; `width` is 0 there.  Sharded commitments compose: a shard's record followed by the cap tree's digest-form PATH of that shard's root (its record without the
 * leading digest) is an opening of the capped root at index g n_local + j with n_leaves = G n_local.
 * zkir_merkle_opening_words: the record length, 0 for an n_leaves that is zero or not a power of two. */
#define ZKIR_OPEN_LEAF_DIGEST 1u
#define ZKIR_VERIFY_FORM_LANE 2u      /* zkir_merkle_verify_launch: run the one-lane-per-record kernel whatever the batch size (tests, measurements) */
#define ZKIR_VERIFY_FORM_ROW16 4u     /* .. the 16-lanes-per-record kernel.  Neither: the library's rule (by n_idx) */
uint64_t zkir_merkle_opening_words(uint32_t width, uint64_t n_leaves, uint32_t flags);
/* out[i] = the record of row indices[i], i < n_idx.  mat: B8, canonical words, as zkir_lde_launch writes it; tree: as zkir_merkle_commit_launch / _cap_launch wrote it;
 * indices, out: DEVICE pointers (out: n_idx records back to back).  mat == NULL selects the digest form (width must be 0).  Asynchronous on the stream, no synchronisation;
 * uses nothing of the context that depends on its rate: any context serves any n_leaves up to 2^27.  An index >= n_leaves reads nothing: its record is filled with
 * 0xFFFFFFFF.  n_idx == 0 is ZKIR_OK without a launch.  A null context, tree, indices or out, an n_leaves that is zero or not a power of two, or mat == NULL with width != 0:
 * ZKIR_ERR_ARGUMENT before any launch. */
int zkir_merkle_open_launch(const zkir_stark_ctx* ctx, const uint32_t* mat, uint32_t width, uint64_t n_leaves, const uint32_t* tree, const uint64_t* indices, uint64_t n_idx,
                            uint32_t* out, void* hip_stream);
/* verdicts[i] of record i (of `openings`, n_idx records back to back) for index indices[i] against `root` (all DEVICE pointers; root may be tree + 4 (2 n_leaves - 2)):
 * 0 the record hashes to root, 1 it does not, 2 a word of the record is >= p (the record is not hashed), 3 the index is >= n_leaves; 3 wins over 2 over 1.
 * summary (may be NULL): summary[0] = the number of non-zero verdicts, summary[1] = the smallest failing position i, 0xFFFFFFFF when there is none; the launch initialises both.
 * flags: ZKIR_OPEN_LEAF_DIGEST (width 0), ZKIR_VERIFY_FORM_*. */
int zkir_merkle_verify_launch(const zkir_stark_ctx* ctx, const uint32_t* root, uint32_t width, uint64_t n_leaves, const uint64_t* indices, uint64_t n_idx, const uint32_t* openings,
                              uint32_t flags, uint32_t* verdicts, uint32_t* summary, void* hip_stream);
/* The same verdicts on the HOST (host pointers everywhere, no device): part of the product, like zkir_verify. */
int zkir_merkle_verify_host(const uint32_t root[4], uint32_t width, uint64_t n_leaves, const uint64_t* indices, uint64_t n_idx, const uint32_t* openings, uint32_t flags,
                            uint32_t* verdicts, uint32_t summary[2]);

/* ---- a low-degree proof of a commitment, at any rate a context serves (log_blowup 1, 2, 3) ----
 * Statement: every column of the B8 matrix committed under `tree` (lde_mat = zkir_lde_launch's output on this context, M = N << log_blowup rows; tree =
 * zkir_merkle_commit_launch's over its `width` columns) is close to a polynomial of degree < N = 2^log_n.  Batched FRI over C(x) = sum_k gamma^k col_k(x), gamma drawn after
 * the root.  It states NO constraint and NO opening at a point: it is what lets a holder of the root alone trust that the rows opened under it (zkir_merkle_open_launch) are
 * rows of a low-degree extension.  Conjectured soundness: about log_blowup bits per query plus pow_bits, under the sponge's ~62-bit cap.
 * Proof words (all canonical): [0..8) 'ZKLD' = 0x444C4B5A, version 1, log_n, log_blowup, width, num_queries, pow_bits, n_layers | [8..12) the root | n_layers x 4 layer roots |
 * (4 << log_blowup) x 4 final layer | the grinding nonce (the smallest that passes) | per query: q < M/2, record(q), record(q + M/2) (zkir_merkle_open_launch's records:
 * width + 4 (log_n + log_blowup) words each), then per layer 4 * 2^k values and 4 * depth sibling words.  A proof is a function of its inputs.
 * zkir_lowdeg_proof_words: the proof's length; 0 unless 3 <= log_n <= 26, log_blowup in {1, 2, 3}, log_n + log_blowup <= 27, 1 <= width <= 512, 1 <= num_queries <= 128.
 * zkir_lowdeg_prove: lde_mat, tree DEVICE pointers, proof_host a HOST buffer of cap_words words (nothing past *n_words is written); 0 <= pow_bits <= 24.  One proof at a time
 * per context (its workspace arena, at most ~48 M bytes, shared with zkir_prove); synchronises the stream.  A null pointer, a context of log_n < 3, a width, num_queries or
 * pow_bits outside its range, or cap_words below zkir_lowdeg_proof_words: ZKIR_ERR_ARGUMENT with a message, before anything is launched.
 * zkir_lowdeg_verify: host only.  0 accepted; else the first failing check: 1 malformed (length not exactly the header's, magic, version, a range, n_layers), 2 not expect_root
 * (NULL: any root), 3 a word >= p, 4 final layer not of degree < 4, 5 grinding, 6 a query's index word, 7 a matrix record does not hash to the root, 8 layer-0 values are not
 * the combination of the rows, 9 a FRI leaf's path, 10 a carried value, 11 the final value; lowest query first. */
uint64_t zkir_lowdeg_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t width, uint32_t num_queries);
int zkir_lowdeg_prove(zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host,
                      uint64_t cap_words, uint64_t* n_words, void* hip_stream);
int zkir_lowdeg_verify(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root);

/* ---- an evaluation proof of a commitment: opening it at out-of-domain points, at any rate a context serves ----
 * Statement: every column k of the committed B8 matrix (lde_mat, tree: as for zkir_lowdeg_prove) is close to a polynomial p_k of degree < N = 2^log_n, and p_k(z_i) = y[i][k]
 * at the n_points (1 or 2) points z_i the caller supplies: E4 elements, four canonical words each.  A point must lie OUTSIDE the base field (one of its coordinates 1 .. 3 is
 * not zero: then z - x is invertible for every x of the domain and (z / 31)^N != 1), and two points must differ.  The points MUST BE CHOSEN AFTER THE ROOT (drawn from a
 * transcript that has observed it): that is the caller's protocol; a point known before the commitment proves nothing.
 * The evaluations are DEFINED as the barycentric sums over the rows j 2^log_blowup (the sub-coset 31 <w_N>):
 *     y[i][k] = ((z_i / 31)^N - 1) / N * sum_j mat[k][j 2^log_blowup] x_j / (z_i - x_j),   x_j = 31 w_N^j
 * whatever the matrix holds: on a matrix that is not low-degree the prover follows the same procedure and its proof is refused.
 * Proof: batched FRI over F(x) = sum_i (a_i - A_i(x)) / (z_i - x) on all M rows, A_i(x) = sum_k gamma^(i width + k) col_k(x), a_i = sum_k gamma^(i width + k) y[i][k],
 * gamma drawn after the header, the root, the points and the evaluations.  Conjectured soundness as for the low-degree proof.
 * Proof words (all canonical): [0..9) 'ZKEV' = 0x56454B5A, version 1, log_n, log_blowup, width, n_points, num_queries, pow_bits, n_layers | [9..13) the root | the points
 * (4 n_points words) | the evaluations (4 n_points width words, point-major: y[i][k] at 4 (i width + k)) | from there on the low-degree proof's layout: layer roots, final
 * layer, nonce, queries.  A proof is a function of its inputs.
 * zkir_eval_proof_words: the proof's length; 0 outside the low-degree proof's ranges or n_points 1 .. 2.
 * zkir_eval_prove: lde_mat, tree DEVICE pointers; points, proof_host HOST (nothing past *n_words is written).  One proof at a time per context (its workspace arena: the
 * low-degree proof's plus 16 n_points (M + N) bytes of inverses and weights); synchronises the stream.  A null pointer, a context of log_n < 3, a width, n_points,
 * num_queries or pow_bits outside its range, a word of points >= p, a point in the base field, two equal points, or cap_words below zkir_eval_proof_words:
 * ZKIR_ERR_ARGUMENT with a message naming the argument, before anything is launched.
 * zkir_eval_verify: host only.  0 accepted; else the first failing check, in this order: 1 malformed (length not exactly the header's, magic, version, a range, n_points,
 * n_layers), 2 not expect_root (NULL: any root), 13 not expect_points (4 n_points words) or not expect_evals (4 n_points width words; NULL: any), 3 a word >= p, 12 a point in
 * the base field or two equal points, 4 final layer not of degree < 4, 5 grinding, 6 a query's index word, 7 a matrix record does not hash to the root, 8 layer-0 values are
 * not F at the two rows, recomputed from the opened records, the points and the evaluations, 9 a FRI leaf's path, 10 a carried value, 11 the final value; lowest query first.
 * expect_points / expect_evals are read at the sizes the PROOF's header states (4 proof[5] and 4 proof[5] proof[4] words) once check 1 has passed: a caller that expects
 * certain sizes compares proof[4] and proof[5] with them before the call. */
uint64_t zkir_eval_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t width, uint32_t n_points, uint32_t num_queries);
int zkir_eval_prove(zkir_stark_ctx* ctx, const uint32_t* lde_mat, uint32_t width, const uint32_t* tree, const uint32_t* points, uint32_t n_points, uint32_t num_queries,
                    uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words, void* hip_stream);
int zkir_eval_verify(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals);

/* ---- a batched evaluation proof: several commitments of one height opened in ONE proof ----
 * Statement: n_mats (1 .. 4) committed B8 matrices of the SAME context (the same log_n and log_blowup; lde_mats[m], trees[m]: as for zkir_lowdeg_prove, widths[m] columns
 * each) have every column close to a polynomial of degree < N, and matrix m's columns take the proof's values at those of the n_points (1 or 2) shared points z_i that
 * masks[m] selects (bit i: opened at z_i).  The points are checked as zkir_eval_prove checks them.  1 <= widths[m] <= 512 and the widths sum to at most 512 (one product per
 * column per point in a 96-bit sum); 1 <= masks[m] < 2^n_points; every point is selected by some matrix.
 * The evaluations are zkir_eval_prove's barycentric sums, taken for the (point, matrix) pairs the masks select and for no others.  One gamma is drawn after the header, the
 * shape, all the roots, the points and all the evaluations; its exponent e runs consecutively: for i over the points, for m over the matrices with bit i of masks[m] set,
 * in order, for k < widths[m].  Then
 *     A_i(x) = sum gamma^e col_{m,k}(x),   a_i = sum gamma^e y[i][m][k]   (over the selected (m, k) of point i),   F(x_j) = sum_i (a_i - A_i(x_j)) / (z_i - x_j)
 * over all M rows, and batched FRI over F as in the low-degree proof: one inverse table, one commit phase, one grind and one set of query rows for all the matrices.
 * With n_mats = 1 and a full mask F is zkir_eval_prove's codeword; splitting a matrix at a multiple of 8 columns into two matrices with full masks leaves F unchanged.
 * Proof words (all canonical): [0..9) 'ZKBE' = 0x45424B5A, version 1, log_n, log_blowup, n_mats, n_points, num_queries, pow_bits, n_layers | (widths[m], masks[m]) per matrix
 * | the n_mats roots | the points (4 n_points words) | the evaluations in the exponent order, 4 words each | from there on the low-degree proof's layout: layer roots, final
 * layer, nonce, queries.  A query: q, then for each matrix in order record_m(q), record_m(q + M/2) (zkir_merkle_open_launch's records, widths[m] + 4 (log_n + log_blowup)
 * words each), then per layer the values and the path.
 * Transcript: every word up to and including the evaluations, gamma; per layer root, beta; the final words; check_pow(nonce); q_t = sample_bits(log_n + log_blowup - 1).
 * zkir_batch_eval_proof_words: the proof's length; 0 for a shape no proof can state.
 * zkir_batch_eval_prove: lde_mats, trees, widths, masks HOST arrays of n_mats entries (the matrices and trees they name are DEVICE pointers); points, proof_host HOST (nothing
 * past *n_words is written).  One proof at a time per context (its workspace arena: the low-degree proof's plus 16 n_points (M + N) bytes of inverses and weights and the
 * matrices' partial sums); synchronises the stream.  ZKIR_ERR_ARGUMENT with *n_words = 0, nothing written and a message naming the cause, before anything is launched, for:
 * a null pointer, n_mats outside 1 .. 4, a width outside 1 .. 512, widths summing above 512, a mask of 0 or with a bit at or above n_points, a point no matrix is opened at,
 * and zkir_eval_prove's refusals of points, num_queries, pow_bits, the context's log_n and cap_words.
 * zkir_batch_eval_verify: host only.  zkir_eval_verify's codes in its order of checks: 1 also covers n_mats, a width, the width total, a mask and an unused point; 2 compares
 * all n_mats roots with expect_roots (4 n_mats words; NULL: any); 13 expect_points (4 n_points words) and expect_evals (the proof's evaluation words, in the exponent order);
 * 7 a record of any matrix, lowest matrix first within a query; 8 recomputes F from all the matrices' records.  The expected arrays are read at the sizes the PROOF's header
 * states, and only once check 1 has passed. */
uint64_t zkir_batch_eval_proof_words(uint32_t log_n, uint32_t log_blowup, uint32_t n_mats, const uint32_t* widths, const uint32_t* masks, uint32_t n_points, uint32_t num_queries);
int zkir_batch_eval_prove(zkir_stark_ctx* ctx, uint32_t n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees, const uint32_t* masks,
                          const uint32_t* points, uint32_t n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words, uint64_t* n_words,
                          void* hip_stream);
int zkir_batch_eval_verify(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals);

/* OPENING COMMITMENTS OF DIFFERENT HEIGHTS IN ONE EVALUATION PROOF ('ZKMH'; zkir_amd/csrc/mixed_eval.inl, verify.cpp; spec of every word: tests/mixed_eval_ref.py).
 * Statement: n_groups (2 or 3) groups at ONE log_blowup b, of strictly decreasing heights log_n_0 > log_n_1 > .. (each >= 3, log_n_0 + b <= 27).  Group h is exactly what
 * zkir_batch_eval_prove states at its own height: n_mats[h] (1 .. 4) B8 matrices of M_h = N_h << b rows on ctxs[h], each under its own tree, widths 1 .. 512 summing to at most
 * 512 in the group, its own n_points[h] (1 or 2) points, a mask per matrix with zkir_batch_eval_prove's rules.  Points of different groups are unrelated.  One group is
 * refused (that is zkir_batch_eval_prove), and so are equal heights (they belong in one group).
 * One gamma is drawn after the header and all roots, points and evaluations; its exponent runs consecutively through the groups in order, and inside a group in
 * zkir_batch_eval_prove's order.  F_h is that proof's quotient of group h over 31 <w_{M_h}> with those exponents.  ONE FRI: layer 0 is F_0; the schedule is the low-degree
 * proof's with one more cap — a step never jumps over a lower M_h, so every M_h is a committed layer's size — and when a fold leaves the layer of size M_h, F_h is added to it
 * by index before it is hashed.  The final layer (4 << b values of degree < 4), grinding and q_t = sample_bits(log M_0 - 1) are the low-degree proof's.
 * Proof words (all canonical): [0..7) 'ZKMH' = 0x484D4B5A, version 1, log_blowup, n_groups, num_queries, pow_bits, n_layers | per group: log_n, n_mats, n_points, then
 * (width, mask) per matrix | all roots (groups in order, matrices in order) | all points | all evaluations in the exponent order | layer roots | final layer | nonce | queries.
 * A query: q; group 0's matrices in order, record_m(q) and record_m(q + M_0/2); each lower group's matrices in order, ONE record_m(q mod M_h) of width + 4 log M_h words; the
 * layers as in the low-degree proof.  Transcript: every word up to and including the evaluations, gamma, then the low-degree proof's steps.
 * The arrays are flat HOST arrays with the groups concatenated: ctxs, n_mats, n_points have n_groups entries; lde_mats, trees (DEVICE pointers), widths, masks one entry per
 * matrix; points 4 words per point.  zkir_mixed_eval_proof_words: the proof's length; 0 for a shape no proof can state.
 * zkir_mixed_eval_prove: the workspace arena and the one-proof-at-a-time lock are ctxs[0]'s; the other contexts are only read.  Synchronises the stream; nothing past *n_words
 * is written.  ZKIR_ERR_ARGUMENT with *n_words = 0, nothing written and nothing launched for: a null pointer, n_groups outside 2 .. 3, a context whose log_blowup is not
 * ctxs[0]'s, heights that do not strictly decrease, and, per group, zkir_batch_eval_prove's refusals.
 * zkir_mixed_eval_verify: host code, no HIP call (zkir_mixed_eval_verify_device below is its device form).  zkir_batch_eval_verify's codes in its order: 1 malformed (exact length, magic, version, ranges, group order, a
 * group's shape, n_layers), 2 roots, 13 points / evaluations, 3 a word >= p, 12 a point in the base field or two equal points WITHIN a group, 4 final layer, 5 grinding,
 * 6 index word, 7 a record (in the order they stand in the query), 8 layer-0 values (from group 0's records), 9 a FRI leaf's path, 10 carried value — before the step into
 * the layer of size M_h the carried value gains F_h(q mod M_h), recomputed from group h's records — 11 final value.  (Which code a false evaluation gets depends on the prover: one that follows the honest
 * procedure after it folds a quotient with a pole and meets check 4, in any group; 8 (group 0) and 10 (a lower group) appear where the committed layers are those of other
 * evaluations than the stated ones.)  The expected
 * arrays (all roots, all points, all evaluations, in the proof's order) are read at the sizes the PROOF's header states, and only once check 1 has passed. */
uint64_t zkir_mixed_eval_proof_words(uint32_t log_blowup, uint32_t n_groups, const uint32_t* log_ns, const uint32_t* n_mats, const uint32_t* n_points, const uint32_t* widths,
                                     const uint32_t* masks, uint32_t num_queries);
int zkir_mixed_eval_prove(zkir_stark_ctx* const* ctxs, uint32_t n_groups, const uint32_t* n_mats, const uint32_t* const* lde_mats, const uint32_t* widths, const uint32_t* const* trees,
                          const uint32_t* masks, const uint32_t* points, const uint32_t* n_points, uint32_t num_queries, uint32_t pow_bits, uint32_t* proof_host, uint64_t cap_words,
                          uint64_t* n_words, void* hip_stream);
int zkir_mixed_eval_verify(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals);

/* VERIFYING ON THE DEVICE.  zkir_lowdeg_verify, zkir_eval_verify, zkir_batch_eval_verify and zkir_mixed_eval_verify — all FOUR proofs — with checks 7 - 11 of ALL the queries run on the current HIP device: one leaf-and-
 * path job per matrix record and FRI layer (a row of 16 lanes each), the layer-0 values and the folds in a second kernel.  Everything else — the shape, the expectations, the
 * word range, the whole transcript, the final layer's degree, grinding, the sampling of the rows, check 6 — is the host entries' own code in its order, and the device is
 * used only after checks 1 and 3 have passed: every extent a kernel uses comes from the checked header, the row it opens is the transcript's sample.
 * The verdict is the host entry's for every input: 0, or the same check's number, first failing check, lowest query first.  A NEGATIVE result is no verdict:
 * -ZKIR_ERR_DEVICE (no usable device, a failed HIP call) or -ZKIR_ERR_OTHER (no host memory); zkir_last_error says which.  proof and the expectations are HOST memory.  No
 * context: the entries use zkir_verify_device's per-device state (device block grown on demand, pinned staging), so calls on one device are serialised inside.  One staged
 * upload, two launches, one download and one synchronisation on hip_stream; nothing is launched when the verdict is 1 - 5, 12 or 13.
 * zkir_mixed_eval_verify_device makes THREE launches: the leaf-and-path jobs (a lower group's record is opened at the sample mod M_h), then the layer-0 values of group 0
 * with one more wave per (query, lower group) that forms F_h(q mod M_h), then the folds, which add the stored F_h where the next layer has size M_h — a launch of their own
 * so that the stream orders them behind the values.  Its limits are its own: at most 10 FRI layers and 26 leaf-and-path jobs a query. */
int zkir_lowdeg_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, void* hip_stream);
int zkir_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_root, const uint32_t* expect_points, const uint32_t* expect_evals, void* hip_stream);
int zkir_batch_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* hip_stream);
int zkir_mixed_eval_verify_device(const uint32_t* proof, uint64_t n_words, const uint32_t* expect_roots, const uint32_t* expect_points, const uint32_t* expect_evals, void* hip_stream);

/* Public inputs of a proof: absorbed by the Fiat-Shamir transcript before the first commitment and carried in the proof header. */
typedef struct zkir_public_inputs {
  uint64_t n_real;             /* executed rows = ExecutionResult.cycles */
  uint64_t entry_point;        /* ProgramHeader.entry_point: pc of row 0 (constrained) */
  uint32_t deferred;           /* the proof's MODE: 0 = default VM mode, 1 = VMConfig.enable_deferred_model (relaxed AIR), 2 = default mode + the I/O argument (below), 3 = 2 + the memory argument */
  uint32_t fri_params;         /* the prover's parameters: num_queries | pow_bits << 16; 0 = the defaults (50 queries, 12 grinding bits).  Set with zkir_public_inputs_set_params.
                                * They are header words 4 and 6 of the proof (observed by the transcript); a verifier with an `expect` requires exactly these. */
  uint32_t program_digest[4];  /* zkir_digest_bytes(program blob) */
  uint32_t io_digest[4];       /* zkir_digest_bytes(LE u64 words [n_inputs, inputs.., n_outputs, outputs.., halt kind, halt code, cycles]) */
  /* PROVER side only (ignored when the struct is the `expect` of a verifier): the program itself, BORROWED — set by
   * zkir_public_inputs_of to the caller's blob, which must stay valid while the struct is passed to zkir_prove.  Its code words are
   * the instruction ROM of the lookup argument; the proof carries the program (format v5 on; zkir_proof_version() = the current format), the verifier checks it against program_digest. */
  const uint8_t* program_blob;
  uint64_t program_blob_len;
  /* MODE 2 (`deferred` == 2, round 4): the default VM mode WITH the I/O argument — WRITE / READ ecalls are tied by a lookup to the tapes below, which the proof then
   * carries (their digest, with the halt reason and the cycle count, is io_digest); the verifier also checks that the run ends on the instruction the halt reason names.
   * PROVER side (BORROWED pointers, filled by zkir_public_inputs_of; ignored in a verifier's `expect`).  For a SEGMENT of a run the caller sets writes_before /
   * reads_before: the WRITE / READ ecalls the run executed before the segment's first row. */
  const uint64_t* inputs;
  uint64_t n_inputs;
  const uint64_t* outputs;
  uint64_t n_outputs;
  uint32_t halt_kind;          /* ZKIR_HALT_* */
  uint32_t reserved2;
  uint64_t halt_code;
  uint64_t writes_before, reads_before;
  /* MODE 3 (`deferred` == 3, round 4): mode 2 WITH the memory argument — loads and stores are constrained and every access is tied to a consistent memory (air.h "MODE 3").
   * PROVER side (ignored in a verifier's `expect`).  mem_old == NULL (what zkir_public_inputs_of leaves): zkir_prove computes the run's memory witness ON THE DEVICE
   * (memcheck.hip: the accesses sorted address-major, a segmented scan per cell).  Otherwise BORROWED pointers set by zkir_public_inputs_set_memory from a zkir_memcheck_witness
   * (the host's independent replay): per ROW the bytes of the accessed 8-byte cell before the access and the time of the cell's previous access (0 on rows that are no load /
   * store), and the touched cells by increasing address.  The proof carries the touched cells either way. */
  const uint64_t* mem_old;     /* [n_real] */
  const uint32_t* mem_told;    /* [n_real] */
  const uint64_t* cell_addr;   /* [n_cells] multiples of 8 below 2^40, strictly increasing */
  const uint64_t* cell_bytes;  /* [n_cells] the cell's final bytes, little-endian */
  const uint32_t* cell_time;   /* [n_cells] the time of its last access = that row's cycle + 1 */
  uint64_t n_cells;
  /* MODE 4 (`deferred` == 4, round 6): mode 3 WITH the wide-arithmetic class (MULH / DIVU / REMU / DIV / REM: constrained by a chunk relation on operands below 2^40; on raw 64-bit operands — `as i64`,
   * 128-bit products — through the WIDE TAPE: one record (cycle, rs1, rs2, opcode) per such row, gathered by zkir_prove itself, the verifier computes the result), the code segment's boundary cell, and
   * HASH SYSCALLS as a tape: the proof carries one record per SHA-256 / Keccak-256 / BLAKE3 call (cycle, pointers, length, kind, and per touched 8-byte cell its bytes before
   * the call and the time of its previous access) and the verifier computes every digest itself.  PROVER side: hash_section = those records in the proof's own word layout
   * (csrc/hashcall.h), BORROWED from a zkir_memcheck_witness made with zkir_memcheck_witness_of_mode(.., 4, ..) (zkir_public_inputs_set_memory sets it).  With mem_old == NULL (what
   * zkir_public_inputs_of leaves) zkir_prove builds the memory witness AND this tape on the device (memcheck.hip): every old byte comes from the program image and earlier
   * writes; what a hash call WROTE comes from hash_outs below (the interpreter's record, one per executed call). */
  const uint32_t* hash_section;
  uint64_t hash_section_words;
  /* (ABI 7) PROVER side, BORROWED from the run's delta log (zkir_public_inputs_of sets them; ignored in a verifier's `expect`): the written digests of the run's hash
   * syscalls in row order.  Needed only by the device witness of a mode-4 run that makes hash calls; their count must be the trace's number of hash rows. */
  const zkir_hash_out* hash_outs;
  uint64_t n_hash_outs;
} zkir_public_inputs;
/* sizeof(zkir_public_inputs) of the library (a binding checks its own struct against it) */
uint64_t zkir_public_inputs_size(void);
/* (mode 3) The memory witness of a WHOLE run (host, sequential like the interpreter: memory is a chain — what a load returns depends on every earlier store): the
 * log's rows are replayed with their register state (rebuilt from the register events), every load / store looks up its aligned 8-byte cell — the program image at first
 * (code at 0x1000, data behind it: vm.rs:153-170), zero elsewhere — and records the cell's bytes and the time of its previous access.  Refused (ZKIR_ERR_ARGUMENT): a shard /
 * window, an address of 2^40 or more (addr_limbs = 2, config.rs:30), an executed hash syscall (its memory effect is not stated by the AIR).  Free with zkir_memcheck_witness_free. */
typedef struct zkir_memcheck_witness zkir_memcheck_witness;
int zkir_memcheck_witness_of(const zkir_delta_log* log, const uint8_t* program_blob, size_t blob_len, zkir_memcheck_witness** out);
/* the same for a given AIR mode: 3 = zkir_memcheck_witness_of; 4 (round 6) also replays the run's hash syscalls (SHA-256 / Keccak-256 / BLAKE3: the message read out of the
 * replayed memory, the digest computed and laid over the output range) and records them as the proof's hash section (zkir_public_inputs::hash_section) */
int zkir_memcheck_witness_of_mode(const zkir_delta_log* log, const uint8_t* program_blob, size_t blob_len, uint32_t mode, zkir_memcheck_witness** out);
uint64_t zkir_memcheck_witness_n_hash_calls(const zkir_memcheck_witness* w);
void zkir_memcheck_witness_free(zkir_memcheck_witness* w);
uint64_t zkir_memcheck_witness_n_cells(const zkir_memcheck_witness* w);
uint64_t zkir_memcheck_witness_n_accesses(const zkir_memcheck_witness* w);
/* The same witness made ON THE DEVICE (memcheck.hip: what zkir_prove runs in mode 3 when the public inputs bring no witness), as a call of its own: trace = the DEVICE columns of
 * a whole run, the outputs are HOST arrays (mem_old / mem_told: n_real entries, zero where the row is no load / store; the cell arrays: capacity `cap`, *n_cells = the count). */
int zkir_memcheck_witness_device(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* program_blob, size_t blob_len, uint64_t* mem_old, uint32_t* mem_told,
                                 uint64_t* cell_addr, uint64_t* cell_bytes, uint32_t* cell_time, uint64_t cap, uint64_t* n_cells, void* hip_stream);
/* (mode 4) The device witness of a run WITH hash syscalls, as a call of its own (what zkir_prove runs in mode 4 when the public inputs bring no witness and hash_outs is not
 * empty): mode must be 4 (3 = zkir_memcheck_witness_device, which refuses hash calls: ZKIR_ERR_ARGUMENT here).  hash_outs: the log's records (host).  The outputs of
 * zkir_memcheck_witness_device (hash rows' own mem_old / mem_told are 0; the cells include those only hash calls touched) + the proof's hash section (csrc/hashcall.h) in
 * hash_words (host, capacity hash_cap_words; *n_hash_words = its length, ZKIR_ERR_ARGUMENT if it exceeds the capacity). */
int zkir_memcheck_witness_device_mode(const zkir_trace_columns* trace, uint64_t n_real, const uint8_t* program_blob, size_t blob_len, uint32_t mode, const zkir_hash_out* hash_outs,
                                      uint64_t n_hash_outs, uint64_t* mem_old, uint32_t* mem_told, uint64_t* cell_addr, uint64_t* cell_bytes, uint32_t* cell_time, uint64_t cap,
                                      uint64_t* n_cells, uint32_t* hash_words, uint64_t hash_cap_words, uint64_t* n_hash_words, void* hip_stream);
/* Host test entry of the closed forms the device witness uses (csrc/hashcall.h): the number of distinct 8-byte cells a hash call (in, len, out) touches, and in *rank the
 * position of `cell` among them in ascending order (~0 if the call does not touch it; rank may be NULL).  Returns ~0 when hashcall::in_range(in, len, out, kind) is false. */
uint64_t zkir_hash_call_cells_host(uint64_t in_ptr, uint64_t len, uint64_t out_ptr, uint32_t kind, uint64_t cell, uint64_t* rank);
/* (mode 4) The hash tape's and the wide tape's share of the lookup table side, as calls of their own.
 * hash_words: a hash section in the proof's layout (host); new_bytes: per touched cell, in the section's order, the
 * cell's bytes after its call (host, n = the section's total cell count); wide_words: a wide section [n] + 8 words
 * per record, any record order (host); alpha, lambda: canonical E4.  Out (host, canonical): sum[4]; hh[4 * n_calls];
 * ww[4 * n_records] in the given record order.  _launch: what zkir_prove runs on the tape its device witness built
 * (csrc/tape_table.inl); _host: the host form (what zkir_prove runs for the hash calls of a caller's host witness).
 * A section hashcall::parse_section rejects (with no row bound and no code segment) is ZKIR_ERR_ARGUMENT in both. */
int zkir_tape_table_side_launch(const uint32_t* hash_words, uint64_t n_hash_words, const uint64_t* new_bytes,
                                const uint32_t* wide_words, uint64_t n_wide_words, const uint32_t alpha[4],
                                const uint32_t lambda[4], uint32_t sum[4], uint32_t* hh, uint32_t* ww, void* hip_stream);
int zkir_tape_table_side_host(const uint32_t* hash_words, uint64_t n_hash_words, const uint64_t* new_bytes,
                              const uint32_t* wide_words, uint64_t n_wide_words, const uint32_t alpha[4],
                              const uint32_t lambda[4], uint32_t sum[4], uint32_t* hh, uint32_t* ww);
/* the device's form of hashcall::parse_section's checks on a hash section (host words, n_real rows, the code segment
 * [0x1000, code_end)): *code = 0 well-formed / 4 truncated / 55 an output on code bytes / 56 a malformed record — of
 * the LOWEST failing record.  _host: parse_section itself. */
int zkir_hash_tape_check_launch(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t n_real, uint64_t code_end,
                                int* code, void* hip_stream);
int zkir_hash_tape_check_host(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t n_real, uint64_t code_end,
                              int* code);
/* (mode 4) What every hash call of a section wrote, recomputed from the tape alone (a verifier has no record of the run): new_bytes[h] = touched cell h's bytes after its
 * call, in the section's cell order — the cell's old bytes with the call's 32 output bytes laid over them, the message read out of the OLD bytes (hashcall::new_bytes).
 * hash_words, new_bytes: host; new_bytes has one entry per touched cell.  _launch: hash_tape_new_bytes_kernel (csrc/tape_digest.inl), a lane per call of at most 1024
 * bytes, longer calls hashed on host threads; _host: hashcall::new_bytes over the parsed calls.  A section hashcall::parse_section rejects (with no row bound and no
 * code segment) is ZKIR_ERR_ARGUMENT in both, the check's number in the message. */
int zkir_hash_tape_new_bytes_launch(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t* new_bytes, void* hip_stream);
int zkir_hash_tape_new_bytes_host(const uint32_t* hash_words, uint64_t n_hash_words, uint64_t* new_bytes);
/* zkir_verify with the three stages that are linear in a mode-4 proof's tapes — the record checks, the sections' chunk digests, the tapes' share of the lookup table side
 * (the digest of every hash call among it) — run on the current HIP device.  The verdict is zkir_verify's for every input: 0, or the same check's number.  Modes 0-3 and a
 * mode-4 proof with both tapes empty ARE zkir_verify: nothing is uploaded, nothing is launched.  A NEGATIVE result is no verdict: -ZKIR_ERR_DEVICE (no usable device, a
 * failed HIP call) or -ZKIR_ERR_OTHER (no host memory); zkir_last_error says which.  Calls on one device are serialised inside; the device block and the pinned staging of the
 * largest tape seen stay with the process, one set per HIP device the entry was called on. */
int zkir_verify_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* hip_stream);
/* THE QUERIES ON THE DEVICE: one proof, many, or a chain.  The three entries below are zkir_verify / zkir_verify_chain with the QUERY STAGE — checks 20 - 27 of all the
 * queries: the Merkle paths of the three commitments' records and of the FRI layers, the layer-0 values, the folds, the final value — run on the current HIP device as ONE
 * batch: a leaf-and-path job per record and layer (a row of 16 lanes each), the layer-0 values (a wave per query and half) and the folds (a lane per query and layer) in a
 * second kernel.  Everything else — header, program, cells, the transcript, the constraints at zeta, the final layer's degree, grinding, the sampling, check 20's index
 * words, check 30 — is zkir_verify's own host code in its order, a mode-4 proof's tape stages run as in zkir_verify_device.  Every extent a kernel uses comes from checked
 * header words, the row it opens is the transcript's sample; only the words from the trace root to the end of the last query that lies wholly inside the proof are
 * uploaded (never the program, the cells or the tapes), and a query the proof's end cuts is the host loop's.  One staged upload, two launches, one download and one
 * synchronisation on hip_stream per call, however many proofs; nothing is launched where no proof reaches its queries.  The verdict is the host entry's for every input.
 * A NEGATIVE result is no verdict: -ZKIR_ERR_DEVICE or -ZKIR_ERR_OTHER, zkir_last_error says which.  Calls on one device are serialised inside (zkir_verify_device's
 * per-device block and pinned staging).
 * zkir_verify_on_device: zkir_verify's verdict, any mode; a batch of one.
 * zkir_verify_many_on_device: n independent proofs, 1 <= n <= 1024 (else ZKIR_ERR_ARGUMENT, as for a null proofs, proof_words or verdicts); expects may be NULL and so may
 * each entry.  The host parts run proof after proof on the calling thread, then ONE stage run serves every proof that reached its queries.  Returns 0 with verdicts[i] =
 * what zkir_verify(proofs[i], proof_words[i], expects[i]) returns for every i, or an error (ZKIR_ERR_ARGUMENT, a negative value) with NO verdict written.
 * zkir_verify_chain_on_device: zkir_verify_chain's verdict; the segments' host parts run up to the first one that fails there, the collected segments' queries are one
 * stage run, and the verdict is resolved in segment order.  A chain of one mode >= 3 proof is zkir_verify_on_device.
 * zkir_verify_queries_last: what the calling thread's last verification (any entry) ran as its device query stage — leaf-and-path jobs, value jobs (two per query and one
 * per query and layer), launches (0 or 2), words uploaded (proof words and the stage's own tables).  All zero after a host entry and after zkir_verify_device.  Any
 * pointer may be NULL.  Whether the device pays for ONE small proof is a measurement (profiles/r20_verify_queries_device.txt); no threshold is built in. */
int zkir_verify_on_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, void* hip_stream);
int zkir_verify_many_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* hip_stream);
int zkir_verify_chain_on_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, void* hip_stream);
int zkir_verify_queries_last(uint64_t* hash_jobs, uint64_t* value_jobs, uint32_t* launches, uint64_t* uploaded_words);

/* A ZKIR-STARK PROOF AT THE CONTEXT'S OWN RATE ('ZKSR', version 1; zkir_amd/csrc/stark_prove.inl, eval_open.inl, verify.cpp; DESIGN.md "Proofs at blow-up 4 and 8").
 * zkir_prove is blow-up 2 and keeps refusing any other context.  zkir_prove_rate proves a WHOLE run in mode 0, 1 or 2 on a context of log_blowup 1, 2 or 3:
 *   the STARK part: exactly the sections of a zkir_prove proof from the header through the quotient root — header, boundary states (mode 2: + counters), program, (mode 2)
 *     I/O section, multiplicities, trace | aux | quotient root — under the header words 0 = 0x52534B5A ('ZKSR'), 1 = 1, 4 = num_queries, 5 = log_blowup, 6 = pow_bits (the
 *     others as in zkir_prove).  The whole header from word 2 on is observed first, so the rate and the parameters are bound; the transcript is zkir_verify's up to zeta.
 *   the embedded evaluation proof: a 'ZKBE' proof word for word as zkir_batch_eval_prove writes it for the three committed matrices (main: zkir_main_trace_width_for(mode)
 *     columns, aux, the quotient's 4) with masks {3, 3, 1} at the points [zeta, w_N zeta] and the entry's num_queries and pow_bits.  It has its own transcript (roots,
 *     points, evaluations ..), which zeta carries the outer one into; zkir_batch_eval_verify accepts these words on their own.
 * num_queries 1 .. 128, pow_bits 0 .. 24 (zkir_batch_eval_prove's ranges); pub->fri_params is NOT consulted.  The usual choices are 50 / 25 / 17 queries at log_blowup
 * 1 / 2 / 3 with 12 bits.  ZKIR_ERR_ARGUMENT with a message, before anything is launched, for: a null argument, mode 3 or 4, a segment (writes_before / reads_before),
 * num_queries or pow_bits out of range, a context whose log_n is not zkir_padded_log_n(n_real), and zkir_prove's refusals of the public inputs.  stage_ms: NULL or ELEVEN
 * floats — zkir_prove's [0..4] (main trace, LDE, trace Merkle, lookup argument, quotient + its Merkle tree), then the evaluation proof's six.  The proof is freed with
 * zkir_proof_free.  The matrices of such a proof rest in canonical form (the commitment layer's), the quotient is evaluated by a kernel of its own over the N << log_blowup
 * coset (quotient_rate_kernel).
 * zkir_verify_rate: host only.  zkir_verify's checks and codes, in its order, through the program, the I/O section, the table side and the challenges (1 malformed header,
 * magic, version; 2 a header range — also: fewer queries than min_queries or fewer bits than min_pow_bits; 3 a word >= p; 4 truncated; 6 not `expect`'s
 * run (fri_params not compared); 7 initial state; 8 program; 50 - 53 the I/O claim), then: 4 too short for the embedded header and evaluations; 5 the embedded proof is
 * not a 'ZKBE' proof of the outer log_n, log_blowup, three widths, masks {3, 3, 1}, two points, num_queries and pow_bits; 10 sum_c alpha^c C_c(zeta) != Q(zeta) Z_H(zeta)
 * on the embedded proof's evaluations; 100 + c where zkir_batch_eval_verify, told the outer roots and the points [zeta, w_N zeta], answers c (so 101 a wrong length,
 * 102 other roots, 113 other points, 105 grinding, 107 a record's path, 108 layer-0 values ..).
 * zkir_verify_rate_device: the same function with the embedded proof's query stage on the current HIP device (zkir_batch_eval_verify_device's); the same verdict for
 * every input; a NEGATIVE result is a device failure, not a verdict.
 *
 * zkir_prove_rate_modes: zkir_prove_rate with modes 0 - 4 admitted (zkir_prove_rate keeps its scope and its refusal).  Modes 0 - 2: zkir_prove_rate's words exactly.  Modes
 * 3 / 4: the public inputs are what zkir_prove takes in those modes — the memory witness made on the device when pub->mem_old == NULL, or the host witness of
 * zkir_memcheck_witness_of(_mode) + zkir_public_inputs_set_memory; in mode 4 the hash tape and the wide tape — and every refusal zkir_prove makes on them stays, under this
 * entry's name (an incomplete witness, a cell that overlaps the code segment, an address at or above 2^40, a store into a boundary-cell alias, a hash call outside what a
 * proof states); a segment stays refused.  The format is 'ZKSR' version 1 with the mode in header word 9: the STARK part is zkir_prove's sections for the mode through the
 * quotient root (header with the four counter words, program, I/O section, touched cells, (mode 4) hash section and wide tape, ROM | range | memory multiplicities, three
 * roots), the embedded proof opens widths {264 | 288, 96 | 128, 4}.  The version number is kept on purpose: a verifier built before these modes refuses such a proof with
 * code 2.  zkir_verify_rate accepts modes 3 / 4 with zkir_verify's codes for the front (54 - 57 the cells and the tapes, 10, 5, 100 + c as above);
 * zkir_verify_rate_device runs a mode-4 proof's three tape stages on the device as zkir_verify_device does (zkir_verify_last_stages reports them) beside the query stage. */
int zkir_prove_rate_modes(zkir_stark_ctx* ctx, const zkir_trace_columns* trace, const zkir_public_inputs* pub, uint32_t num_queries, uint32_t pow_bits, uint32_t** proof_out,
                          uint64_t* proof_words, float* stage_ms, void* hip_stream);
int zkir_prove_rate(zkir_stark_ctx* ctx, const zkir_trace_columns* trace, const zkir_public_inputs* pub, uint32_t num_queries, uint32_t pow_bits, uint32_t** proof_out,
                    uint64_t* proof_words, float* stage_ms, void* hip_stream);
int zkir_verify_rate(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits);
int zkir_verify_rate_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, void* hip_stream);
/* A RUN PROVEN IN SEGMENTS AT THE CONTEXT'S OWN RATE (DESIGN.md "Run segments at blow-up 4 and 8"; INTEGRATION.md has the recipe).
 * zkir_prove_rate_segment: zkir_prove_rate's signature, stage_ms and format ('ZKSR' version 1, unchanged) for the K1 output of a ROW SHARD of a run, or of a whole run, in
 * mode 0, 1 or 2 on a context of log_blowup 1, 2 or 3.  The header's boundary states are the trace's first and last rows; in mode 2 the four counter words follow from
 * pub->writes_before / reads_before as zkir_prove forms them for a segment, and pub carries the WHOLE run's tapes, halt reason and io digest.  pub->n_real is the shard's
 * row count.  On a whole run (writes_before = reads_before = 0, first row the initial state) the words are zkir_prove_rate's exactly.  ZKIR_ERR_ARGUMENT with a message
 * that names this entry, before anything is launched, for modes 3 and 4 (the memory argument spans the run: zkir_prove refuses such segments too); zkir_prove_rate's other
 * refusals stay (num_queries 1 .. 128, pow_bits 0 .. 24, log_n against n_real, the public inputs).  zkir_prove_rate and zkir_prove_rate_modes keep refusing
 * writes_before / reads_before.  Not covered: segments in modes 3 / 4; zkir_prove_result_rate on a shard handle (zkir_prove_result refuses one too).
 * zkir_verify_rate_segment: host only.  zkir_verify_rate without check 7 — the same codes in the same order; a mode >= 3 proof is never a segment: 2.  On acceptance the
 * header's boundary states are written to first_state / last_state (68 words each; either may be NULL).
 * zkir_verify_rate_chain: host only.  zkir_verify_chain's meaning and codes for 'ZKSR' segments, through the same linking code: 40 an empty chain (or null arguments);
 * 1000 (i + 1) + c: segment i fails zkir_verify_rate_segment(.., NULL, min_queries, min_pow_bits) with code c (c <= 113); 41 the first state is not the VM's initial state;
 * 42 a segment does not start in the state its predecessor ends in; 43 a segment's mode, entry point or digests (header words 9 .. 20) or its num_queries, log_blowup or
 * pow_bits (words 4, 5, 6) are not segment 0's, or the chain is not `expect`'s run; 44 expect->n_real != sum (n_i - 1) + 1 (neighbours share a row); mode 2: 45, 46, 51,
 * 50, 52 / 53 over the I/O sections and the counters, as in zkir_verify_chain.  min_queries / min_pow_bits hold for every segment; expect->fri_params is not consulted.  A
 * chain of one mode >= 3 proof is zkir_verify_rate.  The segments' host fronts run segment after segment up to the first one that fails there, then ONE run of the query
 * stage over the collected segments' embedded proofs, then the verdict is resolved in segment order (per segment its code, then 43), the linking checks last.
 *
 * THE COMMITMENT LAYER'S QUERY STAGE FOR MANY PROOFS (zkir_amd/csrc/pcs_verify_many.inl).  The four *_device entries below run checks 7 - 11 of ALL their proofs' queries on
 * the current HIP device as one batch: the proofs may differ in log_n, log_blowup (so the final layer and the fold schedule), the number of matrices (1 .. 4) and their
 * widths, the points (0 .. 2), the masks and the number of queries — a per-proof shape record lies in device memory and a job finds its proof in a prefix table.  One
 * staged upload, two launches, one download of the flags and one synchronisation on hip_stream per call, however many proofs; nothing is launched where no proof reaches its
 * queries.  Only 'ZKBE' / 'ZKEV' / 'ZKLD' words and the stage's tables are uploaded: of a 'ZKSR' proof the embedded evaluation proof, never its program, cells or tapes.
 * Every extent a kernel reads is a function of header words the host has checked (a proof's length is checked EXACTLY before its queries), the row a job opens is the
 * transcript's sample.  The verdict is the host entry's for every input.  A NEGATIVE result is a device failure, not a verdict (zkir_last_error says which).  Calls on one
 * device are serialised inside.  zkir_verify_queries_last reports the calling thread's last stage run: hash jobs = sum_i nq_i (2 n_mats_i + n_layers_i), value jobs =
 * sum_i nq_i (2 + n_layers_i), launches 0 or 2, uploaded words.
 * zkir_verify_rate_segment_device: zkir_verify_rate_segment's verdict; a batch of one.
 * zkir_verify_rate_chain_device: zkir_verify_rate_chain's verdict for every input, all segments' queries as one stage run.  A chain of one mode >= 3 proof is
 * zkir_verify_rate_device.
 * zkir_verify_rate_many_device: n independent WHOLE-RUN 'ZKSR' proofs of any mode and rate, 1 <= n <= 1024 (else ZKIR_ERR_ARGUMENT, as for a null proofs, proof_words or
 * verdicts); expects, min_queries and min_pow_bits may be NULL (no expectation; 1; 0), and so may entries of expects.  Returns 0 with verdicts[i] = what
 * zkir_verify_rate(proofs[i], proof_words[i], expects[i], min_queries[i], min_pow_bits[i]) returns for every i, or an error (ZKIR_ERR_ARGUMENT, a negative value) with NO
 * verdict written.  A mode-4 proof's tape stages run on the device as in zkir_verify_rate_device, proof after proof, before the shared query stage.
 * zkir_pcs_verify_many_device: n stand-alone proofs of the commitment layer, 1 <= n <= 1024; kinds[i] = 0 'ZKLD', 1 'ZKEV', 2 'ZKBE' (anything else: ZKIR_ERR_ARGUMENT);
 * expect_roots / expect_points / expect_evals may be NULL and so may their entries (sized as the proof's header states, as in the single entries).  Returns 0 with
 * verdicts[i] = what zkir_lowdeg_verify / zkir_eval_verify / zkir_batch_eval_verify answers, or an error with NO verdict written. */
int zkir_prove_rate_segment(zkir_stark_ctx* ctx, const zkir_trace_columns* trace, const zkir_public_inputs* pub, uint32_t num_queries, uint32_t pow_bits, uint32_t** proof_out,
                            uint64_t* proof_words, float* stage_ms, void* hip_stream);
int zkir_verify_rate_segment(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, uint32_t first_state[68],
                             uint32_t last_state[68]);
int zkir_verify_rate_chain(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries,
                           uint32_t min_pow_bits);
int zkir_verify_rate_segment_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits,
                                    uint32_t first_state[68], uint32_t last_state[68], void* hip_stream);
int zkir_verify_rate_chain_device(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect, uint32_t min_queries,
                                  uint32_t min_pow_bits, void* hip_stream);
int zkir_verify_rate_many_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                 const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* hip_stream);
int zkir_pcs_verify_many_device(const uint32_t* kinds, const uint32_t* const* proofs, const uint64_t* proof_words, const uint32_t* const* expect_roots,
                                const uint32_t* const* expect_points, const uint32_t* const* expect_evals, uint32_t n, int32_t* verdicts, void* hip_stream);
/* diagnostics of the calling thread's last zkir_verify* call: host wall time in ms of [0] parsing (the tapes' record checks among it), [1] the sections' chunk digests,
 * [2] the hash tape's share of the table side, [3] the wide tape's, [4] the rest; *device_stages = how many of these stages ran on the device (0 for every host entry).
 * Either pointer may be NULL.  ZKIR_ERR_ARGUMENT before the thread's first verification.  ZKIR_VERIFY_TIMES in the environment prints the clocks on stderr. */
int zkir_verify_last_stages(double ms[5], uint32_t* device_stages);
/* ---- (modes 3 / 4) the TOUCHED-CELL section's three stages on the current HIP device --------------------------------------------------------------------------------
 * The section is [n] + 7 n words: per cell [address limb 0 (20 bits, a multiple of 8)] [limb 1 (20 bits)] [time of the last access] [final bytes: four 16-bit pieces].
 * Linear in it are (a) the cell checks 54 / 55 (and 4: the proof ends inside the section), (b) its chunk digests in the transcript, (c) its share of the lookup table
 * side: per cell + 1 / (alpha - fp(cell, 0, the program image's bytes)) - 1 / (alpha - fp(cell, t_last, final bytes)).  zkir_verify and EVERY entry above run them on the
 * host, unchanged; the two entries below run them as kernels (csrc/mem_stage.inl), one upload of the section and the program image, three launches, a synchronisation
 * where each result is needed — the same verdict as the host entry on every input, well-formed or not.  An empty section touches no device memory, and a section
 * below 512 cells stays with the host stages (the measured crossover: profiles/r24_verify_memory_device.txt); ZKIR_VERIFY_DEVICE_MIN_CELLS in the environment sets
 * another threshold (0: every non-empty section on the device), for measuring the routes against each other.
 * zkir_verify_last_stages' device_stages counts the memory stages beside the tape stages: 3 for a non-empty section.
 * zkir_verify_many_on_device / zkir_verify_rate_many_device keep their mode-3 / mode-4 fronts' memory sections on the host; the *_many_memory_device entries below are
 * their forms with the sections of ALL proofs as one device batch. */
/* zkir_verify's verdict; the memory section's three stages and a mode-4 proof's tape stages on the device;
   queries != 0: the query stage too (zkir_verify_on_device's). Modes 0-2: the existing entry's behaviour. */
int zkir_verify_memory_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, int queries, void* hip_stream);
/* zkir_verify_rate_device with the memory stages on the device */
int zkir_verify_rate_memory_device(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t min_queries, uint32_t min_pow_bits, void* hip_stream);
/* MANY PROOFS, ONE BATCH (csrc/mem_stage_many.inl).  zkir_verify_many_on_device / zkir_verify_rate_many_device with the memory sections of all their mode-3 / mode-4
 * proofs verified together: every section is uploaded once and checked and hashed by ONE launch each before any front runs; the fronts then run on the host, proof
 * after proof, and DEFER check 10 (the only reader of the cells' share of the table side, on which no challenge, grinding or sample depends); behind the last front ONE
 * launch forms every deferred proof's share, the host completes the kept checks, and a proof whose deferred check fails has verdict 10 whatever its front answered
 * afterwards.  Three launches and two synchronisations for the memory stages of the whole call; a mode-4 proof's tape stages run per proof behind the batch region; the
 * queries are the existing batched stage.  n = 1 .. 1024, modes 0 - 4 mixed; verdicts[i] is zkir_verify's / zkir_verify_rate's on every input.  The batch goes to the
 * device when the TOTAL cells of its sections reach the threshold above (ZKIR_VERIFY_DEVICE_MIN_CELLS overrides it); below it every front runs the inline host code.
 * zkir_verify_memory_last then reports the batch: the cells of all sections that went up, launches = 3 (2 when no front deferred, 0 when the batch stayed on the
 * host) and the uploaded words.  Returns ZKIR_OK, ZKIR_ERR_ARGUMENT, or a negative value: no verdict for any proof. */
int zkir_verify_many_memory_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* hip_stream);
int zkir_verify_rate_many_memory_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                        const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* hip_stream);
/* this thread's last verification: cells whose stages ran on the device, launches, words uploaded for them (all 0 after any other entry) */
int zkir_verify_memory_last(uint64_t* cells, uint32_t* launches, uint64_t* uploaded_words);
/* MANY MODE-4 PROOFS' TAPES, ONE BATCH (csrc/tape_stage_many.inl).  The *_many_memory_device entries PLUS the hash and wide tapes of all their mode-4 proofs verified
 * together, around the same pass of fronts and the same query stage.  Before any front: one upload of every located tape, ONE launch each for the hash record checks, the
 * wide record checks and both sections' chunk digests, one synchronisation; the bytes every hash call wrote are then formed by two launches that overlap the host fronts.
 * A front whose tape checks were answered by the batch DEFERS check 10 exactly as it does for its cells (the tapes' shares of the table side enter nothing else); behind
 * the last front two side launches (and one patch launch where a call is longer than 1024 bytes) serve every deferred proof, and the kept check is evaluated with the sum
 * of all deferred shares: cells, hash calls, wide records.  At most 8 launches and 2 synchronisations for the tapes of the whole call, however many proofs.  n = 1 .. 1024,
 * modes 0 - 4 mixed; verdicts[i] is zkir_verify's / zkir_verify_rate's on every input.  The tape batch goes to the device when the located tapes' records (hash calls plus
 * wide records) in all reach ZKIR_VERIFY_DEVICE_MIN_RECORDS (default 0: every batch that holds a record); below it every mode-4 front keeps its own tape stages, as in the
 * *_many_memory_device entries.  zkir_verify_tapes_last then reports the batch: its records, launches (0 when the batch stayed with the fronts) and uploaded words; it is
 * all 0 after every other entry.  Returns ZKIR_OK, ZKIR_ERR_ARGUMENT, or a negative value: no verdict for any proof. */
int zkir_verify_many_tapes_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, uint32_t n, int32_t* verdicts, void* hip_stream);
int zkir_verify_rate_many_tapes_device(const uint32_t* const* proofs, const uint64_t* proof_words, const zkir_public_inputs* const* expects, const uint32_t* min_queries,
                                       const uint32_t* min_pow_bits, uint32_t n, int32_t* verdicts, void* hip_stream);
int zkir_verify_tapes_last(uint64_t* records, uint32_t* launches, uint64_t* uploaded_words);
/* the stages on their own, as zkir_hash_tape_check_* and zkir_tape_table_side_* are: sec = [n] + 7 n words (host).
 * _check_*: *verdict = 0 / 4 (n_words < 1 + 7 n) / 54 / 55 — of the LOWEST failing cell, and within it the first failing check in the host's order (limb ranges, byte
 * pieces, strictly increasing address, overlap with the code_words code words at 0x1000; mode 4 admits the boundary cell of an odd code_words); a malformed section is a
 * verdict and ZKIR_OK, not a refusal.  _table_side_*: n_words == 1 + 7 n and cells that pass check 54 (else ZKIR_ERR_ARGUMENT); blob: the program (its image bytes; a
 * blob shorter than 32 bytes, or than its header claims, has an all-zero image); alpha, lambda and sum canonical.  _host: verify.cpp's code, no HIP call. */
int zkir_mem_section_check_host  (const uint32_t* sec, uint64_t n_words, uint32_t mode, uint64_t code_words, int32_t* verdict);
int zkir_mem_section_check_launch(const uint32_t* sec, uint64_t n_words, uint32_t mode, uint64_t code_words, int32_t* verdict, void* hip_stream);
int zkir_mem_table_side_host  (const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], uint32_t sum[4]);
int zkir_mem_table_side_launch(const uint32_t* sec, uint64_t n_words, const uint8_t* blob, size_t blob_len, const uint32_t alpha[4], const uint32_t lambda[4], uint32_t sum[4], void* hip_stream);
/* points pub's mode-3 fields at the witness (which must outlive the proving call) and sets pub->deferred = 3 */
void zkir_public_inputs_set_memory(zkir_public_inputs* pub, const zkir_memcheck_witness* w);
/* Poseidon2 sponge digest of a byte string (host): [len as four 16-bit pieces] ++ [LE 16-bit halfwords] */
void zkir_digest_bytes(const uint8_t* bytes, size_t len, uint32_t out[4]);
/* the public inputs of a finished run (host; `log`: the run's delta log, a shard of it, or the trace window that reached the run's
 * halt — anything whose cycles / outputs / halt reason are the finished run's; a window with zkir_delta_log_window_open() is refused) */
int zkir_public_inputs_of(const zkir_delta_log* log, const uint8_t* program_blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs,
                          uint32_t deferred, zkir_public_inputs* out);

/* The prover's parameters (zkir_prover_params).  mode: the proof's mode, the same value as zkir_public_inputs.deferred (0 default VM mode, 1 deferred carry model, 2 default +
 * the I/O argument, 3 = 2 + the memory argument).  num_queries / pow_bits: FRI queries and grinding bits, 0 = the defaults (50, 12); accepted: 50..128 queries, 12..24 bits (a
 * proof may say more than the defaults, never less).  Conjectured FRI soundness at blow-up 2 is one bit per query + the grinding bits: 50 + 12 = 62, 84 + 16 = 100 — the
 * capacity-4 Poseidon2 sponge (rate 8, digests of 4 x 31 bits) caps collision resistance at ~62 bits whatever these say (README: a demonstrator instance). */
typedef struct zkir_result zkir_result;   /* the drop-in layer's handle (zkir_exec, below) */
typedef struct zkir_prover_params {
  uint32_t mode;
  uint32_t num_queries;
  uint32_t pow_bits;
} zkir_prover_params;
/* validates `params` (ZKIR_ERR_ARGUMENT otherwise: the ranges above; params->mode must be pub->deferred) and records the FRI parameters in pub->fri_params */
int zkir_public_inputs_set_params(zkir_public_inputs* pub, const zkir_prover_params* params);

/* Full proof of the execution whose K1 output is `trace` (pub->n_real rows; ctx built for zkir_padded_log_n(pub->n_real)).  *proof_out is a
 * malloc'ed array of u32 words (little-endian canonical field elements; format v10 in modes 0 / 1, v11 in modes 2 / 3 — zkir_proof_version_of_mode; layout in oracle/stark_oracle.cpp so::prove),
 * pub->program_blob must be the program that ran: every row's (pc, instruction word) is looked up in its code table, and a run that executes
 * anything else (self-modified code, a pc outside the code segment) is refused with ZKIR_ERR_ARGUMENT — it has no proof in this AIR.
 * released with zkir_proof_free.  stage_ms (NINE floats, nullable): main trace, LDE, trace Merkle, lookup argument (aux trace + its LDE and tree), quotient, openings, DEEP, FRI, queries.
 * The trace may be that of a whole run or of a SEGMENT of one (the K1 output of a row shard, zkir_delta_log_shard(log, a, b) with
 * cycle_base = a): the proof header records the 68-word state (cycle, pc limbs, register limbs, storage states) of the first and of
 * the last row and the AIR pins those rows to it; pub->n_real is then the segment's row count, pub->io_digest the RUN's. */
int zkir_prove(const zkir_stark_ctx* ctx, const zkir_trace_columns* trace, const zkir_public_inputs* pub, uint32_t** proof_out, uint64_t* proof_words,
               float* stage_ms, void* hip_stream);
void zkir_proof_free(uint32_t* proof);
/* SURVEY 8(b)'s shape of the call: the WHOLE-RUN handle of zkir_exec in (enable_execution_trace), the proof out as bytes (the little-endian u32 words of zkir_prove; free with
 * zkir_proof_bytes_free).  params may be NULL (mode 0, 50 queries, 12 bits).  Makes and frees a context for the run's size: a caller proving many runs keeps one and uses zkir_prove. */
int zkir_prove_result(const zkir_result* result, const zkir_prover_params* params, uint8_t** proof, size_t* proof_len);
/* The same at log_blowup 1, 2 or 3: a context of that rate and zkir_prove_rate_modes — a 'ZKSR' proof (any mode; verify with zkir_verify_rate).  params->num_queries 0 means
 * 50 / 25 / 17 by rate, params->pow_bits 0 means 12; otherwise the rate entry's ranges (1 .. 128 queries, 0 .. 24 bits).  params may be NULL (mode 0). */
int zkir_prove_result_rate(const zkir_result* result, const zkir_prover_params* params, uint32_t log_blowup, uint8_t** proof, size_t* proof_len);
void zkir_proof_bytes_free(uint8_t* proof);
uint32_t zkir_proof_num_queries(void);            /* the default (50) */
uint32_t zkir_proof_version(void);                /* of modes 0 / 1 (10) */
uint32_t zkir_proof_version_of_mode(uint32_t mode);   /* modes 2 / 3: 11 (round 5: EBREAK is a class of its own, the I/O section is in the transcript, mode 3 refuses accesses to the code segment); mode 4: 12 (round 6) */
/* Verifier of the proof of a WHOLE run (host only, no device): 0 = accepted, otherwise the number of the failed check (1-5
 * malformed, 6 public inputs differ from `expect`, 7 the run does not start in the VM's initial state (cycle 0, entry point, zero
 * registers), 8 the program carried in the proof is malformed or is not the one program_digest / entry_point name, 10 constraints at
 * zeta (incl. the lookup argument: the verifier computes the table side from that program and the multiplicities in the proof), 11 final
 * codeword degree, 12 grinding, 20-27 query / Merkle / FRI checks, 30 length; modes 2 / 3 also 50-53 = zkir_verify_io's checks on the tapes the proof carries, 51 the
 * counters' ends; mode 3 also 54 = the touched cells are not canonical 8-byte cell addresses in strictly increasing order; a mode-3 proof is never a segment: 2;
 * modes 3 / 4 also 55 = a touched cell / a hash call's output overlaps the code segment (mode 4 admits the boundary cell); mode 4 also 56 = a malformed hash-tape record
 * (ranges, order, cell count, a previous access that is not before the call, a SHA-256 output pointer that is not a multiple of 4), 57 = a malformed wide-tape record (a limb out of range, not an opcode 3..7, a zero divisor, cycles
 * not increasing); a tape whose records are well-formed but are not the run's fails the lookup argument (10)).
 * expect may be NULL: the header's own public inputs are then only checked for internal consistency.
 * The queries (independent, ~10,000 Poseidon2 permutations of Merkle paths at 2^20 rows) are checked on up to eight host threads (half the logical cores; ZKIR_VERIFY_THREADS=n
 * overrides); the verdict is the first failing query's in query order, as a sequential check would give. */
int zkir_verify(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect);
/* A run proven in SEGMENTS (multi-GPU: one row shard per device; consecutive segments overlap by one row — the last row of segment i,
 * labelled "halt" there, is row 0 of segment i + 1).  zkir_verify_segment: the same checks without check 7; first_state / last_state
 * (68 words each, nullable) receive the header's boundary states.  zkir_verify_chain: every segment verifies, the first starts in the
 * initial state, each later one starts in exactly the state its predecessor ended in (the cycle counter is part of the state), mode /
 * entry point / program digest / io digest agree; expect (nullable) = the RUN's public inputs, n_real = its total rows
 * = sum(n_i - 1) + 1.  0 = accepted; 40 empty, 41 first state, 42 link, 43 public inputs, 44 row count; 1000 (i + 1) + c = check c
 * of segment i. */
int zkir_verify_segment(const uint32_t* proof, uint64_t proof_words, const zkir_public_inputs* expect, uint32_t first_state[68], uint32_t last_state[68]);
int zkir_verify_chain(const uint32_t* const* proofs, const uint64_t* proof_words, uint32_t n_segments, const zkir_public_inputs* expect);
/* The run's CLAIM in the clear on top of zkir_verify / zkir_verify_chain (round 4): the I/O tapes and the halt reason (ZKIR_HALT_*, exit code) must hash to the proof's io
 * digest together with the proof's row count (else 50), and the HALT ROW — the last executed row, pinned to the public last state by the AIR — must be the instruction the
 * halt reason names, looked up in the program the proof carries: EBREAK for an Ebreak halt, ECALL reading R10 = 0 and R11 = the exit code for Exit(code) (52: another
 * instruction; 53: another syscall / exit code) — vm.rs:302-347, syscall.rs:101-107.  CycleLimit names no instruction.  The outputs themselves stay unproven (air.h). */
int zkir_verify_io(const uint32_t* proof, uint64_t words, const zkir_public_inputs* expect, const uint64_t* inputs, size_t n_inputs, const uint64_t* outputs, size_t n_outputs,
                   int halt_kind, uint64_t halt_code);
int zkir_verify_chain_io(const uint32_t* const* proofs, const uint64_t* words, uint32_t n_segments, const zkir_public_inputs* expect, const uint64_t* inputs, size_t n_inputs,
                         const uint64_t* outputs, size_t n_outputs, int halt_kind, uint64_t halt_code);
uint32_t zkir_proof_state_words(void);
/* Host-side Poseidon2-12 permutation of the transcript (canonical words in and out; no device needed): what a verifier or an
 * integrator re-deriving the Fiat-Shamir challenges calls.  Same code as the device kernels (poseidon2.h), compiled for the host. */
void zkir_poseidon2_permute(uint32_t state[12]);
/* The same permutation in the formulation the hash kernels run (scaled state words, poseidon2.h: permute_scaled), host build:
 * `rounds` chained applications, canonical words in and out.  Exists so that the formulation can be checked without a device. */
void zkir_poseidon2_permute_scaled(uint32_t state[12], uint32_t rounds);

/* ---- drop-in layer: VM::new + VM::run --------------------------------------------------------- */
/* (zkir_result: the opaque handle declared above with zkir_prove_result; owns host metadata + device columns) */

/* program_blob is Program::to_bytes() (program.rs:300-315).  On success the trace columns are resident
 * on the current HIP device.  Fails with ZKIR_ERR_DEVICE if no GPU is usable (no CPU fallback). */
int zkir_exec(const uint8_t* program_blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs,
              const zkir_vm_config* cfg, zkir_result** out);
/* The same call for ONE GPU'S SHARE of a run: rows [0, row_begin) are executed untraced on the calling thread, rows [row_begin,
 * row_end) are traced, uploaded and filled on the current device while the interpreter runs (zkir_interpret_window + the streaming
 * of zkir_exec).  The handle's trace columns hold absolute cycles; zkir_result_delta_log(r): cycle_base = row_begin. */
int zkir_exec_window(const uint8_t* program_blob, size_t blob_len, const uint64_t* inputs, size_t n_inputs, const zkir_vm_config* cfg,
                     uint64_t row_begin, uint64_t row_end, zkir_result** out);
/* The same handle for a ROW SHARD of a finished interpretation (zkir_interpret): rows [row_begin, row_end) of `log` are cut out
 * (zkir_delta_log_shard), uploaded to the CURRENT HIP device and filled there.  Multi-GPU: one call per device, each with its row range
 * (hipSetDevice / one process per GPU); segment proofs: ranges that share one row.  The result owns the shard (zkir_result_delta_log:
 * cycle_base = row_begin); trace columns hold absolute cycles; the witness accessors describe the shard's rows. */
int zkir_exec_shard(const zkir_delta_log* log, uint64_t row_begin, uint64_t row_end, zkir_result** out);
void zkir_result_free(zkir_result* r);
const zkir_delta_log* zkir_result_delta_log(const zkir_result* r);       /* host-side metadata */
const zkir_trace_columns* zkir_result_trace(const zkir_result* r);       /* device pointers */
/* wall-clock breakdown of the zkir_exec call that produced r (ms): host interpretation | device allocation | H2D of the delta log |
 * K1 launch + synchronisation */
void zkir_result_stage_ms(const zkir_result* r, float out[4]);
/* copy one device column to host: field = 0 cycle,1 pc,2 instruction,3 registers,4 bound_bits,5 bound_tag,
 * 6 bound_payload,7 reg_state; reg ignored for fields 0-2.  dst must hold n_rows elements. */
int zkir_result_copy_column(const zkir_result* r, int field, int reg, void* dst);


/* ---- the rest of ExecutionResult (vm.rs:54-103) behind the handle: witness streams as DEVICE columns ---------------------------
 * Each call expands the corresponding side log of the run on the device the first time it is made (witness.hip kernels), caches
 * the columns in the handle and returns the same pointers afterwards; they stay valid until zkir_result_free.  Thread-safe. */
typedef struct zkir_memory_witness {     /* TraceRow.memory_ops of every row + ExecutionResult::get_memory_trace() (vm.rs:85-94) */
  uint64_t n_ops;                        /* = ExecutionResult::memory_op_count() (vm.rs:97-102) */
  uint64_t n_rows;
  zkir_memop_columns row_order;          /* ops in execution order; row r owns ops [row_offsets[r], row_offsets[r+1]) */
  const uint64_t* row_offsets;           /* device, [n_rows+1] */
  zkir_memop_columns sorted;             /* stable order by (timestamp, address, Read<Write): trace.rs:210-223 */
} zkir_memory_witness;
int zkir_result_memory_trace(zkir_result* r, zkir_memory_witness* out);

typedef struct zkir_range_check_witness { /* ExecutionResult.range_check_witnesses: Vec<RangeCheckWitness> (range_check.rs:209-238) */
  uint64_t n_checks;                     /* total checks over all witnesses */
  uint64_t n_witnesses;                  /* non-empty checkpoints (vm.rs:340-342) */
  const uint64_t* witness_offsets;       /* HOST, [n_witnesses+1]: witness k owns checks [off[k], off[k+1]) */
  const uint64_t* witness_cycles;        /* HOST, [n_witnesses]: cycle of the checkpoint */
  const uint64_t* value;                 /* device [n_checks] */
  const uint64_t* pc;                    /* device [n_checks] */
  const uint16_t* chunks;                /* device [4][chunk_stride]: chunk c of check i at chunks[c*chunk_stride + i] (range_check.rs:175-192) */
  uint64_t chunk_stride;
  uint32_t chunk_bits;
  const uint32_t* multiplicity;          /* device [2^chunk_bits]: lookup multiplicities of all chunks */
} zkir_range_check_witness;
int zkir_result_range_check_witnesses(zkir_result* r, zkir_range_check_witness* out);

typedef struct zkir_normalization_witness { /* ExecutionResult.normalization_witnesses (normalization_witness.rs:129-138) */
  uint64_t n_events;
  zkir_norm_columns columns;             /* device */
} zkir_normalization_witness;
int zkir_result_normalization_witnesses(zkir_result* r, zkir_normalization_witness* out);

typedef struct zkir_sha256_witness {     /* Sha256Witness per single-block SHA-256 syscall (trace.rs:236-285); never reached from VM::run in the
                                            reference (syscall.rs:127 passes None) — BASELINE configs[4]'s "syscall-chip trace columns" */
  uint64_t n_blocks;
  const uint32_t* columns;               /* device [608][stride], layout of zkir_sha256_chip_launch */
  uint64_t stride;
  const uint64_t* timestamps;            /* device [n_blocks] */
} zkir_sha256_witness;
int zkir_result_sha256_witnesses(zkir_result* r, zkir_sha256_witness* out);

/* D2H copy for hosts that do not link a HIP runtime themselves (the pointers above are device memory) */
int zkir_device_to_host(void* host_dst, const void* device_src, size_t bytes);
/* H2D copy of a host-side log array (zkir_delta_log_* pointers) into caller-owned device memory, ordered on `hip_stream`: the copy
 * path of zkir_exec for callers that drive the stages themselves */
int zkir_host_to_device(void* device_dst, const void* host_src, size_t bytes, void* hip_stream);

const char* zkir_last_error(void);
/* The ABI revision of this header: bumped whenever a struct layout, a buffer size or a signature of an EXISTING entry point changes (new entry points alone do not bump it).
 *   4: zkir_prove's stage_ms is NINE floats (round 4 added the lookup stage: a caller built against eight overflows by 4 bytes)
 *   5: zkir_public_inputs.reserved became fri_params (same offset; zero = the old behaviour); zkir_verify* compare the proof's FRI parameters with `expect`'s
 * A binding checks zkir_abi_version() == ZKIR_AMD_ABI_VERSION when it loads the library. */
#define ZKIR_AMD_ABI_VERSION 7u   /* 6 (round 6): zkir_public_inputs grew (hash_section), mode 4 entry points, pinned log blocks; 7: zkir_public_inputs grew at its end (hash_outs, n_hash_outs) */
uint32_t zkir_abi_version(void);
const char* zkir_version(void);

#ifdef __cplusplus
}
#endif
#endif /* ZKIR_AMD_H */

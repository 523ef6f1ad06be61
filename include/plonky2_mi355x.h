/*
 * plonky2_mi355x.h -- C ABI of libplonky2_mi355x.so, the MI355X (gfx950) backend for the prove() hot path
 * of the Plonky2 matrix-multiplication demo circuit.
 *
 * The reference (Lain-Iwakuro/Plonky2-Demo, a plonky2 fork) has no FFI seam; this header cuts one at the
 * `PolynomialBatch` type (plonky2/src/fri/oracle.rs:30-37) and at the prover-side consumers that reach
 * into it (plonky2/src/plonk/prover.rs:102-329).  Every entry point names the reference interface it
 * replaces.  INTEGRATION.md shows the Rust `extern "C"` block and the patch to the call sites.
 *
 * Conventions
 *  - A field element is a little-endian uint64_t, layout-compatible with `#[repr(transparent)]
 *    GoldilocksField(pub u64)` (field/src/goldilocks_field.rs:23-25).  Inputs may be non-canonical
 *    (any u64); every output is canonical (< p = 2^64 - 2^32 + 1).
 *  - An extension element (F_p[X]/(X^2-7)) is two consecutive uint64_t: (a0, a1)
 *    (field/src/extension/quadratic.rs:14).  A digest (HashOut) is four uint64_t
 *    (plonky2/src/hash/hash_types.rs:20-24).
 *  - `hasher` selects the reference's `C::Hasher` (plonk/config.rs:95-118): GL_HASHER_POSEIDON = PoseidonGoldilocksConfig, the default
 *    of every entry point without the argument, or GL_HASHER_KECCAK = KeccakGoldilocksConfig (Hasher = KeccakHash<25>, hash/keccak.rs;
 *    InnerHasher stays Poseidon).  A BytesHash<25> (hash_types.rs:156-192) travels in the same four-uint64_t slot as a HashOut: its 25
 *    bytes little-endian in words 0..3, the top 7 bytes of word 3 zero; an input slot whose padding bytes are not zero is GL_ERR_ARG
 *    (verifier: "malformed").  On the wire such a hash is 25 bytes (util/serialization/mod.rs:248-256), so caps, Merkle-proof siblings
 *    and VerifierOnlyCircuitData are 7 bytes per hash shorter than under Poseidon.  Entry points that take a hasher of their own carry
 *    the suffix _h; handles (gl_merkle, gl_batch, gl_circuit, gl_fri, gl_challenger) remember theirs, and mixing them is GL_ERR_ARG.
 *  - `h_` pointers are host memory owned by the caller; `d_` pointers are device (HIP) memory on the
 *    context's device.  Opaque handles own device memory and are released with their *_free.
 *  - Footprint of a `d_` argument, stated at every entry point in one of three words: READ-ONLY (no word of it is written),
 *    OUTPUT (every word of the documented shape is written, whatever it held, and no word outside it), IN PLACE (the words named
 *    are overwritten, every other word of the buffer keeps its value).  Scratch comes from the context's own pool, never from the caller's
 *    buffers.  tests/test_footprint.py holds every entry to this with guard bands around the caller's buffers.
 *  - Alignment: the kernels read and write a caller's device buffer one 64-bit word at a time (one 32-bit field at a time for
 *    gl_memory_op), so a `d_` pointer needs the alignment of its element type and no more: 8 bytes for uint64_t data -- extension
 *    pairs, digests, 12-word states and matrix columns included -- and 4 bytes for gl_memory_op.  No entry asks for the 256 bytes
 *    hipMalloc gives, and a column or row may start at any word of an allocation.
 *  - All functions return GL_OK (0) or a GL_ERR_* code and never unwind; gl_last_error() gives the
 *    text for the calling thread.  The reference panics on shape errors (oracle.rs:114,
 *    merkle_tree.rs:137-143, fft.rs:175-181); here they are GL_ERR_ARG.  A C++ exception inside the
 *    library (in practice std::bad_alloc: out of host memory; std::system_error: a thread could not be
 *    started) is caught at the entry point and becomes GL_ERR_INTERNAL with its text in gl_last_error();
 *    gl_challenger_new / gl_challenger_new_h return NULL for it, with the last error set.  The functions
 *    marked GL_NOEXCEPT (the *_free functions and the plain getters) contain nothing that can throw.  After
 *    such an error every out-handle is NULL, nothing is leaked, and the handles passed in stay usable or freeable.
 *  - A gl_ctx is bound to one device and one HIP stream; calls on one ctx are issued in order on that
 *    stream.  Different ctxs may be used concurrently from different threads; ONE ctx runs one computing call at a
 *    time.  The plain copies out of a handle -- gl_batch_cap / gl_batch_coeffs / gl_batch_lde, gl_merkle_cap,
 *    gl_circuit_digest / gl_circuit_constants_sigmas_cap -- go through the context the handle was created on and MAY be
 *    called from any thread while that context is computing on another (a verifier thread reads the cap of a circuit that
 *    is proving); the getters that gather on the device first (get_leaf, prove, get_lde_values) count as computing calls.
 *  - Lifetime: every handle created on a context (gl_batch, gl_merkle, gl_circuit, gl_fri, gl_matmul_witgen) holds a
 *    reference to it.  gl_ctx_destroy() drops the creator's reference: after it the gl_ctx pointer must not be passed to
 *    any entry point again, but handles created earlier stay valid (they keep the stream, tables and allocator alive)
 *    and may be used and freed afterwards IN ANY ORDER; the context is torn down when the last of them is freed.  A
 *    binding may therefore give every handle a plain destructor (Rust `Drop`) without ordering them.  A gl_batch passed
 *    to gl_fri_combine, and the gl_host_circuit passed to gl_matmul_witgen_create / gl_prover_pool_create, are
 *    borrowed and must outlive the borrower.  Memory from gl_dev_alloc is not tied to the context (gl_dev_free accepts a
 *    null ctx).
 *  - There is NO CPU fallback: without a HIP device every compute entry point fails with GL_ERR_HIP.
 */
#ifndef PLONKY2_MI355X_H
#define PLONKY2_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#define GL_NOEXCEPT noexcept  /* the *_free functions and plain getters: nothing in them can throw */
#else
#define GL_NOEXCEPT
#endif

#define GL_OK 0
#define GL_ERR_ARG 1          /* bad shape / null pointer / unsupported size          */
#define GL_ERR_HIP 2          /* HIP runtime error (no device, OOM, launch failure)   */
#define GL_ERR_UNSUPPORTED 3  /* e.g. gl_batch_from_values with blinding != 0 (use the _blinded entries), zk with lookups */
#define GL_ERR_ZETA_IN_SUBGROUP 4 /* prover.rs:280-283: opening point lies in H       */
#define GL_ERR_INTERNAL 5
#define GL_ERR_VERIFY 6       /* gl_verify: the proof is rejected (gl_last_error says which check failed) */

#define GL_HASHER_POSEIDON 0u /* PoseidonGoldilocksConfig (plonk/config.rs:95-105)  */
#define GL_HASHER_KECCAK 1u   /* KeccakGoldilocksConfig (plonk/config.rs:107-118)   */

typedef struct gl_ctx gl_ctx;
typedef struct gl_batch gl_batch;      /* device-resident PolynomialBatch (fri/oracle.rs:30-37)  */
typedef struct gl_merkle gl_merkle;    /* device-resident MerkleTree (hash/merkle_tree.rs:39-55) */
typedef struct gl_host_circuit gl_host_circuit;   /* host-only circuit description + witness recipe        */
typedef struct gl_circuit gl_circuit;  /* device-resident prover data (ProverOnlyCircuitData + CommonCircuitData) */
typedef struct gl_proof gl_proof;      /* ProofWithPublicInputs + the prover's intermediate values              */

/* What prove() needs from CommonCircuitData / ProverOnlyCircuitData (plonky2/src/plonk/circuit_data.rs:240-330,
 * 380-440) besides the constants/sigma value columns.  Gate types: 0 Noop, 1 Constant, 2 PublicInput,
 * 3 Arithmetic(20 ops), 4 Poseidon -- the gate set of the matmul demo circuit -- and 5 BaseSumGate<2> with the 63 limbs
 * of BaseSumGate::new_from_config (gates/base_sum.rs:31-35; range_check / split_le), 6 LookupGate and 7 LookupTableGate
 * (the lookup argument, several tables: fields at the end of this struct; phase API: the *_lookups variants), 8 ExponentiationGate
 * with the 66 power bits of new_from_config (gates/exponentiation.rs:43-53; CircuitBuilder::exp), 9 RandomAccessGate::new_from_config
 * (gates/random_access.rs:55-72; CircuitBuilder::random_access, Merkle caps) with its index bits (1..6) in `gate_params`, and the four
 * extension-field arithmetic gates (two adjacent wires = one element of F_p[X]/(X^2 - 7)), each in its new_from_config layout under
 * standard_recursion_config only, `gate_params` 0, parity unpinned against a Rust proof like every gate above the demo's five:
 *   10 ArithmeticExtensionGate (gates/arithmetic_extension.rs:35-51,150-164): num_ops = 80 / 8 = 10; op i owns wires 8i .. 8i+8 = m0, m1,
 *      addend, output; 20 constraints, the components of output - (c0 m0 m1 + c1 addend); 2 constants; degree 3
 *   11 MulExtensionGate (gates/multiplication_extension.rs:35-48,137-151): num_ops = 80 / 6 = 13; op i owns wires 6i .. 6i+6 = m0, m1,
 *      output; 26 constraints output - c0 m0 m1; 1 constant; degree 3
 *   12 ReducingGate (gates/reducing.rs:29-55,163-177): num_coeffs = min(80 - 6, (135 - 4) / 3) = 43; wires 0-1 output, 2-3 alpha, 4-5
 *      old_acc, 6..48 base-field coefficients, accumulator i at 49 + 2i for i < 42, the last accumulator IS the output; 86 constraints
 *      acc_(i-1) alpha + coeff_i - acc_i with acc_(-1) = old_acc; no constants; degree 2
 *   13 ReducingExtensionGate (gates/reducing_extension.rs:29-58,163-177): num_coeffs = min((80 - 6) / 2, (135 - 4) / 4) = 32; coefficient
 *      i at 6 + 2i (extension elements), accumulator i at 70 + 2i for i < 31, the last accumulator is the output; 64 constraints; degree 2
 * (CircuitBuilder::arithmetic_extension / mul_extension, ReducingFactorTarget::reduce*).  gl_common_data_to_bytes / _from_bytes refuse
 * (GL_ERR_UNSUPPORTED) a gate list that is not in build()'s order (degree, then id: circuit_builder.rs:987).  `gate_types` is the list
 * `common_data.gates` (sorted by degree, id) and the group arrays are `selectors_info`
 * (plonky2/src/gates/selectors.rs:17-26).
 * This comment describes; the library itself reads every one of these facts (code, id() name, serialisation tag and parameter words,
 * degree, number of constraints, quotient launch) from ONE table, GATE_TABLE in plonky2_demo_amd/csrc/gates.hpp.  A new gate type is a
 * row there, its constraints for the prover (prover_kernels.cuh) and for the verifier (gate_constraints_at, verifier.hip), a line
 * here and its name in plonky2_demo_amd/_lib.py (and in GL_GATE_LIST beside the table). */
typedef struct gl_circuit_desc {
    uint32_t degree_bits;              /* log2 of the trace length n                                */
    uint32_t num_wires;                /* 135                                                       */
    uint32_t num_routed_wires;         /* 80                                                        */
    uint32_t num_constants;            /* selector columns + gate-constant columns (4)              */
    uint32_t num_selectors;            /* 2                                                         */
    uint32_t num_challenges;           /* 2                                                         */
    uint32_t quotient_degree_factor;   /* 8                                                         */
    uint32_t rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t num_fri_rounds;           /* reduction_arity_bits.len()                                */
    uint32_t fri_arity_bits[8];
    uint32_t num_public_inputs;
    uint32_t num_gates;                /* <= GL_MAX_GATES                                           */
    uint8_t gate_types[16];
    uint8_t gate_params[16];           /* LookupGate / LookupTableGate: the gate's table (index into the lists below); RandomAccessGate: its index bits; else 0 */
    uint32_t gate_selector_index[16];
    uint32_t gate_group_start[16], gate_group_end[16];
    uint64_t k_is[80];                 /* coset shifts 7^j (field/src/cosets.rs:9-24)               */
    /* ---- lookup argument (up to GL_MAX_LUTS tables; all zero without lookups).  Gate types 6 = LookupGate (40 slots), 7 =
     * LookupTableGate (26 slots) (gates/lookup.rs, gates/lookup_table.rs): one of each PER TABLE in `gate_types`, told apart by
     * `gate_params`; `num_constants` counts the lookup selector columns, which sit between the gate selectors and the gates' constants
     * (circuit_builder.rs:991-1004) ---- */
    uint32_t num_lookup_polys;         /* per challenge: 1 RE + ceil(40 / 7) partial SLDC = 7 (circuit_builder.rs:1079-1085)     */
    uint32_t num_lookup_selectors;     /* TransSre, TransLdc, InitSre, LastLdc + one end selector per table = 4 + num_luts     */
    uint32_t num_luts;                 /* common_data.luts.len(); every table has lookups (gadgets/lookup.rs:79-84)            */
    /* LookupWire per table (circuit_builder.rs:73-85; the gate rows are upside down: last_lu_row < last_lut_row <= first_lut_row).
     * ProverOnlyCircuitData: a description read from CommonCircuitData bytes has last_lu_row = 0, and build() fills the rows in
     * from the lookup selector columns (gl_circuit_description returns them). */
    uint32_t last_lu_row[4], last_lut_row[4], first_lut_row[4];
    uint32_t lut_len[4];               /* entries per table; their sum <= GL_MAX_LUT_ENTRIES                                   */
    uint16_t lut[2 * 1024];            /* (input, output) pairs (gates/lookup_table.rs:22), the tables one after the other     */
    /* ---- zero knowledge (CircuitConfig::standard_recursion_zk_config, circuit_data.rs:104-110): the wires, Z / partial-products and
     * quotient commitments are salted (config.zero_knowledge = fri_params.hiding), and blind_and_pad appended blinding rows
     * (circuit_builder.rs:713-818).  Not together with lookups (GL_ERR_UNSUPPORTED). ---- */
    uint32_t zero_knowledge;           /* 0 / 1                                                                                 */
    uint32_t num_gate_rows;            /* rows before blind_and_pad, or 0 when unknown (a description read from bytes); when set,
                                          degree_bits must be what blinding_counts + padding give, and gl_witness_blind needs it */
    /* ---- C::Hasher (a type parameter in Rust, not part of CommonCircuitData's bytes): Merkle trees, transcript, proof of work ---- */
    uint32_t hasher;                   /* GL_HASHER_POSEIDON (0) / GL_HASHER_KECCAK (1)                                         */
} gl_circuit_desc;
#define GL_MAX_GATES 16
#define GL_MAX_LUTS 4
#define GL_MAX_LUT_ENTRIES 1024

/* ---- context ------------------------------------------------------------------------------------ */
/* stream: a hipStream_t to enqueue on (e.g. torch.cuda.current_stream().cuda_stream), or NULL to let
 * the context create its own non-blocking stream. */
int gl_ctx_create(int device, void* stream, gl_ctx** out);
/* A context that creates its own stream asks for one with a hardware queue of its own, so that its kernels do not wait behind
 * those of other contexts (the runtime otherwise folds all streams onto GPU_MAX_HW_QUEUES queues).  At most GL_LANE_QUEUES
 * (environment, default 24, 0 = never; none at all when GPU_MAX_HW_QUEUES >= 16) such streams are live per device and process;
 * contexts past that, and contexts on a caller's stream, share the runtime's pool.
 * gl_ctx_has_own_queue: 1 if the context's stream has its own queue.  gl_lane_queues_live: such streams live on `device`. */
int gl_ctx_has_own_queue(const gl_ctx* ctx) GL_NOEXCEPT;
int gl_lane_queues_live(int device) GL_NOEXCEPT;
/* drops the creator's reference (see "Lifetime" above); synchronises the stream first */
void gl_ctx_destroy(gl_ctx* ctx) GL_NOEXCEPT;
int gl_ctx_synchronize(gl_ctx* ctx);
/* scratch used between the two NTT passes (elements); default 2^24 (128 MiB). */
int gl_ctx_set_scratch_elems(gl_ctx* ctx, size_t elems);
const char* gl_last_error(void) GL_NOEXCEPT;
/* Per-scope device timings (HIP events on the context's stream), the analogue of the reference's TimingTree
 * (plonky2/src/util/timing.rs:8-192; scopes as in fri/oracle.rs:51-89, plonk/prover.rs:118-316).
 * Off by default; gl_ctx_timing_report synchronises and writes a JSON object into buf. */
int gl_ctx_timing_enable(gl_ctx* ctx, int on);
int gl_ctx_timing_reset(gl_ctx* ctx);
int gl_ctx_timing_report(gl_ctx* ctx, char* buf, size_t cap);
/* device memory helpers so that a host language needs no HIP binding of its own */
int gl_dev_alloc(gl_ctx* ctx, size_t bytes, void** d_out);
int gl_dev_free(gl_ctx* ctx, void* d_ptr);
int gl_copy_h2d(gl_ctx* ctx, void* d_dst, const void* h_src, size_t bytes);
int gl_copy_d2h(gl_ctx* ctx, void* h_dst, const void* d_src, size_t bytes);   /* synchronises */

/* ---- field micro-kernels (tests; replace nothing on the path by themselves) ----------------------
 * op: 0 add, 1 sub, 2 mul, 3 neg(a), 4 inverse(a), 5 canonicalise(a), 6 a + b*c, 7 a * 2^(b mod 192)
 * (field/src/goldilocks_field.rs:186-274,138-142); b mod 192 is taken of the 64-bit word as it stands.  d_a, d_b, d_c: READ-ONLY, n
 * words each (d_b may be null for ops 3..5, d_c for all but 6); d_out: OUTPUT, n words.  d_out may alias d_a (then d_a is IN PLACE, all n
 * words); any other overlap is undefined. */
int gl_field_op(gl_ctx* ctx, int op, const uint64_t* d_a, const uint64_t* d_b, const uint64_t* d_c,
                uint64_t* d_out, size_t n);
/* op: 0 add, 1 sub, 2 mul, 3 inverse on interleaved (a0,a1) pairs (extension/quadratic.rs:143-193).  d_a, d_b: READ-ONLY, 2 n words
 * (d_b may be null for op 3); d_out: OUTPUT, 2 n words. */
int gl_ext_op(gl_ctx* ctx, int op, const uint64_t* d_a, const uint64_t* d_b, uint64_t* d_out, size_t n);

/* ---- NTT family: d_data is [batch][2^log_n], transformed in place, natural order in and out ------
 * d_data: IN PLACE, all batch * 2^log_n words; the passes between, and the twiddle tables, live in the context's scratch. */
/* fft_with_options(poly, None, root_table) (field/src/fft.rs:56-65): values[i] = P(w^i) */
int gl_ntt_forward(gl_ctx* ctx, uint64_t* d_data, uint32_t log_n, uint32_t batch);
/* ifft_with_options (field/src/fft.rs:72-95) */
int gl_ntt_inverse(gl_ctx* ctx, uint64_t* d_data, uint32_t log_n, uint32_t batch);
/* PolynomialCoeffs::coset_fft (field/src/polynomial/mod.rs:276-295): evaluations on shift*H */
int gl_ntt_coset_forward(gl_ctx* ctx, uint64_t* d_data, uint32_t log_n, uint32_t batch, uint64_t shift);
/* PolynomialValues::coset_ifft (field/src/polynomial/mod.rs:58-70) */
int gl_ntt_coset_inverse(gl_ctx* ctx, uint64_t* d_data, uint32_t log_n, uint32_t batch, uint64_t shift);
/* p.lde(rate_bits).coset_fft_with_options(F::coset_shift(), Some(rate_bits), table)
 * (plonky2/src/fri/oracle.rs:111-118): d_coeffs [batch][2^log_n] -> d_out [batch][2^(log_n+rate_bits)],
 * natural order (index i <-> point 7*w^i).  d_coeffs: READ-ONLY; d_out: OUTPUT, all batch * 2^(log_n+rate_bits) words; the two may not
 * overlap. */
int gl_ntt_coset_lde(gl_ctx* ctx, const uint64_t* d_coeffs, uint32_t log_n, uint32_t rate_bits,
                     uint32_t batch, uint64_t* d_out);
/* host-buffer convenience (H2D + transform + D2H): direction 0 forward, 1 inverse */
int gl_fft_host(gl_ctx* ctx, uint64_t* h_data, uint32_t log_n, uint32_t batch, int inverse);

/* ---- Poseidon / hashing --------------------------------------------------------------------------*/
/* Poseidon::poseidon (plonky2/src/hash/poseidon.rs:598-609) on `count` 12-word states.  d_states: IN PLACE, all 12 * count words */
int gl_poseidon_permute(gl_ctx* ctx, uint64_t* d_states, size_t count);
/* the same permutation with the MDS layer chosen by `layer` (0: vector ALU, 1: i8 matrix cores), leaving the raw u64
   representatives (not canonicalised): the two layers return the same words.  d_states: IN PLACE, all 12 * count words */
int gl_poseidon_permute_raw(gl_ctx* ctx, uint64_t* d_states, size_t count, int layer);
/* Hasher::hash_or_noop (plonky2/src/plonk/config.rs:55-66) of `count` rows of `len` elements,
 * row-major d_rows[count][len] -> d_out[count][4].  d_rows: READ-ONLY; d_out: OUTPUT, all 4 * count words (the words of a short row's
 * digest beyond `len` are written as zero) */
int gl_hash_rows(gl_ctx* ctx, const uint64_t* d_rows, size_t count, size_t len, uint64_t* d_out);
/* the same under `hasher`; KeccakHash<25> (hash/keccak.rs:105-117): a row of <= 3 elements is copied into the 25 bytes, a longer one is
 * Keccak-256 (original padding: domain byte 0x01) over its canonical little-endian words, truncated to 25 bytes.  d_rows: READ-ONLY;
 * d_out: OUTPUT, all 4 * count words */
int gl_hash_rows_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* d_rows, size_t count, size_t len, uint64_t* d_out);
/* Hasher::hash_or_noop (plonk/config.rs:55-66) and Hasher::two_to_one (hash/hashing.rs:98-115 PoseidonHash, hash/keccak.rs:119-126
 * KeccakHash<25>) on the host, no GPU needed: h_rows[count][len] -> h_out[count][4]; h_left[count][4], h_right[count][4] -> h_out[count][4] */
int gl_hash_or_noop_host(uint32_t hasher, const uint64_t* h_rows, size_t count, size_t len, uint64_t* h_out);
int gl_two_to_one_host(uint32_t hasher, const uint64_t* h_left, const uint64_t* h_right, size_t count, uint64_t* h_out);

/* ---- Merkle tree ---------------------------------------------------------------------------------*/
/* MerkleTree::new(leaves, cap_height) (plonky2/src/hash/merkle_tree.rs:135-165) for row-major host
 * leaves h_leaves[num_leaves][leaf_len]; the tree keeps a device copy of the leaves. */
int gl_merkle_new(gl_ctx* ctx, const uint64_t* h_leaves, size_t num_leaves, size_t leaf_len,
                  uint32_t cap_height, gl_merkle** out);
/* MerkleTree::<F, H>::new for H = `hasher` (merkle_tree.rs:69-165: hash_or_noop on the leaves, two_to_one inside) */
int gl_merkle_new_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* h_leaves, size_t num_leaves, size_t leaf_len,
                    uint32_t cap_height, gl_merkle** out);
/* field `cap` (merkle_tree.rs:54): h_out[2^cap_height][4] */
int gl_merkle_cap(const gl_merkle* t, uint64_t* h_out);
/* MerkleTree::prove (merkle_tree.rs:171-207): siblings bottom-up, h_out[log2(n) - cap_height][4] */
int gl_merkle_prove(const gl_merkle* t, size_t leaf_index, uint64_t* h_out, uint32_t* n_siblings);
void gl_merkle_free(gl_merkle* t) GL_NOEXCEPT;

/* ---- PolynomialBatch -----------------------------------------------------------------------------*/
/* PolynomialBatch::from_values(values, rate_bits, blinding, cap_height, timing, fft_root_table)
 * (plonky2/src/fri/oracle.rs:43-66).  h_cols[c] points at the n = 2^k values of polynomial c.
 * blinding must be 0 (GL_ERR_UNSUPPORTED otherwise): blinding = true is gl_batch_from_values_blinded below.  Keeps
 * coefficients, LDE values and all Merkle digests device-resident. */
int gl_batch_from_values(gl_ctx* ctx, const uint64_t* const* h_cols, size_t ncols, size_t n,
                         uint32_t rate_bits, uint32_t blinding, uint32_t cap_height, gl_batch** out);
/* PolynomialBatch::from_coeffs (plonky2/src/fri/oracle.rs:68-98) */
int gl_batch_from_coeffs(gl_ctx* ctx, const uint64_t* const* h_cols, size_t ncols, size_t n,
                         uint32_t rate_bits, uint32_t blinding, uint32_t cap_height, gl_batch** out);
/* from_values / from_coeffs with blinding = true: every leaf salted with SALT_SIZE = 4 random elements (fri/oracle.rs:100-125); salt
 * column j is stream 0x200 + j of the keystream below, keyed by `seed` (NULL = a fresh OS seed).  The salt enters the Merkle leaves
 * only (get_leaf / prove: ncols + 4 elements), never the polynomials (get_lde_values, the coefficients, the LDE). */
int gl_batch_from_values_blinded(gl_ctx* ctx, const uint64_t* const* h_cols, size_t ncols, size_t n, uint32_t rate_bits,
                                 uint32_t cap_height, const uint8_t seed[32], gl_batch** out);
int gl_batch_from_coeffs_blinded(gl_ctx* ctx, const uint64_t* const* h_cols, size_t ncols, size_t n, uint32_t rate_bits,
                                 uint32_t cap_height, const uint8_t seed[32], gl_batch** out);
/* same, from a device-resident column-major matrix d_cols[ncols][n]; is_values selects from_values.  d_cols: READ-ONLY (the batch keeps
 * a copy of its own and does not need it after the call) */
int gl_batch_from_device(gl_ctx* ctx, const uint64_t* d_cols, size_t ncols, size_t n, uint32_t rate_bits,
                         uint32_t cap_height, int is_values, gl_batch** out);
/* The five constructors above for PolynomialBatch<F, C, D> with C::Hasher = `hasher` (fri/oracle.rs:43-125): the same polynomials and
 * LDE values, the Merkle tree under that hasher.  seed as above; gl_batch_from_device_h commits without salt (d_cols: READ-ONLY). */
int gl_batch_from_values_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* const* h_cols, size_t ncols, size_t n,
                           uint32_t rate_bits, uint32_t blinding, uint32_t cap_height, gl_batch** out);
int gl_batch_from_coeffs_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* const* h_cols, size_t ncols, size_t n,
                           uint32_t rate_bits, uint32_t blinding, uint32_t cap_height, gl_batch** out);
int gl_batch_from_values_blinded_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* const* h_cols, size_t ncols, size_t n, uint32_t rate_bits,
                                   uint32_t cap_height, const uint8_t seed[32], gl_batch** out);
int gl_batch_from_coeffs_blinded_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* const* h_cols, size_t ncols, size_t n, uint32_t rate_bits,
                                   uint32_t cap_height, const uint8_t seed[32], gl_batch** out);
int gl_batch_from_device_h(gl_ctx* ctx, uint32_t hasher, const uint64_t* d_cols, size_t ncols, size_t n, uint32_t rate_bits,
                           uint32_t cap_height, int is_values, gl_batch** out);
uint32_t gl_batch_hasher(const gl_batch* b) GL_NOEXCEPT;
/* field `merkle_tree.cap` (used at prover.rs:164,225,273,319-321): h_out[2^cap_height][4] */
int gl_batch_cap(const gl_batch* b, uint64_t* h_out);
/* merkle_tree.get(i) (merkle_tree.rs:167-169): the leaf at Merkle index i, h_out[ncols] (h_out[ncols + 4] with blinding: the salt last) */
int gl_batch_get_leaf(const gl_batch* b, size_t leaf_index, uint64_t* h_out);
/* PolynomialBatch::get_lde_values(index, step) (oracle.rs:128-133), h_out[ncols] */
int gl_batch_get_lde_values(const gl_batch* b, size_t index, size_t step, uint64_t* h_out);
/* merkle_tree.prove(i) (merkle_tree.rs:171-207) */
int gl_batch_prove(const gl_batch* b, size_t leaf_index, uint64_t* h_out, uint32_t* n_siblings);
/* field `polynomials` (oracle.rs:32): h_out[ncols][n] coefficients */
int gl_batch_coeffs(const gl_batch* b, uint64_t* h_out);
/* all LDE values in natural order, column-major h_out[ncols][n << rate_bits] (index i <-> 7*w^i) */
int gl_batch_lde(const gl_batch* b, uint64_t* h_out);
size_t gl_batch_ncols(const gl_batch* b) GL_NOEXCEPT;
size_t gl_batch_degree(const gl_batch* b) GL_NOEXCEPT;
const uint64_t* gl_batch_dev_coeffs(const gl_batch* b) GL_NOEXCEPT;   /* d [ncols][n]  */
const uint64_t* gl_batch_dev_lde(const gl_batch* b) GL_NOEXCEPT;      /* d [ncols][N]  */
void gl_batch_free(gl_batch* b) GL_NOEXCEPT;

/* ---- randomness of zero-knowledge proving ------------------------------------------------------------
 * A keyed counter-based generator: ChaCha20's block function (RFC 8439 section 2.3) with key = the 32-byte seed, nonce =
 * (stream as u32 LE, 0, 0) and block counter = block index; element i of a stream is (w_{2i} + 2^64 w_{2i+1}) mod p over the
 * keystream's little-endian u64 words (canonical, within 2^-64 of uniform).  Streams: 0x100 + w = blinding values of wire column w
 * (element index = row), 0x200 + 4 o + j = salt column j of PlonkOracle o (1 wires, 2 zs_partial_products, 3 quotient; element
 * index = natural LDE row).  Everywhere a seed is taken, NULL means 32 fresh bytes from getrandom(2), one per proof.
 * A seed must never be reused for two different witnesses of a circuit: the two proofs' blinding and salts cancel, and hiding is
 * lost.  Fixed seeds are for tests and reproducible runs. */
/* d_out[i] = element first + i of `stream`, i < count (first + count <= 2^34).  d_out: OUTPUT, exactly `count` words, wherever first and
 * first + count fall inside a 4-element keystream block */
int gl_random_elements(gl_ctx* ctx, const uint8_t seed[32], uint32_t stream, uint64_t first, uint64_t count, uint64_t* d_out);
/* the same on the host (no GPU needed) */
int gl_random_elements_host(const uint8_t seed[32], uint32_t stream, uint64_t first, uint64_t count, uint64_t* h_out);

/* ---- circuit data ----------------------------------------------------------------------------------*/
/* Host side of the demo (no GPU needed): the matmul circuit of plonky2/src/bin/matrix_mul.rs:25-67 after
 * CircuitBuilder::build() (plonk/circuit_builder.rs:913-1146): descriptor, gate type per row, and the
 * constants || sigmas VALUE columns, h_out[(num_constants + 80)][n]. */
int gl_matmul_circuit_build(size_t m, gl_host_circuit** out);
/* The same circuit built with standard_recursion_zk_config: the same gate rows (gates, constants, copy classes), then blind_and_pad's
 * blinding rows and padding -- NoopGate rows with singleton copy classes -- and degree_bits / FRI arities of the longer trace.
 * desc.zero_knowledge = 1, desc.num_gate_rows = the rows before blinding.  gl_matmul_witness and the witness generator leave the
 * rows from num_gate_rows on zero; gl_witness_blind fills them in before proving. */
int gl_matmul_circuit_build_zk(size_t m, gl_host_circuit** out);
/* either of the two with the configuration's hasher chosen: the circuit the demo builds under `C = KeccakGoldilocksConfig`
 * (plonky2/src/bin/matrix_mul.rs:21-23 names the type parameter).  Gates, constants, sigmas and witness are the same; desc.hasher differs. */
int gl_matmul_circuit_build_h(size_t m, uint32_t zero_knowledge, uint32_t hasher, gl_host_circuit** out);
int gl_host_circuit_desc(const gl_host_circuit* hc, gl_circuit_desc* out);
int gl_host_circuit_row_gates(const gl_host_circuit* hc, uint8_t* h_out /* n */);
int gl_host_circuit_constants_sigmas(const gl_host_circuit* hc, uint64_t* h_out);
/* generate_partial_witness + full_witness (plonk/prover.rs:118-133) for this circuit: a, b row-major m x m;
 * the 131 values the reference draws from OsRng for the unused PublicInputGate wires
 * (circuit_builder.rs:904-910) come from splitmix64(filler_seed).  h_wires[135][n], h_public_inputs[3 m^2]. */
int gl_matmul_witness(const gl_host_circuit* hc, const uint64_t* h_a, const uint64_t* h_b, uint64_t filler_seed,
                      uint64_t* h_wires, uint64_t* h_public_inputs);
void gl_host_circuit_free(gl_host_circuit* hc) GL_NOEXCEPT;
/* The same witness produced directly in HBM: the m^3 ArithmeticGate operations are filled by the GPU, the sequential
 * public-input hash sponge (PoseidonGate rows) by the calling host thread meanwhile.  d_wires[135][n]: OUTPUT, all 135 n words;
 * h_public_inputs[3 m^2].  The generator borrows `hc` and belongs to `ctx` (one per context / stream). */
typedef struct gl_matmul_witgen gl_matmul_witgen;
int gl_matmul_witgen_create(gl_ctx* ctx, const gl_host_circuit* hc, gl_matmul_witgen** out);
int gl_matmul_witgen_run(gl_matmul_witgen* g, const uint64_t* a, const uint64_t* b, uint64_t filler_seed,
                         uint64_t* d_wires, uint64_t* h_public_inputs, uint64_t* h_public_inputs_hash /* [4], may be null */);
void gl_matmul_witgen_free(gl_matmul_witgen* g) GL_NOEXCEPT;

/* The device half of build(): PolynomialBatch::from_values(constants || sigmas) (circuit_builder.rs:1020-1028),
 * circuit_digest (:1089-1100), sigma / subgroup tables.  h_constants_sigmas[(num_constants + 80)][n]. */
int gl_circuit_create(gl_ctx* ctx, const gl_circuit_desc* desc, const uint64_t* h_constants_sigmas, gl_circuit** out);
/* The same with the sigma polynomials computed ON THE DEVICE (circuit_builder.rs:1007-1014 sigma_vecs; plonk/permutation_argument.rs:
 * 85-170): h_wire_classes[80][n] holds, for every routed wire (wire (row, col) at col * n + row), the id of its copy-constraint
 * class -- the representative the reference's union-find Forest assigns; any u64, equal ids = wires constrained equal.
 * h_constants[num_constants][n] are the selector and gate-constant VALUE columns. */
int gl_circuit_create_from_classes(gl_ctx* ctx, const gl_circuit_desc* desc, const uint64_t* h_constants, const uint64_t* h_wire_classes,
                                   gl_circuit** out);
/* build() of the demo circuit: constants from the host description, sigma polynomials on the device */
int gl_circuit_from_host(gl_ctx* ctx, const gl_host_circuit* hc, gl_circuit** out);
/* the wire classes of the host description, h_out[80][n] (gl_circuit_create_from_classes takes them) */
int gl_host_circuit_wire_classes(const gl_host_circuit* hc, uint64_t* h_out);
/* The description the circuit was built with, completed: for a circuit with lookups build() reads last_lu_row / last_lut_row /
 * first_lut_row from the lookup selector columns (they are ProverOnlyCircuitData::lookup_rows in the reference and are not part of
 * CommonCircuitData's bytes), checks any the caller named against them, and refuses a mismatch with GL_ERR_ARG. */
int gl_circuit_description(const gl_circuit* c, gl_circuit_desc* out);
/* Optional, once per (context, circuit) before the first proof: one pass of the proving pipeline over a zero witness, thrown away,
 * so that the first gl_prove on this context does not pay for loading the kernels' code objects, building the twiddle tables of the
 * circuit's transform sizes and growing the context's pool (m = 64: 15 ms for the first proof without it, 7 ms with). */
int gl_circuit_warm_up(gl_ctx* ctx, const gl_circuit* c);
/* The RandomValueGenerators and CopyGenerators of blind() (circuit_builder.rs:777-818) on the device, for a zero-knowledge circuit with
 * num_gate_rows set: from row num_gate_rows on, `regular` rows of 135 random wires, then `pairs` row pairs whose first row's 80 routed
 * wires are random and copied to the second, every other wire of those rows and the padding rows 0 (full_witness, iop/witness.rs:340-352).
 * seed NULL = OS entropy.  A Rust-built zk circuit's witness arrives blinded by Rust's own generators and goes straight to gl_prove*.
 * d_wires[135][n]: IN PLACE, rows num_gate_rows .. n of all 135 columns (the zeros too); rows below num_gate_rows keep their values. */
int gl_witness_blind(gl_ctx* ctx, const gl_circuit* c, uint64_t* d_wires, const uint8_t seed[32]);
int gl_circuit_digest(const gl_circuit* c, uint64_t h_out[4]);                 /* verifier_only.circuit_digest */
int gl_circuit_constants_sigmas_cap(const gl_circuit* c, uint64_t* h_out);     /* [2^cap_height][4]            */
const gl_batch* gl_circuit_constants_sigmas_batch(const gl_circuit* c) GL_NOEXCEPT;
void gl_circuit_free(gl_circuit* c) GL_NOEXCEPT;

/* ---- prover phases ---------------------------------------------------------------------------------*/
/* Not for zero-knowledge circuits (GL_ERR_UNSUPPORTED): they are proved by gl_prove* only. */
/* The seam for a caller that keeps the Fiat-Shamir transcript (iop/challenger.rs) on its own side: each entry
 * point replaces one call of plonk::prover::prove and returns exactly what the transcript absorbs next.
 * gl_prove() below is these calls in the order of prover.rs:102-329 with the Challenger in C++.
 * All polynomial-sized data stays in HBM; challenges may be non-canonical u64, outputs are canonical. */
typedef struct gl_fri gl_fri;

/* all_wires_permutation_partial_products (plonk/prover.rs:189-200,332-416) followed by the commitment of
 * prover.rs:212-223: d_wires[135][n] witness VALUES on the device -> PolynomialBatch of the 2 Z and 18 partial
 * product polynomials (column order zs, then partial products, as prover.rs:202-210).  d_wires: READ-ONLY (here and in
 * gl_partial_products_lookups). */
int gl_partial_products(gl_ctx* ctx, const gl_circuit* c, const uint64_t* d_wires, const uint64_t betas[2],
                        const uint64_t gammas[2], gl_batch** out);
/* compute_quotient_polys + the split into quotient_degree_factor chunks + from_coeffs (plonk/prover.rs:229-271,
 * 574-744; vanishing_poly.rs:164-330): PolynomialBatch of the 2 x 8 chunk polynomials. */
int gl_quotient_polys(gl_ctx* ctx, const gl_circuit* c, const gl_batch* wires, const gl_batch* zs_partial_products,
                      const uint64_t public_inputs_hash[4], const uint64_t betas[2], const uint64_t gammas[2],
                      const uint64_t alphas[2], gl_batch** out);
/* The same two phases for a circuit WITH the lookup argument: `deltas[8]` = per challenge ChallengeA, ChallengeB, ChallengeAlpha,
 * ChallengeDelta, i.e. [betas | gammas | the 4 challenges drawn after them] (plonk/prover.rs:166-184).  The batch of the first has the
 * 2 x 7 lookup polynomials behind the 20 columns (compute_all_lookup_polys, prover.rs:202-211); the second adds
 * check_lookup_constraints (vanishing_poly.rs:503-670) to the quotient.  gl_fri_combine and gl_open_at need no variant: the batch
 * carries its columns (openings in FriOpenings order: ..., quotient, lookups | zs_next, lookups_next, plonk/proof.rs:346-380). */
int gl_partial_products_lookups(gl_ctx* ctx, const gl_circuit* c, const uint64_t* d_wires, const uint64_t betas[2],
                                const uint64_t gammas[2], const uint64_t deltas[8], gl_batch** out);
int gl_quotient_polys_lookups(gl_ctx* ctx, const gl_circuit* c, const gl_batch* wires, const gl_batch* zs_partial_products_lookups,
                              const uint64_t public_inputs_hash[4], const uint64_t betas[2], const uint64_t gammas[2],
                              const uint64_t alphas[2], const uint64_t deltas[8], gl_batch** out);
/* OpeningSet::new's eval_commitment (plonk/proof.rs:306-344): polynomials first_col .. first_col + num_cols of a
 * batch at the extension point z; h_out[num_cols][2]. */
int gl_open_at(gl_ctx* ctx, const gl_batch* b, const uint64_t z[2], size_t first_col, size_t num_cols, uint64_t* h_out);
/* PolynomialBatch::prove_openings up to the call of fri_proof (fri/oracle.rs:162-204): batches in oracle order
 * constants||sigmas, wires, Z||partial products, quotient (circuit_data.rs:586-595); opens everything at zeta and
 * the Z polynomials at g*zeta, final = alpha^2 Q0 + Q1, LDE onto the coset.  The batches must outlive the gl_fri. */
int gl_fri_combine(gl_ctx* ctx, const gl_circuit* c, const gl_batch* const batches[4], const uint64_t zeta[2],
                   const uint64_t alpha[2], gl_fri** out);
/* fri_committed_trees, one loop iteration in two halves (fri/prover.rs:76-103): Merkle tree of the current
 * codeword -> its cap h_cap_out[2^cap_height][4]; then, with the beta drawn after observing that cap, the fold. */
int gl_fri_commit_round(gl_fri* f, uint64_t* h_cap_out);
int gl_fri_fold(gl_fri* f, const uint64_t beta[2]);
/* final_poly (fri/prover.rs:106-111): *num_words = 2 * len; h_out (may be null to query the size) = (a, b) pairs */
int gl_fri_final_poly(gl_fri* f, uint64_t* h_out, size_t cap_words, size_t* num_words);
/* fri_proof_of_work (fri/prover.rs:115-160): the SMALLEST witness w with
 * leading_zeros(permute(sponge_state overlaid with input_buffer[0..input_len) and w at input_len)[7]) >= min_leading_zeros */
int gl_pow_grind(gl_ctx* ctx, const uint64_t sponge_state[12], const uint64_t* input_buffer, uint32_t input_len,
                 uint32_t min_leading_zeros, uint64_t* witness);
/* the same over `hasher`'s permutation.  KeccakPermutation (hash/keccak.rs:64-95): the candidate goes into its state word, H1 =
 * Keccak-256 of the 96 state bytes, H2 = Keccak-256(H1), ...; the response is element 7 of the stream of their words < p (normally
 * word 3 of H2; a rejected word moves it, possibly into H3, and the kernel follows). */
int gl_pow_grind_h(gl_ctx* ctx, uint32_t hasher, const uint64_t sponge_state[12], const uint64_t* input_buffer, uint32_t input_len,
                   uint32_t min_leading_zeros, uint64_t* witness);
/* fri_prover_query_rounds (fri/prover.rs:162-216) for the given x_index values (challenge mod lde_size), as the
 * serialised Vec<FriQueryRound> body (util/serialization/mod.rs:1477-1546).  h_blob may be null to query the size. */
int gl_fri_query(gl_fri* f, const uint32_t* x_index, uint32_t num_queries, uint8_t* h_blob, size_t cap_bytes,
                 size_t* num_bytes);
void gl_fri_free(gl_fri* f) GL_NOEXCEPT;

/* A Challenger (iop/challenger.rs:30-153: duplex sponge, challenges pop from the end of the rate) for callers of the
 * phase API that have no transcript of their own.  Host code.  `gl_challenger_state` exposes sponge_state / input_buffer
 * the way fri_proof_of_work reads them (fri/prover.rs:127-140), for gl_pow_grind. */
typedef struct gl_challenger gl_challenger;
gl_challenger* gl_challenger_new(void);
/* Challenger<F, H> for H = `hasher` (NULL for another value); under Keccak the permutation is KeccakPermutation (hash/keccak.rs:64-95) */
gl_challenger* gl_challenger_new_h(uint32_t hasher);
/* observe_hash::<OH> / observe_cap::<OH> (challenger.rs:72-80) of `count` digests h_hashes[count][4] of hasher `oh`: a HashOut is its
 * four elements, a BytesHash<25> the four elements of its bytes in chunks of 7, 7, 7, 4 (hash_types.rs:181-191) */
int gl_challenger_observe_hashes(gl_challenger* c, uint32_t oh, const uint64_t* h_hashes, size_t count);
int gl_challenger_observe(gl_challenger* c, const uint64_t* h_elements, size_t count);
int gl_challenger_get_challenges(gl_challenger* c, uint64_t* h_out, size_t count);
int gl_challenger_state(const gl_challenger* c, uint64_t h_sponge_state[12], uint64_t h_input_buffer[8], uint32_t* input_len);
/* Challenger::compact (iop/challenger.rs:146-152): absorb any pending input (one duplexing), then drop the buffered outputs, so that
 * the next challenge comes from a fresh permutation.  evm's prove_single_table and its verifier begin every table with it. */
int gl_challenger_compact(gl_challenger* c);
void gl_challenger_free(gl_challenger* c) GL_NOEXCEPT;

/* ---- FRI openings of any instance ------------------------------------------------------------------
 * PolynomialBatch::prove_openings (fri/oracle.rs:162-219) and verify_fri_proof (fri/verifier.rs:62-241) for an arbitrary
 * FriInstanceInfo (fri/structure.rs): any number of oracles, any (point, polynomials) batches, any rate_bits / cap_height, salted
 * oracles, either hasher.  This is the call through which provers other than plonk::prover (starky/src/prover.rs) reach the seam.
 * A circuit proof is the instance of four oracles (constants||sigmas, wires, Z||partial products(||lookups), quotient; the last three
 * blinded) and two batches (everything at zeta; the Zs and the lookup polynomials at g zeta): gl_verify above verifies it through
 * gl_verify_openings' code; gl_fri_combine / gl_prove* above keep a combine and a fri_proof loop of their own over the same list. */
#define GL_MAX_FRI_ORACLES 8
#define GL_MAX_FRI_BATCHES 4
typedef struct gl_fri_params {          /* FriParams (fri/mod.rs) + C::Hasher */
    uint32_t degree_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds;
    uint32_t num_fri_rounds, fri_arity_bits[8];
    uint32_t hiding, hasher;
} gl_fri_params;
typedef struct gl_fri_instance {        /* FriInstanceInfo (fri/structure.rs) */
    uint32_t num_oracles, oracle_num_polys[GL_MAX_FRI_ORACLES], oracle_blinding[GL_MAX_FRI_ORACLES];
    uint32_t num_batches;               /* 1..GL_MAX_FRI_BATCHES */
    uint64_t points[GL_MAX_FRI_BATCHES][2];
    uint32_t batch_len[GL_MAX_FRI_BATCHES];      /* >= 1 each */
    const uint32_t* polys;              /* sum(batch_len) pairs (oracle_index, polynomial_index), batch after batch */
} gl_fri_instance;
/* Validation, the same in the three calls below: GL_ERR_ARG for a count out of range (1..8 oracles of >= 1 polynomials, 1..4 batches,
 * at most 65536 listed polynomials, 1..256 query rounds, at most 8 reductions of arity bits 1..8, at most 40 bits of work), an empty
 * batch, polys == NULL, an oracle / polynomial index out of range, degree_bits < 1 or degree_bits + rate_bits > 24, a total reduction
 * above degree_bits or above degree_bits + rate_bits - cap_height (circuit_builder.rs:977-980), an opening point on the LDE coset
 * 7 H_N (the reference panics dividing by zero there), and a batch handle whose n, rate_bits, cap_height, hasher, column count or
 * salt (oracle_blinding && hiding) differs from params / instance.  The two prover calls answer GL_ERR_UNSUPPORTED for a reduction
 * of arity other than 16, as for circuits; the verifier takes arity bits 1..8.  Points and alpha may be non-canonical.  One
 * polynomial may stand in several batches and several times in one. */
/* prove_openings up to the call of fri_proof (fri/oracle.rs:183-204): per batch F_i = sum_j alpha^j f_ij and (F_i - F_i(z_i)) / (X - z_i)
 * with the zero pushed back on, final = sum_i quotient_i alpha^(sum_{j > i} len_j) (reduce_polys_base and shift_poly on their shared
 * counter, util/reducing.rs:83-106), LDE by rate_bits onto the coset.  batches[num_oracles] in the instance's oracle order; they must
 * outlive the gl_fri, which gl_fri_commit_round / gl_fri_fold / gl_fri_final_poly / gl_fri_query drive as for a circuit; gl_fri_query
 * writes the initial-tree proofs of all num_oracles oracles in order. */
int gl_fri_combine_instance(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches,
                            const uint64_t alpha[2], gl_fri** out);
/* Diagnostic: the same result by the sequence gl_fri_combine ran before it used the one-pass kernels, one batch after the other (four launches per batch, a column read
 * once per batch that lists it), for measuring the one-pass kernels against it (tools/openings_rate.py) and testing them against it. */
int gl_fri_combine_instance_per_batch(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance,
                                      const gl_batch* const* batches, const uint64_t alpha[2], gl_fri** out);
/* The whole of prove_openings (fri/oracle.rs:162-219, fri/prover.rs:20-216) on the caller's Challenger, from the draw of alpha on (the
 * caller has observed the openings): commit caps and betas, final polynomial, proof of work, query indices.  Writes the FriProof in
 * write_fri_proof order (util/serialization/mod.rs:1568-1582): commit-phase caps, query rounds, final polynomial, PoW witness.
 * *num_bytes = its size, which the params and the instance fix; with h_out null only the size is answered: nothing runs and the
 * challenger stays where it is.  A call that fails later leaves the challenger advanced. */
int gl_prove_openings(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance, const gl_batch* const* batches,
                      gl_challenger* challenger, uint8_t* h_out, size_t cap_bytes, size_t* num_bytes);
/* verify_fri_proof (fri/verifier.rs:62-241) with the challenges of fri/challenges.rs:24-64 drawn from `challenger`, which is in the
 * state gl_prove_openings expects.  Host code, no GPU.  caps[num_oracles][2^cap_height][4]; openings: the batches' values, batch
 * after batch, two words each (FriOpenings).  GL_OK, or GL_ERR_VERIFY with gl_last_error() and *check (may be null) = the GL_CHECK_*
 * code below of the first failing check, in the order: TRUNCATED / LENGTH / *_PATH_LENGTH from the decode; POW; then per query,
 * ascending: INITIAL_MERKLE (oracles in order), per reduction FRI_CONSISTENCY before STEP_MERKLE, FINAL_POLY.  Only the unsalted prefix
 * of a leaf enters fri_combine_initial (salt_size(oracle.blinding && params.hiding), fri/proof.rs unsalted_eval). */
int gl_verify_openings(const gl_fri_params* params, const gl_fri_instance* instance, const uint64_t* caps, const uint64_t* openings,
                       gl_challenger* challenger, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check);

/* ---- STARK: an AIR as data, and the two prover phases it needs ---------------------------------------
 * starky's `Stark` states its constraints as code (eval_packed_generic, starky/src/stark.rs:26-62); over a C ABI they are data: one
 * term list per constraint, in the order the Stark yields them.  Constraint c is  sum_t coeff_t * prod_f operand_{t,f}  with every
 * operand a trace column on the local row, the same on the next row, or a public input; its filter names the ConstraintConsumer
 * method it goes through (constraint_consumer.rs:53-76).  The FRI side of StarkConfig (starky/src/config.rs) is a gl_fri_params;
 * num_challenges stands here.  Derived as stark.rs:79-221 does: quotient_degree_factor q = max(1, constraint_degree - 1),
 * quotient_degree_bits = ceil(log2 q), permutation batch size q, ceil(pairs * num_challenges / q) Z polynomials, and the
 * FriInstanceInfo of stark.rs:88-137 (oracles trace, Z if there are pairs, quotient; batches at zeta and g zeta).
 * What is here: the description and its validation, and the two phases between the commitments -- the permutation argument's Z
 * polynomials and the quotient -- as phase entries shaped like gl_partial_products / gl_quotient_polys, every polynomial
 * device-resident; gl_stark_prove, which is those phases in the order of starky/src/prover.rs:32-194 on the library's own challenger;
 * and gl_stark_verify (verifier.rs:21-145), host code.  Public inputs are NOT observed by the transcript: this version of the
 * reference does not observe them (get_challenges.rs:21-73).
 * Proof bytes -- PARITY UNPINNED: the reference has no writer for StarkProofWithPublicInputs and no Rust-written STARK proof exists
 * here, so the layout is this project's, in the circuit proof's conventions (little-endian words, no length prefixes, every count
 * fixed by the description and the params; a hash is 32 bytes under Poseidon, 25 under Keccak):
 *   trace_cap | permutation_zs_cap (with pairs) | quotient_polys_cap            2^cap_height hashes each
 *   local_values[num_columns] | next_values[num_columns]                       two words each (StarkOpeningSet, proof.rs:129-135)
 *   permutation_zs[nz] | permutation_zs_next[nz] (with pairs) | quotient_polys[num_challenges q]
 *   the FriProof exactly as gl_prove_openings writes it
 *   public_inputs[num_public_inputs]                                            one word each */
#define GL_STARK_ALL 0u          /* ConstraintConsumer::constraint            */
#define GL_STARK_TRANSITION 1u   /* ::constraint_transition  (times x - g^-1) */
#define GL_STARK_FIRST_ROW 2u    /* ::constraint_first_row   (times L_first)  */
#define GL_STARK_LAST_ROW 3u     /* ::constraint_last_row    (times L_last)   */
#define GL_STARK_LOCAL 0u        /* operand kinds, bits 31..30 of a factor word; bits 29..0 = column / public-input index */
#define GL_STARK_NEXT 1u
#define GL_STARK_PUBLIC 2u
#define GL_STARK_MAX_COLUMNS 1024u
#define GL_STARK_MAX_PUBLIC_INPUTS 256u
#define GL_STARK_MAX_DEGREE 9u          /* q <= 8, quotient_degree_bits <= 3 */
#define GL_STARK_MAX_CHALLENGES 4u
#define GL_STARK_MAX_CONSTRAINTS 4096u
#define GL_STARK_MAX_TERMS 65536u       /* over all constraints */
#define GL_STARK_MAX_FACTORS 64u        /* per term, public inputs included */
#define GL_STARK_MAX_PAIRS 64u
#define GL_STARK_MAX_PAIR_LEN 64u
typedef struct gl_stark_desc {
    uint32_t num_columns, num_public_inputs;   /* S::COLUMNS, S::PUBLIC_INPUTS */
    uint32_t constraint_degree;                /* Stark::constraint_degree()   */
    uint32_t num_challenges;                   /* StarkConfig::num_challenges  */
    uint32_t num_constraints;
    const uint32_t* constraint_filter;         /* [num_constraints] GL_STARK_ALL .. LAST_ROW, in the order the Stark yields them */
    const uint32_t* constraint_num_terms;      /* [num_constraints] */
    const uint64_t* term_coeff;                /* [sum of terms]  may be non-canonical */
    const uint32_t* term_num_factors;          /* [sum of terms]  0 = a constant term  */
    const uint32_t* factors;                   /* [sum of factors] kind << 30 | index  */
    uint32_t num_permutation_pairs;            /* Stark::permutation_pairs()           */
    const uint32_t* pair_len;                  /* [num_permutation_pairs] column_pairs.len() >= 1 */
    const uint32_t* pair_columns;              /* [sum pair_len][2] (lhs, rhs)         */
} gl_stark_desc;
typedef struct gl_stark gl_stark;      /* a checked description + params with its tables in HBM */
/* Validation, the same in every entry below; host code, no GPU.  GL_ERR_ARG for: a null table, a count outside the GL_STARK_MAX_* caps
 * above (at least 1 column, 1 constraint, 1 challenge, degree 1), an unknown filter or operand kind, a column / public-input index out
 * of range, a pair without column pairs, and a term with more LOCAL / NEXT factors than the quotient can hold: more than q + 1, or
 * more than q under GL_STARK_FIRST_ROW / GL_STARK_LAST_ROW (the quotient's degree must stay below q n; DESIGN.md section 15 derives it).
 * GL_ERR_UNSUPPORTED for params.hiding != 0 (StarkConfig::fri_params passes false) and for quotient_degree_bits > rate_bits (the
 * reference asserts "not supported yet", prover.rs:222-225).  The gl_fri_params rules, arity 16 only among them, are gl_prove_openings'
 * own, applied to the STARK's instance. */
int gl_stark_check(const gl_stark_desc* desc, const gl_fri_params* params);
/* Copies the description, uploads the term program and the pair tables once and precomputes what depends on degree_bits only: g^-1,
 * 1/n, Z_H and 1/Z_H on the quotient coset, and L_first / L_last on it.  The handle holds a reference to the context, and every entry
 * below that takes it takes THAT context (GL_ERR_ARG for another: the tables are blocks of its stream-ordered pool); threads that
 * prove concurrently create one gl_stark per context. */
int gl_stark_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_fri_params* params, gl_stark** out);
void gl_stark_free(gl_stark* s) GL_NOEXCEPT;
/* compute_permutation_z_polys (starky/src/permutation.rs:66-117) followed by the commitment of prover.rs:89-100: d_trace_values
 * [num_columns][n] trace VALUES on the device, challenges[q][num_challenges][2] = (beta, gamma) of challenge set j, challenge c at
 * [j][c] (get_n_permutation_challenge_sets(challenger, num_challenges, q) in the order drawn) -> PolynomialBatch of the Z polynomials.
 * Instance j of a batch takes challenge_sets[j].challenges[chal], (pair, chal) running over pairs x 0..num_challenges in chunks of q
 * (get_permutation_batches, permutation.rs:228-249).  GL_ERR_ARG for a description without pairs, and -- where the reference panics
 * inverting zero -- GL_ERR_ARG "a permutation denominator is zero" (probability about n / p: draw other challenges).  d_trace_values: READ-ONLY. */
int gl_stark_permutation_zs(gl_ctx* ctx, const gl_stark* s, const uint64_t* d_trace_values, const uint64_t* challenges, gl_batch** zs);
/* compute_quotient_polys up to its coset_ifft (prover.rs:198-311): the values of (sum_i alpha^i C_i) / Z_H at the points 7 w^i of the
 * quotient coset of size n << quotient_degree_bits, natural order, h_out[num_challenges][n << quotient_degree_bits]; the Stark's
 * constraints first, then the permutation checks of permutation.rs:282-320.  No degree check: inputs that do not satisfy the
 * constraints are answered by value.  zs and challenges are null exactly for a description without pairs; alphas[num_challenges],
 * public_inputs[num_public_inputs]; the batches must match the description and params (GL_ERR_ARG). */
int gl_stark_quotient_values(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges,
                             const uint64_t* alphas, const uint64_t* public_inputs, uint64_t* h_out);
/* The same, then coset_ifft, trim_to_len(q n) -- a non-zero coefficient from index q n on is GL_ERR_ARG "the trace does not satisfy the
 * constraints", the reference's expect("Quotient has failed...") (prover.rs:123-128) -- the split into chunks of n and from_coeffs
 * (prover.rs:129-144): PolynomialBatch of the num_challenges x q chunk polynomials, challenge after challenge. */
int gl_stark_quotient_polys(gl_ctx* ctx, const gl_stark* s, const gl_batch* trace, const gl_batch* zs, const uint64_t* challenges,
                            const uint64_t* alphas, const uint64_t* public_inputs, gl_batch** quotient);
/* The size of every proof of this description under these params. */
size_t gl_stark_proof_size(const gl_stark* s) GL_NOEXCEPT;
/* starky::prover::prove (prover.rs:32-194) given the trace: h_trace_cols[num_columns] -> n values each (may be non-canonical),
 * h_public_inputs[num_public_inputs].  In order: trace commitment, its cap observed; with pairs the challenge sets
 * (get_n_permutation_challenge_sets(challenger, num_challenges, q)), the Z polynomials, their cap observed; alphas; the quotient chunks,
 * their cap observed; zeta, and GL_ERR_ZETA_IN_SUBGROUP for zeta^n = 1 (prover.rs:150-157); the openings at zeta and g zeta, observed in
 * FriOpenings order (proof.rs:161-182); gl_prove_openings' path on the STARK's instance.  *num_bytes = gl_stark_proof_size(s) always;
 * cap_bytes below it is GL_ERR_ARG.  A trace that does not satisfy the constraints is GL_ERR_ARG as in gl_stark_quotient_polys where the
 * trim can see it (q no power of two); otherwise it yields a proof the verifier rejects.  A zero permutation denominator is GL_ERR_ARG
 * as in gl_stark_permutation_zs.  Two calls on the same input give the same bytes (the PoW witness is the smallest). */
int gl_stark_prove(gl_ctx* ctx, const gl_stark* s, const uint64_t* const* h_trace_cols, const uint64_t* h_public_inputs, uint8_t* h_out,
                   size_t cap_bytes, size_t* num_bytes);
/* the same with the trace already in HBM, d_cols[num_columns][n]: READ-ONLY */
int gl_stark_prove_device(gl_ctx* ctx, const gl_stark* s, const uint64_t* d_cols, const uint64_t* h_public_inputs, uint8_t* h_out,
                          size_t cap_bytes, size_t* num_bytes);
/* verify_stark_proof (starky/src/verifier.rs:21-145).  Host code, no GPU; degree_bits comes from params and the proof's path lengths
 * are checked against it.  GL_OK, or GL_ERR_VERIFY with gl_last_error() and *check (may be null) = the GL_CHECK_* code of the first
 * failing check, in the order: TRUNCATED / LENGTH (the size the description and the params fix); the challenges of
 * get_challenges.rs:21-73; eval_vanishing_poly at zeta over the extension field, by a host interpreter of the same term list with
 * eval_l_0_and_l_last and zeta - g^-1, and per challenge vanishing == Z_H(zeta) reduce_with_powers(chunk, zeta^n): VANISHING; then
 * gl_verify_openings' checks in its order.  The verifier takes FRI arity bits 1..8, as gl_verify_openings does. */
int gl_stark_verify(const gl_stark_desc* desc, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check);

/* ---- STARK constraints as an expression DAG -----------------------------------------------------------
 * The other form of a table's constraints: the straight-line program a Stark writes in eval_packed_generic, with shared
 * subexpressions, for AIRs whose expanded form passes GL_STARK_MAX_TERMS.  A gl_stark_dag is passed BESIDE a
 * gl_stark_desc that carries num_constraints = 0 and null term tables; columns, public inputs, constraint_degree, num_challenges and
 * the pairs keep their meaning.  It is one form or the other per table.
 * Node k is  node_op[k](node_a[k], node_b[k]),  nodes in SSA order.  An operand word is  kind << 28 | index  (GL_STARK_OPERAND): LOCAL /
 * NEXT a trace column, PUBLIC a public input, NODE an EARLIER node, CONST an index into constants[] (64-bit words, may be
 * non-canonical).  Constraint c is constraint_operand[c] -- one operand word of any kind -- under constraint_filter[c], in the order
 * the Stark yields them.
 * Degree, counted formally: LOCAL / NEXT 1, PUBLIC / CONST 0, ADD / SUB the maximum of their operands, MUL the sum.  A constraint's
 * operand has degree at most q + 1 under GL_STARK_ALL / TRANSITION and at most q under FIRST_ROW / LAST_ROW.
 * Scheduling and liveness, the same in the host check, the kernel's program and the verifier: the nodes run in the given order; a
 * node no constraint reaches is dropped; constraint c is consumed at the first position -- before node 0, or right after a node -- at
 * which its value exists and constraint c - 1 has been consumed, so the Horner order in alpha is the yield order.  A value is live
 * from its definition to its last use by a node or by a constraint's consumption; live(k) counts the values defined at or before
 * node k whose last use is after node k (an operand that dies at node k does not count: node k may take its slot).  max live above
 * GL_STARK_DAG_MAX_LIVE is refused: on the device every thread keeps its live values in LDS.
 * Proof bytes -- PARITY UNPINNED, as for gl_stark_prove: the layout is the same, and a DAG that states the same polynomials as a
 * term list yields the same bytes. */
#define GL_STARK_NODE 3u         /* operand kinds beyond GL_STARK_PUBLIC, in an operand word of a gl_stark_dag only */
#define GL_STARK_CONST 4u
#define GL_STARK_OPERAND(kind, index) ((uint32_t)(kind) << 28 | (uint32_t)(index))    /* index < 2^28 */
#define GL_STARK_OP_ADD 0u
#define GL_STARK_OP_SUB 1u
#define GL_STARK_OP_MUL 2u
#define GL_STARK_DAG_MAX_NODES 65536u
#define GL_STARK_DAG_MAX_CONSTANTS 65536u
#define GL_STARK_DAG_MAX_LIVE 128u      /* values live at once: 64 KiB of LDS per 64-thread workgroup at the cap */
typedef struct gl_stark_dag {
    uint32_t num_nodes;
    const uint32_t* node_op;                   /* [num_nodes] GL_STARK_OP_ADD / SUB / MUL */
    const uint32_t* node_a;                    /* [num_nodes] operand words */
    const uint32_t* node_b;                    /* [num_nodes] */
    uint32_t num_constants;
    const uint64_t* constants;                 /* [num_constants] may be non-canonical */
    uint32_t num_constraints;
    const uint32_t* constraint_filter;         /* [num_constraints] GL_STARK_ALL .. LAST_ROW, in the order the Stark yields them */
    const uint32_t* constraint_operand;        /* [num_constraints] operand words of any kind */
} gl_stark_dag;
/* gl_stark_check for a table in DAG form.  GL_ERR_ARG for: a null dag (use gl_stark_check), a desc that carries a term list as well
 * (num_constraints != 0 or a non-null term table), a count outside the caps (at least 1 constraint), a null table, an unknown op,
 * filter or operand kind, an index out of range, a NODE operand that is no earlier node (forward or self reference), a constraint
 * above the degree rule, max live above GL_STARK_DAG_MAX_LIVE; and everything gl_stark_check refuses in the rest of the desc and in
 * the params, with its status. */
int gl_stark_dag_check(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params);
/* What the definitions above give for a DAG that passes the DAG's own rules (params are not looked at): max live, the largest
 * degree of a constraint, and the number of instructions of the compiled program (one per node kept, one per constraint).  Any
 * out pointer may be null. */
int gl_stark_dag_stats(const gl_stark_desc* desc, const gl_stark_dag* dag, uint32_t* max_live, uint32_t* max_degree, uint32_t* num_instructions);
/* gl_stark_create for a table in DAG form: the DAG is compiled once into instructions (`op dst_slot, a, b` and `emit filter, a`, four
 * words each; the host is the scheduler and a linear-scan slot allocator, the constants are canonicalised) and uploaded.  The handle is an ordinary
 * gl_stark: every entry above that takes one works on it unchanged, and the proof's layout is the one documented there. */
int gl_stark_dag_create(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, gl_stark** out);
/* gl_stark_verify for a table in DAG form: the same checks in the same order with the same GL_CHECK_* codes; the constraints at zeta
 * come from a host interpreter of the same compiled program over the extension field. */
int gl_stark_dag_verify(const gl_stark_desc* desc, const gl_stark_dag* dag, const gl_fri_params* params, const uint8_t* proof_bytes, size_t num_bytes,
                        uint32_t* check);

/* ---- STARK table sets: cross-table lookups as data ----------------------------------------------------
 * evm/src/cross_table_lookup.rs for any number of tables: every table is a gl_stark_desc with its gl_fri_params (degree_bits may
 * differ per table), and the lookups between them are data.  What is here: the description and its validation; the CTL running
 * products Z -- `partial_products` (cross_table_lookup.rs:279-306) -- computed on the device and committed together with the table's
 * permutation Zs (the from_values of evm/src/prover.rs:341-352); and the quotient with the CTL checks after the permutation checks, as
 * phase entries per table.  With gl_challenger_compact, gl_open_at (the CTL Zs at g^-1) and gl_prove_openings on the three-batch
 * instance a caller that keeps the transcript has every device phase of evm's prove_single_table; gl_stark_set_prove is all of them in
 * one call on the library's challenger, gl_stark_set_verify the host verifier.  evm's own tables and trace generation, PublicValues,
 * the recursive circuits, hiding and a lane pool for set proofs stay out of scope.
 * Proof bytes -- PARITY UNPINNED, as for gl_stark_prove: the concatenation, in table order, of per-table proofs in that layout with
 * two changes: the Z cap is always present, and ctl_zs_last[num_ctl_zs] (ONE word each: base-field evaluations at g^-1) stands between
 * permutation_ctl_zs_next and quotient_polys:
 *   trace_cap | permutation_ctl_zs_cap | quotient_polys_cap
 *   local_values | next_values | permutation_ctl_zs[nz + nctl] | permutation_ctl_zs_next[nz + nctl] | ctl_zs_last[nctl] | quotient_polys
 *   the FriProof of the three-batch instance | public_inputs
 * The CTL challenges are not written: they are derived.  The size is fixed by the description.
 * The flat encoding.  Three pools, each consumed in order:
 *   Columns (cross_table_lookup.rs:24-116): Column k is  constant_k + sum_t coeff_t * trace[column_t]  over its column_num_terms[k]
 *     terms (0 terms = a constant); coefficients and constants may be non-canonical; one trace column twice in a Column is refused
 *     (the reference's debug_assert "Duplicate columns").
 *   TableWithColumns: twc_table[i], and its twc_num_columns[i] (1..16) Columns are the next of the Column pool, followed by ONE more,
 *     the filter Column, where twc_has_filter[i] = 1.
 *   CrossTableLookups: lookup l takes the next lookup_num_looking[l] (1..8) TableWithColumns as its looking tables and the one after
 *     them as its looked table; all of them have the same number of Columns (cross_table_lookup.rs:169-171).
 * A table may stand in several lookups, be looking and looked, and stand twice in one lookup.
 * Derived as the reference does: a table's CTL Zs are in the order of cross_table_lookup_data (cross_table_lookup.rs:220-277): lookup
 * by lookup, challenge by challenge, the looking tables in order, then the looked one; num_ctl_zs is that of :178-185; a table's Z
 * oracle holds its permutation Zs first, then its CTL Zs; the FriInstanceInfo is that of evm/src/stark.rs:83-142 (a third batch at
 * g^-1 with the CTL Zs only; without a CTL Z there is no third batch). */
#define GL_STARK_SET_MAX_TABLES 8u
#define GL_CTL_MAX_TERMS 64u            /* per Column */
#define GL_CTL_MAX_COLUMNS 16u          /* per TableWithColumns, the filter not counted */
#define GL_CTL_MAX_LOOKING 8u           /* looking tables per lookup */
#define GL_CTL_MAX_LOOKUPS 32u
typedef struct gl_stark_set_desc {
    uint32_t num_tables;                       /* 1..8 */
    const gl_stark_desc* tables;               /* [num_tables] */
    const gl_fri_params* params;               /* [num_tables] */
    uint32_t num_ctl_columns;                  /* the Column pool */
    const uint32_t* column_num_terms;          /* [num_ctl_columns] 0..64 */
    const uint64_t* column_constant;           /* [num_ctl_columns] */
    const uint32_t* term_column;               /* [sum of terms] trace column of the table the Column is used in */
    const uint64_t* term_coeff;                /* [sum of terms] */
    uint32_t num_twcs;                         /* the TableWithColumns pool */
    const uint32_t* twc_table;                 /* [num_twcs] */
    const uint32_t* twc_num_columns;           /* [num_twcs] 1..16 */
    const uint32_t* twc_has_filter;            /* [num_twcs] 0 | 1 */
    uint32_t num_lookups;                      /* 0..32 */
    const uint32_t* lookup_num_looking;        /* [num_lookups] 1..8 */
} gl_stark_set_desc;
typedef struct gl_stark_set gl_stark_set;      /* a checked set with every table's tables and CTL programs in HBM */
/* Validation, the same in every entry below; host code, no GPU.  Per table everything gl_stark_check refuses.  Across tables
 * GL_ERR_ARG unless hasher, rate_bits, cap_height, num_query_rounds, proof_of_work_bits and num_challenges agree and every reduction
 * of every table has the same arity bits (one reduction strategy).  GL_ERR_ARG for a count outside the caps above, a null table, a
 * table index or a trace column out of range, a duplicate column in a Column, lookups whose TableWithColumns differ in their number
 * of Columns, pools that the lookups do not consume exactly, a table with neither permutation pairs nor a CTL Z (the reference asserts
 * "No CTL?", evm/src/prover.rs:339), and a filtered TableWithColumns on a table of constraint_degree < 3: with a filter f the
 * transition check Z(g x) - Z(x) (f c + 1 - f) has three trace-degree factors and needs q >= 2; without one it has two and q >= 1
 * suffices.  The gl_fri_params rules are applied to each table's three-batch instance. */
int gl_stark_set_check(const gl_stark_set_desc* desc);
/* The counts the description fixes for table `table`: permutation Zs (stark.rs:216-221) and CTL Zs (cross_table_lookup.rs:178-185).
 * Host code; either out may be null. */
int gl_stark_set_num_zs(const gl_stark_set_desc* desc, uint32_t table, uint32_t* num_permutation_zs, uint32_t* num_ctl_zs);
/* gl_stark_create for every table and the CTL Column programs of every table uploaded once.  One context per handle, as for gl_stark. */
int gl_stark_set_create(gl_ctx* ctx, const gl_stark_set_desc* desc, gl_stark_set** out);
void gl_stark_set_free(gl_stark_set* s) GL_NOEXCEPT;
/* Diagnostic: the CTL Zs of table `table` by value, h_out[num_ctl_zs][n].  d_trace_values [num_columns][n] trace VALUES on the device
 * (may be non-canonical), ctl_challenges[num_challenges][2] = (beta, gamma) of get_grand_product_challenge_set, may be non-canonical.
 * Z[i] = prod_{i' <= i} factor[i'] -- INCLUSIVE, unlike the permutation Zs -- with factor = combine(columns(row)) =
 * reduce_with_powers(evals, beta) + gamma where filter(row) = 1 (or there is no filter) and 1 where filter(row) = 0; any other filter
 * value is GL_ERR_ARG "non-binary CTL filter" (the reference asserts).  GL_ERR_ARG for a table without CTL Zs.  d_trace_values: READ-ONLY. */
int gl_stark_set_ctl_z_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* ctl_challenges,
                              uint64_t* h_out);
/* The committed Z batch of table `table` (evm/src/prover.rs:341-352): its permutation Zs (gl_stark_permutation_zs' values under
 * permutation_challenges[q][num_challenges][2]; null exactly for a table without pairs), then its CTL Zs.  d_trace_values: READ-ONLY. */
int gl_stark_set_zs(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const uint64_t* d_trace_values, const uint64_t* permutation_challenges,
                    const uint64_t* ctl_challenges, gl_batch** zs);
/* gl_stark_quotient_values for table `table` of a set: after the Stark's constraints and the permutation checks,
 * eval_cross_table_lookup_checks (cross_table_lookup.rs:374-414, the order of evm/src/vanishing_poly.rs): per CTL Z, in order,
 * constraint_first_row(Z - select(f, combine(local))) and constraint_transition(Z_next - Z select(f_next, combine(next))) with
 * select(f, x) = f x + 1 - f.  zs is the batch gl_stark_set_zs returns (permutation Zs, then CTL Zs; never null);
 * permutation_challenges is null exactly for a table without pairs.  h_out[num_challenges][n << quotient_degree_bits]; no degree check. */
int gl_stark_set_quotient_values(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs,
                                 const uint64_t* permutation_challenges, const uint64_t* ctl_challenges, const uint64_t* alphas,
                                 const uint64_t* public_inputs, uint64_t* h_out);
/* The same, then what gl_stark_quotient_polys does with the values: coset_ifft, the trim_to_len(q n) check (GL_ERR_ARG where it sees a
 * non-zero coefficient; with q a power of two it has nothing to look at), the chunks of n and from_coeffs. */
int gl_stark_set_quotient_polys(gl_ctx* ctx, const gl_stark_set* s, uint32_t table, const gl_batch* trace, const gl_batch* zs,
                                const uint64_t* permutation_challenges, const uint64_t* ctl_challenges, const uint64_t* alphas,
                                const uint64_t* public_inputs, gl_batch** quotient);
/* The size of every proof of this set. */
size_t gl_stark_set_proof_size(const gl_stark_set* s) GL_NOEXCEPT;
/* prove_with_traces + prove_with_commitments (evm/src/prover.rs:94-285).  h_trace_cols[num_tables] -> [num_columns of the table] -> n
 * values (may be non-canonical); h_public_inputs[num_tables] -> [num_public_inputs of the table] (an entry may be null for a table
 * without any).  In order: every trace committed; every trace cap observed in table order; the CTL challenge set
 * (get_grand_product_challenge_set: beta, gamma per challenge); then per table in order, on the SAME challenger: compact; the
 * permutation challenge sets if it has pairs; the Z batch (gl_stark_set_zs), its cap observed; alphas; the quotient, its cap observed;
 * zeta, GL_ERR_ZETA_IN_SUBGROUP as for gl_stark_prove; StarkOpeningSet::new (evm/src/proof.rs:224-259); the openings observed in
 * to_fri_openings order (three batches, ctl_zs_last lifted to the extension); gl_prove_openings' path on the three-batch instance.
 * *num_bytes = gl_stark_set_proof_size(s) always.  A non-binary filter, a zero permutation denominator and a trace the trim check can see
 * to be wrong are GL_ERR_ARG as in the phase entries; traces that are not consistent across tables yield a proof the verifier rejects. */
int gl_stark_set_prove(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* const* h_trace_cols, const uint64_t* const* h_public_inputs,
                       uint8_t* h_out, size_t cap_bytes, size_t* num_bytes);
/* the same with the traces already in HBM: d_cols is a HOST array of num_tables device pointers -> [num_columns][n], each READ-ONLY */
int gl_stark_set_prove_device(gl_ctx* ctx, const gl_stark_set* s, const uint64_t* const* d_cols, const uint64_t* const* h_public_inputs,
                              uint8_t* h_out, size_t cap_bytes, size_t* num_bytes);
/* verify_proof + verify_stark_proof_with_challenges + verify_cross_table_lookups (evm/src/verifier.rs:29-216, cross_table_lookup.rs:542-569).
 * Host code, no GPU.  GL_OK, or GL_ERR_VERIFY with *check (may be null) = the GL_CHECK_* code of the first failing check and *table (may
 * be null) = the table it failed in (num_tables for a check that belongs to no single table: the total length, GL_CHECK_CTL).  Order:
 * TRUNCATED / LENGTH on the total size; the trace caps and the CTL challenges; then TABLE BY TABLE in order: its challenges
 * (compact first), the vanishing identity at zeta over the extension field with the CTL checks on the Zs after the permutation ones
 * (CtlCheckVars::from_proofs): VANISHING; gl_verify_openings' checks on its three-batch instance in their order; LAST, over all tables,
 * per lookup and challenge prod looking ctl_zs_last == looked ctl_zs_last: GL_CHECK_CTL.  So a changed ctl_zs_last word is answered by the
 * FRI checks of its table (the batch at g^-1 no longer matches the committed polynomial), not by GL_CHECK_CTL; GL_CHECK_CTL is what
 * an honestly proven but inconsistent system gets. */
int gl_stark_set_verify(const gl_stark_set_desc* desc, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check, uint32_t* table);
/* The same three for a set some of whose tables are in DAG form: dags[num_tables], a null entry = that table's term list, a non-null
 * one = a gl_stark_dag beside a table desc without a term list (gl_stark_dag_check's rules).  A null dags is the plain entry.  The
 * handle is an ordinary gl_stark_set: every gl_stark_set_* phase and prove entry works on it unchanged, and the CTL checks follow the
 * DAG's constraints and the permutation checks exactly as they follow a term list's. */
int gl_stark_set_dag_check(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags);
int gl_stark_set_dag_create(gl_ctx* ctx, const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, gl_stark_set** out);
int gl_stark_set_dag_verify(const gl_stark_set_desc* desc, const gl_stark_dag* const* dags, const uint8_t* proof_bytes, size_t num_bytes, uint32_t* check,
                            uint32_t* table);

/* ---- STARK lookups: the permuted columns of a range check ----------------------------------------------
 * evm/src/lookup.rs: a table is range-checked with the Halo2-style lookup argument.  Its two constraints (eval_lookups, lookup.rs:13-34)
 * are ordinary terms of a gl_stark_desc and its two permutations ordinary pairs; what is here are its COLUMNS, permuted_cols
 * (lookup.rs:65-127), the one generic trace-generation function of the reference: both columns canonicalised and sorted ascending as
 * unsigned 64-bit integers (:79-88); then the merge of :93-117, which gives input position i the table value equal to it where one is
 * left, else the top of a LIFO stack of the table values passed over, else defers it; the deferred positions and the positions the loop
 * did not reach take the stack's values from the bottom followed by the table values the loop did not reach (:119-124).
 * ArithmeticStark::generate_range_checks calls it once per shared column against one RANGE_COUNTER column (arithmetic_stark.rs:97-118),
 * MemoryStark once (memory_stark.rs:148). */
typedef struct gl_stark_lookup { uint32_t col_input, col_table, col_permuted_input, col_permuted_table; } gl_stark_lookup;
/* permuted_cols for `count` lookups of one device trace d_cols[num_columns][n], in place: for every lookup column col_permuted_input
 * becomes the sorted canonical input column and col_permuted_table exactly the permuted_table of the reference's loop.  d_cols: IN
 * PLACE, all n words of the two output columns of every lookup; input and table columns, and columns no lookup names, keep their
 * values (the inputs may hold non-canonical words: they are canonicalised in the context's scratch); outputs are canonical.  Defined for any input: a value that is not
 * in the table is no error here (the reference does not assert; such a trace fails the constraints).  Two lookups may share an input
 * or a table column -- a shared column is sorted once (a shared table once per call, a shared input once per chunk of 2^23 / n lookups:
 * DESIGN.md section 19) -- but not an output.  Stream-ordered on the context; temporaries come from its pool.  No per-lookup serial pass: sorts, binary searches, two prefix sums and a stable sort by stack level.
 * GL_ERR_ARG for: a null pointer; count == 0 or count > 1024; n no power of two, n < 2 or n > 2^24; a column index >= num_columns; an
 * output column that is also an input, table or output column of any lookup of the call. */
int gl_stark_lookup_columns(gl_ctx* ctx, uint64_t* d_cols, uint32_t num_columns, size_t n, const gl_stark_lookup* lookups, uint32_t count);
/* The same function on host arrays, any n >= 1: the reference's sequential algorithm, statement by statement (lookup.rs:65-127).  No
 * GPU.  The outputs may not overlap the inputs. */
int gl_permuted_cols_host(const uint64_t* h_inputs, const uint64_t* h_table, size_t n, uint64_t* h_permuted_inputs, uint64_t* h_permuted_table);

/* ---- MemoryStark: evm's memory table, its description and its trace ------------------------------------
 * evm/src/memory: the table every other table of evm/ feeds through ctl_memory (all_stark.rs:174-204).  What is here: its columns
 * (memory/columns.rs), its constraints as a gl_stark_desc (memory_stark.rs:243-321, :450-459), and MemoryStark::generate_trace
 * (memory_stark.rs:120-237) from a log of memory operations -- on the host, the reference's loops statement by statement, and on the
 * device without a per-op serial pass.  evm's other tables, the CPU table's memory columns, eval_ext_circuit and
 * timestamps above 32 bits stay out of scope. */
#define GL_MEMORY_NUM_CHANNELS 6u                 /* memory/mod.rs: NUM_CHANNELS */
#define GL_MEMORY_VALUE_LIMBS 8u                  /* memory/mod.rs: VALUE_LIMBS  */
#define GL_MEMORY_FILTER 0u                       /* memory/columns.rs:7-38 */
#define GL_MEMORY_TIMESTAMP 1u
#define GL_MEMORY_IS_READ 2u
#define GL_MEMORY_ADDR_CONTEXT 3u
#define GL_MEMORY_ADDR_SEGMENT 4u
#define GL_MEMORY_ADDR_VIRTUAL 5u
#define GL_MEMORY_VALUE_START 6u                  /* value_limb(i) = GL_MEMORY_VALUE_START + i, i < 8 */
#define GL_MEMORY_CONTEXT_FIRST_CHANGE 14u
#define GL_MEMORY_SEGMENT_FIRST_CHANGE 15u
#define GL_MEMORY_VIRTUAL_FIRST_CHANGE 16u        /* columns 17..21 are unused and zero: RANGE_CHECK = VIRTUAL_FIRST_CHANGE + NUM_CHANNELS */
#define GL_MEMORY_RANGE_CHECK 22u
#define GL_MEMORY_COUNTER 23u
#define GL_MEMORY_RANGE_CHECK_PERMUTED 24u
#define GL_MEMORY_COUNTER_PERMUTED 25u
#define GL_MEMORY_NUM_COLUMNS 26u
#define GL_MEMORY_MAX_LOG_ROWS 24u
/* MemoryOp (witness/memory.rs:80-87), 56 bytes */
typedef struct gl_memory_op {
    uint32_t filter, is_read;             /* 0 / 1 */
    uint32_t context, segment, virt;      /* MemoryAddress; 32 bits each, as new_u256s enforces */
    uint32_t timestamp;                   /* clock * NUM_CHANNELS + channel; this library: < 2^32 */
    uint32_t value[8];                    /* U256, little-endian 32-bit limbs */
} gl_memory_op;
/* MemoryStark as data (memory_stark.rs:243-321, :450-459): *out points at static tables, host code, no GPU.  26 columns, no public
 * inputs, constraint_degree 3, num_challenges left 0 for the caller's StarkConfig to fill in a copy; the 21 constraints of
 * eval_packed_generic in the order it yields them with their products expanded to term lists, then the two of eval_lookups on
 * (RANGE_CHECK_PERMUTED, COUNTER_PERMUTED) (lookup.rs:13-34); the permutation pairs (22, 24) and (23, 25). */
int gl_memory_stark_desc(const gl_stark_desc** out);
/* MemoryStark::generate_trace (memory_stark.rs:120-237) on host memory, statement by statement, no GPU: the stable sort_by_key by
 * (context, segment, virt, timestamp), fill_gaps (:163-192), pad_memory_ops (:194-212), the second sort, into_row (:52-70),
 * generate_first_change_flags_and_rc (:73-118), COUNTER and permuted_cols (:143-151).  *n_rows = the trace's height n, a power of
 * two; cols_out[26][n] canonical, or null to ask for n alone.  Refusals, all before anything is written: GL_ERR_ARG for a null ops
 * or n_rows, num_ops == 0, a filter or is_read other than 0 / 1, a log on which the assertion of :112-116 fails (a context or segment
 * step, minus one, that is >= n: fill_gaps does not fill those), and capacity_rows < n with a non-null cols_out; GL_ERR_UNSUPPORTED
 * for n above 2^24. */
int gl_memory_trace_host(const gl_memory_op* ops, size_t num_ops, uint64_t* cols_out, size_t capacity_rows, size_t* n_rows);
/* The same on the device, as a handle: the height is known before the caller makes its gl_stark.  _new takes the log from host
 * memory, _new_device from HBM (d_ops: READ-ONLY; it is not needed after the call returns); both sort it, count the rows fill_gaps
 * will add per neighbour pair, and wait ONCE for the stream, for n.  The refusals and their codes are gl_memory_trace_host's.  The
 * handle holds a reference to the context. */
typedef struct gl_memory_trace gl_memory_trace;
int gl_memory_trace_new(gl_ctx* ctx, const gl_memory_op* h_ops, size_t num_ops, gl_memory_trace** out);
int gl_memory_trace_new_device(gl_ctx* ctx, const gl_memory_op* d_ops, size_t num_ops, gl_memory_trace** out);
size_t gl_memory_trace_rows(const gl_memory_trace* t) GL_NOEXCEPT;
/* All 26 columns of the trace, d_cols[26][n], the two permuted columns included (gl_stark_lookup_columns' body on the lookup
 * (22, 23, 24, 25); a trace of one row is written without it).  d_cols: OUTPUT, all 26 n words, the unused columns 17..21 (zero)
 * included.  Stream-ordered on the handle's context, temporaries from its pool, no
 * host synchronisation; may be called any number of times.  No per-op serial pass: a prefix sum over the per-pair counts places every
 * op, one thread per output row finds its source by binary search. */
int gl_memory_trace_fill(gl_memory_trace* t, uint64_t* d_cols);
void gl_memory_trace_free(gl_memory_trace* t) GL_NOEXCEPT;

/* ---- prove() ---------------------------------------------------------------------------------------*/
/* plonk::prover::prove (plonky2/src/plonk/prover.rs:102-329) from step 4 on, i.e. given the FULL witness matrix
 * `MatrixWitness.wire_values` (iop/witness.rs:256-258) h_wires[num_wires][n] and the public inputs.  Every
 * polynomial stays device-resident; the host only sees Merkle caps, openings and query answers.  The PoW
 * witness is the smallest valid one (the 1-thread order of fri/prover.rs:141-152).
 * Returns GL_ERR_ZETA_IN_SUBGROUP for prover.rs:280-283. */
int gl_prove(gl_ctx* ctx, const gl_circuit* c, const uint64_t* h_wires, const uint64_t* h_public_inputs,
             size_t num_public_inputs, gl_proof** out);
/* same with the witness as the reference stores it, one host vector per wire: h_wire_columns[num_wires] -> n values each
 * (`MatrixWitness.wire_values: Vec<Vec<F>>`), so that the caller does not have to flatten 135 vectors first */
int gl_prove_columns(gl_ctx* ctx, const gl_circuit* c, const uint64_t* const* h_wire_columns,
                     const uint64_t* h_public_inputs, size_t num_public_inputs, gl_proof** out);
/* same with the witness matrix already resident in HBM (d_wires[num_wires][n]: READ-ONLY, in all four gl_prove_device* entries) */
int gl_prove_device(gl_ctx* ctx, const gl_circuit* c, const uint64_t* d_wires, const uint64_t* h_public_inputs,
                    size_t num_public_inputs, gl_proof** out);
/* same, with public_inputs_hash = hash_no_pad(public_inputs) (prover.rs:126-127) supplied by the caller -- the witness
 * generator's sponge produces it as a by-product, and hashing 3 m^2 inputs is a sequential host job */
int gl_prove_device_hashed(gl_ctx* ctx, const gl_circuit* c, const uint64_t* d_wires, const uint64_t* h_public_inputs,
                           size_t num_public_inputs, const uint64_t public_inputs_hash[4], gl_proof** out);
/* gl_prove_device with the salt of the three salted commitments of a zero-knowledge circuit drawn from `seed` (NULL = OS entropy, which is
 * what every other gl_prove* entry and both pools use).  Ignored without zero knowledge. */
int gl_prove_device_seeded(gl_ctx* ctx, const gl_circuit* c, const uint64_t* d_wires, const uint64_t* h_public_inputs,
                           size_t num_public_inputs, const uint8_t seed[32], gl_proof** out);
/* Many independent proofs in flight on one GPU from one call -- what the reference gets from its Rayon pool when a batch of
 * witnesses is proved.  The pool owns one device-resident circuit and `lanes` contexts (HIP stream, allocator, witness
 * generator each); item i is proved on lane i % lanes by `lanes` host threads inside the call.  `hc` is borrowed. */
typedef struct gl_prover_pool gl_prover_pool;
int gl_prover_pool_create(int device, const gl_host_circuit* hc, uint32_t lanes, gl_prover_pool** out);
uint32_t gl_prover_pool_lanes(const gl_prover_pool* p) GL_NOEXCEPT;
const gl_circuit* gl_prover_pool_circuit(const gl_prover_pool* p) GL_NOEXCEPT;     /* for gl_circuit_digest / _constants_sigmas_cap */
/* a[i], b[i]: row-major m x m operands on the host; filler_seeds may be null (seed i); out_proofs[count] */
int gl_prover_pool_prove_matmul(gl_prover_pool* p, size_t count, const uint64_t* const* a, const uint64_t* const* b,
                                const uint64_t* filler_seeds, gl_proof** out_proofs);
/* The pool for ANY circuit the library proves (what gl_circuit_create takes), every lane warmed up (gl_circuit_warm_up), and `count`
 * proofs from HOST witnesses on it: columns[i][j] = wire column j (n values) of witness i, as MatrixWitness.wire_values holds them
 * (iop/witness.rs:256-258), public_inputs[i] = its num_public_inputs values; item i goes through gl_prove_columns on lane i % lanes.
 * The batch analogue of the INTEGRATION.md section-3 patch: a Rayon `par_iter` over witnesses becomes one call. */
int gl_prover_pool_create_generic(int device, const gl_circuit_desc* desc, const uint64_t* h_constants_sigmas, uint32_t lanes, gl_prover_pool** out);
int gl_prover_pool_prove_columns(gl_prover_pool* p, size_t count, const uint64_t* const* const* columns, const uint64_t* const* public_inputs,
                                 gl_proof** out_proofs);
void gl_prover_pool_free(gl_prover_pool* p) GL_NOEXCEPT;

/* ProofWithPublicInputs::to_bytes (plonk/proof.rs:104-110; util/serialization/mod.rs:1939-1981) */
size_t gl_proof_num_bytes(const gl_proof* p) GL_NOEXCEPT;
int gl_proof_bytes(const gl_proof* p, uint8_t* h_out, size_t cap);
/* intermediates, for parity tests: betas[2] gammas[2] alphas[2] zeta[2] fri_alpha[2] pow_witness pi_hash[4],
 * then the FRI betas (2 words each); returns the number of words written */
size_t gl_proof_challenges(const gl_proof* p, uint64_t* h_out) GL_NOEXCEPT;
int gl_proof_caps(const gl_proof* p, uint64_t* h_out /* [3][2^cap_height][4]: wires, zs_pp, quotient */);
/* the next two need gl_ctx_capture_intermediates(ctx, 1) before proving (two extra device->host copies per proof) */
int gl_ctx_capture_intermediates(gl_ctx* ctx, int enable);
int gl_proof_zs_partial_products(const gl_proof* p, uint64_t* h_out /* [20][n] values; [34][n] with lookups: the 14 lookup polynomials follow */);
int gl_proof_quotient_chunks(const gl_proof* p, uint64_t* h_out /* [16][n] coefficients */);
size_t gl_proof_query_indices(const gl_proof* p, uint64_t* h_out) GL_NOEXCEPT;
void gl_proof_free(gl_proof* p) GL_NOEXCEPT;

/* ---- verify() --------------------------------------------------------------------------------------*/
/* VerifierCircuitData::verify (plonky2/src/plonk/circuit_data.rs:208-215 -> plonk/verifier.rs:15-115, fri/verifier.rs:
 * 62-260) for circuits over the demo's gate set: CommonCircuitData = *desc, VerifierOnlyCircuitData =
 * (constants_sigmas_cap[2^cap_height][4], circuit_digest), proof = ProofWithPublicInputs::to_bytes().  Host code, no
 * GPU needed (as in the reference).  GL_OK = accepted; GL_ERR_VERIFY = rejected, gl_last_error() names the failing
 * check ("vanishing polynomial identity fails at zeta", "invalid proof of work witness", "initial Merkle proof fails",
 * "FRI consistency check fails", "FRI step Merkle proof fails", "final polynomial evaluation is invalid",
 * "malformed proof: ..."). */
int gl_verify(const gl_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
              const uint8_t* proof_bytes, size_t num_bytes);
int gl_host_circuit_verify(const gl_host_circuit* hc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                           const uint8_t* proof_bytes, size_t num_bytes);

/* ---- verify(), many proofs at once -------------------------------------------------------------------*/
/* The rejecting site of gl_verify as a number: one code per check, in the order gl_verify makes them.  gl_verify_check_message
 * gives the text gl_verify leaves in gl_last_error() for that site ("" for GL_CHECK_ACCEPTED).  Host code. */
#define GL_CHECK_ACCEPTED 0
#define GL_CHECK_VERIFIER_DATA 1          /* malformed verifier data: a 25-byte hash with non-zero padding bytes */
#define GL_CHECK_STEP_PATH_LENGTH 2       /* malformed proof: FRI step Merkle path has the wrong length */
#define GL_CHECK_INITIAL_PATH_LENGTH 3    /* malformed proof: initial Merkle path has the wrong length */
#define GL_CHECK_TRUNCATED 4              /* malformed proof: truncated */
#define GL_CHECK_PUBLIC_INPUT_COUNT 5     /* malformed proof: wrong number of public inputs */
#define GL_CHECK_LENGTH 6                 /* malformed proof: length mismatch */
#define GL_CHECK_VANISHING 7              /* vanishing polynomial identity fails at zeta (plonk/verifier.rs:64-101) */
#define GL_CHECK_POW 8                    /* invalid proof of work witness (fri/verifier.rs:49-60) */
#define GL_CHECK_INITIAL_MERKLE 9         /* initial Merkle proof fails (fri/verifier.rs:104-122, hash/merkle_proofs.rs:54-75) */
#define GL_CHECK_FRI_CONSISTENCY 10       /* FRI consistency check fails (fri/verifier.rs:206-209) */
#define GL_CHECK_STEP_MERKLE 11           /* FRI step Merkle proof fails (fri/verifier.rs:219-225) */
#define GL_CHECK_FINAL_POLY 12            /* final polynomial evaluation is invalid (fri/verifier.rs:231-239) */
#define GL_CHECK_DESCRIPTION 13           /* not a rejection: gl_verify answers GL_ERR_ARG, the proof is too short for the description's counts */
#define GL_CHECK_CTL 14                   /* gl_stark_set_verify: a cross-table lookup's looking Z products differ from the looked Z (cross_table_lookup.rs:542-569) */
const char* gl_verify_check_message(uint32_t check) GL_NOEXCEPT;
/* VerifierCircuitData::verify for `count` proofs of one circuit.  Per proof the decode, the transcript, the vanishing identity at
 * zeta and the proof of work run on the host (on up to host_threads threads; 0 means 1, at most 64); the Merkle paths
 * (hash/merkle_proofs.rs:54-75) and the FRI queries (fri/verifier.rs:124-241) of all proofs that pass them run on the device in two
 * launches per chunk of max_batch (1..4096) proofs, on the context's stream.
 * gl_batch_verifier_new accepts the descriptions gl_verify accepts, with its checks, order and codes; in addition a
 * fri_arity_bits[r] > 4 is GL_ERR_UNSUPPORTED (no builder here produces one), and a description whose proofs exceed 2^24 words
 * is GL_ERR_ARG.  It uploads the cap and allocates device and pinned staging for max_batch proofs once.
 * gl_batch_verifier_verify returns GL_OK when every proof was judged, whatever the verdicts, and another code only for a failure
 * of the machinery (HIP, memory, null argument).  verdicts[i] is what gl_verify returns for proofs[i] alone (GL_OK or
 * GL_ERR_VERIFY; GL_ERR_ARG with GL_CHECK_DESCRIPTION for a proof shorter than the description's counts), checks[i] (may be null)
 * the GL_CHECK_* code of the check gl_verify would have reported first.  count may exceed max_batch and may be 0.  Calls on one
 * verifier are serialised; verifiers on different contexts run side by side. */
typedef struct gl_batch_verifier gl_batch_verifier;
int gl_batch_verifier_new(gl_ctx* ctx, const gl_circuit_desc* desc, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                          uint32_t max_batch, uint32_t host_threads, gl_batch_verifier** out);
int gl_batch_verifier_verify(gl_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count,
                             int32_t* verdicts /* [count] */, uint32_t* checks /* [count], may be null */);
void gl_batch_verifier_free(gl_batch_verifier* v) GL_NOEXCEPT;

/* verify_fri_proof (fri/verifier.rs:62-241) for `count` claims over one (gl_fri_params, gl_fri_instance): the batched
 * gl_verify_openings.  Per claim everything gl_verify_openings does before its query loop runs on the host (the coset check of the
 * claim's points, the decode, the challenges, the proof of work, the reduced openings; on up to host_threads threads; 0 means 1, at
 * most 64); the Merkle paths and the queries of all claims that pass run on the device in two launches per chunk of max_batch
 * (1..4096) claims, on the context's stream.  The instance's own points are ignored: every claim brings its own.
 * gl_openings_batch_verifier_new accepts what gl_verify_openings accepts of params and instance, with its checks, order, codes and
 * texts; in addition a fri_arity_bits[r] > 4 is GL_ERR_UNSUPPORTED, and a proof above 2^24 words or a batch above 2^31 paths is
 * GL_ERR_ARG.  Device and pinned staging for max_batch claims is allocated once, there.
 * gl_openings_batch_verifier_verify returns GL_OK when every claim was judged, whatever the verdicts, and another code only for a
 * failure of the machinery (HIP, memory, a null argument).  verdicts[i] is what gl_verify_openings returns for claim i alone: GL_OK,
 * GL_ERR_VERIFY, or GL_ERR_ARG (a point on the LDE coset, a challenger under another hasher than the params'); checks[i] (may be
 * null) the GL_CHECK_* code it reports first.  count may exceed max_batch and may be 0.  A claim's challenger is consumed: its state
 * after the call is unspecified, and two claims must not share one.  Calls on one verifier are serialised; verifiers on different
 * contexts run side by side. */
typedef struct gl_openings_claim {     /* one verify_fri_proof */
    const uint64_t* caps;              /* [num_oracles][2^cap_height][4] */
    const uint64_t* openings;          /* as gl_verify_openings */
    const uint64_t (*points)[2];       /* [num_batches]: this claim's opening points */
    gl_challenger* challenger;         /* in the state gl_verify_openings expects; one per claim */
    const uint8_t* proof; size_t num_bytes;
} gl_openings_claim;
typedef struct gl_openings_batch_verifier gl_openings_batch_verifier;
int gl_openings_batch_verifier_new(gl_ctx* ctx, const gl_fri_params* params, const gl_fri_instance* instance /* points ignored */,
                                   uint32_t max_batch, uint32_t host_threads, gl_openings_batch_verifier** out);
int gl_openings_batch_verifier_verify(gl_openings_batch_verifier* v, const gl_openings_claim* claims, size_t count,
                                      int32_t* verdicts /* [count] */, uint32_t* checks /* [count], may be null */);
void gl_openings_batch_verifier_free(gl_openings_batch_verifier* v) GL_NOEXCEPT;

/* verify_stark_proof (starky/src/verifier.rs:21-145) for `count` proofs of one Stark, on top of the above.  Per proof everything
 * gl_stark_verify / gl_stark_dag_verify (dag != NULL) does before its final gl_verify_openings runs on the host threads: the byte
 * count, caps, openings, get_challenges, the vanishing identity at zeta through the term list or the compiled DAG; then the proof's
 * FriProof is a claim of the batch above at its own zeta and g zeta.  gl_stark_batch_verifier_new accepts exactly what
 * gl_stark_check (gl_stark_dag_check) accepts, with its codes and texts (a reduction of arity other than 16 is GL_ERR_UNSUPPORTED,
 * hiding too), copies the description and compiles the DAG once.  verdicts[i] / checks[i] are gl_stark_verify's (gl_stark_dag_verify's)
 * for proofs[i] alone; everything else is as for gl_openings_batch_verifier_verify. */
typedef struct gl_stark_batch_verifier gl_stark_batch_verifier;
int gl_stark_batch_verifier_new(gl_ctx* ctx, const gl_stark_desc* desc, const gl_stark_dag* dag /* null: the term-list form */,
                                const gl_fri_params* params, uint32_t max_batch, uint32_t host_threads, gl_stark_batch_verifier** out);
int gl_stark_batch_verifier_verify(gl_stark_batch_verifier* v, const uint8_t* const* proofs, const size_t* num_bytes, size_t count,
                                   int32_t* verdicts /* [count] */, uint32_t* checks /* [count], may be null */);
void gl_stark_batch_verifier_free(gl_stark_batch_verifier* v) GL_NOEXCEPT;

/* ---- circuit data as bytes --------------------------------------------------------------------------*/
/* The reference's serialised forms (plonky2/src/plonk/circuit_data.rs:125-142,208-238; util/serialization/mod.rs:739-800,
 * 1736-1790 CommonCircuitData, :909-930,1889-1906 VerifierOnlyCircuitData, :1908-1919 VerifierCircuitData = verifier_only ||
 * common; gates tagged as by DefaultGateSerializer, util/serialization/gate_serialization.rs:87-108), so that a Rust-built
 * circuit's CommonCircuitData / VerifierCircuitData bytes can be handed over instead of a hand-filled gl_circuit_desc.  Host code.
 * Representable: the demo's gates, standard_recursion_config's shape, and its zero-knowledge form (zero_knowledge = hiding = 1;
 * num_gate_rows reads as 0); anything else, mixed zero_knowledge / hiding flags among it, is GL_ERR_UNSUPPORTED when reading.  h_out may be null to query *num_bytes.  The value columns (constants, sigmas) and the
 * generators of ProverOnlyCircuitData are not part of these forms: gl_circuit_create still takes the columns. */
int gl_common_data_to_bytes(const gl_circuit_desc* desc, uint8_t* h_out, size_t cap, size_t* num_bytes);
int gl_common_data_from_bytes(const uint8_t* h_bytes, size_t num_bytes, gl_circuit_desc* out, size_t* consumed /* may be null */);
int gl_verifier_only_to_bytes(uint32_t cap_height, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4], uint8_t* h_out,
                              size_t cap, size_t* num_bytes);
int gl_verifier_only_from_bytes(const uint8_t* h_bytes, size_t num_bytes, uint32_t* cap_height, uint64_t* h_cap /* [2^h][4], may be null */,
                                size_t cap_words, uint64_t circuit_digest[4], size_t* consumed /* may be null */);
/* VerifierCircuitData::from_bytes(data).verify(proof): GL_OK = accepted, GL_ERR_VERIFY = rejected (as gl_verify) */
int gl_verify_bytes(const uint8_t* h_verifier_data, size_t num_data_bytes, const uint8_t* proof_bytes, size_t num_proof_bytes);
/* The hasher is a type parameter of these forms in Rust and not in their bytes (gl_common_data_from_bytes returns hasher = 0): the three
 * entries above for `C::Hasher = hasher`.  Under Keccak a hash is 25 bytes (util/serialization/mod.rs:248-256,1332-1338). */
int gl_verifier_only_to_bytes_h(uint32_t hasher, uint32_t cap_height, const uint64_t* constants_sigmas_cap, const uint64_t circuit_digest[4],
                                uint8_t* h_out, size_t cap, size_t* num_bytes);
int gl_verifier_only_from_bytes_h(uint32_t hasher, const uint8_t* h_bytes, size_t num_bytes, uint32_t* cap_height, uint64_t* h_cap, size_t cap_words,
                                  uint64_t circuit_digest[4], size_t* consumed);
int gl_verify_bytes_h(uint32_t hasher, const uint8_t* h_verifier_data, size_t num_data_bytes, const uint8_t* proof_bytes, size_t num_proof_bytes);

#ifdef __cplusplus
}
#endif
#endif /* PLONKY2_MI355X_H */

"""ctypes binding of libplonky2_mi355x.so (the C ABI declared in include/plonky2_mi355x.h).

The library is HIP-only: importing this module works without a GPU (so that symbol/ABI checks can run on a
CPU box), but creating a context fails loudly when no MI355X is visible.  There is no CPU fallback and the
CPU oracle under oracle/ is never imported from here.
"""
import ctypes
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
# PLONKY2_MI355X_LIB: another build of the same library (e.g. the -DNTT_ABLATION diagnostic build of tools/ablation.sh)
LIB_PATH = os.environ.get("PLONKY2_MI355X_LIB") or os.path.join(_HERE, "libplonky2_mi355x.so")

GL_OK = 0
GL_ERR_VERIFY = 6
# gl_batch_verifier_verify's per-proof codes (include/plonky2_mi355x.h GL_CHECK_*): the check of gl_verify that rejected the proof
(GL_CHECK_ACCEPTED, GL_CHECK_VERIFIER_DATA, GL_CHECK_STEP_PATH_LENGTH, GL_CHECK_INITIAL_PATH_LENGTH, GL_CHECK_TRUNCATED, GL_CHECK_PUBLIC_INPUT_COUNT,
 GL_CHECK_LENGTH, GL_CHECK_VANISHING, GL_CHECK_POW, GL_CHECK_INITIAL_MERKLE, GL_CHECK_FRI_CONSISTENCY, GL_CHECK_STEP_MERKLE, GL_CHECK_FINAL_POLY,
 GL_CHECK_DESCRIPTION, GL_CHECK_CTL) = range(15)
ERRORS = {1: "GL_ERR_ARG", 2: "GL_ERR_HIP", 3: "GL_ERR_UNSUPPORTED", 4: "GL_ERR_ZETA_IN_SUBGROUP", 5: "GL_ERR_INTERNAL", 6: "GL_ERR_VERIFY"}


class Plonky2Mi355xError(RuntimeError):
    def __init__(self, code, text):
        super().__init__("%s: %s" % (ERRORS.get(code, "error %d" % code), text))
        self.code = code


def _load():
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            "libplonky2_mi355x.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; g.build()'` "
            "or `make -C plonky2_demo_amd/csrc`.  There is no CPU fallback." % LIB_PATH)
    return ctypes.CDLL(LIB_PATH)


lib = _load()

c_u64p = ctypes.POINTER(ctypes.c_uint64)
c_vp = ctypes.c_void_p
c_sz = ctypes.c_size_t
c_u32 = ctypes.c_uint32
c_u64 = ctypes.c_uint64
c_int = ctypes.c_int

# name -> (restype, argtypes); every symbol include/plonky2_mi355x.h declares must appear here
SIGNATURES = {
    "gl_ctx_create": (c_int, [c_int, c_vp, ctypes.POINTER(c_vp)]),
    "gl_ctx_has_own_queue": (c_int, [c_vp]),
    "gl_lane_queues_live": (c_int, [c_int]),
    "gl_ctx_destroy": (None, [c_vp]),
    "gl_ctx_synchronize": (c_int, [c_vp]),
    "gl_ctx_set_scratch_elems": (c_int, [c_vp, c_sz]),
    "gl_last_error": (ctypes.c_char_p, []),
    "gl_ctx_timing_enable": (c_int, [c_vp, c_int]),
    "gl_ctx_timing_reset": (c_int, [c_vp]),
    "gl_ctx_timing_report": (c_int, [c_vp, ctypes.c_char_p, c_sz]),
    "gl_dev_alloc": (c_int, [c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_dev_free": (c_int, [c_vp, c_vp]),
    "gl_copy_h2d": (c_int, [c_vp, c_vp, c_vp, c_sz]),
    "gl_copy_d2h": (c_int, [c_vp, c_vp, c_vp, c_sz]),
    "gl_field_op": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_vp, c_sz]),
    "gl_ext_op": (c_int, [c_vp, c_int, c_vp, c_vp, c_vp, c_sz]),
    "gl_ntt_forward": (c_int, [c_vp, c_vp, c_u32, c_u32]),
    "gl_ntt_inverse": (c_int, [c_vp, c_vp, c_u32, c_u32]),
    "gl_ntt_coset_forward": (c_int, [c_vp, c_vp, c_u32, c_u32, c_u64]),
    "gl_ntt_coset_inverse": (c_int, [c_vp, c_vp, c_u32, c_u32, c_u64]),
    "gl_ntt_coset_lde": (c_int, [c_vp, c_vp, c_u32, c_u32, c_u32, c_vp]),
    "gl_fft_host": (c_int, [c_vp, c_vp, c_u32, c_u32, c_int]),
    "gl_poseidon_permute": (c_int, [c_vp, c_vp, c_sz]),
    "gl_poseidon_permute_raw": (c_int, [c_vp, c_vp, c_sz, c_int]),
    "gl_hash_rows": (c_int, [c_vp, c_vp, c_sz, c_sz, c_vp]),
    "gl_merkle_new": (c_int, [c_vp, c_vp, c_sz, c_sz, c_u32, ctypes.POINTER(c_vp)]),
    "gl_merkle_cap": (c_int, [c_vp, c_vp]),
    "gl_merkle_prove": (c_int, [c_vp, c_sz, c_vp, ctypes.POINTER(c_u32)]),
    "gl_merkle_free": (None, [c_vp]),
    "gl_batch_from_values": (c_int, [c_vp, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_from_coeffs": (c_int, [c_vp, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_from_device": (c_int, [c_vp, c_vp, c_sz, c_sz, c_u32, c_u32, c_int, ctypes.POINTER(c_vp)]),
    "gl_batch_cap": (c_int, [c_vp, c_vp]),
    "gl_batch_get_leaf": (c_int, [c_vp, c_sz, c_vp]),
    "gl_batch_get_lde_values": (c_int, [c_vp, c_sz, c_sz, c_vp]),
    "gl_batch_prove": (c_int, [c_vp, c_sz, c_vp, ctypes.POINTER(c_u32)]),
    "gl_batch_coeffs": (c_int, [c_vp, c_vp]),
    "gl_batch_lde": (c_int, [c_vp, c_vp]),
    "gl_batch_ncols": (c_sz, [c_vp]),
    "gl_batch_degree": (c_sz, [c_vp]),
    "gl_batch_dev_coeffs": (c_vp, [c_vp]),
    "gl_batch_dev_lde": (c_vp, [c_vp]),
    "gl_batch_free": (None, [c_vp]),
    "gl_matmul_circuit_build": (c_int, [c_sz, ctypes.POINTER(c_vp)]),
    "gl_matmul_circuit_build_zk": (c_int, [c_sz, ctypes.POINTER(c_vp)]),
    "gl_batch_from_values_blinded": (c_int, [c_vp, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_vp, ctypes.POINTER(c_vp)]),
    "gl_batch_from_coeffs_blinded": (c_int, [c_vp, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_vp, ctypes.POINTER(c_vp)]),
    "gl_random_elements": (c_int, [c_vp, c_vp, c_u32, c_u64, c_u64, c_vp]),
    "gl_random_elements_host": (c_int, [c_vp, c_u32, c_u64, c_u64, c_vp]),
    "gl_witness_blind": (c_int, [c_vp, c_vp, c_vp, c_vp]),
    "gl_host_circuit_desc": (c_int, [c_vp, c_vp]),
    "gl_host_circuit_row_gates": (c_int, [c_vp, c_vp]),
    "gl_host_circuit_constants_sigmas": (c_int, [c_vp, c_vp]),
    "gl_matmul_witness": (c_int, [c_vp, c_vp, c_vp, c_u64, c_vp, c_vp]),
    "gl_host_circuit_free": (None, [c_vp]),
    "gl_matmul_witgen_create": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_matmul_witgen_run": (c_int, [c_vp, c_vp, c_vp, c_u64, c_vp, c_vp, c_vp]),
    "gl_matmul_witgen_free": (None, [c_vp]),
    "gl_circuit_create": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_circuit_from_host": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_circuit_description": (c_int, [c_vp, c_vp]),
    "gl_circuit_warm_up": (c_int, [c_vp, c_vp]),
    "gl_prover_pool_create_generic": (c_int, [c_int, c_vp, c_vp, c_u32, ctypes.POINTER(c_vp)]),
    "gl_prover_pool_prove_columns": (c_int, [c_vp, c_sz, c_vp, c_vp, c_vp]),
    "gl_circuit_digest": (c_int, [c_vp, c_vp]),
    "gl_circuit_constants_sigmas_cap": (c_int, [c_vp, c_vp]),
    "gl_circuit_constants_sigmas_batch": (c_vp, [c_vp]),
    "gl_circuit_free": (None, [c_vp]),
    "gl_partial_products": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_quotient_polys": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_partial_products_lookups": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_quotient_polys_lookups": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_open_at": (c_int, [c_vp, c_vp, c_vp, c_sz, c_sz, c_vp]),
    "gl_fri_combine": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_fri_commit_round": (c_int, [c_vp, c_vp]),
    "gl_fri_fold": (c_int, [c_vp, c_vp]),
    "gl_fri_final_poly": (c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_pow_grind": (c_int, [c_vp, c_vp, c_vp, c_u32, c_u32, c_vp]),
    "gl_fri_query": (c_int, [c_vp, c_vp, c_u32, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_fri_free": (None, [c_vp]),
    "gl_ctx_capture_intermediates": (c_int, [c_vp, c_int]),
    "gl_challenger_new": (c_vp, []),
    "gl_challenger_observe": (c_int, [c_vp, c_vp, c_sz]),
    "gl_challenger_get_challenges": (c_int, [c_vp, c_vp, c_sz]),
    "gl_challenger_state": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_u32)]),
    "gl_challenger_free": (None, [c_vp]),
    "gl_prove": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_prove_columns": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_prove_device": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_prove_device_hashed": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(c_vp)]),
    "gl_prove_device_seeded": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, c_vp, ctypes.POINTER(c_vp)]),
    "gl_prover_pool_create": (c_int, [c_int, c_vp, c_u32, ctypes.POINTER(c_vp)]),
    "gl_prover_pool_lanes": (c_u32, [c_vp]),
    "gl_prover_pool_circuit": (c_vp, [c_vp]),
    "gl_prover_pool_prove_matmul": (c_int, [c_vp, c_sz, c_vp, c_vp, c_vp, c_vp]),
    "gl_prover_pool_free": (None, [c_vp]),
    "gl_proof_num_bytes": (c_sz, [c_vp]),
    "gl_proof_bytes": (c_int, [c_vp, c_vp, c_sz]),
    "gl_proof_challenges": (c_sz, [c_vp, c_vp]),
    "gl_proof_caps": (c_int, [c_vp, c_vp]),
    "gl_proof_zs_partial_products": (c_int, [c_vp, c_vp]),
    "gl_proof_quotient_chunks": (c_int, [c_vp, c_vp]),
    "gl_proof_query_indices": (c_sz, [c_vp, c_vp]),
    "gl_proof_free": (None, [c_vp]),
    "gl_verify": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz]),
    "gl_host_circuit_verify": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz]),
    "gl_circuit_create_from_classes": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp]),
    "gl_host_circuit_wire_classes": (c_int, [c_vp, c_vp]),
    "gl_common_data_to_bytes": (c_int, [c_vp, c_vp, c_sz, c_vp]),
    "gl_common_data_from_bytes": (c_int, [c_vp, c_sz, c_vp, c_vp]),
    "gl_verifier_only_to_bytes": (c_int, [c_u32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "gl_verifier_only_from_bytes": (c_int, [c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_verify_bytes": (c_int, [c_vp, c_sz, c_vp, c_sz]),
    # the hasher-carrying entry points (hasher: 0 Poseidon, 1 Keccak)
    "gl_hash_rows_h": (c_int, [c_vp, c_u32, c_vp, c_sz, c_sz, c_vp]),
    "gl_hash_or_noop_host": (c_int, [c_u32, c_vp, c_sz, c_sz, c_vp]),
    "gl_two_to_one_host": (c_int, [c_u32, c_vp, c_vp, c_sz, c_vp]),
    "gl_merkle_new_h": (c_int, [c_vp, c_u32, c_vp, c_sz, c_sz, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_from_values_h": (c_int, [c_vp, c_u32, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_from_coeffs_h": (c_int, [c_vp, c_u32, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_from_values_blinded_h": (c_int, [c_vp, c_u32, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_vp, ctypes.POINTER(c_vp)]),
    "gl_batch_from_coeffs_blinded_h": (c_int, [c_vp, c_u32, ctypes.POINTER(c_vp), c_sz, c_sz, c_u32, c_u32, c_vp, ctypes.POINTER(c_vp)]),
    "gl_batch_from_device_h": (c_int, [c_vp, c_u32, c_vp, c_sz, c_sz, c_u32, c_u32, c_int, ctypes.POINTER(c_vp)]),
    "gl_batch_hasher": (c_u32, [c_vp]),
    "gl_matmul_circuit_build_h": (c_int, [c_sz, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_pow_grind_h": (c_int, [c_vp, c_u32, c_vp, c_vp, c_u32, c_u32, c_vp]),
    "gl_challenger_new_h": (c_vp, [c_u32]),
    "gl_challenger_observe_hashes": (c_int, [c_vp, c_u32, c_vp, c_sz]),
    "gl_verifier_only_to_bytes_h": (c_int, [c_u32, c_u32, c_vp, c_vp, c_vp, c_sz, c_vp]),
    "gl_verifier_only_from_bytes_h": (c_int, [c_u32, c_vp, c_sz, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_verify_bytes_h": (c_int, [c_u32, c_vp, c_sz, c_vp, c_sz]),
    # batch verification (device Merkle paths and FRI queries)
    "gl_verify_check_message": (ctypes.c_char_p, [c_u32]),
    "gl_batch_verifier_new": (c_int, [c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_batch_verifier_verify": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_batch_verifier_free": (None, [c_vp]),
    # FRI openings of any instance (gl_fri_params*, gl_fri_instance*, ...)
    "gl_fri_combine_instance": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, ctypes.POINTER(c_vp)]),
    "gl_fri_combine_instance_per_batch": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, ctypes.POINTER(c_vp)]),
    "gl_prove_openings": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_verify_openings": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_u32)]),
    # STARK: an AIR as data (gl_stark_desc*, gl_fri_params*, ...)
    "gl_stark_check": (c_int, [c_vp, c_vp]),
    "gl_stark_create": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_free": (None, [c_vp]),
    "gl_stark_permutation_zs": (c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_quotient_values": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "gl_stark_quotient_polys": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_proof_size": (c_sz, [c_vp]),
    "gl_stark_prove": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp), c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_stark_prove_device": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_stark_verify": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_u32)]),
    # STARK constraints as an expression DAG (gl_stark_desc*, gl_stark_dag*, ...)
    "gl_stark_dag_check": (c_int, [c_vp, c_vp, c_vp]),
    "gl_stark_dag_stats": (c_int, [c_vp, c_vp, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    "gl_stark_dag_create": (c_int, [c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_dag_verify": (c_int, [c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_u32)]),
    "gl_stark_set_dag_check": (c_int, [c_vp, c_vp]),
    "gl_stark_set_dag_create": (c_int, [c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_set_dag_verify": (c_int, [c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    # STARK table sets: cross-table lookups as data (gl_stark_set_desc*, ...)
    "gl_challenger_compact": (c_int, [c_vp]),
    "gl_stark_set_check": (c_int, [c_vp]),
    "gl_stark_set_num_zs": (c_int, [c_vp, c_u32, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    "gl_stark_set_create": (c_int, [c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_set_free": (None, [c_vp]),
    "gl_stark_set_ctl_z_values": (c_int, [c_vp, c_vp, c_u32, c_vp, c_vp, c_vp]),
    "gl_stark_set_zs": (c_int, [c_vp, c_vp, c_u32, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_set_quotient_values": (c_int, [c_vp, c_vp, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp]),
    "gl_stark_set_quotient_polys": (c_int, [c_vp, c_vp, c_u32, c_vp, c_vp, c_vp, c_vp, c_vp, c_vp, ctypes.POINTER(c_vp)]),
    "gl_stark_set_proof_size": (c_sz, [c_vp]),
    "gl_stark_set_prove": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_stark_set_prove_device": (c_int, [c_vp, c_vp, c_vp, c_vp, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_stark_set_verify": (c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_u32), ctypes.POINTER(c_u32)]),
    # STARK lookups: permuted_cols (ctx, d_cols, num_columns, n, gl_stark_lookup*, count) and its host form
    "gl_stark_lookup_columns": (c_int, [c_vp, c_vp, c_u32, c_sz, c_vp, c_u32]),
    "gl_permuted_cols_host": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_memory_stark_desc": (c_int, [ctypes.POINTER(c_vp)]),
    "gl_memory_trace_host": (c_int, [c_vp, c_sz, c_vp, c_sz, ctypes.POINTER(c_sz)]),
    "gl_memory_trace_new": (c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_memory_trace_new_device": (c_int, [c_vp, c_vp, c_sz, ctypes.POINTER(c_vp)]),
    "gl_memory_trace_rows": (c_sz, [c_vp]),
    "gl_memory_trace_fill": (c_int, [c_vp, c_vp]),
    "gl_memory_trace_free": (None, [c_vp]),
    # batch verification of FRI openings of any instance, and of STARK proofs on top of it (device Merkle paths and FRI queries)
    "gl_openings_batch_verifier_new": (c_int, [c_vp, c_vp, c_vp, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_openings_batch_verifier_verify": (c_int, [c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_openings_batch_verifier_free": (None, [c_vp]),
    "gl_stark_batch_verifier_new": (c_int, [c_vp, c_vp, c_vp, c_vp, c_u32, c_u32, ctypes.POINTER(c_vp)]),
    "gl_stark_batch_verifier_verify": (c_int, [c_vp, c_vp, c_vp, c_sz, c_vp, c_vp]),
    "gl_stark_batch_verifier_free": (None, [c_vp]),
}
GL_MAX_FRI_ORACLES, GL_MAX_FRI_BATCHES = 8, 4

HASHERS = {"poseidon": 0, "keccak": 1}

# gl_circuit_desc.gate_types codes: the enum of csrc/gates.hpp, spelt out (tests/test_ext_gates.py holds the two against each other)
(G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_POSEIDON, G_BASE_SUM, G_LOOKUP, G_LOOKUP_TABLE, G_EXPONENTIATION, G_RANDOM_ACCESS,
 G_ARITHMETIC_EXT, G_MUL_EXT, G_REDUCING, G_REDUCING_EXT) = range(14)


def hasher_id(hasher):
    """"poseidon" | "keccak" (or 0 | 1) -> the C ABI's number; anything else is a ValueError."""
    if hasher in HASHERS:
        return HASHERS[hasher]
    if hasher in (0, 1) and not isinstance(hasher, bool):
        return int(hasher)
    raise ValueError("hasher must be 'poseidon' or 'keccak', not %r" % (hasher,))



class CircuitDesc(ctypes.Structure):
    """gl_circuit_desc (include/plonky2_mi355x.h)."""
    _fields_ = [
        ("degree_bits", c_u32), ("num_wires", c_u32), ("num_routed_wires", c_u32), ("num_constants", c_u32),
        ("num_selectors", c_u32), ("num_challenges", c_u32), ("quotient_degree_factor", c_u32),
        ("rate_bits", c_u32), ("cap_height", c_u32), ("proof_of_work_bits", c_u32), ("num_query_rounds", c_u32),
        ("num_fri_rounds", c_u32), ("fri_arity_bits", c_u32 * 8), ("num_public_inputs", c_u32), ("num_gates", c_u32),
        ("gate_types", ctypes.c_uint8 * 16), ("gate_params", ctypes.c_uint8 * 16), ("gate_selector_index", c_u32 * 16),
        ("gate_group_start", c_u32 * 16), ("gate_group_end", c_u32 * 16), ("k_is", c_u64 * 80),
        ("num_lookup_polys", c_u32), ("num_lookup_selectors", c_u32), ("num_luts", c_u32),
        ("last_lu_row", c_u32 * 4), ("last_lut_row", c_u32 * 4), ("first_lut_row", c_u32 * 4), ("lut_len", c_u32 * 4),
        ("lut", ctypes.c_uint16 * 2048),
        ("zero_knowledge", c_u32), ("num_gate_rows", c_u32),
        ("hasher", c_u32),
    ]

    def lookup_table(self, t):
        """Table t as a list of (input, output) pairs: `lut` holds the tables one after the other."""
        off = sum(self.lut_len[i] for i in range(t))
        return [(self.lut[2 * (off + k)], self.lut[2 * (off + k) + 1]) for k in range(self.lut_len[t])]


class FriParams(ctypes.Structure):
    """gl_fri_params: FriParams (fri/mod.rs) + C::Hasher."""
    _fields_ = [("degree_bits", c_u32), ("rate_bits", c_u32), ("cap_height", c_u32), ("proof_of_work_bits", c_u32), ("num_query_rounds", c_u32),
                ("num_fri_rounds", c_u32), ("fri_arity_bits", c_u32 * 8), ("hiding", c_u32), ("hasher", c_u32)]

    def __init__(self, degree_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, reduction_arity_bits=(), hiding=False, hasher="poseidon"):
        arity = [int(a) for a in reduction_arity_bits]
        if len(arity) > 8:
            raise ValueError("at most 8 FRI reductions")
        super().__init__(degree_bits, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, len(arity), (c_u32 * 8)(*arity), 1 if hiding else 0,
                         hasher_id(hasher))

    @classmethod
    def of_circuit(cls, d):
        """The FriParams of a gl_circuit_desc."""
        return cls(d.degree_bits, d.rate_bits, d.cap_height, d.proof_of_work_bits, d.num_query_rounds, list(d.fri_arity_bits[:d.num_fri_rounds]),
                   bool(d.zero_knowledge), d.hasher)

    @property
    def reduction_arity_bits(self):
        return list(self.fri_arity_bits[:self.num_fri_rounds])


class FriInstance(ctypes.Structure):
    """gl_fri_instance: FriInstanceInfo (fri/structure.rs).  oracles: [(num_polys, blinding), ...]; batches: [(point (2 words), [(oracle_index,
    polynomial_index), ...]), ...].  Counts beyond the C arrays are a ValueError; everything else is the library's to refuse."""
    _fields_ = [("num_oracles", c_u32), ("oracle_num_polys", c_u32 * GL_MAX_FRI_ORACLES), ("oracle_blinding", c_u32 * GL_MAX_FRI_ORACLES),
                ("num_batches", c_u32), ("points", (c_u64 * 2) * GL_MAX_FRI_BATCHES), ("batch_len", c_u32 * GL_MAX_FRI_BATCHES),
                ("polys", ctypes.POINTER(c_u32))]

    def __init__(self, oracles, batches):
        super().__init__()
        oracles, batches = list(oracles), [(tuple(int(w) for w in pt), [(int(o), int(c)) for o, c in polys]) for pt, polys in batches]
        if len(oracles) > GL_MAX_FRI_ORACLES or len(batches) > GL_MAX_FRI_BATCHES:
            raise ValueError("at most %d oracles and %d batches" % (GL_MAX_FRI_ORACLES, GL_MAX_FRI_BATCHES))
        self.num_oracles, self.num_batches = len(oracles), len(batches)
        for i, (k, blinding) in enumerate(oracles):
            self.oracle_num_polys[i], self.oracle_blinding[i] = int(k), 1 if blinding else 0
        flat = []
        for i, (pt, polys) in enumerate(batches):
            self.points[i][0], self.points[i][1] = pt
            self.batch_len[i] = len(polys)
            for o, c in polys:
                flat += [o, c]
        self._polys = (c_u32 * max(len(flat), 1))(*flat)      # kept alive with the structure
        self.polys = ctypes.cast(self._polys, ctypes.POINTER(c_u32))
        self.oracles, self.batches = oracles, batches

    @property
    def num_opened(self):
        return sum(len(polys) for _, polys in self.batches)


class OpeningsClaim(ctypes.Structure):
    """gl_openings_claim: one verify_fri_proof of gl_openings_batch_verifier_verify."""
    _fields_ = [("caps", c_vp), ("openings", c_vp), ("points", c_vp), ("challenger", c_vp), ("proof", c_vp), ("num_bytes", c_sz)]


(GL_STARK_ALL, GL_STARK_TRANSITION, GL_STARK_FIRST_ROW, GL_STARK_LAST_ROW) = range(4)      # constraint filters
(GL_STARK_LOCAL, GL_STARK_NEXT, GL_STARK_PUBLIC) = range(3)                                # operand kinds


class StarkDescStruct(ctypes.Structure):
    """gl_stark_desc.  constraints: [(filter, [(coeff, [(kind, index), ...]), ...]), ...] in the order the Stark yields them; pairs:
    [[(lhs, rhs), ...], ...] (Stark::permutation_pairs).  Nothing is checked here: refusing is gl_stark_check's."""
    _fields_ = [("num_columns", c_u32), ("num_public_inputs", c_u32), ("constraint_degree", c_u32), ("num_challenges", c_u32),
                ("num_constraints", c_u32), ("constraint_filter", ctypes.POINTER(c_u32)), ("constraint_num_terms", ctypes.POINTER(c_u32)),
                ("term_coeff", ctypes.POINTER(c_u64)), ("term_num_factors", ctypes.POINTER(c_u32)), ("factors", ctypes.POINTER(c_u32)),
                ("num_permutation_pairs", c_u32), ("pair_len", ctypes.POINTER(c_u32)), ("pair_columns", ctypes.POINTER(c_u32))]

    def __init__(self, num_columns, num_public_inputs, constraint_degree, num_challenges, constraints, pairs=()):
        super().__init__()
        filters, num_terms, coeffs, num_factors, factors = [], [], [], [], []
        for filt, terms in constraints:
            filters.append(int(filt))
            num_terms.append(len(terms))
            for coeff, ops in terms:
                coeffs.append(int(coeff))
                num_factors.append(len(ops))
                factors += [(int(kind) << 30 | int(index)) & 0xFFFFFFFF for kind, index in ops]
        pair_len = [len(p) for p in pairs]
        pair_columns = [int(c) for p in pairs for lr in p for c in lr]
        self.num_columns, self.num_public_inputs = num_columns, num_public_inputs
        self.constraint_degree, self.num_challenges = constraint_degree, num_challenges
        self.num_constraints, self.num_permutation_pairs = len(filters), len(pair_len)
        self._keep = []                                       # the tables live as long as the structure

        def table(ctype, values):
            arr = (ctype * max(len(values), 1))(*values)
            self._keep.append(arr)
            return ctypes.cast(arr, ctypes.POINTER(ctype))
        self.constraint_filter, self.constraint_num_terms = table(c_u32, filters), table(c_u32, num_terms)
        self.term_coeff, self.term_num_factors, self.factors = table(c_u64, coeffs), table(c_u32, num_factors), table(c_u32, factors)
        self.pair_len, self.pair_columns = table(c_u32, pair_len), table(c_u32, pair_columns)


# MemoryStark's columns (include/plonky2_mi355x.h GL_MEMORY_*, evm/src/memory/columns.rs) and gl_memory_op as a numpy record
GL_MEMORY_NUM_CHANNELS, GL_MEMORY_VALUE_LIMBS = 6, 8
(GL_MEMORY_FILTER, GL_MEMORY_TIMESTAMP, GL_MEMORY_IS_READ, GL_MEMORY_ADDR_CONTEXT, GL_MEMORY_ADDR_SEGMENT, GL_MEMORY_ADDR_VIRTUAL, GL_MEMORY_VALUE_START) = range(7)
(GL_MEMORY_CONTEXT_FIRST_CHANGE, GL_MEMORY_SEGMENT_FIRST_CHANGE, GL_MEMORY_VIRTUAL_FIRST_CHANGE) = (14, 15, 16)
(GL_MEMORY_RANGE_CHECK, GL_MEMORY_COUNTER, GL_MEMORY_RANGE_CHECK_PERMUTED, GL_MEMORY_COUNTER_PERMUTED, GL_MEMORY_NUM_COLUMNS) = (22, 23, 24, 25, 26)
MEMORY_OP_FIELDS = [("filter", "<u4"), ("is_read", "<u4"), ("context", "<u4"), ("segment", "<u4"), ("virt", "<u4"), ("timestamp", "<u4"), ("value", "<u4", (8,))]


(GL_STARK_NODE, GL_STARK_CONST) = (3, 4)                                                   # operand kinds of a gl_stark_dag only
(GL_STARK_OP_ADD, GL_STARK_OP_SUB, GL_STARK_OP_MUL) = range(3)
GL_STARK_DAG_MAX_NODES, GL_STARK_DAG_MAX_LIVE, GL_STARK_MAX_TERMS, GL_STARK_MAX_CONSTRAINTS = 65536, 128, 65536, 4096


def stark_operand(kind, index):
    """GL_STARK_OPERAND: an operand word of a gl_stark_dag"""
    return (int(kind) << 28 | int(index)) & 0xFFFFFFFF


class StarkDagStruct(ctypes.Structure):
    """gl_stark_dag.  nodes: [(op, operand word a, operand word b), ...] in SSA order; constants: 64-bit words; constraints: [(filter,
    operand word), ...] in the order the Stark yields them.  Nothing is checked here: refusing is gl_stark_dag_check's."""
    _fields_ = [("num_nodes", c_u32), ("node_op", ctypes.POINTER(c_u32)), ("node_a", ctypes.POINTER(c_u32)), ("node_b", ctypes.POINTER(c_u32)),
                ("num_constants", c_u32), ("constants", ctypes.POINTER(c_u64)),
                ("num_constraints", c_u32), ("constraint_filter", ctypes.POINTER(c_u32)), ("constraint_operand", ctypes.POINTER(c_u32))]

    def __init__(self, nodes, constants, constraints):
        super().__init__()
        self._keep = []

        def table(ctype, values):
            arr = (ctype * max(len(values), 1))(*values)
            self._keep.append(arr)
            return ctypes.cast(arr, ctypes.POINTER(ctype))
        self.num_nodes, self.num_constants, self.num_constraints = len(nodes), len(constants), len(constraints)
        self.node_op = table(c_u32, [int(op) & 0xFFFFFFFF for op, _, _ in nodes])
        self.node_a, self.node_b = table(c_u32, [int(a) & 0xFFFFFFFF for _, a, _ in nodes]), table(c_u32, [int(b) & 0xFFFFFFFF for _, _, b in nodes])
        self.constants = table(c_u64, [int(v) & 0xFFFFFFFFFFFFFFFF for v in constants])
        self.constraint_filter = table(c_u32, [int(f) & 0xFFFFFFFF for f, _ in constraints])
        self.constraint_operand = table(c_u32, [int(w) & 0xFFFFFFFF for _, w in constraints])


class StarkSetDescStruct(ctypes.Structure):
    """gl_stark_set_desc.  tables: [(StarkDescStruct, FriParams), ...]; lookups: [([looking, ...], looked), ...] with every TableWithColumns
    (table index, [Column, ...], filter Column or None) and every Column ([(trace column, coeff), ...], constant).  The three pools are
    written in the order the lookups consume them.  Nothing is checked here: refusing is gl_stark_set_check's."""
    _fields_ = [("num_tables", c_u32), ("tables", ctypes.POINTER(StarkDescStruct)), ("params", ctypes.POINTER(FriParams)),
                ("num_ctl_columns", c_u32), ("column_num_terms", ctypes.POINTER(c_u32)), ("column_constant", ctypes.POINTER(c_u64)),
                ("term_column", ctypes.POINTER(c_u32)), ("term_coeff", ctypes.POINTER(c_u64)),
                ("num_twcs", c_u32), ("twc_table", ctypes.POINTER(c_u32)), ("twc_num_columns", ctypes.POINTER(c_u32)),
                ("twc_has_filter", ctypes.POINTER(c_u32)), ("num_lookups", c_u32), ("lookup_num_looking", ctypes.POINTER(c_u32))]

    def __init__(self, tables, lookups):
        super().__init__()
        tables = list(tables)
        self._keep = [tables]                                  # the per-table structures own the tables the copies below point into
        descs, params = (StarkDescStruct * max(len(tables), 1))(), (FriParams * max(len(tables), 1))()
        for i, (desc, fri) in enumerate(tables):
            ctypes.memmove(ctypes.byref(descs[i]), ctypes.byref(desc), ctypes.sizeof(StarkDescStruct))
            ctypes.memmove(ctypes.byref(params[i]), ctypes.byref(fri), ctypes.sizeof(FriParams))
        self._keep += [descs, params]
        self.num_tables, self.tables, self.params = len(tables), descs, params
        num_terms, constants, term_column, term_coeff, twc_table, twc_ncols, twc_filter, looking_counts = [], [], [], [], [], [], [], []
        for looking, looked in lookups:
            looking_counts.append(len(looking))
            for table, columns, filter_column in list(looking) + [looked]:
                twc_table.append(int(table))
                twc_ncols.append(len(columns))
                twc_filter.append(0 if filter_column is None else 1)
                for terms, constant in list(columns) + ([] if filter_column is None else [filter_column]):
                    num_terms.append(len(terms))
                    constants.append(int(constant) & 0xFFFFFFFFFFFFFFFF)
                    term_column += [int(c) & 0xFFFFFFFF for c, _ in terms]
                    term_coeff += [int(f) & 0xFFFFFFFFFFFFFFFF for _, f in terms]

        def table(ctype, values):
            arr = (ctype * max(len(values), 1))(*values)
            self._keep.append(arr)
            return ctypes.cast(arr, ctypes.POINTER(ctype))
        self.num_ctl_columns, self.num_twcs, self.num_lookups = len(num_terms), len(twc_table), len(looking_counts)
        self.column_num_terms, self.column_constant = table(c_u32, num_terms), table(c_u64, constants)
        self.term_column, self.term_coeff = table(c_u32, term_column), table(c_u64, term_coeff)
        self.twc_table, self.twc_num_columns, self.twc_has_filter = table(c_u32, twc_table), table(c_u32, twc_ncols), table(c_u32, twc_filter)
        self.lookup_num_looking = table(c_u32, looking_counts)


for _name, (_res, _args) in SIGNATURES.items():
    _fn = getattr(lib, _name)   # AttributeError here = the .so does not export a declared symbol
    _fn.restype = _res
    _fn.argtypes = _args


def check(status):
    if status != GL_OK:
        raise Plonky2Mi355xError(status, (lib.gl_last_error() or b"").decode())

"""plonky2_demo_amd -- MI355X-native backend for the prove() hot path of the Plonky2 matmul demo circuit.

Host-side mirror (Python, over the C ABI of libplonky2_mi355x.so) of the reference interfaces on the path:
``fft`` / ``ifft`` (field/src/fft.rs:52-95), ``PolynomialBatch`` (plonky2/src/fri/oracle.rs:30-133),
``MerkleTree`` (plonky2/src/hash/merkle_tree.rs:39-207), ``poseidon`` (plonky2/src/hash/poseidon.rs:598-609).
Names and argument meaning follow the reference so that the parity tests read like its own tests.
"""
from ._lib import LIB_PATH, FriInstance, FriParams, Plonky2Mi355xError  # noqa: F401
from ._lib import (  # noqa: F401  (gl_stark_desc filters and operand kinds)
    GL_STARK_ALL, GL_STARK_TRANSITION, GL_STARK_FIRST_ROW, GL_STARK_LAST_ROW, GL_STARK_LOCAL, GL_STARK_NEXT, GL_STARK_PUBLIC,
    GL_STARK_NODE, GL_STARK_CONST, GL_STARK_OP_ADD, GL_STARK_OP_SUB, GL_STARK_OP_MUL, GL_STARK_DAG_MAX_NODES, GL_STARK_DAG_MAX_LIVE, GL_STARK_MAX_TERMS,
    stark_operand,
)
from . import api  # noqa: F401
from .api import (  # noqa: F401
    BatchVerifier, Challenger, CircuitData, Context, FriProver, GenericCircuitData, MatmulCircuit, MerkleTree, PolynomialBatch, Proof, ProverPool, coset_fft, coset_ifft, default_context, fft, hash_or_noop, ifft,
    lde_onto_coset, poseidon, pow_grind, random_elements, GOLDILOCKS_ORDER, COSET_SHIFT,
    hash_from_bytes, hash_or_noop_host, hash_to_bytes, hash_to_elements, two_to_one_host, verify_fri_proof,
    Stark, StarkConfig, StarkDesc, fibonacci_stark, stark_verify,
    StarkDagBuilder, StarkDagDesc, StarkDagExpr, stark_dag_verify,
    CrossTableLookup, CtlColumn, StarkSet, StarkSetDesc, TableWithColumns, stark_set_verify,
    OpeningsBatchVerifier, StarkBatchVerifier,
    lookup_constraints, permuted_cols, permuted_cols_host,
    MEMORY_OP_DTYPE, MemoryTrace, memory_ctl_data, memory_ctl_filter, memory_stark, memory_trace_host,
)

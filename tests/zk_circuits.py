"""Small zero-knowledge circuits for the tests, and the restatements they share (no tests here).

  chacha20_blocks, model_elements    the keystream of csrc/rng.cuh from RFC 8439 2.3
  fri_arity_bits, blinding_counts    ConstantArityBits(4, 5) and blind()'s row counts (circuit_builder.rs:718-766) for any num_query_rounds
  model_blinded_wires, salted_cap    the witness after blind() (circuit_builder.rs:777-818); a blinded PolynomialBatch's cap (oracle.rs:100-125)
  embed_zk                           a plain circuit as a zero-knowledge build of the reference would lay it out: the gate rows, then the
                                     blinding rows and the padding (NoopGates, identity sigma), at the length blind_and_pad pads to
Nothing here imports the product: a description is the ctypes structure the caller hands in, edited on a copy.
"""
import copy
import math

import numpy as np

from oracle_lib import P

GL_STREAM_WIRE, GL_STREAM_SALT, SALT_SIZE = 0x100, 0x200, 4          # rng.cuh: wire w of blind() is stream 0x100 + w, salt column j of PlonkOracle o 0x200 + 4 o + j
NUM_WIRES, NUM_ROUTED = 135, 80


# ---------------------------------------------------------------------------------------------------- ChaCha20 model (RFC 8439 2.3)
def chacha20_blocks(key, nonce_words, counters):
    """Serialised keystream blocks [len(counters)][16] (u32 words) of the RFC 8439 block function."""
    counters = np.asarray(counters, dtype=np.uint32)
    init = np.zeros((16, counters.size), dtype=np.uint32)
    init[0:4] = np.array([0x61707865, 0x3320646E, 0x79622D32, 0x6B206574], dtype=np.uint32)[:, None]
    init[4:12] = np.frombuffer(bytes(key), dtype="<u4")[:, None]
    init[12] = counters
    init[13:16] = np.array(nonce_words, dtype=np.uint32)[:, None]
    x = init.copy()

    def qr(a, b, c, d):
        for (p, q, r, rot) in ((a, b, d, 16), (c, d, b, 12), (a, b, d, 8), (c, d, b, 7)):
            x[p] += x[q]
            x[r] ^= x[p]
            x[r] = (x[r] << np.uint32(rot)) | (x[r] >> np.uint32(32 - rot))

    for _ in range(10):
        qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
        qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
    return (x + init).T.copy()


def model_elements(seed, stream, first, count):
    """Element i = (w_2i + 2^64 w_2i+1) mod p over the little-endian u64 words of stream `stream`'s keystream (nonce = stream, 0, 0)."""
    if count == 0:
        return np.zeros(0, dtype=np.uint64)
    b0, b1 = first // 4, (first + count - 1) // 4
    words = chacha20_blocks(seed, (stream, 0, 0), np.arange(b0, b1 + 1)).astype(np.uint64).reshape(-1, 4)
    lo = (words[:, 0] | (words[:, 1] << np.uint64(32))).astype(object)
    hi = (words[:, 2] | (words[:, 3] << np.uint64(32))).astype(object)
    vals = np.array((lo + hi * (1 << 64)) % P, dtype=np.uint64)
    return vals[first - 4 * b0: first - 4 * b0 + count]


# ---------------------------------------------------------------------------------------------------- blinding layout
def fri_arity_bits(lg, rate_bits=3, cap_height=4):
    """ConstantArityBits(4, 5) (fri/reduction_strategies.rs:39-49)."""
    out, db = [], lg
    while db > 5 and db + rate_bits - 4 >= cap_height:
        out.append(4)
        db -= 4
    return out


def num_blinding_gates(degree_estimate, num_query_rounds=28, D=2):
    """circuit_builder.rs:747-766: (regular rows, Z row pairs) at a degree estimate"""
    arities = [1 << a for a in fri_arity_bits(degree_estimate.bit_length() - 1)]
    total_points = sum(a - 1 for a in arities)
    final_poly_coeffs = degree_estimate // math.prod(arities)
    fri_openings = num_query_rounds * (1 + D * total_points + D * final_poly_coeffs)
    return D + fri_openings, 2 * D + fri_openings


def blinding_counts(num_gates, num_query_rounds=28):
    """circuit_builder.rs:718-745: the estimate doubles until the gate rows and the blinding rows fit"""
    degree_estimate = 1 << (num_gates - 1).bit_length()
    while True:
        regular, z = num_blinding_gates(degree_estimate, num_query_rounds)
        if num_gates + regular + 2 * z <= degree_estimate:
            return regular, z
        degree_estimate *= 2


def padded_degree_bits(num_gates, zk, num_query_rounds=28):
    """log2 of the length blind_and_pad pads to (circuit_builder.rs:767-774): the rows actually used, not the estimate they were counted at"""
    total = num_gates + (sum(x * k for x, k in zip(blinding_counts(num_gates, num_query_rounds), (1, 2))) if zk else 0)
    return (total - 1).bit_length()


def bitrev(lg):
    idx = np.arange(1 << lg, dtype=np.int64)
    r = np.zeros_like(idx)
    for i in range(lg):
        r |= ((idx >> i) & 1) << (lg - 1 - i)
    return r


def model_salt(seed, oracle, lgN):
    """[N][4]: the salt words of every leaf of PlonkOracle `oracle`, in Merkle (leaf) order: column j is stream 0x200 + 4 oracle + j, the
    element index the natural LDE row, and leaf i is LDE row bitrev(i)"""
    N = 1 << lgN
    salt = np.stack([model_elements(seed, GL_STREAM_SALT + SALT_SIZE * oracle + j, 0, N) for j in range(SALT_SIZE)])
    return salt[:, bitrev(lgN)].T.copy()


def salted_cap(orc, cols, from_values, oracle, seed, cap_height=4, rate_bits=3):
    """The cap of a blinded PolynomialBatch built here: the oracle's LDE leaves (Merkle order) followed by the model's salt."""
    ob = orc.batch(cols, rate_bits, cap_height, from_values=from_values, threads=8)
    leaves = ob.leaves()
    full = np.concatenate([leaves, model_salt(seed, oracle, leaves.shape[0].bit_length() - 1)], axis=1)
    return orc.merkle(full, cap_height).cap


def model_blinded_wires(wires, g, seed, num_query_rounds=28):
    """Expected witness after blind(): the RandomValueGenerators and CopyGenerators of circuit_builder.rs:777-818, zeros elsewhere."""
    out = wires.copy()
    n = out.shape[1]
    regular, pairs = blinding_counts(g, num_query_rounds)
    out[:, g:] = 0
    for w in range(NUM_WIRES):
        vals = model_elements(seed, GL_STREAM_WIRE + w, g, regular + 2 * pairs)
        out[w, g:g + regular] = vals[:regular]
        if w < NUM_ROUTED:
            first = vals[regular::2]
            out[w, g + regular:g + regular + 2 * pairs:2] = first
            out[w, g + regular + 1:g + regular + 2 * pairs:2] = first
    assert g + regular + 2 * pairs <= n
    return out


# ---------------------------------------------------------------------------------------------------- a plain circuit as a zk build
def gate_rows_of(row_gates):
    """the rows up to the last one that holds a gate other than NoopGate"""
    return int(np.nonzero(np.asarray(row_gates))[0][-1]) + 1


def embed_zk(desc, constants_sigmas, wires, g, num_query_rounds, proof_of_work_bits, hasher="poseidon"):
    """-> (the zero-knowledge description, constants || sigmas at its length, the unblinded wires at its length).
    `desc`, `constants_sigmas` [num_constants + 80][n] (values on H) and `wires` [135][n] describe a plain circuit whose rows from g on are
    NoopGate padding.  The description gets zero_knowledge = 1, num_gate_rows = g, the FRI parameters asked for, and degree_bits, the
    reduction rounds and their arities from blinding_counts above.  The gate rows keep their constants; their sigmas are re-mapped to the
    new root of unity (k_j w_n^r -> k_j w_n2^r); from row g on sigma is the identity and the constants are the padding row's."""
    from vanishing_model import primitive_root
    n, nc = 1 << desc.degree_bits, desc.num_constants
    cs, wires = np.asarray(constants_sigmas, dtype=np.uint64), np.asarray(wires, dtype=np.uint64)
    assert cs.shape == (nc + NUM_ROUTED, n) and wires.shape == (NUM_WIRES, n)
    assert 0 < g < n and desc.gate_types[0] == 0                      # a NoopGate padding row exists to copy constants from
    lg =padded_degree_bits(g, True, num_query_rounds)
    n2 = 1 << lg
    zd = copy.copy(desc)
    zd.degree_bits, zd.zero_knowledge, zd.num_gate_rows = lg, 1, g
    zd.num_query_rounds, zd.proof_of_work_bits, zd.hasher = num_query_rounds, proof_of_work_bits, 1 if hasher == "keccak" else 0
    arities = fri_arity_bits(lg, desc.rate_bits, desc.cap_height)
    zd.num_fri_rounds = len(arities)
    for i in range(8):
        zd.fri_arity_bits[i] = arities[i] if i < len(arities) else 0
    root_n, root_n2 = primitive_root(desc.degree_bits), primitive_root(lg)
    k_is = [int(desc.k_is[j]) for j in range(NUM_ROUTED)]
    decode, x = {}, 1
    for r in range(n):
        for j in range(NUM_ROUTED):
            decode[k_is[j] * x % P] = (j, r)
        x = x * root_n % P
    powers, x = [], 1
    for r in range(n2):
        powers.append(x)
        x = x * root_n2 % P
    cs2 = np.zeros((nc + NUM_ROUTED, n2), dtype=np.uint64)
    cs2[:nc, :g] = cs[:nc, :g]
    cs2[:nc, g:] = cs[:nc, n - 1:n]
    for c in range(NUM_ROUTED):
        for r in range(n2):
            j, rr = decode[int(cs[nc + c, r])] if r < g else (c, r)
            assert rr < g or r >= g, "a gate row's wire is copied to a padding row"
            cs2[nc + c, r] = k_is[j] * powers[rr] % P
    wires2 = np.zeros((NUM_WIRES, n2), dtype=np.uint64)
    wires2[:, :g] = wires[:, :g]
    return zd, cs2, wires2


def plain_matmul(p, m, a, b, filler_seed):
    """(description, constants || sigmas, wires, public inputs, gate rows) of the plain m x m matmul circuit; `p` is the product package the
    test hands in (its host-side circuit builder needs no GPU)"""
    hc = p.MatmulCircuit(m)
    wires, pis = hc.witness(a, b, filler_seed=filler_seed)
    return hc.desc, hc.constants_sigmas(), wires, pis, gate_rows_of(hc.row_gates())


# ---------------------------------------------------------------------------------------------------- the cases the zk model tests share
SEED = bytes(range(32))
SEED2 = bytes(range(100, 132))
MAX_OPERAND = 2**32 - 2                                               # the operands of the matmul tests are taken mod 2^32 - 1
# name: (source, hasher, num_query_rounds, proof_of_work_bits, salt seed, the n and the FRI reduction rounds the restatement has to give)
#   ("matmul", m, operand seed | "edges", filler seed)   the plain m x m circuit of the product's host-side builder
#   ("merkle", height, leaf index)                       the oracle-built Merkle-proof circuit (kind 14): BaseSumGate besides the matmul's gates
# The m = 8 circuit (75 gate rows) with 2 query rounds counts its blinding rows at the estimate 1024 but then needs only 499 rows: it pads
# to n = 512 with one reduction round, the one case where the estimate and the length differ; with 3 it has n = 1024 and two rounds.
CASES = {
    "matmul2-poseidon-q1": (("matmul", 2, 3, 5), "poseidon", 1, 8, SEED, 256, 1),
    "matmul2-keccak-q1": (("matmul", 2, 3, 5), "keccak", 1, 8, SEED, 256, 1),
    "matmul8-poseidon-q4": (("matmul", 8, 7, 6), "poseidon", 4, 12, SEED, 1024, 2),
    "matmul8-keccak-q2": (("matmul", 8, 7, 6), "keccak", 2, 12, SEED, 512, 1),
    "matmul8-keccak-q3": (("matmul", 8, 7, 6), "keccak", 3, 8, SEED2, 1024, 2),
    "merkle4-poseidon-q1": (("merkle", 4, 11), "poseidon", 1, 8, SEED2, 256, 1),
    "matmul2-edges-q1": (("matmul", 2, "edges", 9), "poseidon", 1, 8, SEED2, 256, 1),
}
FIXTURE_CASE = "matmul2-poseidon-q1"
EDGE_OPERANDS = ([0, 1, MAX_OPERAND, MAX_OPERAND], [MAX_OPERAND, MAX_OPERAND, 1, 0])      # a 2 x 2 product with 0, 1 and the largest operand in both factors


def matmul_operands(m, operand_seed):
    from oracle_lib import rand_field
    if operand_seed == "edges":
        assert m == 2
        return tuple(np.array(v, dtype=np.uint64) for v in EDGE_OPERANDS)
    return rand_field(operand_seed, m * m) % (MAX_OPERAND + 1), rand_field(operand_seed + 100, m * m) % (MAX_OPERAND + 1)


def build_case(p, orc, name):
    """-> (zk description, constants || sigmas, unblinded wires, public inputs, salt seed) of CASES[name]; `p` is the product package the
    test hands in for the matmul circuits (host code), `orc` the oracle library for the Merkle-proof circuit"""
    source, hasher, queries, pow_bits, seed, n, rounds = CASES[name]
    if source[0] == "matmul":
        _, m, operand_seed, filler_seed = source
        desc, cs, wires, pis, g = plain_matmul(p, m, *matmul_operands(m, operand_seed), filler_seed)
    else:
        from test_verifier import merkle_proof_circuit_inputs
        _, height, index = source
        oc = orc.circuit_of_kind(14, height, threads=4)
        w = oc.witness(merkle_proof_circuit_inputs(orc, height, index)[0], np.zeros(0, dtype=np.uint64), filler_seed=height)
        desc, cs, wires, pis, g = oc.product_desc(), oc.constants_sigmas(), w.wires(), w.public_inputs(), gate_rows_of(oc.row_gates())
    zd, cs2, wires2 = embed_zk(desc, cs, wires, g, queries, pow_bits, hasher)
    assert (1 << zd.degree_bits, zd.num_fri_rounds) == (n, rounds), (name, zd.degree_bits, zd.num_fri_rounds)
    return zd, cs2, wires2, np.asarray(pis, dtype=np.uint64), seed

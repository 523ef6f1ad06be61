"""The parser of a proof's bytes that the tests share, and its inverse (no tests here)."""
import numpy as np

U64 = np.uint64

# the column counts of the standard configuration: wires, sigmas (routed wires), Z polynomials (num_challenges), partial products, quotient
# chunks (num_challenges * quotient_degree_factor); the lookup polynomials sit behind the NUM_ZS_PP columns of the second batch
NUM_WIRES, NUM_SIGMAS, NUM_ZS, NUM_PP, NUM_QUOTIENT = 135, 80, 2, 18, 16
NUM_ZS_PP = NUM_ZS + NUM_PP


def opening_columns(d):
    """(name, extension values) of the OpeningSet in the order of its bytes (util/serialization/mod.rs:1409-1423)."""
    nlp = d.num_lookup_polys
    return (("constants", d.num_constants), ("sigmas", NUM_SIGMAS), ("wires", NUM_WIRES), ("zs", NUM_ZS), ("zs_next", NUM_ZS),
            ("lookups", 2 * nlp), ("lookups_next", 2 * nlp), ("pp", NUM_PP), ("quotient", NUM_QUOTIENT))


def leaf_lens(d):
    """The words of a leaf of each of the four initial trees; a blinded tree's leaves end in SALT_SIZE = 4 more."""
    salt = 4 if d.zero_knowledge else 0
    return [d.num_constants + NUM_SIGMAS, NUM_WIRES + salt, NUM_ZS_PP + 2 * d.num_lookup_polys + salt, NUM_QUOTIENT + salt]


def hash_bytes(d):
    """A hash is 25 bytes under the Keccak configuration (d.hasher = 1), 32 under Poseidon."""
    return 25 if d.hasher else 32


class ParsedProof:
    """ProofWithPublicInputs::to_bytes (util/serialization/mod.rs:1939-1981) by description."""

    def __init__(self, d, by):
        self.pos, self.by, self.hash_bytes = 0, by, hash_bytes(d)
        ncap = 1 << d.cap_height
        lgN = d.degree_bits + d.rate_bits
        self.caps = [self.hashes(ncap) for _ in range(3)]
        self.openings = {name: self.words(2 * k) for name, k in opening_columns(d)}
        self.fri_caps = [self.hashes(ncap) for _ in range(d.num_fri_rounds)]
        self.queries = []
        for _ in range(d.num_query_rounds):
            init, steps, lg = [], [], lgN
            for k in leaf_lens(d):
                leaf = self.words(k)
                init.append((leaf, self.hashes(self.u8())))
                assert len(init[-1][1]) == lgN - d.cap_height
            for r in range(d.num_fri_rounds):
                leaf = self.words(2 << d.fri_arity_bits[r])
                lg -= d.fri_arity_bits[r]
                steps.append((leaf, self.hashes(self.u8())))
                assert len(steps[-1][1]) == lg - d.cap_height
            self.queries.append((init, steps))
        final_len = (1 << d.degree_bits) >> sum(d.fri_arity_bits[r] for r in range(d.num_fri_rounds))
        self.final_poly = self.words(2 * final_len)
        self.pow_witness = int(self.words(1)[0])
        self.public_inputs = self.words(int(self.words(1)[0]))
        assert self.pos == len(by)

    def u8(self):
        self.pos += 1
        return self.by[self.pos - 1]

    def words(self, k):
        out = np.frombuffer(self.by, dtype="<u8", count=k, offset=self.pos).astype(U64)
        self.pos += 8 * k
        return out

    def hashes(self, k):
        out = np.zeros((k, 4), dtype=U64)
        for i in range(k):
            out[i] = np.frombuffer(self.by[self.pos:self.pos + self.hash_bytes].ljust(32, b"\0"), dtype="<u8")
            self.pos += self.hash_bytes
        return out


def proof_bytes(d, caps, openings, fri_caps, queries, final_poly, pow_witness, public_inputs):
    """The inverse of ParsedProof: its fields -> ProofWithPublicInputs bytes.  `queries` is ParsedProof.queries, or the rounds' bytes
    as gl_fri_query wrote them."""
    def words(a):
        return np.ascontiguousarray(np.asarray(a, dtype="<u8")).tobytes()

    def hashes(h):
        return b"".join(words(row)[:hash_bytes(d)] for row in np.asarray(h, dtype=U64).reshape(-1, 4))

    def path(leaf, siblings):
        return words(leaf) + bytes([len(siblings)]) + hashes(siblings)

    if not isinstance(queries, bytes):
        queries = b"".join(path(*tree) for init, steps in queries for tree in init + steps)
    by = b"".join(hashes(c) for c in caps) + b"".join(words(openings[name]) for name, _ in opening_columns(d))
    by += b"".join(hashes(c) for c in fri_caps) + queries + words(final_poly) + words([pow_witness])
    return by + words([len(public_inputs)]) + words(public_inputs)

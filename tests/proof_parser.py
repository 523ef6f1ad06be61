"""The parser of a proof's bytes that the tests share (no tests here)."""
import numpy as np

U64 = np.uint64


class ParsedProof:
    """ProofWithPublicInputs::to_bytes (util/serialization/mod.rs:1939-1981) by description: a hash is 25 bytes under the Keccak
    configuration (d.hasher = 1), 32 under Poseidon."""

    def __init__(self, d, by):
        self.pos, self.by, self.hash_bytes = 0, by, 25 if d.hasher else 32
        ncap, nlp, salt = 1 << d.cap_height, d.num_lookup_polys, 4 if d.zero_knowledge else 0
        lgN = d.degree_bits + d.rate_bits
        self.caps = [self.hashes(ncap) for _ in range(3)]
        o = {}
        for name, k in (("constants", d.num_constants), ("sigmas", 80), ("wires", 135), ("zs", 2), ("zs_next", 2), ("lookups", 2 * nlp), ("lookups_next", 2 * nlp),
                        ("pp", 18), ("quotient", 16)):
            o[name] = self.words(2 * k)
        self.openings = o
        self.fri_caps = [self.hashes(ncap) for _ in range(d.num_fri_rounds)]
        leaf_lens = [d.num_constants + 80, 135 + salt, 20 + 2 * nlp + salt, 16 + salt]
        self.queries = []
        for _ in range(d.num_query_rounds):
            init, steps, lg = [], [], lgN
            for o_ in range(4):
                leaf = self.words(leaf_lens[o_])
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

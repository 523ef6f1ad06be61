"""Host-side mirror of the reference's operator interfaces for the hot path (numpy in / numpy out).

Everything here is plumbing over the C ABI: no arithmetic happens in Python.  Arrays are uint64, an
extension element is a pair, a digest is four words.  Reference lines are cited per function.
"""
import ctypes

import numpy as np

from . import _lib
from ._lib import check, hasher_id, lib
from ._lib import (  # noqa: F401  (gl_circuit_desc.gate_types codes)
    G_NOOP, G_CONSTANT, G_PUBLIC_INPUT, G_ARITHMETIC, G_POSEIDON, G_BASE_SUM, G_LOOKUP, G_LOOKUP_TABLE, G_EXPONENTIATION, G_RANDOM_ACCESS,
    G_ARITHMETIC_EXT, G_MUL_EXT, G_REDUCING, G_REDUCING_EXT,
)

GOLDILOCKS_ORDER = 0xFFFFFFFF00000001   # field/src/goldilocks_field.rs:152
COSET_SHIFT = 7                          # field/src/types.rs:437-439, goldilocks_field.rs:80


def _u64(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a


def _p(a):
    return a.ctypes.data_as(ctypes.c_void_p)


def _log2_strict(n):
    lg = int(n).bit_length() - 1
    if n <= 0 or (1 << lg) != n:
        raise ValueError("length %d is not a power of two" % n)   # util/src/lib.rs:35-40 panics
    return lg


def _verdict(st):
    """A verifier's status -> (accepted, reason); a status that is neither accept nor reject raises."""
    if st == _lib.GL_OK:
        return True, ""
    if st == _lib.GL_ERR_VERIFY:
        return False, (lib.gl_last_error() or b"").decode()
    check(st)


class _Owned:
    """Base of the classes that own a C handle: close() frees `handle` once with the library function named `_free`, or only forgets it
    when it is borrowed (`handle_owned` False).  The finaliser calls close() and swallows a failure (at interpreter exit the library may
    be gone already)."""
    handle = None
    handle_owned = True
    _free = None

    def close(self):
        if self.handle:
            if self.handle_owned:
                getattr(lib, self._free)(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class DeviceBuffer(_Owned):
    def __init__(self, ctx, nbytes):
        self.ctx = ctx
        self.nbytes = int(nbytes)
        p = ctypes.c_void_p()
        check(lib.gl_dev_alloc(ctx.handle, self.nbytes, ctypes.byref(p)))
        self.ptr = p.value

    def upload(self, arr):
        arr = _u64(arr)
        assert arr.nbytes <= self.nbytes
        check(lib.gl_copy_h2d(self.ctx.handle, self.ptr, _p(arr), arr.nbytes))
        return self

    def download(self, shape):
        out = np.empty(shape, dtype=np.uint64)
        assert out.nbytes <= self.nbytes
        check(lib.gl_copy_d2h(self.ctx.handle, _p(out), self.ptr, out.nbytes))
        return out

    def free(self):
        if self.ptr:
            check(lib.gl_dev_free(self.ctx.handle, self.ptr))      # a closed context (handle None) is accepted
            self.ptr = None

    close = free


class Context(_Owned):
    """One per (device, stream).  `stream` may be a raw hipStream_t (int), e.g.
    torch.cuda.current_stream().cuda_stream, so that torch events bracket the library's kernels.

    close() drops this object's reference to the context (gl_ctx_destroy).  Batches / trees / circuits created on it hold references of
    their own, so they stay valid and may be freed afterwards in any order; buffers from alloc() must be freed before.  The finaliser is
    safe in any order too: the library tears the context down when its last handle is freed."""
    _free = "gl_ctx_destroy"

    def __init__(self, device=0, stream=None):
        h = ctypes.c_void_p()
        check(lib.gl_ctx_create(int(device), ctypes.c_void_p(stream) if stream else None, ctypes.byref(h)))
        self.handle = h.value
        self.device = device

    @property
    def has_own_queue(self):
        """True if the context's stream has a hardware queue of its own (gl_ctx_has_own_queue; knob GL_LANE_QUEUES)."""
        return bool(lib.gl_ctx_has_own_queue(self.handle))

    def synchronize(self):
        check(lib.gl_ctx_synchronize(self.handle))

    def set_scratch_elems(self, elems):
        check(lib.gl_ctx_set_scratch_elems(self.handle, int(elems)))

    def alloc(self, nbytes):
        return DeviceBuffer(self, nbytes)

    def capture_intermediates(self, on=True):
        """Keep each proof's Z / partial-product values and quotient chunks on the host (parity tests)."""
        check(lib.gl_ctx_capture_intermediates(self.handle, 1 if on else 0))

    def timing(self, on=True):
        check(lib.gl_ctx_timing_reset(self.handle))
        check(lib.gl_ctx_timing_enable(self.handle, 1 if on else 0))

    def timing_report(self):
        import json
        buf = ctypes.create_string_buffer(1 << 16)
        check(lib.gl_ctx_timing_report(self.handle, buf, len(buf)))
        return json.loads(buf.value.decode())

    def lookup_columns(self, d_cols_ptr, num_columns, n, lookups):
        """gl_stark_lookup_columns: permuted_cols (evm/src/lookup.rs:65-127) for every lookup of the device trace d_cols[num_columns][n],
        in place.  lookups = [(col_input, col_table, col_permuted_input, col_permuted_table), ...]."""
        flat = np.ascontiguousarray([[int(c) for c in lk] for lk in lookups], dtype=np.uint32).reshape(-1, 4) if len(lookups) else np.zeros((0, 4), dtype=np.uint32)
        check(lib.gl_stark_lookup_columns(self.handle, d_cols_ptr, int(num_columns), int(n), _p(flat) if flat.size else None, flat.shape[0]))


_default = None


def default_context():
    global _default
    if _default is None:
        _default = Context(0)
    return _default


def _ctx(ctx):
    return ctx if ctx is not None else default_context()


# ---------------------------------------------------------------------------------------------- field
def field_op(op, a, b=None, c=None, ctx=None):
    """op: 0 add 1 sub 2 mul 3 neg 4 inverse 5 canonicalise 6 a+b*c 7 a*2^(b%192)."""
    ctx = _ctx(ctx)
    a = _u64(a)
    n = a.size
    da = ctx.alloc(max(8, a.nbytes)).upload(a)
    db = ctx.alloc(max(8, a.nbytes)).upload(_u64(b)) if b is not None else None
    dc = ctx.alloc(max(8, a.nbytes)).upload(_u64(c)) if c is not None else None
    do = ctx.alloc(max(8, a.nbytes))
    check(lib.gl_field_op(ctx.handle, op, da.ptr, db.ptr if db else None, dc.ptr if dc else None, do.ptr, n))
    return do.download(a.shape)


def ext_op(op, a, b=None, ctx=None):
    ctx = _ctx(ctx)
    a = _u64(a)
    n = a.size // 2
    da = ctx.alloc(max(8, a.nbytes)).upload(a)
    db = ctx.alloc(max(8, a.nbytes)).upload(_u64(b)) if b is not None else None
    do = ctx.alloc(max(8, a.nbytes))
    check(lib.gl_ext_op(ctx.handle, op, da.ptr, db.ptr if db else None, do.ptr, n))
    return do.download(a.shape)


# ------------------------------------------------------------------------------------------------ NTT
def _transform(kind, arr, shift=None, ctx=None):
    ctx = _ctx(ctx)
    arr = _u64(arr)
    single = arr.ndim == 1
    a2 = arr.reshape(1, -1) if single else arr
    batch, n = a2.shape
    lg = _log2_strict(n)
    d = ctx.alloc(max(8, a2.nbytes)).upload(a2)
    if kind == "fft":
        check(lib.gl_ntt_forward(ctx.handle, d.ptr, lg, batch))
    elif kind == "ifft":
        check(lib.gl_ntt_inverse(ctx.handle, d.ptr, lg, batch))
    elif kind == "coset_fft":
        check(lib.gl_ntt_coset_forward(ctx.handle, d.ptr, lg, batch, shift))
    elif kind == "coset_ifft":
        check(lib.gl_ntt_coset_inverse(ctx.handle, d.ptr, lg, batch, shift))
    out = d.download(a2.shape)
    return out.reshape(-1) if single else out


def fft(coeffs, ctx=None):
    """field::fft::fft (field/src/fft.rs:52-65): values[i] = P(w^i); [n] or [batch][n]."""
    return _transform("fft", coeffs, ctx=ctx)


def ifft(values, ctx=None):
    """field::fft::ifft (field/src/fft.rs:67-95)."""
    return _transform("ifft", values, ctx=ctx)


def coset_fft(coeffs, shift=COSET_SHIFT, ctx=None):
    """PolynomialCoeffs::coset_fft (field/src/polynomial/mod.rs:276-295)."""
    return _transform("coset_fft", coeffs, shift=shift, ctx=ctx)


def coset_ifft(values, shift=COSET_SHIFT, ctx=None):
    """PolynomialValues::coset_ifft (field/src/polynomial/mod.rs:58-70)."""
    return _transform("coset_ifft", values, shift=shift, ctx=ctx)


def lde_onto_coset(coeffs, rate_bits, ctx=None):
    """coeffs.lde(rate_bits).coset_fft_with_options(7, Some(rate_bits)) (plonky2/src/fri/oracle.rs:111-118)."""
    ctx = _ctx(ctx)
    c2 = _u64(coeffs)
    single = c2.ndim == 1
    if single:
        c2 = c2.reshape(1, -1)
    batch, n = c2.shape
    lg = _log2_strict(n)
    src = ctx.alloc(max(8, c2.nbytes)).upload(c2)
    dst = ctx.alloc(c2.nbytes << rate_bits)
    check(lib.gl_ntt_coset_lde(ctx.handle, src.ptr, lg, rate_bits, batch, dst.ptr))
    out = dst.download((batch, n << rate_bits))
    return out.reshape(-1) if single else out


# ------------------------------------------------------------------------------------------- hashing
def poseidon(states, ctx=None):
    """Poseidon::poseidon (plonky2/src/hash/poseidon.rs:598-609) on [12] or [count][12]."""
    ctx = _ctx(ctx)
    s = _u64(states)
    if s.shape[-1] != 12:
        raise ValueError("Poseidon state width is 12")
    d = ctx.alloc(s.nbytes).upload(s)
    check(lib.gl_poseidon_permute(ctx.handle, d.ptr, s.size // 12))
    return d.download(s.shape)


def hash_to_bytes(digests, hasher="keccak"):
    """[k][4] digest words -> k byte strings as they go on the wire: 32 bytes of a HashOut, the 25 bytes of a BytesHash<25>."""
    d = _u64(digests).reshape(-1, 4)
    size = 25 if hasher_id(hasher) else 32
    return [d[i].tobytes()[:size] for i in range(d.shape[0])]


def hash_from_bytes(strings, hasher="keccak"):
    """The inverse of hash_to_bytes: byte strings -> [k][4] digest words (a 25-byte hash zero-padded into its slot)."""
    size = 25 if hasher_id(hasher) else 32
    out = np.zeros((len(strings), 4), dtype=np.uint64)
    for i, b in enumerate(strings):
        if len(b) != size:
            raise ValueError("a %s hash is %d bytes" % ("keccak" if size == 25 else "poseidon", size))
        out[i] = np.frombuffer(bytes(b).ljust(32, b"\0"), dtype="<u8")
    return out


def hash_to_elements(digests, hasher="keccak"):
    """GenericHashOut::to_vec per digest, [k][4] -> [k][4] field elements: what a Challenger observes of a hash.  A BytesHash<25> is
    its bytes in chunks of 7, 7, 7, 4 (hash/hash_types.rs:181-191); a HashOut is its own elements."""
    d = _u64(digests).reshape(-1, 4)
    if not hasher_id(hasher):
        return d.copy()
    raw = np.ascontiguousarray(d).view(np.uint8).reshape(-1, 32)
    out = np.zeros((d.shape[0], 4, 8), dtype=np.uint8)
    for j, (lo, hi) in enumerate(((0, 7), (7, 14), (14, 21), (21, 25))):
        out[:, j, : hi - lo] = raw[:, lo:hi]
    return out.view("<u8").reshape(-1, 4)


def hash_or_noop_host(rows, hasher="poseidon"):
    """hash_or_noop per row on the host (no GPU): [count][len] -> [count][4]."""
    r = _u64(rows)
    single = r.ndim == 1
    if single:
        r = r.reshape(1, -1)
    out = np.zeros((r.shape[0], 4), dtype=np.uint64)
    check(lib.gl_hash_or_noop_host(hasher_id(hasher), _p(r) if r.size else None, r.shape[0], r.shape[1], _p(out)))
    return out[0] if single else out


def two_to_one_host(left, right, hasher="poseidon"):
    """Hasher::two_to_one on the host (no GPU): [k][4], [k][4] -> [k][4] (or [4], [4] -> [4])."""
    l, r = _u64(left), _u64(right)
    single = l.ndim == 1
    l, r = l.reshape(-1, 4), r.reshape(-1, 4)
    out = np.zeros_like(l)
    check(lib.gl_two_to_one_host(hasher_id(hasher), _p(l), _p(r), l.shape[0], _p(out)))
    return out[0] if single else out


def hash_or_noop(rows, ctx=None, hasher="poseidon"):
    """Hasher::hash_or_noop (plonky2/src/plonk/config.rs:55-66) per row of [count][len] -> [count][4]."""
    ctx = _ctx(ctx)
    hid = hasher_id(hasher)
    r = _u64(rows)
    single = r.ndim == 1
    if single:
        r = r.reshape(1, -1)
    count, ln = r.shape
    if ln == 0:
        return np.zeros((4,) if single else (count, 4), dtype=np.uint64)
    d = ctx.alloc(max(8, r.nbytes)).upload(r)
    o = ctx.alloc(max(32, count * 32))
    check(lib.gl_hash_rows_h(ctx.handle, hid, d.ptr, count, ln, o.ptr))
    out = o.download((count, 4))
    return out[0] if single else out


class MerkleTree(_Owned):
    """plonky2::hash::merkle_tree::MerkleTree (merkle_tree.rs:39-207) with device-resident digests."""
    _free = "gl_merkle_free"

    def __init__(self, leaves, cap_height, ctx=None, hasher="poseidon"):
        self.ctx = _ctx(ctx)
        self.hasher = hasher_id(hasher)
        l2 = _u64(leaves)
        if l2.ndim != 2:
            raise ValueError("leaves must be [num_leaves][leaf_len]")
        self.num_leaves, self.leaf_len = l2.shape
        self.cap_height = cap_height
        self.leaves = l2
        h = ctypes.c_void_p()
        check(lib.gl_merkle_new_h(self.ctx.handle, self.hasher, _p(l2), self.num_leaves, self.leaf_len, cap_height, ctypes.byref(h)))
        self.handle = h.value

    @property
    def cap(self):
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        check(lib.gl_merkle_cap(self.handle, _p(out)))
        return out

    def get(self, i):
        return self.leaves[i]

    def prove(self, leaf_index):
        n = ctypes.c_uint32()
        out = np.empty((64, 4), dtype=np.uint64)
        check(lib.gl_merkle_prove(self.handle, leaf_index, _p(out), ctypes.byref(n)))
        return out[: n.value].copy()


class PolynomialBatch(_Owned):
    """plonky2::fri::oracle::PolynomialBatch (fri/oracle.rs:30-133), device-resident."""
    _free = "gl_batch_free"

    salt = 0        # SALT_SIZE random elements behind every leaf of a blinded batch (oracle.rs:100-125)

    def __init__(self, handle, ctx, rate_bits, cap_height):
        self.handle, self.ctx, self.rate_bits, self.cap_height = handle, ctx, rate_bits, cap_height
        self.ncols = lib.gl_batch_ncols(handle)
        self.degree = lib.gl_batch_degree(handle)
        self.degree_log = _log2_strict(self.degree)
        self.hasher = lib.gl_batch_hasher(handle)

    @classmethod
    def _from_host(cls, fn, cols, rate_bits, cap_height, ctx, *args, salt=0, hasher="poseidon"):
        """fn(ctx, hasher, column pointers, ncols, n, rate_bits, *args, out)"""
        ctx = _ctx(ctx)
        cols = [_u64(c) for c in cols]
        if not cols:
            raise ValueError("empty batch")
        n = cols[0].size
        if any(c.size != n for c in cols):
            raise ValueError("Polynomial degrees inconsistent")   # oracle.rs:114
        ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        h = ctypes.c_void_p()
        check(fn(ctx.handle, hasher_id(hasher), ptrs, len(cols), n, rate_bits, *args, ctypes.byref(h)))
        b = cls(h.value, ctx, rate_bits, cap_height)
        b.salt = salt
        return b

    @classmethod
    def from_values(cls, values, rate_bits, blinding, cap_height, ctx=None, hasher="poseidon"):
        """PolynomialBatch::from_values (fri/oracle.rs:43-66); blinding = True is from_values_blinded."""
        return cls._from_host(lib.gl_batch_from_values_h, values, rate_bits, cap_height, ctx, 1 if blinding else 0, cap_height, hasher=hasher)

    @classmethod
    def from_coeffs(cls, polynomials, rate_bits, blinding, cap_height, ctx=None, hasher="poseidon"):
        """PolynomialBatch::from_coeffs (fri/oracle.rs:68-98); blinding = True is from_coeffs_blinded."""
        return cls._from_host(lib.gl_batch_from_coeffs_h, polynomials, rate_bits, cap_height, ctx, 1 if blinding else 0, cap_height, hasher=hasher)

    @classmethod
    def from_values_blinded(cls, values, rate_bits, cap_height, seed=None, ctx=None, hasher="poseidon"):
        """from_values with blinding = true: every leaf salted with SALT_SIZE elements keyed by `seed` (32 bytes; None = OS entropy)."""
        return cls._from_host(lib.gl_batch_from_values_blinded_h, values, rate_bits, cap_height, ctx, cap_height,
                              _seed(seed) if seed is not None else None, salt=SALT_SIZE, hasher=hasher)

    @classmethod
    def from_coeffs_blinded(cls, polynomials, rate_bits, cap_height, seed=None, ctx=None, hasher="poseidon"):
        """from_coeffs with blinding = true (see from_values_blinded)."""
        return cls._from_host(lib.gl_batch_from_coeffs_blinded_h, polynomials, rate_bits, cap_height, ctx, cap_height,
                              _seed(seed) if seed is not None else None, salt=SALT_SIZE, hasher=hasher)

    @classmethod
    def from_device(cls, d_ptr, ncols, n, rate_bits, cap_height, is_values, ctx=None, hasher="poseidon"):
        ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        check(lib.gl_batch_from_device_h(ctx.handle, hasher_id(hasher), d_ptr, ncols, n, rate_bits, cap_height, 1 if is_values else 0, ctypes.byref(h)))
        return cls(h.value, ctx, rate_bits, cap_height)

    @property
    def cap(self):
        out = np.empty((1 << self.cap_height, 4), dtype=np.uint64)
        check(lib.gl_batch_cap(self.handle, _p(out)))
        return out

    @property
    def polynomials(self):
        out = np.empty((self.ncols, self.degree), dtype=np.uint64)
        check(lib.gl_batch_coeffs(self.handle, _p(out)))
        return out

    def lde_values(self):
        out = np.empty((self.ncols, self.degree << self.rate_bits), dtype=np.uint64)
        check(lib.gl_batch_lde(self.handle, _p(out)))
        return out

    def get_leaf(self, i):
        """merkle_tree.get(i): the LDE row with its salt (ncols + salt elements)."""
        out = np.empty(self.ncols + self.salt, dtype=np.uint64)
        check(lib.gl_batch_get_leaf(self.handle, i, _p(out)))
        return out

    def get_lde_values(self, index, step):
        """PolynomialBatch::get_lde_values (fri/oracle.rs:128-133)."""
        out = np.empty(self.ncols, dtype=np.uint64)
        check(lib.gl_batch_get_lde_values(self.handle, index, step, _p(out)))
        return out

    def prove(self, leaf_index):
        n = ctypes.c_uint32()
        out = np.empty((64, 4), dtype=np.uint64)
        check(lib.gl_batch_prove(self.handle, leaf_index, _p(out), ctypes.byref(n)))
        return out[: n.value].copy()

    def open_at(self, z, first_col=0, num_cols=None, ctx=None):
        """eval_commitment of OpeningSet::new (plonk/proof.rs:306-344): [num_cols][2] extension values."""
        num_cols = self.ncols - first_col if num_cols is None else num_cols
        out = np.empty((num_cols, 2), dtype=np.uint64)
        check(lib.gl_open_at((ctx or self.ctx).handle, self.handle, _p(_u64(z)), first_col, num_cols, _p(out)))
        return out

    @staticmethod
    def prove_openings(instance, oracles, challenger, fri_params, ctx=None):
        """PolynomialBatch::prove_openings (fri/oracle.rs:162-219) for any FriInstance: the FriProof bytes in write_fri_proof order.  The
        challenger has observed the openings; it is left behind the last query index."""
        oracles = list(oracles)
        ctx = ctx or oracles[0].ctx
        arr = (ctypes.c_void_p * max(len(oracles), 1))(*[b.handle for b in oracles])
        k = ctypes.c_size_t()
        check(lib.gl_prove_openings(ctx.handle, ctypes.byref(fri_params), ctypes.byref(instance), arr, challenger.handle, None, 0, ctypes.byref(k)))
        out = np.empty(k.value, dtype=np.uint8)
        check(lib.gl_prove_openings(ctx.handle, ctypes.byref(fri_params), ctypes.byref(instance), arr, challenger.handle, _p(out), out.size, ctypes.byref(k)))
        return out.tobytes()

    free = _Owned.close     # a batch borrowed from a circuit (handle_owned False) is only forgotten


# ------------------------------------------------------------------------------------- circuit and prove()
class MatmulCircuit(_Owned):
    """Host side of the demo (plonky2/src/bin/matrix_mul.rs:25-67 + CircuitBuilder::build()): needs no GPU.  zero_knowledge=True
    builds it with standard_recursion_zk_config: blinding rows after the gate rows, salted commitments (blind the witness with
    CircuitData.blind_witness before proving).  hasher="keccak" builds it under KeccakGoldilocksConfig: the same gates, constants,
    sigmas and witness; Merkle trees, transcript and proof of work under Keccak-256."""
    _free = "gl_host_circuit_free"

    def __init__(self, m, zero_knowledge=False, hasher="poseidon"):
        h = ctypes.c_void_p()
        check(lib.gl_matmul_circuit_build_h(int(m), 1 if zero_knowledge else 0, hasher_id(hasher), ctypes.byref(h)))
        self.handle, self.m, self.zero_knowledge = h.value, int(m), bool(zero_knowledge)
        self.desc = _lib.CircuitDesc()
        check(lib.gl_host_circuit_desc(self.handle, ctypes.byref(self.desc)))
        self.degree_bits = self.desc.degree_bits
        self.n = 1 << self.degree_bits

    def row_gates(self):
        out = np.empty(self.n, dtype=np.uint8)
        check(lib.gl_host_circuit_row_gates(self.handle, _p(out)))
        return out

    def constants_sigmas(self):
        out = np.empty((self.desc.num_constants + 80, self.n), dtype=np.uint64)
        check(lib.gl_host_circuit_constants_sigmas(self.handle, _p(out)))
        return out

    def witness(self, a, b, filler_seed=0x504C4F4E4B5932):
        """(wires[135][n], public_inputs[3 m^2]) -- generate_partial_witness + full_witness (prover.rs:118-133)."""
        a, b = _u64(a).reshape(-1), _u64(b).reshape(-1)
        if a.size != self.m ** 2 or b.size != self.m ** 2:
            raise ValueError("a and b must be m x m")
        wires = np.empty((135, self.n), dtype=np.uint64)
        pis = np.empty(3 * self.m ** 2, dtype=np.uint64)
        check(lib.gl_matmul_witness(self.handle, _p(a), _p(b), filler_seed, _p(wires), _p(pis)))
        return wires, pis

    def verify(self, proof_bytes, constants_sigmas_cap, circuit_digest):
        """VerifierCircuitData::verify (plonk/circuit_data.rs:208-215): (accepted, reason).  Host code, no GPU needed."""
        buf = np.frombuffer(bytes(proof_bytes), dtype=np.uint8)
        cap, dig = _u64(constants_sigmas_cap), _u64(circuit_digest)
        if cap.size != 4 << self.desc.cap_height or dig.size != 4:
            raise ValueError("cap must be [2^cap_height][4], digest [4]")
        return _verdict(lib.gl_host_circuit_verify(self.handle, _p(cap), _p(dig), _p(buf), buf.size))

    def witness_generator(self, ctx=None):
        """Witness generation straight into HBM (GPU arithmetic rows + host hash-sponge rows), one per context."""
        return WitnessGenerator(self, _ctx(ctx))

    def build(self, ctx=None):
        """CircuitBuilder::build(): the device half (constants/sigmas commitment, digest)."""
        return CircuitData(self, _ctx(ctx))


class WitnessGenerator(_Owned):
    """generate_partial_witness + full_witness (plonk/prover.rs:118-133) for the matmul family, wire matrix in HBM."""
    _free = "gl_matmul_witgen_free"

    def __init__(self, host, ctx):
        self.host, self.ctx = host, ctx
        h = ctypes.c_void_p()
        check(lib.gl_matmul_witgen_create(ctx.handle, host.handle, ctypes.byref(h)))
        self.handle = h.value

    def run(self, a, b, d_wires_ptr, filler_seed=0x504C4F4E4B5932):
        """Overwrites the device matrix d_wires[135][n]; returns the public inputs."""
        a, b = _u64(a).reshape(-1), _u64(b).reshape(-1)
        if a.size != self.host.m ** 2 or b.size != self.host.m ** 2:
            raise ValueError("a and b must be m x m")
        pis = np.empty(3 * self.host.m ** 2, dtype=np.uint64)
        self.public_inputs_hash = np.empty(4, dtype=np.uint64)      # by-product of the sponge rows
        check(lib.gl_matmul_witgen_run(self.handle, _p(a), _p(b), filler_seed, d_wires_ptr, _p(pis), _p(self.public_inputs_hash)))
        return pis

SALT_SIZE = 4     # fri/oracle.rs:26


def _seed(seed):
    """A 32-byte seed as a ctypes buffer (kept alive by the caller's expression)."""
    seed = bytes(seed)
    if len(seed) != 32:
        raise ValueError("a seed is 32 bytes")
    return ctypes.create_string_buffer(seed, 32)


def random_elements(seed, stream, first, count, ctx=None):
    """Elements first .. first + count of a stream of the zero-knowledge generator (ChaCha20 keystream, include/plonky2_mi355x.h),
    computed on the device.  `ctx=False` computes them on the host instead (gl_random_elements_host)."""
    out = np.empty(int(count), dtype=np.uint64)
    if ctx is False:
        check(lib.gl_random_elements_host(_seed(seed), stream, first, count, _p(out)))
        return out
    ctx = _ctx(ctx)
    buf = ctx.alloc(max(1, out.size) * 8)
    try:
        check(lib.gl_random_elements(ctx.handle, _seed(seed), stream, first, count, buf.ptr))
        return buf.download(out.size)
    finally:
        buf.free()


def _circuit_digest(handle):
    out = np.empty(4, dtype=np.uint64)
    check(lib.gl_circuit_digest(handle, _p(out)))
    return out


def _constants_sigmas_cap(handle, cap_height):
    out = np.empty((1 << cap_height, 4), dtype=np.uint64)
    check(lib.gl_circuit_constants_sigmas_cap(handle, _p(out)))
    return out


class HostColumns:
    """135 host vectors of n field elements with their pointer table (what a Rust caller passes as `*const *const u64`); built
    once so that a timed loop measures gl_prove_columns, not numpy."""

    def __init__(self, columns, n):
        self.cols = [np.ascontiguousarray(_u64(c)) for c in columns]
        if len(self.cols) != 135 or any(c.size != n for c in self.cols):
            raise ValueError("need 135 columns of n values")
        self.ptrs = (ctypes.c_void_p * 135)(*[c.ctypes.data for c in self.cols])


class _CircuitApi(_Owned):
    """A device-resident circuit (gl_circuit `handle`) used from the context `ctx`: prove() and verify() of
    plonky2::plonk::circuit_data::CircuitData, and the phase-level seam for a caller that owns the Challenger.  `desc` is
    its gl_circuit_desc (by default the library's completed copy: lookup rows read from the selector columns), `n` its degree.
    Circuits with the lookup argument pass the 8 delta challenges to the phases."""
    _free = "gl_circuit_free"

    def __init__(self, handle, ctx, desc=None):
        self.handle, self.ctx = handle, ctx
        if desc is None:
            desc = _lib.CircuitDesc()
            check(lib.gl_circuit_description(handle, ctypes.byref(desc)))
        self.desc, self.n = desc, 1 << desc.degree_bits

    @property
    def circuit_digest(self):
        return _circuit_digest(self.handle)

    @property
    def constants_sigmas_cap(self):
        return _constants_sigmas_cap(self.handle, self.desc.cap_height)

    def verify(self, proof):
        """CircuitData::verify (plonk/circuit_data.rs:153-155): (accepted, reason); `proof` is a Proof or its bytes.  Host code."""
        by = proof.to_bytes() if hasattr(proof, "to_bytes") else proof
        buf = np.frombuffer(bytes(by), dtype=np.uint8)
        return _verdict(lib.gl_verify(ctypes.byref(self.desc), _p(self.constants_sigmas_cap), _p(self.circuit_digest), _p(buf), buf.size))

    def batch_verifier(self, max_batch=64, host_threads=1):
        """A BatchVerifier for this circuit on its context: many proofs per call, Merkle paths and FRI queries on the device."""
        return BatchVerifier(self.desc, self.constants_sigmas_cap, self.circuit_digest, ctx=self.ctx, max_batch=max_batch, host_threads=host_threads)

    def _prove(self, entry, wires_ptr, public_inputs, *hash_arg):
        pis = _u64(public_inputs)
        keep = pis if pis.size else np.zeros(1, dtype=np.uint64)          # a valid pointer even for zero public inputs
        h = ctypes.c_void_p()
        check(entry(self.ctx.handle, self.handle, wires_ptr, _p(keep), pis.size, *hash_arg, ctypes.byref(h)))
        return Proof(h.value, self.desc)

    def prove(self, wires, public_inputs):
        """CircuitData::prove (circuit_data.rs:144-151) at the full-witness boundary: the wire matrix [135][n] on the host."""
        wires = _u64(wires)
        if wires.shape != (135, self.n):
            raise ValueError("wire matrix must be [135][n]")
        return self._prove(lib.gl_prove, _p(wires), public_inputs)

    def prove_columns(self, columns, public_inputs):
        """prove() from one host array per wire, as the reference keeps MatrixWitness.wire_values (iop/witness.rs:256-258):
        the drop-in entry INTEGRATION.md patches into plonk/prover.rs:145.  `columns` may be a HostColumns (pointer table built once)."""
        hc = columns if isinstance(columns, HostColumns) else HostColumns(columns, self.n)
        return self._prove(lib.gl_prove_columns, hc.ptrs, public_inputs)

    def prove_device(self, d_wires_ptr, public_inputs, public_inputs_hash=None, seed=None):
        """prove() with the witness matrix already in HBM (raw device pointer to [135][n] u64).  `seed` (32 bytes) keys the salts of a
        zero-knowledge circuit (gl_prove_device_seeded); without it they come from the OS."""
        if seed is not None:
            if public_inputs_hash is not None:
                raise ValueError("prove_device takes a seed or a public-inputs hash, not both")
            return self._prove(lib.gl_prove_device_seeded, d_wires_ptr, public_inputs, _seed(seed))
        if public_inputs_hash is None:
            return self._prove(lib.gl_prove_device, d_wires_ptr, public_inputs)
        return self._prove(lib.gl_prove_device_hashed, d_wires_ptr, public_inputs, _p(_u64(public_inputs_hash)))

    def blind_witness(self, d_wires_ptr, seed=None, ctx=None):
        """gl_witness_blind: the blinding rows of a zero-knowledge circuit's device witness [135][n] (RandomValueGenerator +
        CopyGenerator of blind(), circuit_builder.rs:777-818); seed None = OS entropy."""
        check(lib.gl_witness_blind((ctx or self.ctx).handle, self.handle, d_wires_ptr, _seed(seed) if seed is not None else None))

    def warm_up(self, ctx=None):
        """gl_circuit_warm_up: one throw-away pass of the proving pipeline on `ctx` (default: this object's context), so that the first
        proof does not pay the one-time costs (kernel code objects, twiddle tables, pool growth)."""
        check(lib.gl_circuit_warm_up((ctx or self.ctx).handle, self.handle))
        return self

    def _batch(self, handle, ctx):
        return PolynomialBatch(handle, ctx, self.desc.rate_bits, self.desc.cap_height)

    @property
    def constants_sigmas_batch(self):
        """`prover_data.constants_sigmas_commitment` (borrowed: owned by the circuit)."""
        b = self._batch(lib.gl_circuit_constants_sigmas_batch(self.handle), self.ctx)
        b.handle_owned = False
        return b

    def partial_products(self, d_wires_ptr, betas, gammas, ctx=None, deltas=None):
        """all_wires_permutation_partial_products (+ compute_all_lookup_polys) + commitment (plonk/prover.rs:189-223)."""
        ctx = ctx or self.ctx
        h = ctypes.c_void_p()
        if deltas is None:
            check(lib.gl_partial_products(ctx.handle, self.handle, d_wires_ptr, _p(_u64(betas)), _p(_u64(gammas)), ctypes.byref(h)))
        else:
            check(lib.gl_partial_products_lookups(ctx.handle, self.handle, d_wires_ptr, _p(_u64(betas)), _p(_u64(gammas)), _p(_u64(deltas)), ctypes.byref(h)))
        return self._batch(h.value, ctx)

    def quotient_polys(self, wires_batch, zs_batch, public_inputs_hash, betas, gammas, alphas, ctx=None, deltas=None):
        """compute_quotient_polys + chunking + commitment (plonk/prover.rs:229-271)."""
        ctx = ctx or self.ctx
        h = ctypes.c_void_p()
        if deltas is None:
            check(lib.gl_quotient_polys(ctx.handle, self.handle, wires_batch.handle, zs_batch.handle, _p(_u64(public_inputs_hash)),
                                        _p(_u64(betas)), _p(_u64(gammas)), _p(_u64(alphas)), ctypes.byref(h)))
        else:
            check(lib.gl_quotient_polys_lookups(ctx.handle, self.handle, wires_batch.handle, zs_batch.handle, _p(_u64(public_inputs_hash)),
                                                _p(_u64(betas)), _p(_u64(gammas)), _p(_u64(alphas)), _p(_u64(deltas)), ctypes.byref(h)))
        return self._batch(h.value, ctx)

    def fri(self, batches, zeta, alpha, ctx=None):
        """PolynomialBatch::prove_openings up to fri_proof (fri/oracle.rs:162-204)."""
        return FriProver(self, batches, zeta, alpha, ctx or self.ctx)


class CircuitData(_CircuitApi):
    """The matmul demo's CircuitData, built from its host circuit (gl_circuit_from_host)."""

    def __init__(self, host, ctx):
        h = ctypes.c_void_p()
        check(lib.gl_circuit_from_host(ctx.handle, host.handle, ctypes.byref(h)))
        super().__init__(h.value, ctx, host.desc)
        self.host = host


class GenericCircuitData(_CircuitApi):
    """Prover + verifier for ANY circuit over the demo's gate set, given what CircuitBuilder::build() produces: the descriptor
    (CommonCircuitData) and the constants || sigmas value columns (gl_circuit_create)."""

    def __init__(self, desc, constants_sigmas, ctx=None):
        ctx = _ctx(ctx)
        cs = _u64(constants_sigmas)
        if cs.shape != (desc.num_constants + 80, 1 << desc.degree_bits):
            raise ValueError("constants_sigmas must be [num_constants + 80][n]")
        h = ctypes.c_void_p()
        check(lib.gl_circuit_create(ctx.handle, ctypes.byref(desc), _p(cs), ctypes.byref(h)))
        super().__init__(h.value, ctx)

    @classmethod
    def from_classes(cls, desc, constants, wire_classes, ctx=None):
        """The same from the constant columns [num_constants][n] and the copy-constraint class id of every routed wire [80][n] (equal id
        = constrained equal): the sigma polynomials are computed on the device (gl_circuit_create_from_classes)."""
        ctx = _ctx(ctx)
        n = 1 << desc.degree_bits
        consts, classes = _u64(constants), _u64(wire_classes)
        if consts.shape != (desc.num_constants, n) or classes.shape != (80, n):
            raise ValueError("constants must be [num_constants][n] and wire_classes [80][n]")
        h = ctypes.c_void_p()
        check(lib.gl_circuit_create_from_classes(ctx.handle, ctypes.byref(desc), _p(consts), _p(classes), ctypes.byref(h)))
        self = cls.__new__(cls)
        _CircuitApi.__init__(self, h.value, ctx)
        return self


class CircuitView(_CircuitApi):
    """The same device-resident CircuitData (or GenericCircuitData) used from another context (stream) of the same device."""
    handle_owned = False

    def __init__(self, circuit_data, ctx):
        super().__init__(circuit_data.handle, ctx, circuit_data.desc)
        self.cd = circuit_data          # the owner of the handle outlives the view


def verify_check_message(check):
    """The text gl_verify leaves in gl_last_error for the rejecting site `check` (a GL_CHECK_* code); "" for an accepted proof."""
    return (lib.gl_verify_check_message(int(check)) or b"").decode()


class BatchVerifier(_Owned):
    """VerifierCircuitData::verify for many proofs of one circuit per call (gl_batch_verifier): per proof the decode, the transcript, the
    vanishing identity and the proof of work on `host_threads` host threads, the Merkle paths (hash/merkle_proofs.rs:54-75) and the FRI
    queries (fri/verifier.rs:124-241) of all of them in two launches per `max_batch` proofs on the context's stream.  Takes what
    gl_verify takes: the description, the constants/sigmas cap and the circuit digest."""
    _free = "gl_batch_verifier_free"

    def __init__(self, desc, constants_sigmas_cap, circuit_digest, ctx=None, max_batch=64, host_threads=1):
        ctx = _ctx(ctx)
        cap, dig = _u64(constants_sigmas_cap), _u64(circuit_digest)
        if cap.size != 4 << desc.cap_height or dig.size != 4:
            raise ValueError("cap must be [2^cap_height][4], digest [4]")
        h = ctypes.c_void_p()
        check(lib.gl_batch_verifier_new(ctx.handle, ctypes.byref(desc), _p(cap), _p(dig), int(max_batch), int(host_threads), ctypes.byref(h)))
        self.handle, self.ctx, self.desc, self.checks = h.value, ctx, desc, []

    def verify(self, proofs):
        """[(accepted, reason)] for `proofs` (Proof objects or their bytes), the pair CircuitData.verify gives for each alone; `checks`
        then holds the GL_CHECK_* codes.  A proof too short for the description's counts raises, as it does there."""
        bufs = [bytes(p.to_bytes() if hasattr(p, "to_bytes") else p) for p in proofs]
        n = len(bufs)
        ptrs = (ctypes.c_char_p * max(n, 1))(*bufs)
        sizes = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bufs])
        verdicts, checks = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32)
        check(lib.gl_batch_verifier_verify(self.handle, ptrs, sizes, n, _p(verdicts), _p(checks)))
        self.checks = [int(c) for c in checks[:n]]
        out = []
        for st, c in zip(verdicts[:n], self.checks):
            if st not in (_lib.GL_OK, _lib.GL_ERR_VERIFY):
                raise _lib.Plonky2Mi355xError(int(st), verify_check_message(c))
            out.append((st == _lib.GL_OK, verify_check_message(c)))
        return out


# ------------------------------------------------------------------------------- circuit data as bytes (host code)
def common_data_to_bytes(desc):
    """CommonCircuitData::to_bytes of a gl_circuit_desc (util/serialization/mod.rs:1736-1790)."""
    n = ctypes.c_size_t()
    check(lib.gl_common_data_to_bytes(ctypes.byref(desc), None, 0, ctypes.byref(n)))
    buf = np.empty(n.value, dtype=np.uint8)
    check(lib.gl_common_data_to_bytes(ctypes.byref(desc), _p(buf), buf.size, ctypes.byref(n)))
    return buf.tobytes()


def common_data_from_bytes(data):
    """-> (CircuitDesc, bytes consumed); GL_ERR_UNSUPPORTED for gates / features outside the demo's set."""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    d, used = _lib.CircuitDesc(), ctypes.c_size_t()
    check(lib.gl_common_data_from_bytes(_p(buf), buf.size, ctypes.byref(d), ctypes.byref(used)))
    return d, used.value


def verifier_only_to_bytes(constants_sigmas_cap, circuit_digest, hasher="poseidon"):
    """VerifierOnlyCircuitData::to_bytes; the hasher is a type parameter on the Rust side and not in the bytes (a Keccak hash is 25 bytes)."""
    cap, dig = _u64(constants_sigmas_cap).reshape(-1, 4), _u64(circuit_digest)
    h = _log2_strict(cap.shape[0])
    n = ctypes.c_size_t()
    buf = np.empty(8 + 32 * cap.shape[0] + 32, dtype=np.uint8)
    check(lib.gl_verifier_only_to_bytes_h(hasher_id(hasher), h, _p(cap), _p(dig), _p(buf), buf.size, ctypes.byref(n)))
    return buf[: n.value].tobytes()


def verifier_only_from_bytes(data, hasher="poseidon"):
    """-> (cap[2^h][4], digest[4], bytes consumed)"""
    buf = np.frombuffer(bytes(data), dtype=np.uint8)
    h, used, hid = ctypes.c_uint32(), ctypes.c_size_t(), hasher_id(hasher)
    dig = np.empty(4, dtype=np.uint64)
    check(lib.gl_verifier_only_from_bytes_h(hid, _p(buf), buf.size, ctypes.byref(h), None, 0, _p(dig), ctypes.byref(used)))
    cap = np.empty((1 << h.value, 4), dtype=np.uint64)
    check(lib.gl_verifier_only_from_bytes_h(hid, _p(buf), buf.size, ctypes.byref(h), _p(cap), cap.size, _p(dig), ctypes.byref(used)))
    return cap, dig, used.value


def verifier_data_to_bytes(desc, constants_sigmas_cap, circuit_digest):
    """VerifierCircuitData::to_bytes = verifier_only || common (util/serialization/mod.rs:1908-1919), under desc.hasher."""
    return verifier_only_to_bytes(constants_sigmas_cap, circuit_digest, hasher=desc.hasher) + common_data_to_bytes(desc)


def verify_bytes(verifier_data, proof_bytes, hasher="poseidon"):
    """VerifierCircuitData::from_bytes(verifier_data).verify(proof): (accepted, reason)."""
    vd = np.frombuffer(bytes(verifier_data), dtype=np.uint8)
    pb = np.frombuffer(bytes(proof_bytes), dtype=np.uint8)
    return _verdict(lib.gl_verify_bytes_h(hasher_id(hasher), _p(vd), vd.size, _p(pb), pb.size))


class GenericProverPool(_Owned):
    """gl_prover_pool_create_generic / _prove_columns: `lanes` warmed-up contexts and host threads inside the library for ANY circuit
    (description + constants || sigmas); a batch of host witnesses (135 column vectors each) becomes one call."""
    _free = "gl_prover_pool_free"

    def __init__(self, desc, constants_sigmas, lanes=4, device=0):
        self.desc, self.n = desc, 1 << desc.degree_bits
        cs = _u64(constants_sigmas)
        if cs.shape != (desc.num_constants + 80, self.n):
            raise ValueError("constants_sigmas must be [num_constants + 80][n]")
        h = ctypes.c_void_p()
        check(lib.gl_prover_pool_create_generic(device, ctypes.byref(desc), _p(cs), lanes, ctypes.byref(h)))
        self.handle = h.value

    def prove_columns(self, witnesses):
        """witnesses: list of (columns, public_inputs), columns = 135 arrays of n u64 (or a [135][n] matrix); returns the Proofs in order."""
        k = len(witnesses)
        keep, col_ptrs, pi_ptrs = [], (ctypes.c_void_p * k)(), (ctypes.c_void_p * k)()
        for i, (cols, pis) in enumerate(witnesses):
            cols = [np.ascontiguousarray(_u64(c).reshape(-1)) for c in cols]
            if len(cols) != 135 or any(c.size != self.n for c in cols):
                raise ValueError("a witness is 135 columns of n values")
            arr = (ctypes.c_void_p * 135)(*[c.ctypes.data for c in cols])
            pv = np.ascontiguousarray(_u64(pis).reshape(-1))
            if pv.size != self.desc.num_public_inputs:
                raise ValueError("wrong number of public inputs")
            keep.append((cols, arr, pv))
            col_ptrs[i] = ctypes.addressof(arr)
            pi_ptrs[i] = pv.ctypes.data if pv.size else None
        out = (ctypes.c_void_p * k)()
        st = lib.gl_prover_pool_prove_columns(self.handle, k, col_ptrs, pi_ptrs, out)
        proofs = [Proof(out[i], self.desc) if out[i] else None for i in range(k)]
        check(st)
        return proofs


class ProverPool(_Owned):
    """Many proofs in flight on one GPU from one call (gl_prover_pool_*): one circuit, `lanes` streams and host threads in C++."""
    _free = "gl_prover_pool_free"

    def __init__(self, host, lanes=4, device=0):
        self.host = host
        h = ctypes.c_void_p()
        check(lib.gl_prover_pool_create(device, host.handle, lanes, ctypes.byref(h)))
        self.handle = h.value

    @property
    def circuit_digest(self):
        return _circuit_digest(lib.gl_prover_pool_circuit(self.handle))

    @property
    def constants_sigmas_cap(self):
        return _constants_sigmas_cap(lib.gl_prover_pool_circuit(self.handle), self.host.desc.cap_height)

    def prove_matmul(self, operands, filler_seeds=None):
        """operands: list of (a, b) m x m arrays; returns the list of Proof objects in the same order."""
        m2 = self.host.m ** 2
        aa = [np.ascontiguousarray(_u64(a).reshape(-1)) for a, _ in operands]
        bb = [np.ascontiguousarray(_u64(b).reshape(-1)) for _, b in operands]
        if any(x.size != m2 for x in aa + bb):
            raise ValueError("operands must be m x m")
        k = len(operands)
        pa = (ctypes.c_void_p * k)(*[x.ctypes.data for x in aa])
        pb = (ctypes.c_void_p * k)(*[x.ctypes.data for x in bb])
        seeds = None if filler_seeds is None else np.ascontiguousarray(np.asarray(filler_seeds, dtype=np.uint64))
        out = (ctypes.c_void_p * k)()
        st = lib.gl_prover_pool_prove_matmul(self.handle, k, pa, pb, _p(seeds) if seeds is not None else None, out)
        proofs = [Proof(out[i], self.host.desc) if out[i] else None for i in range(k)]      # owned from here on: freed even when a lane failed
        check(st)
        return proofs


class FriProver(_Owned):
    """fri_proof (fri/prover.rs:20-66) split at every transcript dependency."""
    _free = "gl_fri_free"

    def __init__(self, cd, batches, zeta, alpha, ctx):
        self.ctx, self.cd, self.batches = ctx, cd, list(batches)     # the batches must outlive the FRI state
        self.params = _lib.FriParams.of_circuit(cd.desc)
        arr = (ctypes.c_void_p * 4)(*[b.handle for b in self.batches])
        h = ctypes.c_void_p()
        check(lib.gl_fri_combine(ctx.handle, cd.handle, arr, _p(_u64(zeta)), _p(_u64(alpha)), ctypes.byref(h)))
        self.handle = h.value

    @classmethod
    def from_instance(cls, instance, oracles, alpha, fri_params, ctx=None, per_batch=False):
        """prove_openings up to fri_proof (fri/oracle.rs:183-204) for any FriInstance (gl_fri_combine_instance).  per_batch: the diagnostic
        form that reduces and divides one batch after the other."""
        self = cls.__new__(cls)
        self.batches = list(oracles)
        self.ctx, self.cd, self.params, self.instance = ctx or self.batches[0].ctx, None, fri_params, instance
        arr = (ctypes.c_void_p * max(len(self.batches), 1))(*[b.handle for b in self.batches])
        h = ctypes.c_void_p()
        check((lib.gl_fri_combine_instance_per_batch if per_batch else lib.gl_fri_combine_instance)(self.ctx.handle, ctypes.byref(fri_params), ctypes.byref(instance), arr, _p(_u64(alpha)), ctypes.byref(h)))
        self.handle = h.value
        return self

    def commit_round(self):
        cap = np.empty((1 << self.params.cap_height, 4), dtype=np.uint64)
        check(lib.gl_fri_commit_round(self.handle, _p(cap)))
        return cap

    def fold(self, beta):
        check(lib.gl_fri_fold(self.handle, _p(_u64(beta))))

    def final_poly(self):
        k = ctypes.c_size_t()
        check(lib.gl_fri_final_poly(self.handle, None, 0, ctypes.byref(k)))
        out = np.empty(k.value, dtype=np.uint64)
        check(lib.gl_fri_final_poly(self.handle, _p(out), out.size, ctypes.byref(k)))
        return out.reshape(-1, 2)

    def query(self, x_index):
        xi = np.ascontiguousarray(np.asarray(x_index, dtype=np.uint32))
        k = ctypes.c_size_t()
        check(lib.gl_fri_query(self.handle, _p(xi), xi.size, None, 0, ctypes.byref(k)))
        blob = np.empty(k.value, dtype=np.uint8)
        check(lib.gl_fri_query(self.handle, _p(xi), xi.size, _p(blob), blob.size, ctypes.byref(k)))
        return blob.tobytes()


class Challenger(_Owned):
    """plonky2::iop::challenger::Challenger (iop/challenger.rs:30-153), host code."""
    _free = "gl_challenger_free"

    def __init__(self, hasher="poseidon"):
        self.hasher = hasher_id(hasher)
        self.handle = lib.gl_challenger_new_h(self.hasher)

    def observe_hashes(self, digests, hasher=None):
        """observe_hash / observe_cap (challenger.rs:72-80) of [k][4] digests of `hasher` (default: the Challenger's own)."""
        d = _u64(digests).reshape(-1, 4)
        check(lib.gl_challenger_observe_hashes(self.handle, self.hasher if hasher is None else hasher_id(hasher), _p(d), d.shape[0]))

    def observe_elements(self, xs):
        a = _u64(np.asarray(xs, dtype=np.uint64).reshape(-1))
        check(lib.gl_challenger_observe(self.handle, _p(a), a.size))

    def get_n_challenges(self, n):
        out = np.empty(n, dtype=np.uint64)
        check(lib.gl_challenger_get_challenges(self.handle, _p(out), n))
        return [int(x) for x in out]

    def compact(self):
        """Challenger::compact (challenger.rs:146-152): absorb pending input, drop the buffered outputs."""
        check(lib.gl_challenger_compact(self.handle))

    def state(self):
        """(sponge_state[12], input_buffer) as fri_proof_of_work reads them."""
        st, buf, k = np.empty(12, dtype=np.uint64), np.empty(8, dtype=np.uint64), ctypes.c_uint32()
        check(lib.gl_challenger_state(self.handle, _p(st), _p(buf), ctypes.byref(k)))
        return st, buf[: k.value].copy()


def verify_fri_proof(instance, caps, openings, challenger, proof, fri_params):
    """verify_fri_proof (fri/verifier.rs:62-241) with the challenges drawn from `challenger` (in the state prove_openings expects): host
    code.  caps [num_oracles][2^cap_height][4], openings: every batch's values in order, [.][2] -> (accepted, message, GL_CHECK_* code)."""
    caps, openings = _u64(caps).reshape(-1), _u64(openings).reshape(-1)
    # counts the C arrays cannot hold are the library's to refuse (before it reads anything); within them the arrays must be long enough
    if instance.num_oracles <= _lib.GL_MAX_FRI_ORACLES and instance.num_batches <= _lib.GL_MAX_FRI_BATCHES and fri_params.cap_height <= min(24, fri_params.degree_bits + fri_params.rate_bits):
        listed = sum(instance.batch_len[b] for b in range(instance.num_batches))
        if caps.size < instance.num_oracles * (4 << fri_params.cap_height) or openings.size < 2 * listed:
            raise ValueError("caps are [num_oracles][2^cap_height][4], openings one extension value per listed polynomial")
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    code = ctypes.c_uint32()
    st = lib.gl_verify_openings(ctypes.byref(fri_params), ctypes.byref(instance), _p(caps), _p(openings), challenger.handle,
                                _p(buf) if buf.size else None, buf.size, ctypes.byref(code))
    ok, why = _verdict(st)
    return ok, why, code.value


def _batch_verdicts(verdicts, checks, what):
    """[(accepted, message, code)] of a batch call's per-item verdicts; one that is neither accept nor reject raises, as alone"""
    out = []
    for i, (st, c) in enumerate(zip(verdicts, checks)):
        if st not in (_lib.GL_OK, _lib.GL_ERR_VERIFY):
            raise _lib.Plonky2Mi355xError(int(st), verify_check_message(c) or "%s %d was refused, as it is alone" % (what, i))
        out.append((st == _lib.GL_OK, verify_check_message(c), int(c)))
    return out


class OpeningsBatchVerifier(_Owned):
    """verify_fri_proof (fri/verifier.rs:62-241) for many claims over one (instance, fri_params) per call (gl_openings_batch_verifier):
    per claim what verify_fri_proof does before its query loop on `host_threads` host threads, the Merkle paths and the queries of all
    of them in two launches per `max_batch` claims on the context's stream.  The instance's own points are ignored."""
    _free = "gl_openings_batch_verifier_free"

    def __init__(self, instance, fri_params, ctx=None, max_batch=64, host_threads=1):
        ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        check(lib.gl_openings_batch_verifier_new(ctx.handle, ctypes.byref(fri_params), ctypes.byref(instance), int(max_batch), int(host_threads), ctypes.byref(h)))
        self.handle, self.ctx, self.instance, self.params = h.value, ctx, instance, fri_params

    def verify(self, claims):
        """claims: [(caps, openings, points, challenger, proof)] with caps [num_oracles][2^cap_height][4], openings every batch's values
        in order, points [num_batches][2], a Challenger of its own per claim (consumed) -> [(accepted, message, GL_CHECK_* code)], what
        verify_fri_proof gives for each alone (the message without the source position)."""
        n = len(claims)
        arr, keep = (_lib.OpeningsClaim * max(n, 1))(), []
        listed = self.instance.num_opened
        for i, (caps, openings, points, challenger, proof) in enumerate(claims):
            caps, openings, points = _u64(caps).reshape(-1), _u64(openings).reshape(-1), _u64(points).reshape(-1)
            by = bytes(proof)
            buf = np.frombuffer(by or b"\0", dtype=np.uint8)                # (an empty proof: a pointer to read nothing from)
            if caps.size < self.instance.num_oracles * (4 << self.params.cap_height) or openings.size < 2 * listed or points.size < 2 * self.instance.num_batches:
                raise ValueError("caps are [num_oracles][2^cap_height][4], openings one extension value per listed polynomial, points [num_batches][2]")
            keep.append((caps, openings, points, challenger, buf))
            arr[i] = _lib.OpeningsClaim(caps.ctypes.data, openings.ctypes.data, points.ctypes.data, challenger.handle, buf.ctypes.data, len(by))
        verdicts, checks = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32)
        check(lib.gl_openings_batch_verifier_verify(self.handle, arr, n, _p(verdicts), _p(checks)))
        self.verdicts, self.checks = [int(v) for v in verdicts[:n]], [int(c) for c in checks[:n]]      # (kept for a caller whom a refusal below leaves without the list)
        return _batch_verdicts(self.verdicts, self.checks, "claim")


# ------------------------------------------------------------------------------------- STARK: an AIR as data
class StarkConfig:
    """starky::config::StarkConfig (starky/src/config.rs): num_challenges and the FriConfig."""

    def __init__(self, num_challenges, rate_bits, cap_height, proof_of_work_bits, num_query_rounds, arity_bits=4, final_poly_bits=5):
        self.num_challenges, self.rate_bits, self.cap_height = num_challenges, rate_bits, cap_height
        self.proof_of_work_bits, self.num_query_rounds = proof_of_work_bits, num_query_rounds
        self.arity_bits, self.final_poly_bits = arity_bits, final_poly_bits

    @classmethod
    def standard_fast_config(cls):
        """config.rs:17-29: rate 2, 84 queries, 16 bits of work, ConstantArityBits(4, 5)."""
        return cls(2, 1, 4, 16, 84, 4, 5)

    def fri_params(self, degree_bits, hasher="poseidon"):
        """StarkConfig::fri_params (config.rs:31-33; hiding = false) with FriReductionStrategy::ConstantArityBits
        (fri/reduction_strategies.rs:39-50)."""
        arities, d = [], degree_bits
        while d > self.final_poly_bits and d + self.rate_bits - self.arity_bits >= self.cap_height:
            arities.append(self.arity_bits)
            d -= self.arity_bits
        return _lib.FriParams(degree_bits, self.rate_bits, self.cap_height, self.proof_of_work_bits, self.num_query_rounds, arities, False, hasher)


class StarkDesc:
    """A Stark (starky/src/stark.rs) as data: constraints = [(filter, [(coeff, [(kind, index), ...]), ...]), ...] in the order
    eval_packed_generic yields them, filter one of GL_STARK_ALL / TRANSITION / FIRST_ROW / LAST_ROW, kind one of GL_STARK_LOCAL / NEXT /
    PUBLIC; pairs = Stark::permutation_pairs() as [[(lhs, rhs), ...], ...]."""

    def __init__(self, num_columns, num_public_inputs, constraint_degree, constraints, pairs=()):
        self.num_columns, self.num_public_inputs, self.constraint_degree = num_columns, num_public_inputs, constraint_degree
        self.constraints = [(f, [(c, list(ops)) for c, ops in terms]) for f, terms in constraints]
        self.pairs = [list(p) for p in pairs]

    @property
    def quotient_degree_factor(self):
        return max(1, self.constraint_degree - 1)                     # stark.rs:79-81

    @property
    def quotient_degree_bits(self):
        return (self.quotient_degree_factor - 1).bit_length()         # log2_ceil

    def num_permutation_batches(self, num_challenges):
        return -(-len(self.pairs) * num_challenges // self.quotient_degree_factor)      # stark.rs:216-221

    def struct(self, num_challenges):
        return _lib.StarkDescStruct(self.num_columns, self.num_public_inputs, self.constraint_degree, num_challenges, self.constraints, self.pairs)

    def check(self, config, degree_bits, hasher="poseidon"):
        """gl_stark_check: raises Plonky2Mi355xError with the refusal; needs no GPU."""
        params = config.fri_params(degree_bits, hasher)
        check(lib.gl_stark_check(ctypes.byref(self.struct(config.num_challenges)), ctypes.byref(params)))


class StarkDagDesc(StarkDesc):
    """A Stark whose constraints are an expression DAG (gl_stark_dag beside a gl_stark_desc without a term list): nodes = [(op, operand
    word a, operand word b), ...] in SSA order, constants = 64-bit words, constraints = [(filter, operand word), ...] in the order the
    Stark yields them; operand words are _lib.stark_operand(kind, index).  StarkDagBuilder writes one.  Stark, StarkSetDesc and
    stark_verify take it wherever they take a StarkDesc."""

    def __init__(self, num_columns, num_public_inputs, constraint_degree, nodes, constants, constraints, pairs=()):
        super().__init__(num_columns, num_public_inputs, constraint_degree, [], pairs)
        self.nodes, self.constants = [tuple(int(w) for w in node) for node in nodes], [int(v) for v in constants]
        self.dag_constraints = [(int(f), int(w)) for f, w in constraints]

    def struct(self, num_challenges):
        st = super().struct(num_challenges)
        for field in ("constraint_filter", "constraint_num_terms", "term_coeff", "term_num_factors", "factors"):
            setattr(st, field, None)                                   # one form or the other per table
        return st

    def dag_struct(self):
        return _lib.StarkDagStruct(self.nodes, self.constants, self.dag_constraints)

    def check(self, config, degree_bits, hasher="poseidon"):
        """gl_stark_dag_check: raises Plonky2Mi355xError with the refusal; needs no GPU."""
        params = config.fri_params(degree_bits, hasher)
        check(lib.gl_stark_dag_check(ctypes.byref(self.struct(config.num_challenges)), ctypes.byref(self.dag_struct()), ctypes.byref(params)))

    def stats(self):
        """gl_stark_dag_stats -> (max live, the largest degree of a constraint, instructions of the compiled program); needs no GPU."""
        a, b, c = ctypes.c_uint32(), ctypes.c_uint32(), ctypes.c_uint32()
        check(lib.gl_stark_dag_stats(ctypes.byref(self.struct(1)), ctypes.byref(self.dag_struct()), ctypes.byref(a), ctypes.byref(b), ctypes.byref(c)))
        return a.value, b.value, c.value


class StarkDagExpr:
    """A value of a StarkDagBuilder: an operand word.  + - * build nodes; an int is coerced to a constant."""
    __slots__ = ("builder", "word")

    def __init__(self, builder, word):
        self.builder, self.word = builder, word

    def __add__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_ADD, self, other)

    def __radd__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_ADD, other, self)

    def __sub__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_SUB, self, other)

    def __rsub__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_SUB, other, self)

    def __mul__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_MUL, self, other)

    def __rmul__(self, other):
        return self.builder._node(_lib.GL_STARK_OP_MUL, other, self)


class StarkDagBuilder:
    """Writes a StarkDagDesc the way a Stark writes eval_packed_generic: local(c) / next(c) / public(i) / const(v) are the leaves, + - *
    on them the nodes, and constraint* the ConstraintConsumer's four methods, in the order they are called.  Expressions are
    hash-consed: the same op on the same operands, written twice, is one node; a constant written twice is one constant."""

    def __init__(self, num_columns, num_public_inputs):
        self.num_columns, self.num_public_inputs = num_columns, num_public_inputs
        self.nodes, self.constants, self.constraints = [], [], []
        self._node_of, self._const_of = {}, {}

    def local(self, c):
        return StarkDagExpr(self, _lib.stark_operand(_lib.GL_STARK_LOCAL, c))

    def next(self, c):
        return StarkDagExpr(self, _lib.stark_operand(_lib.GL_STARK_NEXT, c))

    def public(self, i):
        return StarkDagExpr(self, _lib.stark_operand(_lib.GL_STARK_PUBLIC, i))

    def const(self, v):
        """a 64-bit word as it stands (it may be non-canonical); any other int mod p"""
        v = int(v)
        if not 0 <= v < 1 << 64:
            v %= GOLDILOCKS_ORDER
        if v not in self._const_of:
            self._const_of[v] = len(self.constants)
            self.constants.append(v)
        return StarkDagExpr(self, _lib.stark_operand(_lib.GL_STARK_CONST, self._const_of[v]))

    def _expr(self, e):
        if isinstance(e, StarkDagExpr):
            if e.builder is not self:
                raise ValueError("an expression of another builder")
            return e
        return self.const(e)

    def _node(self, op, a, b):
        key = (op, self._expr(a).word, self._expr(b).word)
        if key not in self._node_of:
            self._node_of[key] = len(self.nodes)
            self.nodes.append(key)
        return StarkDagExpr(self, _lib.stark_operand(_lib.GL_STARK_NODE, self._node_of[key]))

    def _constraint(self, filt, e):
        self.constraints.append((filt, self._expr(e).word))

    def constraint(self, e):
        self._constraint(_lib.GL_STARK_ALL, e)

    def constraint_transition(self, e):
        self._constraint(_lib.GL_STARK_TRANSITION, e)

    def constraint_first_row(self, e):
        self._constraint(_lib.GL_STARK_FIRST_ROW, e)

    def constraint_last_row(self, e):
        self._constraint(_lib.GL_STARK_LAST_ROW, e)

    def build(self, constraint_degree, pairs=()):
        return StarkDagDesc(self.num_columns, self.num_public_inputs, constraint_degree, self.nodes, self.constants, self.constraints, pairs)


class Stark(_Owned):
    """A checked description with its tables in HBM (gl_stark): starky's prove() and verify, and the two STARK-only prover phases on their
    own, every polynomial device-resident."""
    _free = "gl_stark_free"

    def __init__(self, desc, config, degree_bits, hasher="poseidon", ctx=None):
        self.ctx, self.desc, self.config, self.degree_bits = _ctx(ctx), desc, config, degree_bits
        self.params = config.fri_params(degree_bits, hasher)
        h = ctypes.c_void_p()
        if isinstance(desc, StarkDagDesc):
            check(lib.gl_stark_dag_create(self.ctx.handle, ctypes.byref(desc.struct(config.num_challenges)), ctypes.byref(desc.dag_struct()),
                                          ctypes.byref(self.params), ctypes.byref(h)))
        else:
            check(lib.gl_stark_create(self.ctx.handle, ctypes.byref(desc.struct(config.num_challenges)), ctypes.byref(self.params), ctypes.byref(h)))
        self.handle = h.value

    def commit_trace(self, trace):
        """PolynomialBatch::from_values of the trace columns (prover.rs:52-65)."""
        return PolynomialBatch.from_values(trace, self.params.rate_bits, False, self.params.cap_height, ctx=self.ctx, hasher=self.params.hasher)

    def _challenges(self, challenge_sets):
        if challenge_sets is None:
            return None
        ch = _u64(challenge_sets)
        if ch.size != self.desc.quotient_degree_factor * self.config.num_challenges * 2:
            raise ValueError("challenge sets are [quotient_degree_factor][num_challenges][2] (beta, gamma)")
        return ch

    def permutation_zs(self, trace, challenge_sets):
        """compute_permutation_z_polys + commitment (permutation.rs:66-117, prover.rs:89-100).  trace: [num_columns][n] values."""
        t = _u64(trace)
        if t.shape != (self.desc.num_columns, 1 << self.degree_bits):
            raise ValueError("the trace is [num_columns][n]")
        if challenge_sets is None:
            raise ValueError("the Z polynomials need the challenge sets")
        d = DeviceBuffer(self.ctx, t.nbytes).upload(t)
        try:
            h = ctypes.c_void_p()
            check(lib.gl_stark_permutation_zs(self.ctx.handle, self.handle, d.ptr, _p(self._challenges(challenge_sets)), ctypes.byref(h)))
        finally:
            d.free()
        return PolynomialBatch(h.value, self.ctx, self.params.rate_bits, self.params.cap_height)

    def _quotient_args(self, trace_batch, zs_batch, challenge_sets, alphas, public_inputs):
        ch, al, pi = self._challenges(challenge_sets), _u64(alphas), _u64(public_inputs)
        if al.size != self.config.num_challenges or pi.size != self.desc.num_public_inputs:
            raise ValueError("alphas are [num_challenges], public inputs [num_public_inputs]")
        return (self.ctx.handle, self.handle, trace_batch.handle, zs_batch.handle if zs_batch is not None else None,
                _p(ch) if ch is not None else None, _p(al), _p(pi) if pi.size else None), (ch, al, pi)

    def quotient_values(self, trace_batch, zs_batch, challenge_sets, alphas, public_inputs):
        """(sum alpha^i C_i) / Z_H on the quotient coset (prover.rs:198-311), [num_challenges][n << quotient_degree_bits]; no degree check."""
        args, keep = self._quotient_args(trace_batch, zs_batch, challenge_sets, alphas, public_inputs)
        out = np.empty((self.config.num_challenges, (1 << self.degree_bits) << self.desc.quotient_degree_bits), dtype=np.uint64)
        check(lib.gl_stark_quotient_values(*args, _p(out)))
        return out

    def quotient_polys(self, trace_batch, zs_batch, challenge_sets, alphas, public_inputs):
        """The same, then coset_ifft, the trim_to_len check, the chunks of n and from_coeffs (prover.rs:114-144)."""
        args, keep = self._quotient_args(trace_batch, zs_batch, challenge_sets, alphas, public_inputs)
        h = ctypes.c_void_p()
        check(lib.gl_stark_quotient_polys(*args, ctypes.byref(h)))
        return PolynomialBatch(h.value, self.ctx, self.params.rate_bits, self.params.cap_height)


    @property
    def proof_size(self):
        return lib.gl_stark_proof_size(self.handle)

    def _public_inputs(self, public_inputs):
        pi = _u64(public_inputs)
        if pi.size != self.desc.num_public_inputs:
            raise ValueError("the Stark has %d public inputs" % self.desc.num_public_inputs)
        return pi

    def prove(self, trace, public_inputs):
        """starky::prover::prove (prover.rs:32-194): trace [num_columns][n] values -> the proof's bytes (layout: include/plonky2_mi355x.h)."""
        cols = [_u64(c) for c in trace]
        if len(cols) != self.desc.num_columns or any(c.size != 1 << self.degree_bits for c in cols):
            raise ValueError("the trace is [num_columns][n]")
        pi = self._public_inputs(public_inputs)
        ptrs = (ctypes.c_void_p * len(cols))(*[c.ctypes.data for c in cols])
        out, k = np.empty(self.proof_size, dtype=np.uint8), ctypes.c_size_t()
        check(lib.gl_stark_prove(self.ctx.handle, self.handle, ptrs, _p(pi) if pi.size else None, _p(out), out.size, ctypes.byref(k)))
        return out[:k.value].tobytes()

    def prove_device(self, d_cols_ptr, public_inputs):
        """The same with the trace in HBM, d_cols[num_columns][n]."""
        pi = self._public_inputs(public_inputs)
        out, k = np.empty(self.proof_size, dtype=np.uint8), ctypes.c_size_t()
        check(lib.gl_stark_prove_device(self.ctx.handle, self.handle, d_cols_ptr, _p(pi) if pi.size else None, _p(out), out.size, ctypes.byref(k)))
        return out[:k.value].tobytes()

    def verify(self, proof):
        """verify_stark_proof (verifier.rs:21-145), host code -> (accepted, message, GL_CHECK_* code)."""
        return stark_verify(self.desc, self.config, self.degree_bits, proof, hasher=self.params.hasher)

    def batch_verifier(self, max_batch=64, host_threads=1):
        """A StarkBatchVerifier for this Stark on its context."""
        return StarkBatchVerifier(self.desc, self.config, self.degree_bits, self.params.hasher, self.ctx, max_batch, host_threads)


def stark_verify(desc, config, degree_bits, proof, hasher="poseidon"):
    """gl_stark_verify (gl_stark_dag_verify for a StarkDagDesc): needs no GPU and no Stark handle -> (accepted, message, GL_CHECK_* code)."""
    if isinstance(desc, StarkDagDesc):
        return stark_dag_verify(desc, config, degree_bits, proof, hasher)
    params = config.fri_params(degree_bits, hasher)
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    code = ctypes.c_uint32()
    st = lib.gl_stark_verify(ctypes.byref(desc.struct(config.num_challenges)), ctypes.byref(params), _p(buf) if buf.size else None, buf.size, ctypes.byref(code))
    ok, why = _verdict(st)
    return ok, why, code.value


def stark_dag_verify(desc, config, degree_bits, proof, hasher="poseidon"):
    """gl_stark_dag_verify of a StarkDagDesc -> (accepted, message, GL_CHECK_* code)."""
    params = config.fri_params(degree_bits, hasher)
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    code = ctypes.c_uint32()
    st = lib.gl_stark_dag_verify(ctypes.byref(desc.struct(config.num_challenges)), ctypes.byref(desc.dag_struct()), ctypes.byref(params),
                                 _p(buf) if buf.size else None, buf.size, ctypes.byref(code))
    ok, why = _verdict(st)
    return ok, why, code.value


class StarkBatchVerifier(_Owned):
    """verify_stark_proof for many proofs of one Stark per call (gl_stark_batch_verifier): per proof what gl_stark_verify
    (gl_stark_dag_verify for a StarkDagDesc) does before its verify_fri_proof on `host_threads` host threads, the Merkle paths and the FRI
    queries of all of them in two launches per `max_batch` proofs on the context's stream."""
    _free = "gl_stark_batch_verifier_free"

    def __init__(self, desc, config, degree_bits, hasher="poseidon", ctx=None, max_batch=64, host_threads=1):
        ctx = _ctx(ctx)
        self.params = config.fri_params(degree_bits, hasher)
        dag = desc.dag_struct() if isinstance(desc, StarkDagDesc) else None
        h = ctypes.c_void_p()
        check(lib.gl_stark_batch_verifier_new(ctx.handle, ctypes.byref(desc.struct(config.num_challenges)), ctypes.byref(dag) if dag is not None else None,
                                              ctypes.byref(self.params), int(max_batch), int(host_threads), ctypes.byref(h)))
        self.handle, self.ctx, self.desc, self.config, self.degree_bits = h.value, ctx, desc, config, degree_bits

    def verify(self, proofs):
        """[(accepted, message, GL_CHECK_* code)] for `proofs` (bytes), what Stark.verify gives for each alone (the message without the
        source position)."""
        bufs = [bytes(p) for p in proofs]
        n = len(bufs)
        ptrs = (ctypes.c_char_p * max(n, 1))(*bufs)
        sizes = (ctypes.c_size_t * max(n, 1))(*[len(b) for b in bufs])
        verdicts, checks = np.zeros(max(n, 1), dtype=np.int32), np.zeros(max(n, 1), dtype=np.uint32)
        check(lib.gl_stark_batch_verifier_verify(self.handle, ptrs, sizes, n, _p(verdicts), _p(checks)))
        self.verdicts, self.checks = [int(v) for v in verdicts[:n]], [int(c) for c in checks[:n]]
        return _batch_verdicts(self.verdicts, self.checks, "proof")


# ------------------------------------------------------------------------------------- STARK table sets: cross-table lookups
class CtlColumn:
    """evm's Column (cross_table_lookup.rs:24-116): a linear combination of trace columns plus a constant."""

    def __init__(self, terms=(), constant=0):
        self.terms, self.const = [(int(c), int(f)) for c, f in terms], int(constant)

    @classmethod
    def single(cls, c):
        return cls([(c, 1)])

    @classmethod
    def singles(cls, cs):
        return [cls.single(c) for c in cs]

    @classmethod
    def constant(cls, constant):
        return cls([], constant)

    @classmethod
    def linear_combination(cls, terms, constant=0):
        """linear_combination_with_constant: a duplicate column is the library's to refuse (gl_stark_set_check)."""
        terms = list(terms)
        if not terms:
            raise ValueError("a linear combination has at least one term (CtlColumn.constant for none)")
        return cls(terms, constant)

    @classmethod
    def le_bits(cls, cs):
        return cls.linear_combination([(c, pow(2, k, GOLDILOCKS_ORDER)) for k, c in enumerate(cs)])

    @classmethod
    def sum(cls, cs):
        return cls.linear_combination([(c, 1) for c in cs])

    def flat(self):
        return self.terms, self.const


class TableWithColumns:
    """cross_table_lookup.rs:141-156: a table index, its Columns and an optional filter Column."""

    def __init__(self, table, columns, filter_column=None):
        self.table, self.columns, self.filter_column = int(table), list(columns), filter_column

    def flat(self):
        return self.table, [c.flat() for c in self.columns], None if self.filter_column is None else self.filter_column.flat()


class CrossTableLookup:
    """cross_table_lookup.rs:158-186: the looking tables and the looked one."""

    def __init__(self, looking_tables, looked_table):
        self.looking_tables, self.looked_table = list(looking_tables), looked_table

    def flat(self):
        return [t.flat() for t in self.looking_tables], self.looked_table.flat()


class StarkSetDesc:
    """Tables [(StarkDesc, degree_bits), ...] under one StarkConfig, tied by cross-table lookups (gl_stark_set_desc)."""

    def __init__(self, tables, lookups, config, hasher="poseidon"):
        self.tables, self.lookups, self.config, self.hasher = [(d, int(lg)) for d, lg in tables], list(lookups), config, hasher

    def fri_params(self, table):
        return self.config.fri_params(self.tables[table][1], self.hasher)

    def struct(self):
        return _lib.StarkSetDescStruct([(d.struct(self.config.num_challenges), self.config.fri_params(lg, self.hasher)) for d, lg in self.tables],
                                       [l.flat() for l in self.lookups])

    def dags(self):
        """(gl_stark_dag*[num_tables] with a null entry per table in term-list form, or None where every table is; what keeps it alive)"""
        structs = [d.dag_struct() if isinstance(d, StarkDagDesc) else None for d, _ in self.tables]
        if not any(s is not None for s in structs):
            return None, structs
        return (ctypes.c_void_p * len(structs))(*[ctypes.addressof(s) if s is not None else None for s in structs]), structs

    def check(self):
        """gl_stark_set_check (gl_stark_set_dag_check with a StarkDagDesc among the tables): raises Plonky2Mi355xError with the refusal."""
        dags, keep = self.dags()
        check(lib.gl_stark_set_check(ctypes.byref(self.struct())) if dags is None else lib.gl_stark_set_dag_check(ctypes.byref(self.struct()), dags))

    def num_zs(self, table):
        """(permutation Zs, CTL Zs) of a table: stark.rs:216-221 and cross_table_lookup.rs:178-185."""
        if self.dags()[0] is not None:                                 # the counts do not depend on the constraints' form
            self.check()
            nc = self.config.num_challenges
            twcs = [t for l in self.lookups for t in list(l.looking_tables) + [l.looked_table]]
            return self.tables[table][0].num_permutation_batches(nc), nc * sum(1 for t in twcs if t.table == table)
        a, b = ctypes.c_uint32(), ctypes.c_uint32()
        check(lib.gl_stark_set_num_zs(ctypes.byref(self.struct()), table, ctypes.byref(a), ctypes.byref(b)))
        return a.value, b.value


class StarkSet(_Owned):
    """A checked table set with every table's tables and CTL programs in HBM (gl_stark_set)."""
    _free = "gl_stark_set_free"

    def __init__(self, desc, ctx=None):
        self.ctx, self.desc = _ctx(ctx), desc
        h = ctypes.c_void_p()
        dags, keep = desc.dags()
        if dags is None:
            check(lib.gl_stark_set_create(self.ctx.handle, ctypes.byref(desc.struct()), ctypes.byref(h)))
        else:
            check(lib.gl_stark_set_dag_create(self.ctx.handle, ctypes.byref(desc.struct()), dags, ctypes.byref(h)))
        self.handle = h.value
        self.counts = [desc.num_zs(t) for t in range(len(desc.tables))]

    def _trace(self, table, trace):
        d, lg = self.desc.tables[table]
        t = _u64(trace)
        if t.shape != (d.num_columns, 1 << lg):
            raise ValueError("the trace of table %d is [num_columns][n]" % table)
        return t

    def _ctl_challenges(self, ctl_challenges):
        ch = _u64(ctl_challenges)
        if ch.size != 2 * self.desc.config.num_challenges:
            raise ValueError("the CTL challenges are [num_challenges][2] (beta, gamma)")
        return ch

    def _permutation_sets(self, table, permutation_challenge_sets):
        if permutation_challenge_sets is None:
            return None
        sets = _u64(permutation_challenge_sets)
        if sets.size != self.desc.tables[table][0].quotient_degree_factor * self.desc.config.num_challenges * 2:
            raise ValueError("challenge sets are [quotient_degree_factor][num_challenges][2] (beta, gamma)")
        return sets

    @property
    def proof_size(self):
        return lib.gl_stark_set_proof_size(self.handle)

    def prove(self, traces, public_inputs=None):
        """prove_with_traces (evm/src/prover.rs:94-285): traces[table] = [num_columns][n] values -> the set proof's bytes."""
        cols = [[_u64(c) for c in self._trace(t, trace)] for t, trace in enumerate(traces)]
        if len(cols) != len(self.desc.tables):
            raise ValueError("one trace per table")
        pis = [_u64([] if public_inputs is None else public_inputs[t]) for t in range(len(cols))]
        if any(pi.size != d.num_public_inputs for pi, (d, _) in zip(pis, self.desc.tables)):
            raise ValueError("public inputs are [num_tables][num_public_inputs of the table]")
        per_table = [(ctypes.c_void_p * len(cs))(*[c.ctypes.data for c in cs]) for cs in cols]
        ptrs = (ctypes.c_void_p * len(cols))(*[ctypes.addressof(a) for a in per_table])
        pi_ptrs = (ctypes.c_void_p * len(cols))(*[pi.ctypes.data if pi.size else None for pi in pis])
        out, k = np.empty(self.proof_size, dtype=np.uint8), ctypes.c_size_t()
        check(lib.gl_stark_set_prove(self.ctx.handle, self.handle, ptrs, pi_ptrs, _p(out), out.size, ctypes.byref(k)))
        return out[:k.value].tobytes()

    def verify(self, proof):
        return stark_set_verify(self.desc, proof)

    def ctl_z_values(self, table, trace, ctl_challenges):
        """partial_products (cross_table_lookup.rs:279-306) of every CTL Z of a table, by value: [num_ctl_zs][n]."""
        t, ch = self._trace(table, trace), self._ctl_challenges(ctl_challenges)
        out = np.empty((self.counts[table][1], t.shape[1]), dtype=np.uint64)
        d = DeviceBuffer(self.ctx, t.nbytes).upload(t)
        try:
            check(lib.gl_stark_set_ctl_z_values(self.ctx.handle, self.handle, table, d.ptr, _p(ch), _p(out) if out.size else None))
        finally:
            d.free()
        return out

    def zs(self, table, trace, permutation_challenge_sets, ctl_challenges):
        """The committed Z batch of a table (evm/src/prover.rs:341-352): its permutation Zs, then its CTL Zs."""
        t, ch = self._trace(table, trace), self._ctl_challenges(ctl_challenges)
        sets = self._permutation_sets(table, permutation_challenge_sets)
        d = DeviceBuffer(self.ctx, t.nbytes).upload(t)
        try:
            h = ctypes.c_void_p()
            check(lib.gl_stark_set_zs(self.ctx.handle, self.handle, table, d.ptr, _p(sets) if sets is not None else None, _p(ch), ctypes.byref(h)))
        finally:
            d.free()
        params = self.desc.fri_params(table)
        return PolynomialBatch(h.value, self.ctx, params.rate_bits, params.cap_height)


    def _quotient_args(self, table, trace_batch, zs_batch, permutation_challenge_sets, ctl_challenges, alphas, public_inputs):
        d = self.desc.tables[table][0]
        sets = self._permutation_sets(table, permutation_challenge_sets)
        ch, al, pi = self._ctl_challenges(ctl_challenges), _u64(alphas), _u64(public_inputs)
        if al.size != self.desc.config.num_challenges or pi.size != d.num_public_inputs:
            raise ValueError("alphas are [num_challenges], public inputs [num_public_inputs]")
        return (self.ctx.handle, self.handle, table, trace_batch.handle, zs_batch.handle, _p(sets) if sets is not None else None, _p(ch), _p(al),
                _p(pi) if pi.size else None), (sets, ch, al, pi)

    def quotient_values(self, table, trace_batch, zs_batch, permutation_challenge_sets, ctl_challenges, alphas, public_inputs):
        """The quotient's values on the quotient coset with the CTL checks after the permutation checks, [num_challenges][n << qdb]."""
        args, keep = self._quotient_args(table, trace_batch, zs_batch, permutation_challenge_sets, ctl_challenges, alphas, public_inputs)
        d, lg = self.desc.tables[table]
        out = np.empty((self.desc.config.num_challenges, (1 << lg) << d.quotient_degree_bits), dtype=np.uint64)
        check(lib.gl_stark_set_quotient_values(*args, _p(out)))
        return out

    def quotient_polys(self, table, trace_batch, zs_batch, permutation_challenge_sets, ctl_challenges, alphas, public_inputs):
        """The same, then coset_ifft, the trim_to_len check, the chunks of n and from_coeffs."""
        args, keep = self._quotient_args(table, trace_batch, zs_batch, permutation_challenge_sets, ctl_challenges, alphas, public_inputs)
        h = ctypes.c_void_p()
        check(lib.gl_stark_set_quotient_polys(*args, ctypes.byref(h)))
        params = self.desc.fri_params(table)
        return PolynomialBatch(h.value, self.ctx, params.rate_bits, params.cap_height)


def stark_set_verify(desc, proof):
    """gl_stark_set_verify: needs no GPU and no handle -> (accepted, message, GL_CHECK_* code, table the check failed in)."""
    buf = np.frombuffer(bytes(proof), dtype=np.uint8)
    code, table = ctypes.c_uint32(), ctypes.c_uint32()
    dags, keep = desc.dags()
    if dags is None:
        st = lib.gl_stark_set_verify(ctypes.byref(desc.struct()), _p(buf) if buf.size else None, buf.size, ctypes.byref(code), ctypes.byref(table))
    else:
        st = lib.gl_stark_set_dag_verify(ctypes.byref(desc.struct()), dags, _p(buf) if buf.size else None, buf.size, ctypes.byref(code), ctypes.byref(table))
    ok, why = _verdict(st)
    return ok, why, code.value, table.value


def fibonacci_stark(num_rows):
    """FibonacciStark (starky/src/fibonacci_stark.rs): (description, trace generator).  generate_trace(x0, x1) -> [4][num_rows] values
    (fibonacci_stark.rs:44-57); the public inputs are x0, x1 and column 1 of the last row."""
    L, N, PUB, p = _lib.GL_STARK_LOCAL, _lib.GL_STARK_NEXT, _lib.GL_STARK_PUBLIC, GOLDILOCKS_ORDER
    m1 = p - 1
    desc = StarkDesc(4, 3, 2, [
        (_lib.GL_STARK_FIRST_ROW, [(1, [(L, 0)]), (m1, [(PUB, 0)])]),
        (_lib.GL_STARK_FIRST_ROW, [(1, [(L, 1)]), (m1, [(PUB, 1)])]),
        (_lib.GL_STARK_LAST_ROW, [(1, [(L, 1)]), (m1, [(PUB, 2)])]),
        (_lib.GL_STARK_TRANSITION, [(1, [(N, 0)]), (m1, [(L, 1)])]),                       # x0' <- x1
        (_lib.GL_STARK_TRANSITION, [(1, [(N, 1)]), (m1, [(L, 0)]), (m1, [(L, 1)])]),       # x1' <- x0 + x1
    ], [[(2, 3)]])

    def generate_trace(x0, x1):
        rows, acc = [], [int(x0) % p, int(x1) % p, 0, 1]
        for _ in range(num_rows):
            rows.append(list(acc))
            acc = [acc[1], (acc[0] + acc[1]) % p, (acc[2] + 1) % p, (acc[3] + 1) % p]
        rows[num_rows - 1][3] = 0                      # so that columns 2 and 3 are permutations of one another
        return np.array(rows, dtype=np.uint64).T.copy()
    return desc, generate_trace


# ------------------------------------------------------------------------------------- STARK lookups (evm/src/lookup.rs)
def lookup_constraints(col_permuted_input, col_permuted_table):
    """eval_lookups (lookup.rs:13-34) as two constraints of a StarkDesc, in the order it yields them:
    constraint((next_in - local_in)(next_in - next_table)), expanded to four terms, and constraint_last_row(next_in - next_table)."""
    L, N, m1 = _lib.GL_STARK_LOCAL, _lib.GL_STARK_NEXT, GOLDILOCKS_ORDER - 1
    i, t = col_permuted_input, col_permuted_table
    return [
        (_lib.GL_STARK_ALL, [(1, [(N, i), (N, i)]), (m1, [(N, i), (N, t)]), (m1, [(L, i), (N, i)]), (1, [(L, i), (N, t)])]),
        (_lib.GL_STARK_LAST_ROW, [(1, [(N, i)]), (m1, [(N, t)])]),
    ]


def permuted_cols_host(inputs, table):
    """permuted_cols (lookup.rs:65-127) on the host, the reference's sequential algorithm -> (permuted_inputs, permuted_table)."""
    a, t = _u64(inputs).ravel(), _u64(table).ravel()
    if a.size != t.size or a.size == 0:
        raise ValueError("inputs and table are two columns of one length >= 1")
    pin, ptab = np.empty(a.size, dtype=np.uint64), np.empty(a.size, dtype=np.uint64)
    check(lib.gl_permuted_cols_host(_p(a), _p(t), a.size, _p(pin), _p(ptab)))
    return pin, ptab


def permuted_cols(inputs, table, ctx=None):
    """permuted_cols (lookup.rs:65-127) through the device entry: a four-column trace whose columns 0 and 1 are uploaded and whose
    columns 2 and 3 come back -> (permuted_inputs, permuted_table)."""
    ctx = _ctx(ctx)
    a, t = _u64(inputs).ravel(), _u64(table).ravel()
    if a.size != t.size:
        raise ValueError("inputs and table are two columns of one length")
    n = a.size
    d = DeviceBuffer(ctx, max(1, 4 * n * 8)).upload(np.stack([a, t]))
    try:
        ctx.lookup_columns(d.ptr, 4, n, [(0, 1, 2, 3)])
        out = np.empty((2, n), dtype=np.uint64)
        check(lib.gl_copy_d2h(ctx.handle, _p(out), d.ptr + 2 * n * 8, out.nbytes))
    finally:
        d.free()
    return out[0], out[1]


# ------------------------------------------------------------------------------------- MemoryStark (evm/src/memory)
MEMORY_OP_DTYPE = np.dtype(_lib.MEMORY_OP_FIELDS)                      # gl_memory_op: MemoryOp (witness/memory.rs:80-87), 56 bytes


def memory_stark():
    """MemoryStark (memory_stark.rs:243-321, :450-459) as a StarkDesc, read from the library's own tables (gl_memory_stark_desc)."""
    ptr = ctypes.c_void_p()
    check(lib.gl_memory_stark_desc(ctypes.byref(ptr)))
    d = ctypes.cast(ptr, ctypes.POINTER(_lib.StarkDescStruct)).contents
    constraints, t, f = [], 0, 0
    for c in range(d.num_constraints):
        terms = []
        for _ in range(d.constraint_num_terms[c]):
            ops = [(d.factors[f + k] >> 30, d.factors[f + k] & 0x3FFFFFFF) for k in range(d.term_num_factors[t])]
            terms.append((int(d.term_coeff[t]), ops))
            f += d.term_num_factors[t]
            t += 1
        constraints.append((int(d.constraint_filter[c]), terms))
    pairs, k = [], 0
    for p in range(d.num_permutation_pairs):
        pairs.append([(int(d.pair_columns[2 * (k + i)]), int(d.pair_columns[2 * (k + i) + 1])) for i in range(d.pair_len[p])])
        k += d.pair_len[p]
    return StarkDesc(d.num_columns, d.num_public_inputs, d.constraint_degree, constraints, pairs)


def memory_ctl_data():
    """ctl_data (memory_stark.rs:30-36): IS_READ, the address, the eight value limbs, TIMESTAMP."""
    cols = [_lib.GL_MEMORY_IS_READ, _lib.GL_MEMORY_ADDR_CONTEXT, _lib.GL_MEMORY_ADDR_SEGMENT, _lib.GL_MEMORY_ADDR_VIRTUAL]
    cols += [_lib.GL_MEMORY_VALUE_START + i for i in range(_lib.GL_MEMORY_VALUE_LIMBS)]
    return CtlColumn.singles(cols + [_lib.GL_MEMORY_TIMESTAMP])


def memory_ctl_filter():
    """ctl_filter (memory_stark.rs:38-40)."""
    return CtlColumn.single(_lib.GL_MEMORY_FILTER)


def _memory_ops(ops):
    a = np.ascontiguousarray(ops)
    if a.dtype != MEMORY_OP_DTYPE or a.ndim != 1:
        raise ValueError("memory ops are a one-dimensional array of MEMORY_OP_DTYPE records")
    return a


def memory_trace_host(ops):
    """MemoryStark::generate_trace (memory_stark.rs:120-237) on the host, the reference's loops -> [26][n]; needs no GPU."""
    a = _memory_ops(ops)
    n = ctypes.c_size_t()
    check(lib.gl_memory_trace_host(_p(a) if a.size else None, a.size, None, 0, ctypes.byref(n)))
    out = np.empty((_lib.GL_MEMORY_NUM_COLUMNS, n.value), dtype=np.uint64)
    check(lib.gl_memory_trace_host(_p(a), a.size, _p(out), n.value, ctypes.byref(n)))
    return out


class MemoryTrace(_Owned):
    """gl_memory_trace: a memory-operation log sorted and counted on the device.  `rows` is the trace's height, known before the Stark
    is made; fill(d_ptr) writes all 26 columns of d_cols[26][rows], stream-ordered, any number of times.  ops: MEMORY_OP_DTYPE records,
    or with device_ptr a log of num_ops records already in HBM."""
    _free = "gl_memory_trace_free"

    def __init__(self, ops=None, ctx=None, device_ptr=None, num_ops=None):
        self.ctx = _ctx(ctx)
        h = ctypes.c_void_p()
        if device_ptr is not None:
            check(lib.gl_memory_trace_new_device(self.ctx.handle, device_ptr, int(num_ops), ctypes.byref(h)))
        else:
            a = _memory_ops(ops)
            check(lib.gl_memory_trace_new(self.ctx.handle, _p(a) if a.size else None, a.size, ctypes.byref(h)))
        self.handle = h.value
        self.rows = lib.gl_memory_trace_rows(self.handle)

    def fill(self, d_cols_ptr):
        check(lib.gl_memory_trace_fill(self.handle, d_cols_ptr))


def pow_grind(sponge_state, input_buffer, min_leading_zeros, ctx=None, hasher="poseidon"):
    """fri_proof_of_work (fri/prover.rs:115-160): the smallest valid witness."""
    ctx = _ctx(ctx)
    st, buf = _u64(sponge_state), _u64(input_buffer)
    if st.size != 12:
        raise ValueError("sponge state has 12 words")
    w = np.zeros(1, dtype=np.uint64)
    check(lib.gl_pow_grind_h(ctx.handle, hasher_id(hasher), _p(st), _p(buf) if buf.size else None, buf.size, min_leading_zeros, _p(w)))
    return int(w[0])


class Proof(_Owned):
    """A proof of the circuit described by `desc` (gl_circuit_desc), which fixes the shapes of what it holds."""
    _free = "gl_proof_free"

    def __init__(self, handle, desc):
        self.handle, self.desc, self.n = handle, desc, 1 << desc.degree_bits

    def to_bytes(self):
        """ProofWithPublicInputs::to_bytes (plonk/proof.rs:104-110)."""
        k = lib.gl_proof_num_bytes(self.handle)
        buf = np.empty(k, dtype=np.uint8)
        check(lib.gl_proof_bytes(self.handle, _p(buf), k))
        return buf.tobytes()

    def challenges(self):
        out = np.zeros(64, dtype=np.uint64)
        k = lib.gl_proof_challenges(self.handle, _p(out))
        v = [int(x) for x in out[:k]]
        return {"betas": v[0:2], "gammas": v[2:4], "alphas": v[4:6], "zeta": v[6:8], "fri_alpha": v[8:10], "pow_witness": v[10],
                "public_inputs_hash": v[11:15], "fri_betas": [v[i:i + 2] for i in range(15, k, 2)]}

    def caps(self):
        """wires_cap, plonk_zs_partial_products_cap, quotient_polys_cap: [3][2^cap_height][4]."""
        out = np.empty((3, 1 << self.desc.cap_height, 4), dtype=np.uint64)
        check(lib.gl_proof_caps(self.handle, _p(out)))
        return out

    def zs_partial_products(self, ncols=None):
        """Z and partial products as value columns, then the lookup polynomials: [20 + 2 num_lookup_polys][n]."""
        want = 20 + 2 * self.desc.num_lookup_polys
        if ncols is not None and ncols != want:
            raise ValueError("this proof holds %d Z / partial-product / lookup columns, not %d" % (want, ncols))
        out = np.empty((want, self.n), dtype=np.uint64)
        check(lib.gl_proof_zs_partial_products(self.handle, _p(out)))
        return out

    def quotient_chunks(self):
        out = np.empty((16, self.n), dtype=np.uint64)
        check(lib.gl_proof_quotient_chunks(self.handle, _p(out)))
        return out

    def query_indices(self):
        out = np.zeros(256, dtype=np.uint64)
        k = lib.gl_proof_query_indices(self.handle, _p(out))
        return [int(x) for x in out[:k]]

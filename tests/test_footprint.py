"""GPU footprint tests: every entry point that takes a device pointer writes its documented output, every word of it, and nothing else.

Each case lays its caller-visible buffers out in ONE guarded arena (tests/footprint.py: guard, region, guard, ..., every word filled
with a position-dependent non-canonical pattern), calls the entry through the public ABI with pointers into the arena, downloads the
whole arena once and asserts: guards unchanged, `in` regions unchanged, `out` / `inout` regions equal to the reference, word for word.
Every case runs in two region orders, outputs before inputs and inputs before outputs.  The reference of an expected array is the one
the entry's by-value test uses (the CPU oracle, the integer models, the host entry pinned against RFC 8439), never the device call.
The host output buffers the library copies into get the same guards (the last section).  The sizes are the smallest that reach the
path named beside them.  What the arena cannot see: the library's own scratch and the buffers inside handles."""
import ctypes
import functools

import numpy as np
import pytest

import footprint as fp
from oracle_lib import P, rand_field

pytestmark = pytest.mark.gpu
U64 = np.uint64
SEED = bytes(range(32))
BOTH_ORDERS = pytest.mark.parametrize("order", fp.ORDERS)
EDGE_WORDS = [0, 1, 2**32 - 1, 2**32, P - 1, P, P + 1, 2**63, 2**64 - 2**32, 2**64 - 1]


def In(name, data, item=1):
    return fp.Region(name, "in", data=data, item=item)


def Out(name, expected, item=1):
    return fp.Region(name, "out", expected=expected, item=item)


def InOut(name, data, expected=None, item=1):
    return fp.Region(name, "inout", data=data, expected=expected, item=item)


def junk(shape, salt=0):
    """words no kernel writes: non-canonical (>= p), different at every index, and not the arena's own fill"""
    count = int(np.prod(shape))
    return (np.arange(count, dtype=U64) + U64(0xFFFFFFFFA5000000 + (salt << 16))).reshape(shape)


def words_with_edges(seed, shape, canonical=False):
    """seeded 64-bit words (any representative unless `canonical`) with the edge words in the first places"""
    rng = np.random.Generator(np.random.PCG64(seed))
    a = rng.integers(0, P if canonical else 2**64, size=shape, dtype=U64)
    flat = a.reshape(-1)
    edges = [e for e in EDGE_WORDS if not canonical or e < P]
    k = min(flat.size, len(edges))
    flat[flat.size - k:] = np.array(edges[:k], dtype=U64)
    return a


def lib_of(p):
    return p._lib.lib, p._lib.check


# ------------------------------------------------------------------------------- field and extension micro-kernels
def field_reference(orc, op, a, b, c):
    if op == 7:                                                       # as tests/test_gpu_parity.py: the integers
        return np.array([int(x) * pow(2, int(k) % 192, P) % P for x, k in zip(a, b)], dtype=U64)
    return orc.field_op(op, a, b, c)


def field_operands(op, n):
    a, b, c = (words_with_edges(100 * op + n + k, n) for k in range(3))
    if op == 4:
        a[a % U64(P) == 0] = 3                                        # the inverse of zero is not defined
    return a, b, c


@BOTH_ORDERS
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("op", range(8))
def test_field_op_separate_buffers(gpu, orc, op, n, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    a, b, c = field_operands(op, n)
    with fp.device_arena(ctx, [In("a", a), In("b", b), In("c", c), Out("out", field_reference(orc, op, a, b, c))], order) as ar:
        check(lib.gl_field_op(ctx.handle, op, ar.ptr("a"), ar.ptr("b"), ar.ptr("c"), ar.ptr("out"), n))
        ar.check()


@BOTH_ORDERS
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("op", range(8))
def test_field_op_with_out_aliasing_a(gpu, orc, op, n, order):
    # "out may alias a": a is read and written in place, b and c stay
    p, ctx = gpu
    lib, check = lib_of(p)
    a, b, c = field_operands(op, n)
    with fp.device_arena(ctx, [InOut("a", a, field_reference(orc, op, a, b, c)), In("b", b), In("c", c)], order) as ar:
        check(lib.gl_field_op(ctx.handle, op, ar.ptr("a"), ar.ptr("b"), ar.ptr("c"), ar.ptr("a"), n))
        ar.check()


@BOTH_ORDERS
@pytest.mark.parametrize("n", [1, 255, 257])
@pytest.mark.parametrize("op", range(4))
def test_ext_op(gpu, orc, op, n, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    a, b = words_with_edges(40 + op + n, 2 * n, canonical=True), words_with_edges(50 + op + n, 2 * n, canonical=True)
    if op == 3:
        a[0::2][(a[0::2] == 0) & (a[1::2] == 0)] = 5                  # no zero element under the inverse
    with fp.device_arena(ctx, [In("a", a, item=2), In("b", b, item=2), Out("out", orc.ext_op(op, a, b), item=2)], order) as ar:
        check(lib.gl_ext_op(ctx.handle, op, ar.ptr("a"), ar.ptr("b"), ar.ptr("out"), n))
        ar.check()


# ------------------------------------------------------------------------------- the NTT family, in place
# (0, 3) (1, 5) (5, 3) (12, 3): the single pass with ragged tail tiles; (13, 3): two passes; (13, 5): two passes with the inter-pass table
NTT_SHAPES = [(0, 3), (1, 5), (5, 3), (12, 3), (13, 3), (13, 5)]
NTT_KINDS = ("forward", "inverse", "coset_forward", "coset_inverse")
COSET_SHIFT_INVERSE = 0x123456789ABCDEF


@functools.lru_cache(maxsize=None)
def ntt_case(kind, lg, batch):
    import oracle_lib
    orc = oracle_lib.load()
    x = words_with_edges(1000 + 10 * lg + batch, (batch, 1 << lg))
    want = {"forward": lambda: orc.fft(x), "inverse": lambda: orc.ifft(x), "coset_forward": lambda: orc.coset_fft(x, 7),
            "coset_inverse": lambda: orc.coset_ifft(x, COSET_SHIFT_INVERSE)}[kind]()
    x.setflags(write=False)
    want.setflags(write=False)
    return x, want


@BOTH_ORDERS
@pytest.mark.parametrize("lg,batch", NTT_SHAPES)
@pytest.mark.parametrize("kind", NTT_KINDS)
def test_ntt_in_place(gpu, orc, kind, lg, batch, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    x, want = ntt_case(kind, lg, batch)
    with fp.device_arena(ctx, [InOut("data", x, want, item=1 << lg)], order) as ar:
        d = ar.ptr("data")
        if kind == "forward":
            check(lib.gl_ntt_forward(ctx.handle, d, lg, batch))
        elif kind == "inverse":
            check(lib.gl_ntt_inverse(ctx.handle, d, lg, batch))
        elif kind == "coset_forward":
            check(lib.gl_ntt_coset_forward(ctx.handle, d, lg, batch, 7))
        else:
            check(lib.gl_ntt_coset_inverse(ctx.handle, d, lg, batch, COSET_SHIFT_INVERSE))
        ar.check()


# (0, 3, 3) (3, 3, 5) (5, 1, 3) (9, 3, 3): the single pass with n_in < N; (12, 1, 3): two passes at rate 2, the STARK shape;
# (10, 3, 5): the zero-padded first stage with the inter-pass table
LDE_SHAPES = [(0, 3, 3), (3, 3, 5), (5, 1, 3), (9, 3, 3), (12, 1, 3), (10, 3, 5)]


@BOTH_ORDERS
@pytest.mark.parametrize("lg,rate,batch", LDE_SHAPES)
def test_ntt_coset_lde(gpu, orc, lg, rate, batch, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    coeffs = words_with_edges(2000 + 10 * lg + batch, (batch, 1 << lg))
    want = orc.lde(coeffs, rate, threads=4)
    assert want.shape == (batch, 1 << (lg + rate))
    with fp.device_arena(ctx, [In("coeffs", coeffs, item=1 << lg), Out("out", want, item=1 << (lg + rate))], order) as ar:
        check(lib.gl_ntt_coset_lde(ctx.handle, ar.ptr("coeffs"), lg, rate, batch, ar.ptr("out")))
        ar.check()


# ------------------------------------------------------------------------------- Poseidon and row hashing
POSEIDON_COUNTS = [1, 63, 65, 257]                                    # one lane, a wave less one, a wave and one, four waves and one


def poseidon_states(count):
    s = words_with_edges(3000 + count, (count, 12))
    s[0] = np.array([EDGE_WORDS[k % len(EDGE_WORDS)] for k in range(12)], dtype=U64)
    return s


@BOTH_ORDERS
@pytest.mark.parametrize("count", POSEIDON_COUNTS)
def test_poseidon_permute_in_place(gpu, orc, count, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    s = poseidon_states(count)
    with fp.device_arena(ctx, [InOut("states", s, orc.poseidon(s), item=12)], order) as ar:
        check(lib.gl_poseidon_permute(ctx.handle, ar.ptr("states"), count))
        ar.check()


@BOTH_ORDERS
@pytest.mark.parametrize("count", POSEIDON_COUNTS)
def test_poseidon_permute_raw_in_place_under_both_layers(gpu, orc, count, order):
    # raw u64 representatives: the words of layer 0, canonicalised, are the oracle's (a state the call left out would still hold its
    # input), and layer 1 leaves the same words; that no raw word equals the fill pattern at its place is asserted, not assumed
    p, ctx = gpu
    lib, check = lib_of(p)
    s = poseidon_states(count)
    want = orc.poseidon(s)
    with fp.device_arena(ctx, [InOut("states", s, item=12)], order) as ar:
        check(lib.gl_poseidon_permute_raw(ctx.handle, ar.ptr("states"), count, 0))
        ar.expect("states", want)
        bad = ar.violations()
        assert [v.kind for v in bad] in ([], ["inout"]), bad         # guards intact; the region holds raw words
        raw = ar.region_words("states").reshape(count, 12)
        assert (raw % U64(P) == want).all()
        ar.expect("states", raw)
        ar.assert_unwritten_words_would_show()
    with fp.device_arena(ctx, [InOut("states", s, raw, item=12)], order) as ar:
        check(lib.gl_poseidon_permute_raw(ctx.handle, ar.ptr("states"), count, 1))
        ar.check()


HASH_LENS = [1, 3, 4, 5, 8, 9, 135]                                   # copied (<= 3 / <= 4), one block, one block and one word, the wire row


@functools.lru_cache(maxsize=None)
def hash_case(hasher, count, length):
    import oracle_lib
    from test_keccak import model_hash_or_noop, noncanonical_rows
    rows = noncanonical_rows(7000 + 10 * count + length, count, length)
    if hasher == "keccak":
        want = model_hash_or_noop(rows)
    else:
        orc = oracle_lib.load()
        want = np.stack([orc.hash_or_noop(r) for r in rows])
    return rows, want


@BOTH_ORDERS
@pytest.mark.parametrize("count", [1, 65, 300])
@pytest.mark.parametrize("entry", ["gl_hash_rows", "gl_hash_rows_h-poseidon", "gl_hash_rows_h-keccak"])
def test_hash_rows(gpu, orc, entry, count, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    for length in HASH_LENS:
        rows, want = hash_case("keccak" if entry.endswith("keccak") else "poseidon", count, length)
        with fp.device_arena(ctx, [In("rows", rows, item=length), Out("out", want, item=4)], order) as ar:
            if entry == "gl_hash_rows":
                check(lib.gl_hash_rows(ctx.handle, ar.ptr("rows"), count, length, ar.ptr("out")))
            else:
                check(lib.gl_hash_rows_h(ctx.handle, 1 if entry.endswith("keccak") else 0, ar.ptr("rows"), count, length, ar.ptr("out")))
            bad = ar.violations()
            assert not bad, "len %d: %s" % (length, bad)


# ------------------------------------------------------------------------------- the keystream
# both ends inside a 4-element ChaCha block, one block, several blocks, several workgroups
RANDOM_SPANS = [(0, 1), (3, 1), (3, 2), (2, 3), (4, 4), (5, 4), (1, 1023), (1021, 1027)]


@BOTH_ORDERS
@pytest.mark.parametrize("first,count", RANDOM_SPANS)
def test_random_elements(gpu, first, count, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    stream = 0x100 + 77
    want = p.random_elements(SEED, stream, first, count, ctx=False)   # the host entry, pinned against RFC 8439 by test_zero_knowledge.py
    with fp.device_arena(ctx, [Out("out", want, item=4)], order) as ar:
        check(lib.gl_random_elements(ctx.handle, ctypes.create_string_buffer(SEED, 32), stream, first, count, ar.ptr("out")))
        ar.check()


# ------------------------------------------------------------------------------- witness generation and blinding
@BOTH_ORDERS
@pytest.mark.parametrize("m", [1, 3, 5])
def test_matmul_witgen_run(gpu, m, order):
    p, ctx = gpu
    hc = p.MatmulCircuit(m)
    a, b = rand_field(9000 + m, m * m), rand_field(9500 + m, m * m)
    wires, pis = hc.witness(a, b, filler_seed=m)
    gen = hc.witness_generator(ctx)
    with fp.device_arena(ctx, [Out("wires", wires, item=hc.n)], order) as ar:
        assert (gen.run(a, b, ar.ptr("wires"), filler_seed=m) == pis).all()
        ar.check()
    gen.close()


@BOTH_ORDERS
def test_witness_blind(gpu, order):
    # rows below num_gate_rows stay as uploaded in all 135 columns; from there on every word is written: random rows, copied pairs, zeros
    from zk_circuits import model_blinded_wires
    p, ctx = gpu
    m = 2
    hc = p.MatmulCircuit(m, zero_knowledge=True)
    cd = hc.build(ctx)
    g = hc.desc.num_gate_rows
    wires, _ = hc.witness(rand_field(3, m * m) % (2**32 - 1), rand_field(4, m * m) % (2**32 - 1), filler_seed=5)
    want = model_blinded_wires(wires, g, SEED)
    assert 0 < g < hc.n and (want[:, :g] == wires[:, :g]).all() and (want[:, g:] == 0).any()
    stale = wires.copy()
    stale[:, g:] = junk((135, hc.n - g))                              # zeros are expected there: they must be written, not found
    with fp.device_arena(ctx, [InOut("wires", stale, want, item=hc.n)], order) as ar:
        cd.blind_witness(ar.ptr("wires"), seed=SEED)
        ar.check()


# ------------------------------------------------------------------------------- commitments and prover phases from a device matrix
@BOTH_ORDERS
@pytest.mark.parametrize("ncols,n", [(1, 8), (5, 32), (135, 256)])
@pytest.mark.parametrize("is_values", [True, False], ids=["values", "coeffs"])
@pytest.mark.parametrize("entry", ["gl_batch_from_device", "gl_batch_from_device_h-poseidon", "gl_batch_from_device_h-keccak"])
def test_batch_from_device(gpu, orc, entry, is_values, ncols, n, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    cols = rand_field(600 + ncols, (ncols, n))
    hasher = "keccak" if entry.endswith("keccak") else "poseidon"
    host = (p.PolynomialBatch.from_values if is_values else p.PolynomialBatch.from_coeffs)(cols, 3, False, 4, ctx=ctx, hasher=hasher)
    if hasher == "poseidon":
        assert (host.cap == orc.batch(cols, 3, 4, from_values=is_values, threads=4).cap).all()
    with fp.device_arena(ctx, [In("cols", cols, item=n)], order) as ar:
        if entry != "gl_batch_from_device":
            b = p.PolynomialBatch.from_device(ar.ptr("cols"), ncols, n, 3, 4, is_values, ctx=ctx, hasher=hasher)
        else:
            h = ctypes.c_void_p()
            check(lib.gl_batch_from_device(ctx.handle, ar.ptr("cols"), ncols, n, 3, 4, 1 if is_values else 0, ctypes.byref(h)))
            b = p.PolynomialBatch(h.value, ctx, 3, 4)
        assert (b.cap == host.cap).all() and (b.polynomials == host.polynomials).all()
        ar.check()
    b.free()
    host.free()


@pytest.fixture(scope="module")
def matmul2(gpu, orc):
    """the m = 2 circuit, its witness and the oracle's proof of it"""
    from types import SimpleNamespace
    p, ctx = gpu
    m = 2
    hc = p.MatmulCircuit(m)
    a, b = rand_field(7000 + m, m * m) % (2**32 - 1), rand_field(7001 + m, m * m) % (2**32 - 1)
    wires, pis = hc.witness(a, b, filler_seed=m)
    op = orc.circuit(m, threads=4).witness(a, b, filler_seed=m).prove(threads=4)
    return SimpleNamespace(hc=hc, cd=hc.build(ctx), wires=wires, pis=pis, op=op, bytes=op.to_bytes())


@BOTH_ORDERS
def test_partial_products(gpu, orc, matmul2, order):
    p, ctx = gpu
    c = matmul2
    ch = c.op.challenges()
    with fp.device_arena(ctx, [In("wires", c.wires, item=c.hc.n)], order) as ar:
        zs = c.cd.partial_products(ar.ptr("wires"), ch["betas"], ch["gammas"], ctx=ctx)
        assert (orc.fft(zs.polynomials) == c.op.zs_partial_products()).all()
        ar.check()
    zs.free()


@BOTH_ORDERS
def test_prove_device(gpu, matmul2, order):
    p, ctx = gpu
    c = matmul2
    with fp.device_arena(ctx, [In("wires", c.wires, item=c.hc.n)], order) as ar:
        assert c.cd.prove_device(ar.ptr("wires"), c.pis).to_bytes() == c.bytes
        ar.check()


# ------------------------------------------------------------------------------- STARK entries on device traces, n = 32
@BOTH_ORDERS
@pytest.mark.parametrize("name", ["cubic", "quartic"])
def test_stark_permutation_zs(gpu, orc, name, order):
    import stark_airs
    import stark_model as sm
    from test_stark import NC, config_of, desc_of, flat_sets, sets_of
    p, ctx = gpu
    lib, check = lib_of(p)
    air = stark_airs.AIRS[name]
    trace, _ = air.trace(32, seed=6)
    sets = sets_of("random", np.random.Generator(np.random.PCG64(31)), air)
    want, _ = sm.permutation_zs(air, NC, trace, sets)
    stark = p.Stark(desc_of(p, air), config_of(p, air), 5, ctx=ctx)
    with fp.device_arena(ctx, [In("trace", trace, item=32)], order) as ar:
        h = ctypes.c_void_p()
        check(lib.gl_stark_permutation_zs(ctx.handle, stark.handle, ar.ptr("trace"), flat_sets(sets).ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)))
        zs = p.PolynomialBatch(h.value, ctx, stark.params.rate_bits, stark.params.cap_height)
        assert (orc.fft(zs.polynomials) == np.array(want, dtype=U64)).all()
        ar.check()
    zs.free()


@BOTH_ORDERS
@pytest.mark.parametrize("name", ["fibonacci", "cubic", "quartic", "wide"])
def test_stark_prove_device(gpu, name, order):
    import stark_airs
    from test_stark import config_of, desc_of
    p, ctx = gpu
    air = stark_airs.AIRS[name]
    trace, pis = air.trace(32, seed=6)
    stark = p.Stark(desc_of(p, air), config_of(p, air), 5, ctx=ctx)
    want = stark.prove(trace, pis)                                    # the host-trace call, checked by tests/test_stark.py
    assert stark.verify(want) == (True, "", 0)
    with fp.device_arena(ctx, [In("trace", trace, item=32)], order) as ar:
        assert stark.prove_device(ar.ptr("trace"), pis) == want
        ar.check()


@pytest.fixture(scope="module")
def ctl_set(gpu):
    import stark_ctl_airs as airs
    from types import SimpleNamespace
    p, ctx = gpu
    lgs = [5, 6, 5]
    config = airs.config(p, 2)
    sset = p.StarkSet(airs.api_set(p, airs.TABLES, airs.LOOKUPS, lgs, config), ctx=ctx)
    return SimpleNamespace(sset=sset, lgs=lgs, traces=airs.traces(lgs, seed=7), config=config)


@BOTH_ORDERS
@pytest.mark.parametrize("table", [0, 1, 2])
def test_stark_set_ctl_z_values(gpu, ctl_set, table, order):
    import stark_ctl_airs as airs
    from test_stark_ctl import challenges_of, flat, model_ctl_zs
    p, ctx = gpu
    lib, check = lib_of(p)
    s, trace = ctl_set, ctl_set.traces[table]
    chs = challenges_of("random", np.random.Generator(np.random.PCG64(90 + table)))
    want = np.array(model_ctl_zs(airs.LOOKUPS, table, trace, chs), dtype=U64)
    n = 1 << s.lgs[table]
    assert want.shape == (s.sset.counts[table][1], n)
    with fp.device_arena(ctx, [In("trace", trace, item=n)], order) as ar, fp.host_out(expected=want, item=n) as out:
        check(lib.gl_stark_set_ctl_z_values(ctx.handle, s.sset.handle, table, ar.ptr("trace"), np.array(flat(chs), dtype=U64).ctypes.data_as(ctypes.c_void_p),
                                            out.ptr("out")))
        ar.check()
        out.check()


@BOTH_ORDERS
@pytest.mark.parametrize("table", [0, 1])
def test_stark_set_zs(gpu, orc, ctl_set, table, order):
    # ops2 (table 1): one permutation Z, then its CTL Zs; ops (table 0): CTL Zs only
    import stark_ctl_airs as airs
    import stark_model as sm
    from test_stark_ctl import NC, challenges_of, flat, model_ctl_zs, values_of
    p, ctx = gpu
    s, trace, air = ctl_set, ctl_set.traces[table], airs.TABLES[table]
    rng = np.random.Generator(np.random.PCG64(95 + table))
    chs = challenges_of("random", rng)
    sets = [[tuple(values_of("random", rng, 2)) for _ in range(NC)] for _ in range(air.q)] if air.pairs else None
    want = (sm.permutation_zs(air, NC, trace, sets)[0] if sets else []) + model_ctl_zs(airs.LOOKUPS, table, trace, chs)
    lib, check = lib_of(p)
    perm = np.array([w for st in sets for ch in st for w in ch], dtype=U64) if sets else None
    with fp.device_arena(ctx, [In("trace", trace, item=1 << s.lgs[table])], order) as ar:
        h = ctypes.c_void_p()
        check(lib.gl_stark_set_zs(ctx.handle, s.sset.handle, table, ar.ptr("trace"), perm.ctypes.data_as(ctypes.c_void_p) if sets else None,
                                  np.array(flat(chs), dtype=U64).ctypes.data_as(ctypes.c_void_p), ctypes.byref(h)))
        zs = p.PolynomialBatch(h.value, ctx, s.config.rate_bits, s.config.cap_height)
        assert (orc.fft(zs.polynomials) == np.array(want, dtype=U64)).all()
        ar.check()
    zs.free()


@BOTH_ORDERS
def test_stark_set_prove_device(gpu, ctl_set, order):
    p, ctx = gpu
    lib, check = lib_of(p)
    s = ctl_set
    want = s.sset.prove(s.traces)                                     # the host-trace call, checked by tests/test_stark_ctl.py
    assert s.sset.verify(want)[:3] == (True, "", 0)
    regions = [In("trace%d" % t, trace, item=1 << s.lgs[t]) for t, trace in enumerate(s.traces)]
    with fp.device_arena(ctx, regions, order) as ar, fp.host_out(expected=want) as out:
        ptrs = (ctypes.c_void_p * 3)(*[ar.ptr("trace%d" % t) for t in range(3)])
        k = ctypes.c_size_t()
        check(lib.gl_stark_set_prove_device(ctx.handle, s.sset.handle, ptrs, None, out.ptr("out"), len(want), ctypes.byref(k)))
        assert k.value == len(want)
        ar.check()
        out.check()


# ------------------------------------------------------------------------------- STARK lookups: permuted_cols inside a wider trace
# seven columns, two lookups that share the table column; outputs and inputs alternate, so that a column overrun of an output lands in
# an input.  The trace is one pointer, so it is one region: the inputs must come back, the four outputs are uploaded as junk
LOOKUP_INPUT_A, LOOKUP_TABLE, LOOKUP_INPUT_B = 1, 3, 5
LOOKUPS = [(LOOKUP_INPUT_A, LOOKUP_TABLE, 0, 2), (LOOKUP_INPUT_B, LOOKUP_TABLE, 4, 6)]


@functools.lru_cache(maxsize=None)
def lookup_case(n):
    import lookup_model as lm
    rng = np.random.Generator(np.random.PCG64(n))
    trace = junk((7, n))
    trace[LOOKUP_TABLE] = rng.permutation(n).astype(U64)
    trace[LOOKUP_INPUT_A] = rng.integers(0, n, size=n, dtype=U64)
    trace[LOOKUP_INPUT_B] = rng.integers(0, n + 3, size=n, dtype=U64)      # some values that are not in the table
    trace[LOOKUP_INPUT_B][::5] += U64(P)                                   # inputs may be non-canonical
    want = trace.copy()
    for a, t, pin, ptab in LOOKUPS:
        got_in, got_table = lm.permuted_cols([int(v) % P for v in trace[a]], [int(v) for v in trace[t]])
        want[pin], want[ptab] = np.array(got_in, dtype=U64), np.array(got_table, dtype=U64)
    return trace, want


@BOTH_ORDERS
@pytest.mark.parametrize("n", [2, 32, 4096])
def test_stark_lookup_columns(gpu, n, order):
    p, ctx = gpu
    trace, want = lookup_case(n)
    with fp.device_arena(ctx, [InOut("trace", trace, want, item=n)], order) as ar:
        ctx.lookup_columns(ar.ptr("trace"), 7, n, LOOKUPS)
        ar.check()


# ------------------------------------------------------------------------------- MemoryStark's trace
MEMORY_CASES = {1: "one-op", 16: "gap-rows-push-the-height-over-a-power-of-two", 512: "random-255"}      # the smallest logs of these heights


@BOTH_ORDERS
@pytest.mark.parametrize("n", sorted(MEMORY_CASES))
def test_memory_trace_from_a_device_log_filled_twice(gpu, n, order):
    import memory_cases as mc
    import memory_model as mm
    p, ctx = gpu
    log = mc.CASES[MEMORY_CASES[n]]
    want = np.array(mm.generate_trace(log), dtype=U64)
    assert want.shape == (26, n)
    ops = np.frombuffer(mc.records(log).tobytes(), dtype=U64)          # 56 bytes an op: seven words
    with fp.device_arena(ctx, [In("ops", ops, item=7), Out("cols", want, item=n)], order) as ar:
        trace = p.MemoryTrace(ctx=ctx, device_ptr=ar.ptr("ops"), num_ops=len(log))
        assert trace.rows == n
        ar.check_untouched()                                           # the log is read, nothing is written before the first fill ...
        trace.fill(ar.ptr("cols"))
        ar.check()
        trace.fill(ar.ptr("cols"))                                     # ... and the second fill runs over its own output
        ar.check()
        trace.close()


# ------------------------------------------------------------------------------- host output buffers
# Every output is a guarded numpy array of exactly the documented length (cap_bytes / cap_words equal to it); the library's copy-out
# must fill it and stop there.
def bitrev(lg):
    return np.array([int(format(i, "0%db" % lg)[::-1], 2) if lg else 0 for i in range(1 << lg)])


@pytest.fixture(scope="module")
def phases(gpu, orc, matmul2):
    """the phase API driven over the m = 2 proof by the model challenger: every value it saw is pinned by the oracle's proof bytes"""
    from transcript import drive_phase_api, poseidon_challenger
    p, ctx = gpu
    r = drive_phase_api(p, ctx, orc, matmul2.cd, poseidon_challenger(orc), matmul2.wires, matmul2.pis)
    assert r.bytes == matmul2.bytes
    return r


def test_host_buffers_of_a_batch(gpu, orc, matmul2, phases):
    p, ctx = gpu
    lib, check = lib_of(p)
    c, b = matmul2, phases.wires_b
    d = c.hc.desc
    n, lgN = c.hc.n, d.degree_bits + d.rate_bits
    ob = orc.batch(c.wires, d.rate_bits, d.cap_height, from_values=True, threads=4)
    leaves = ob.leaves()
    with fp.host_out(expected=ob.cap, item=4) as out:
        check(lib.gl_batch_cap(b.handle, out.ptr("out")))
        out.check()
    assert leaves.shape == (1 << lgN, 135)
    for i in (0, (5 << lgN) // 7, (1 << lgN) - 1):
        with fp.host_out(expected=leaves[i]) as out:
            check(lib.gl_batch_get_leaf(b.handle, i, out.ptr("out")))
            out.check()
        with fp.host_out(expected=leaves[bitrev(lgN)[i]]) as out:
            check(lib.gl_batch_get_lde_values(b.handle, i, 1, out.ptr("out")))
            out.check()
        path = ob.prove(i)
        assert path.shape == (lgN - d.cap_height, 4)
        with fp.host_out(expected=path, item=4) as out:
            k = ctypes.c_uint32()
            check(lib.gl_batch_prove(b.handle, i, out.ptr("out"), ctypes.byref(k)))
            assert k.value == path.shape[0]
            out.check()
    with fp.host_out(expected=ob.polynomials, item=n) as out:
        check(lib.gl_batch_coeffs(b.handle, out.ptr("out")))
        out.check()
    for name, first, count in (("pp", 2, 18), ("zs", 0, 2)):
        want = np.asarray(phases.openings[name], dtype=U64)
        assert want.shape == (count, 2)
        with fp.host_out(expected=want, item=2) as out:
            check(lib.gl_open_at(ctx.handle, phases.zs_b.handle, np.array(phases.zeta, dtype=U64).ctypes.data_as(ctypes.c_void_p), first, count, out.ptr("out")))
            out.check()


def test_host_buffer_of_a_salted_leaf(gpu, orc):
    from zk_circuits import model_salt
    p, ctx = gpu
    lib, check = lib_of(p)
    ncols, lg = 5, 5
    vals = rand_field(31, (ncols, 1 << lg))
    b = p.PolynomialBatch.from_values_blinded(vals, 3, 4, seed=SEED, ctx=ctx)
    leaves = np.concatenate([orc.batch(vals, 3, 4, from_values=True, threads=4).leaves(), model_salt(SEED, 0, lg + 3)], axis=1)
    assert leaves.shape == (8 << lg, ncols + 4)
    assert (b.cap == orc.merkle(leaves, 4).cap).all()
    for i in (0, 5, (8 << lg) - 1):
        with fp.host_out(expected=leaves[i]) as out:
            check(lib.gl_batch_get_leaf(b.handle, i, out.ptr("out")))
            out.check()
        with fp.host_out(expected=leaves[bitrev(lg + 3)[i], :ncols]) as out:      # the polynomials' values carry no salt
            check(lib.gl_batch_get_lde_values(b.handle, i, 1, out.ptr("out")))
            out.check()
    b.free()


def test_host_buffers_of_a_merkle_tree(gpu, orc):
    p, ctx = gpu
    lib, check = lib_of(p)
    leaves = rand_field(41, (64, 7))
    for cap_height in (0, 2):
        t, ot = p.MerkleTree(leaves, cap_height, ctx=ctx), orc.merkle(leaves, cap_height)
        with fp.host_out(expected=ot.cap, item=4) as out:
            check(lib.gl_merkle_cap(t.handle, out.ptr("out")))
            out.check()
        for i in (0, 37, 63):
            path = ot.prove(i)
            assert path.shape == (6 - cap_height, 4)
            with fp.host_out(expected=path, item=4) as out:
                k = ctypes.c_uint32()
                check(lib.gl_merkle_prove(t.handle, i, out.ptr("out"), ctypes.byref(k)))
                assert k.value == path.shape[0]
                out.check()
        t.close()


def test_host_buffers_of_the_fri_phase(gpu, phases):
    p, ctx = gpu
    lib, check = lib_of(p)
    want = np.asarray(phases.final_poly, dtype=U64)
    with fp.host_out(expected=want, item=2) as out:
        k = ctypes.c_size_t()
        check(lib.gl_fri_final_poly(phases.fri.handle, out.ptr("out"), want.size, ctypes.byref(k)))
        assert k.value == want.size
        out.check()
    xi = np.array(phases.x_index, dtype=np.uint32)
    with fp.host_out(expected=phases.query_blob) as out:
        k = ctypes.c_size_t()
        check(lib.gl_fri_query(phases.fri.handle, xi.ctypes.data_as(ctypes.c_void_p), xi.size, out.ptr("out"), len(phases.query_blob), ctypes.byref(k)))
        assert k.value == len(phases.query_blob)
        out.check()


def test_host_buffers_of_a_proof(gpu, matmul2):
    p, ctx = gpu
    lib, check = lib_of(p)
    c = matmul2
    proof = c.cd.prove(c.wires, c.pis)
    assert lib.gl_proof_num_bytes(proof.handle) == len(c.bytes)
    with fp.host_out(expected=c.bytes) as out:
        check(lib.gl_proof_bytes(proof.handle, out.ptr("out"), len(c.bytes)))
        out.check()
    with fp.host_out(expected=c.op.caps(), item=4) as out:
        check(lib.gl_proof_caps(proof.handle, out.ptr("out")))
        out.check()


def test_host_buffer_of_prove_openings(gpu, orc, matmul2, phases):
    # gl_prove_openings on the circuit's own instance writes the FRI section of the oracle's proof (tests/test_fri_openings.py)
    from proof_parser import ParsedProof, hash_bytes, opening_columns
    from test_fri_openings import plonk_instance
    from transcript import LibraryChallenger, replay_to_openings
    p, ctx = gpu
    lib, check = lib_of(p)
    c, r = matmul2, phases
    d = c.cd.desc
    pp = ParsedProof(d, c.bytes)
    fri_at = (3 << d.cap_height) * hash_bytes(d) + 16 * sum(k for _, k in opening_columns(d))
    want = c.bytes[fri_at:len(c.bytes) - 8 * (1 + len(pp.public_inputs))]
    ch = LibraryChallenger(p, "poseidon")
    assert list(replay_to_openings(d, ch, c.cd.circuit_digest, r.pi_hash, pp)[-1]) == list(r.zeta)
    inst, params = plonk_instance(p, d, r.zeta, r.gzeta), p.FriParams.of_circuit(d)
    arr = (ctypes.c_void_p * 4)(*[b.handle for b in r.batches])
    k = ctypes.c_size_t()
    check(lib.gl_prove_openings(ctx.handle, ctypes.byref(params), ctypes.byref(inst), arr, ch.ch.handle, None, 0, ctypes.byref(k)))
    assert k.value == len(want)
    with fp.host_out(expected=want) as out:
        check(lib.gl_prove_openings(ctx.handle, ctypes.byref(params), ctypes.byref(inst), arr, ch.ch.handle, out.ptr("out"), len(want), ctypes.byref(k)))
        out.check()


def test_host_buffer_of_stark_prove(gpu):
    import os
    p, ctx = gpu
    lib, check = lib_of(p)
    desc, generate = p.fibonacci_stark(32)
    trace = generate(0, 1)
    stark = p.Stark(desc, p.StarkConfig.standard_fast_config(), 5, ctx=ctx)
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "stark_fibonacci_n32.bin"), "rb") as f:
        want = f.read()                                               # kept current by tests/test_stark.py
    assert stark.proof_size == len(want)
    cols = [np.ascontiguousarray(col) for col in trace]
    ptrs = (ctypes.c_void_p * 4)(*[col.ctypes.data for col in cols])
    pis = np.array([0, 1, int(trace[1, 31])], dtype=U64)
    with fp.host_out(expected=want) as out:
        k = ctypes.c_size_t()
        check(lib.gl_stark_prove(ctx.handle, stark.handle, ptrs, pis.ctypes.data_as(ctypes.c_void_p), out.ptr("out"), len(want), ctypes.byref(k)))
        assert k.value == len(want)
        out.check()

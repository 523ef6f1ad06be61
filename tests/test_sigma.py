"""The sigma polynomials of build() on the device (csrc/sigma.hip: k_sigma_keys, a 64-bit radix sort, k_sigma_heads, a max-scan,
k_sigma_values), every one of the 80 n words against the Python-integer restatement of the reference's forest construction
(tests/sigma_model.py, itself pinned by tests/test_sigma_model.py against the oracle, the host's closed form and the ext-gate builder).

The circuits a proof is made for have partitions of mostly singletons and a few classes of some hundred wires.  The header promises any u64
id, equal ids = wires constrained equal.  Here the partitions are crafted (tests/sigma_cases.py; a CPU guard in test_sigma_model.py asserts
what each has): a class that is all of the circuit, classes whose members lie 80 apart in the sort's input, ids that differ in exactly one
bit for each of the 64 bits, runs that start at sorted position 0 and end at the last one, a class across a 256-thread block, at sizes on
either side of a block, of the sort's single-block path and of the power table's second level.  A sigma that is wrong but still a
permutation gives proofs the library's own verifier accepts, for another circuit: only a by-value comparison sees it."""
import functools

import numpy as np
import pytest

import prover_phase_model as pm
import sigma_cases as sc
import sigma_model as sm
from oracle_lib import m1_desc
from test_prover_phases import describe_zs, draw, first_differences, perm_challenges, rng_of
from test_quotient_model import EDGES, edge_targets
from test_sigma_model import MATMULS, ORACLE_KINDS, k_is_of, oracle_circuit

pytestmark = pytest.mark.gpu
P = pm.P
U64 = np.uint64
POWERS_OF_THREE = [pow(3, j + 1, P) for j in range(80)]
# degree_bits 1 with cap_height 4 is admitted: the LDE has 16 leaves, the cap is the 16 leaf hashes


@functools.lru_cache(maxsize=None)
def crafted(name, lg_n, powers_of_three=False):
    """(classes, the model's sigma values) of a crafted partition, computed once"""
    classes = sc.partition(name, lg_n)
    k_is = POWERS_OF_THREE if powers_of_three else [pow(7, j, P) for j in range(80)]
    want = np.array(sm.sigma_values(classes, k_is, lg_n), dtype=U64)
    classes.setflags(write=False)
    want.setflags(write=False)
    return classes, want


def description(orc, lg_n, k_is=None, hasher=0):
    d = m1_desc(orc, lg_n)
    assert k_is_of(d) == [pow(7, j, P) for j in range(80)]
    for j in range(80 if k_is is not None else 0):
        d.k_is[j] = k_is[j]
    d.hasher = hasher
    return d


def device_sigma(gpu, orc, d, constants, classes):
    """from_classes -> the sigma VALUES [80][n] of the committed constants || sigmas batch; the constant columns must come back unchanged"""
    p, ctx = gpu
    cd = p.GenericCircuitData.from_classes(d, constants, classes, ctx=ctx)
    values = orc.fft(cd.constants_sigmas_batch.polynomials)
    cd.close()
    assert values.shape == (d.num_constants + 80, 1 << d.degree_bits)
    assert (values[:d.num_constants] == constants).all(), "the constant columns changed"
    return values[d.num_constants:]


def sigma_differences(got, want, classes, lg_n, pairs=()):
    """the failure message: the first differing wires as (row, column), the size of the wire's class and its position inside it"""
    part = sm.wire_partition(classes, lg_n)
    cls = np.asarray(classes)

    def describe(col, row):
        members = part[int(cls[col][row])]
        return "wire (row %d, column %d), member %d of a class of %d with id %#x" % (row, col, members.index((row, col)), len(members), int(cls[col][row]))

    text = first_differences(got, want, describe)
    if pairs:
        wrong = {int(v) for v in cls[np.asarray(got) != np.asarray(want)]}
        text += "; one-bit pairs with a wrong wire: bits %s" % [b for b, pair in enumerate(pairs) if wrong & set(pair)]
    return text


# ------------------------------------------------------------------------------- crafted partitions
@pytest.mark.parametrize("name", sc.NAMES)
@pytest.mark.parametrize("lg_n", sc.SIZES)
def test_sigma_of_a_crafted_partition(gpu, orc, lg_n, name):
    classes, want = crafted(name, lg_n)
    d = description(orc, lg_n)
    constants = edge_targets(rng_of(7000 + lg_n), d.num_constants, 1 << lg_n)
    got = device_sigma(gpu, orc, d, constants, classes)
    pairs = sc.one_bit_pairs(lg_n)[1] if name == "one-bit id pairs" else ()
    assert (got == want).all(), "%s (%s): %s" % (name, sc.WHY[name], sigma_differences(got, want, classes, lg_n, pairs))
    if name == "singletons, ids descending":                        # sigma is the identity k_c w^r
        xs = sm.subgroup(lg_n)
        assert (got == np.array([[k * x % P for x in xs] for k in k_is_of(d)], dtype=U64)).all()


@pytest.mark.parametrize("lg_n", sc.SIZES)
def test_sigma_with_coset_shifts_that_are_not_powers_of_seven(gpu, orc, lg_n):
    # a kernel that regenerated 7^j instead of reading k_is would pass everything else
    classes, want = crafted("random", lg_n, powers_of_three=True)
    d = description(orc, lg_n, k_is=POWERS_OF_THREE)
    constants = edge_targets(rng_of(7050 + lg_n), d.num_constants, 1 << lg_n)
    got = device_sigma(gpu, orc, d, constants, classes)
    assert (got == want).all(), sigma_differences(got, want, classes, lg_n)
    assert (crafted("random", lg_n)[1] != want).any()               # and the shifts matter to the result


# ------------------------------------------------------------------------------- real partitions
@pytest.mark.parametrize("ids", ["decoded", "high word"])
@pytest.mark.parametrize("key", MATMULS + list(ORACLE_KINDS), ids=lambda k: "matmul m = %d" % k if isinstance(k, int) else "kind %d (%d)" % k)
def test_sigma_of_an_oracle_circuit_partition(gpu, orc, key, ids):
    # the oracle's own description and constants (lookup selectors among them); the partition decoded from its sigma columns, with ids
    # q = row * 80 + column < 2^32 as decoded, or rotated by 32 bits so that they differ in the high word only
    oc = oracle_circuit(orc, key)
    d = oc.product_desc()
    cs = oc.constants_sigmas()
    want = cs[d.num_constants:]
    classes = np.array(sm.classes_from_sigma(want, k_is_of(d), d.degree_bits), dtype=U64)
    assert int(classes.max()) < 2**32
    if ids == "high word":
        classes = sc.high_word_relabel(classes)
        assert (classes & U64(0xFFFFFFFF) == 0).all()
    got = device_sigma(gpu, orc, d, np.ascontiguousarray(cs[:d.num_constants]), classes)
    assert (got == want).all(), sigma_differences(got, want, classes, d.degree_bits)


# ------------------------------------------------------------------------------- the two entry points
@pytest.mark.parametrize("hasher,name", [(0, "random"), (1, "one-bit id pairs")], ids=["Poseidon", "Keccak"])
def test_sigma_columns_and_classes_build_the_same_circuit(gpu, orc, hasher, name):
    p, ctx = gpu
    lg_n = 5
    classes, want = crafted(name, lg_n)
    d = description(orc, lg_n, hasher=hasher)
    constants = edge_targets(rng_of(7060 + hasher), d.num_constants, 1 << lg_n)
    from_columns = p.GenericCircuitData(d, np.vstack([constants, want]), ctx)
    from_classes = p.GenericCircuitData.from_classes(d, constants, classes, ctx=ctx)
    singletons = p.GenericCircuitData.from_classes(d, constants, crafted("singletons, ids descending", lg_n)[0], ctx=ctx)
    assert from_columns.desc.hasher == from_classes.desc.hasher == hasher
    assert (from_columns.constants_sigmas_cap == from_classes.constants_sigmas_cap).all()
    assert (from_columns.circuit_digest == from_classes.circuit_digest).all()
    assert (singletons.circuit_digest != from_classes.circuit_digest).any() and (singletons.constants_sigmas_cap != from_classes.constants_sigmas_cap).any()
    for cd in (from_columns, from_classes, singletons):
        cd.close()


# ------------------------------------------------------------------------------- sigma and the permutation kernels together
PERM_LG_N = 5


def class_constant_wires(classes, seed):
    """[135][n]: one seeded value per class on the 80 routed columns (a quarter of the classes take theirs from EDGES), the 55 others random"""
    rng = rng_of(seed)
    ids, inverse = np.unique(classes, return_inverse=True)
    values = np.array(draw(rng, len(ids)), dtype=U64)
    edge = rng.integers(0, 4, size=len(ids)) == 0
    values[edge] = np.array(EDGES, dtype=U64)[rng.integers(0, len(EDGES), size=int(edge.sum()))]
    n = classes.shape[1]
    wires = np.empty((135, n), dtype=U64)
    wires[:80] = values[inverse.reshape(classes.shape)]
    wires[80:] = np.array(draw(rng, 55 * n), dtype=U64).reshape(55, n)
    return wires


def closing_product(wires, sigmas, k_is, beta, gamma, lg_n):
    """Z after the last row: the product over all 80 n cells of (w + beta k_j x + gamma) / (w + beta sigma_j + gamma), in any order"""
    num = den = 1
    for j in range(80):
        for w, s, x in zip(wires[j].tolist(), sigmas[j].tolist(), sm.subgroup(lg_n)):
            num = num * ((w + beta * (k_is[j] * x % P) + gamma) % P) % P
            den = den * ((w + beta * s + gamma) % P) % P
    assert den
    return num * pow(den, P - 2, P) % P


@pytest.mark.parametrize("challenges", ["random", "edges"])
def test_partial_products_over_the_device_sigma_close_exactly_when_the_wires_respect_the_classes(gpu, orc, challenges):
    # from_classes keeps the sigma values for gl_partial_products: Z and the partial products over them equal the model over the model's
    # sigma, and the model's running product closes (Z after the last row = 1) because the wires are constant on every class.  With one
    # wire of a class of eight changed the kernels still equal the model, and the model's product no longer closes.
    # The committed seeds raise no UndefinedResult (pm.partial_products checks every factor on the CPU): no cell is omitted or repaired.
    p, ctx = gpu
    lg_n = PERM_LG_N
    classes, sigma = crafted("random", lg_n)
    d = description(orc, lg_n)
    k_is = k_is_of(d)
    ch = perm_challenges(challenges, 7500)
    cd = p.GenericCircuitData.from_classes(d, edge_targets(rng_of(7070), d.num_constants, 1 << lg_n), classes, ctx=ctx)
    wires = class_constant_wires(classes, 7600)
    assert len(set(EDGES) & set(wires[:80].reshape(-1).tolist())) == len(EDGES)
    part = sm.wire_partition(classes, lg_n)
    row, col = next(s for s in part.values() if len(s) == 8)[3]
    broken = wires.copy()
    broken[col, row] = (int(wires[col, row]) + 1) % P
    for w, closes in ((wires, True), (broken, False)):
        d_w = ctx.alloc(w.nbytes).upload(w)
        got = orc.fft(cd.partial_products(d_w.ptr, ch["betas"], ch["gammas"]).polynomials)
        d_w.free()
        want = np.array(pm.partial_products(w, sigma, k_is, ch["betas"], ch["gammas"], lg_n), dtype=U64)      # raises on a zero factor
        assert got.shape == want.shape == (20, 1 << lg_n)
        assert (got == want).all(), "challenges %r, wires %s: %s" % (challenges, "constant on every class" if closes else "with one wire changed",
                                                                      first_differences(got, want, describe_zs))
        for a in range(2):
            assert (closing_product(w, sigma, k_is, ch["betas"][a], ch["gammas"][a], lg_n) == 1) == closes, (a, closes)
    cd.close()

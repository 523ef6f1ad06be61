"""Wave priority of the small, latency-bound launches (csrc/context.hpp gl_launch_prio, knob GL_URGENT_MAX_WAVES).

A priority cannot change a value; these tests exist to run every guarded kernel with its `s_setprio` branch taken and not taken.
The knob is read once per process, so every setting runs in a fresh child (this file run as a script), all children at once.
GL_URGENT_MAX_WAVES: 0 = nothing urgent, unset = the default, 2^30 = every guarded kernel raised at every size.  Each of them
runs twice: with GL_COOP_MAX_NODES unset (a lone process: the 16-lane cooperative leaf and level kernels up to 8192 nodes, so
of the guarded tree kernels only k_merkle_top_coop runs) and with 1024, the value with many proofs in flight (one lane per hash:
k_merkle_level on the 2048 nodes above 2^12 leaves).  The m = 8 proof runs the guarded launches of the FRI and permutation
chains and the NTT passes.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WAVES = ("0", None, "1073741824")
COOP = (None, "1024")
SETTINGS = [(w, c) for w in WAVES for c in COOP]
# (log2 leaves, leaf length, cap height): 2^4 has no level launch, 2^5 the top kernel only, 2^11 and 2^12 leaf / level kernels plus
# the top; 3 is the no-hash path, 8 one permutation, 9 two, 135 the wires' 17.  The last tree has cap height 0: one level launch
# of 128 nodes below the top kernel's 64.
TREES = [(lg, ll, 4) for lg in (4, 5, 11, 12) for ll in (3, 8, 9, 135)] + [(8, 9, 0)]
M = 8


def _leaves(k, lg, ll):
    from oracle_lib import rand_field
    return rand_field(1000 + k, (1 << lg, ll))


def _proof_inputs():
    from oracle_lib import rand_field
    return rand_field(3, M * M) % (2**32 - 1), rand_field(4, M * M) % (2**32 - 1)


def _child(out_path):
    sys.path.insert(0, ROOT)
    import plonky2_demo_amd as p
    ctx = p.default_context()
    out = {}
    for k, (lg, ll, cap) in enumerate(TREES):
        t = p.MerkleTree(_leaves(k, lg, ll), cap, ctx=ctx)
        out["cap%d" % k] = t.cap
        # the siblings of every leaf's path: every digest of every level below the cap
        out["sib%d" % k] = np.stack([t.prove(i) for i in range(1 << lg)])
    a, b = _proof_inputs()
    hc = p.MatmulCircuit(M)
    cd = hc.build(ctx)
    buf = ctx.alloc(135 * hc.n * 8)
    gen = hc.witness_generator(ctx)
    pis = gen.run(a, b, buf.ptr, filler_seed=5)
    proof = cd.prove_device(buf.ptr, pis, gen.public_inputs_hash).to_bytes()
    ok, why = cd.verify(proof)
    out["proof"] = np.frombuffer(proof, dtype=np.uint8)
    out["verified"] = np.array([1 if ok else 0])
    np.savez(out_path, **out)


@pytest.fixture(scope="module")
def reference():
    """level l of tree k on the host: hash_or_noop of the leaves, two_to_one up to the cap"""
    import plonky2_demo_amd as p
    ref = []
    for k, (lg, ll, cap) in enumerate(TREES):
        levels = [p.hash_or_noop_host(_leaves(k, lg, ll))]
        while levels[-1].shape[0] > (1 << cap):
            levels.append(p.two_to_one_host(levels[-1][0::2], levels[-1][1::2]))
        ref.append(levels)
    return ref


@pytest.fixture(scope="module")
def children(gpu):
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for n, (waves, coop) in enumerate(SETTINGS):
            env = dict(os.environ)
            for name, v in (("GL_URGENT_MAX_WAVES", waves), ("GL_COOP_MAX_NODES", coop)):
                env.pop(name, None)
                if v is not None:
                    env[name] = v
            path = os.path.join(d, "s%d.npz" % n)
            procs.append((path, subprocess.Popen([sys.executable, os.path.abspath(__file__), path], env=env, stdout=subprocess.PIPE,
                                                 stderr=subprocess.STDOUT, text=True)))
        res = []
        for path, pr in procs:
            log, _ = pr.communicate(timeout=300)
            assert pr.returncode == 0, log
            with np.load(path) as z:
                res.append({name: z[name] for name in z.files})
        return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(len(SETTINGS)), ids=["waves=%s,coop=%s" % s for s in SETTINGS])
def test_trees_match_the_host_hashes_word_for_word(children, reference, n):
    got = children[n]
    for k, (lg, ll, cap) in enumerate(TREES):
        levels = reference[k]
        assert got["cap%d" % k].shape == levels[-1].shape and (got["cap%d" % k] == levels[-1]).all(), ("cap", lg, ll, cap)
        sib = got["sib%d" % k]
        assert sib.shape == (1 << lg, lg - cap, 4)
        i = np.arange(1 << lg)
        for l in range(lg - cap):
            assert (sib[:, l] == levels[l][(i >> l) ^ 1]).all(), ("level", l, lg, ll, cap)


@pytest.mark.gpu
def test_proof_bytes_do_not_depend_on_the_setting(children):
    for got in children:
        assert got["verified"][0] == 1
        assert got["proof"].shape == children[0]["proof"].shape and (got["proof"] == children[0]["proof"]).all()


if __name__ == "__main__":
    _child(sys.argv[1])

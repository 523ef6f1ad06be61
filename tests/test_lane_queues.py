"""A context's own hardware queue (csrc/context.hip "lane queues", knob GL_LANE_QUEUES).

Which queue a stream runs on cannot change a value: these tests run proofs and trees on own-queue streams, on the pool's streams
and on both side by side, and check the bookkeeping (the budget, its release, the caller's stream, an environment that already
grants 16 pool queues).  The knob is read once per process, so every setting runs in a fresh child (this file run as a script),
all children at once.

proofs children (GL_LANE_QUEUES = 0, unset, 1): three contexts prove the m = 8 circuit at the same time from three threads; with the
budget at 1 two of them run on fall-back streams beside the one own-queue stream.  Each child also builds two trees on its first
context: 2^6 leaves of 9 columns (the cooperative leaf kernel, then the fused top) and 2^10 leaves of 135 (lane-per-hash leaves,
k_merkle_level on the 512 nodes above them, the cooperative level, the fused top); GL_COOP_MAX_NODES = 256 puts the thresholds there.
"""
import os
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROOF_SETTINGS = ("0", None, "1")
TREES = [(6, 9, 2), (10, 135, 2)]      # (log2 leaves, leaf length, cap height)
M = 8
LANES = 3
CAP = 4                                 # the lifecycle child's budget
ROUNDS, PER_ROUND = 8, 5                # 40 contexts, five live at a time


def _leaves(k, lg, ll):
    from oracle_lib import rand_field
    return rand_field(2000 + k, (1 << lg, ll))


def _child_proofs(out_path):
    import threading
    import plonky2_demo_amd as p
    from oracle_lib import rand_field
    a, b = rand_field(3, M * M) % (2**32 - 1), rand_field(4, M * M) % (2**32 - 1)
    ctxs = [p.Context(0) for _ in range(LANES)]
    out = {"own": np.array([int(c.has_own_queue) for c in ctxs]), "live": np.array([p._lib.lib.gl_lane_queues_live(0)])}
    hc = p.MatmulCircuit(M)
    lanes = []
    for c in ctxs:                       # set-up one lane after the other, the proofs together
        cd = hc.build(c)
        buf = c.alloc(135 * hc.n * 8)
        gen = hc.witness_generator(c)
        lanes.append((cd, buf, gen, gen.run(a, b, buf.ptr, filler_seed=5)))
    res, go = [None] * LANES, threading.Barrier(LANES)

    def prove(i):
        cd, buf, gen, pis = lanes[i]
        go.wait()
        res[i] = [cd.prove_device(buf.ptr, pis, gen.public_inputs_hash).to_bytes() for _ in range(2)]

    ts = [threading.Thread(target=prove, args=(i,)) for i in range(LANES)]
    for t in ts:
        t.start()
    for t in ts:
        t.join()
    assert all(r is not None for r in res), "a proving thread failed"
    out["proofs"] = np.stack([np.frombuffer(x, dtype=np.uint8) for r in res for x in r])
    out["verified"] = np.array([1 if lanes[i][0].verify(x)[0] else 0 for i, r in enumerate(res) for x in r])
    for k, (lg, ll, cap) in enumerate(TREES):
        t = p.MerkleTree(_leaves(k, lg, ll), cap, ctx=ctxs[0])
        out["cap%d" % k] = t.cap
        out["sib%d" % k] = np.stack([t.prove(i) for i in range(1 << lg)])
    np.savez(out_path, **out)


def _child_lifecycle(out_path):
    import torch
    import plonky2_demo_amd as p
    live = lambda: p._lib.lib.gl_lane_queues_live(0)
    own, lives, after = [], [], []
    for _ in range(ROUNDS):
        ctxs = []
        for _ in range(PER_ROUND):
            ctxs.append(p.Context(0))
            own.append(int(ctxs[-1].has_own_queue))
            lives.append(live())
        for c in ctxs:
            c.close()
        after.append(live())
    ts = torch.cuda.Stream()
    before = live()
    c = p.Context(0, stream=ts.cuda_stream)
    caller = [int(c.has_own_queue), before, live()]
    x = p.fft(np.arange(1 << 10, dtype=np.uint64).reshape(1, -1), ctx=c)      # the context works
    caller.append(int((p.ifft(x, ctx=c)[0] == np.arange(1 << 10, dtype=np.uint64)).all()))
    c.close()
    caller.append(live())
    np.savez(out_path, own=np.array(own), lives=np.array(lives), after=np.array(after), caller=np.array(caller))


def _child_pool16(out_path):
    import plonky2_demo_amd as p
    ctxs = [p.Context(0) for _ in range(3)]
    np.savez(out_path, own=np.array([int(c.has_own_queue) for c in ctxs]), live=np.array([p._lib.lib.gl_lane_queues_live(0)]))


# (the suite's own environment may grant 16 or more pool queues, under which no own queues are made: the children that expect own
# queues run with the runtime's default of 4)
CHILDREN = [("proofs", {"GL_LANE_QUEUES": v, "GL_COOP_MAX_NODES": "256", "GPU_MAX_HW_QUEUES": "4"}) for v in PROOF_SETTINGS] + [
    ("lifecycle", {"GL_LANE_QUEUES": str(CAP), "GPU_MAX_HW_QUEUES": "4"}), ("pool16", {"GL_LANE_QUEUES": None, "GPU_MAX_HW_QUEUES": "16"})]


@pytest.fixture(scope="module")
def children(gpu):
    with tempfile.TemporaryDirectory() as d:
        procs = []
        for n, (mode, knobs) in enumerate(CHILDREN):
            env = dict(os.environ)
            for name, v in knobs.items():
                env.pop(name, None)
                if v is not None:
                    env[name] = v
            path = os.path.join(d, "c%d.npz" % n)
            procs.append((path, subprocess.Popen([sys.executable, os.path.abspath(__file__), mode, path], env=env, stdout=subprocess.PIPE,
                                                 stderr=subprocess.STDOUT, text=True)))
        res = []
        for path, pr in procs:
            log, _ = pr.communicate(timeout=300)
            assert pr.returncode == 0, log
            with np.load(path) as z:
                res.append({name: z[name] for name in z.files})
        return res


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


@pytest.mark.gpu
def test_contexts_get_own_queues_up_to_the_budget(children):
    off, default, one = children[:3]
    assert list(off["own"]) == [0, 0, 0] and off["live"][0] == 0
    assert list(default["own"]) == [1, 1, 1] and default["live"][0] == LANES
    assert list(one["own"]) == [1, 0, 0] and one["live"][0] == 1


@pytest.mark.gpu
def test_proof_bytes_do_not_depend_on_the_queues(children):
    want = children[0]["proofs"]
    assert want.shape[0] == 2 * LANES and (want == want[0]).all()      # same circuit, same witness, deterministic prover
    for got in children[:3]:
        assert (got["verified"] == 1).all()
        assert got["proofs"].shape == want.shape and (got["proofs"] == want).all()


@pytest.mark.gpu
@pytest.mark.parametrize("n", range(3), ids=["lane_queues=%s" % v for v in PROOF_SETTINGS])
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
def test_forty_contexts_stay_within_the_budget_and_give_it_back(children):
    got = children[3]
    own, lives = got["own"].reshape(ROUNDS, PER_ROUND), got["lives"].reshape(ROUNDS, PER_ROUND)
    assert lives.max() <= CAP
    assert (own == [1] * CAP + [0] * (PER_ROUND - CAP)).all()            # the first four live at a time, never the fifth
    assert (lives == [min(i + 1, CAP) for i in range(PER_ROUND)]).all()
    assert (got["after"] == 0).all()                                     # back to 0 after every round, the last one included


@pytest.mark.gpu
def test_a_callers_stream_has_no_own_queue_and_leaves_the_count_alone(children):
    own, before, during, works, after = children[3]["caller"]
    assert own == 0 and before == 0 and during == 0 and after == 0 and works == 1


@pytest.mark.gpu
def test_sixteen_pool_queues_mean_no_own_queues(children):
    got = children[4]
    assert list(got["own"]) == [0, 0, 0] and got["live"][0] == 0


if __name__ == "__main__":
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    {"proofs": _child_proofs, "lifecycle": _child_lifecycle, "pool16": _child_pool16}[sys.argv[1]](sys.argv[2])

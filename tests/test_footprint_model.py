"""CPU tests of the guarded arena of tests/footprint.py over plain numpy memory: fake "entries" that each make one footprint error
must be reported at the right region and offset, and a correct fake entry must pass in both region orders.  This is where the
arena's ability to fail is shown; the GPU tests only ever run the library's own kernels."""
import ctypes

import numpy as np
import pytest

import footprint as fp

U64 = np.uint64
ITEM = 1000          # one "polynomial" of the fake entry: above 512 words, so the guards are one item (1024 after rounding)
BATCH = 3


def regions(expected_last=None):
    """a fake out-of-place transform: src [BATCH][ITEM] -> dst [BATCH][ITEM] = src + 1, with a small table read beside it"""
    src = (np.arange(BATCH * ITEM, dtype=U64) * U64(7) + U64(3)).reshape(BATCH, ITEM)
    want = src + U64(1)
    if expected_last is not None:
        want[-1, -1] = expected_last
    return [fp.Region("src", "in", data=src, item=ITEM), fp.Region("table", "in", data=np.arange(5, dtype=U64)),
            fp.Region("dst", "out", expected=want, item=ITEM)], src, want


def words_of(arena):
    return arena.memory.array


def correct_entry(arena, src):
    r = arena.by_name["dst"]
    words_of(arena)[r.start:r.start + r.words] = src.reshape(-1) + U64(1)


def run(order, fault=None, expected_last=None):
    rs, src, want = regions(expected_last)
    with fp.host_arena(rs, order) as arena:
        correct_entry(arena, src)
        if fault is not None:
            fault(arena, words_of(arena))
        return arena.violations(), arena


@pytest.mark.parametrize("order", fp.ORDERS)
def test_layout(order):
    rs, src, want = regions()
    with fp.host_arena(rs, order) as arena:
        names = [r.name for r in arena.regions]
        assert names == (["dst", "src", "table"] if order == "outputs-first" else ["src", "table", "dst"])
        assert arena.base == words_of(arena).ctypes.data
        for r in arena.regions:
            assert r.start % 32 == 0 and arena.ptr(r.name) == arena.base + 8 * r.start and arena.ptr(r.name, 3) == arena.ptr(r.name) + 24
        sizes = {(g[2].name if g[2] else None, g[3].name if g[3] else None): g[1] for g in arena.guards}
        assert all(w % 32 == 0 and w >= 512 for w in sizes.values())
        if order == "outputs-first":
            assert sizes == {(None, "dst"): 1024, ("dst", "src"): 1024, ("src", "table"): 1024, ("table", None): 512}
        else:
            assert sizes == {(None, "src"): 1024, ("src", "table"): 1024, ("table", "dst"): 1024, ("dst", None): 1024}
        # the fill: every word of the upload that is no input is the pattern of its position, and the inputs are in place
        mem = words_of(arena)
        fill = fp.pattern(0, arena.words)
        assert (fill >= U64(0xFFFFFFFF00000001)).all() and len(set(fill.tolist())) == fill.size
        inside = np.zeros(arena.words, dtype=bool)
        for r in arena.regions:
            if r.role == "in":
                inside[r.start:r.start + r.words] = True
        assert (mem[~inside] == fill[~inside]).all()
        assert (mem[arena.by_name["src"].start:][:BATCH * ITEM] == src.reshape(-1)).all()


@pytest.mark.parametrize("order", fp.ORDERS)
def test_a_correct_entry_passes(order):
    bad, arena = run(order)
    assert bad == []
    rs, src, want = regions()
    with fp.host_arena(rs, order) as arena:
        correct_entry(arena, src)
        arena.check()
        assert (arena.region_words("dst") == want.reshape(-1)).all()


@pytest.mark.parametrize("order", fp.ORDERS)
def test_a_word_in_the_guard_just_before_a_region(order):
    def fault(arena, mem):
        mem[arena.by_name["dst"].start - 1] = 0
    bad, arena = run(order, fault)
    assert len(bad) == 1
    v = bad[0]
    assert (v.kind, v.before, v.short, v.count) == ("guard", "dst", 1, 1)
    assert v.after == (None if order == "outputs-first" else "table")
    assert "1 before the start of dst" in str(v)


@pytest.mark.parametrize("order", fp.ORDERS)
def test_a_word_in_the_guard_just_after_a_region(order):
    def fault(arena, mem):
        r = arena.by_name["dst"]
        mem[r.start + r.words] = 5
    bad, arena = run(order, fault)
    assert len(bad) == 1
    v = bad[0]
    assert (v.kind, v.after, v.past, v.offset, v.count, v.got) == ("guard", "dst", 0, 0, 1, 5)
    assert v.before == ("src" if order == "outputs-first" else None)


@pytest.mark.parametrize("order", fp.ORDERS)
def test_a_word_one_whole_item_after_a_region(order):
    # what a tail tile does: the last word of the item that would follow the region's last one
    def fault(arena, mem):
        r = arena.by_name["dst"]
        mem[r.start + r.words + ITEM - 1] = mem[r.start + r.words - 1]
    bad, arena = run(order, fault)
    assert len(bad) == 1
    v = bad[0]
    assert (v.kind, v.after, v.past, v.count) == ("guard", "dst", ITEM - 1, 1)
    assert (v.past + 1) % ITEM == 0


@pytest.mark.parametrize("order", fp.ORDERS)
def test_a_write_into_an_input(order):
    def fault(arena, mem):
        mem[arena.by_name["src"].start + ITEM + 7] += U64(1)
        mem[arena.by_name["src"].start + 2 * ITEM] = 0
    bad, arena = run(order, fault)
    assert len(bad) == 1
    v = bad[0]
    assert (v.kind, v.name, v.offset, v.count) == ("in", "src", ITEM + 7, 2)


@pytest.mark.parametrize("order", fp.ORDERS)
def test_an_unwritten_last_word_where_zero_is_expected(order):
    # memory that happens to hold zero would hide it; the pattern does not
    def fault(arena, mem):
        r = arena.by_name["dst"]
        mem[r.start + r.words - 1] = fp.pattern(r.start + r.words - 1, 1)[0]      # as the upload left it
    bad, arena = run(order, fault, expected_last=0)
    assert len(bad) == 1
    v = bad[0]
    assert (v.kind, v.name, v.offset, v.count, v.want) == ("out", "dst", BATCH * ITEM - 1, 1, 0)
    assert v.got == fp.PATTERN | (arena.by_name["dst"].start + BATCH * ITEM - 1)


@pytest.mark.parametrize("order", fp.ORDERS)
def test_eight_words_of_one_guard_copied_over_another(order):
    def fault(arena, mem):
        a, b = arena.guards[0], arena.guards[-1]
        mem[b[0] + 16:b[0] + 24] = mem[a[0] + 16:a[0] + 24]
    bad, arena = run(order, fault)
    assert len(bad) == 1
    v = bad[0]
    last = arena.regions[-1]
    slack = fp.round_up(last.words, 32) - last.words
    assert (v.kind, v.after, v.before, v.past, v.count) == ("guard", last.name, None, slack + 16, 8)


def test_several_errors_are_all_reported_in_address_order():
    def fault(arena, mem):
        mem[0] = 1
        mem[arena.by_name["table"].start + 4] = 9
        mem[arena.words - 1] = 2
    bad, arena = run("outputs-first", fault)
    assert [(v.kind, v.name if v.kind != "guard" else v.before) for v in bad] == [("guard", "dst"), ("in", "table"), ("guard", None)]
    assert bad[0].offset == 0 and bad[1].offset == 4 and bad[2].after == "table"


def test_an_expected_word_equal_to_the_pattern_is_refused_before_the_call():
    rs, src, want = regions()
    arena = fp.Arena(fp.NumpyMemory, rs)
    at = arena.by_name["dst"].start + 17
    want.reshape(-1)[17] = fp.pattern(at, 1)[0]
    arena.expect("dst", want)
    with pytest.raises(AssertionError, match="word 17 equals the fill pattern"):
        arena.upload()
    # the same value at another position is no collision
    want.reshape(-1)[17], want.reshape(-1)[18] = 0, fp.pattern(at, 1)[0]
    arena.expect("dst", want)
    arena.upload()
    with pytest.raises(AssertionError):
        fp.Region("x", "out", words=4, expected=np.zeros(5, dtype=U64))
    with pytest.raises(AssertionError):
        fp.Region("x", "in", words=4)


@pytest.mark.parametrize("nbytes", [1, 8, 25, 1001])
def test_a_guarded_host_byte_buffer(nbytes):
    # what the library's copy-out entries get: an interior pointer, exactly nbytes long, guards on both sides
    payload = (np.arange(nbytes) % 251 + 1).astype(np.uint8)
    with fp.host_out("blob", nbytes=nbytes) as arena:
        arena.expect("blob", payload)
        ctypes.memmove(arena.ptr("blob"), payload.ctypes.data, nbytes)
        arena.check()
    with fp.host_out("blob", nbytes=nbytes) as arena:
        arena.expect("blob", payload)
        ctypes.memmove(arena.ptr("blob"), np.append(payload, np.uint8(0)).ctypes.data, nbytes + 1)      # one byte too many
        bad = arena.violations()
        assert len(bad) == 1
        v = bad[0]
        if nbytes % 8:
            assert (v.kind, v.name, v.offset) == ("out", "blob", nbytes // 8)      # the last word of the region is part pattern
        else:
            assert (v.kind, v.after, v.past) == ("guard", "blob", 0)
    with fp.host_out("blob", nbytes=nbytes) as arena:
        arena.expect("blob", payload)
        ctypes.memmove(arena.ptr("blob"), payload.ctypes.data, nbytes - 1)                          # one byte short
        bad = arena.violations()
        assert [(v.kind, v.name, v.offset) for v in bad] == [("out", "blob", (nbytes - 1) // 8)]

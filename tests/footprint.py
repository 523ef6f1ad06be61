"""TEST-ONLY helper: a guarded arena for footprint tests (no tests in here).

One allocation holds every caller-visible buffer of one call, each a named region with a role:
  "in"     uploaded, must come back as uploaded;
  "out"    not uploaded, must equal the expected array afterwards;
  "inout"  uploaded, then must equal the expected array.
Layout: guard, region, guard, region, ..., guard.  A guard is max(512 words, one item of the regions beside it) rounded up to a
multiple of 32 words, so every region starts 256-byte aligned and a tail tile one whole item past a region still lands in a guard.
Before the upload word i of the whole arena, guards and regions, is 0xFFFFFFFF80000000 | i: every such word is >= p, so no canonical
output equals it, and it depends on its position, so a block copied from one guard to another is seen too.  An `out` region keeps the
pattern until the call writes it: a word the call leaves out shows up as a mismatch, because no expected word may equal the pattern at
its own position (asserted on the CPU, for raw u64 outputs too).

The arena talks to memory through two methods, write(byte offset, array) and read() -> every word, plus `base`, the address of word 0:
DeviceMemory is a gl_dev_alloc block, NumpyMemory a plain numpy array (the CPU tests of the arena itself, and the guarded host output
buffers the library copies into)."""
import ctypes

import numpy as np

U64 = np.uint64
PATTERN = 0xFFFFFFFF80000000
MIN_GUARD = 512
MAX_WORDS = 1 << 31
ORDERS = ("outputs-first", "inputs-first")


def pattern(first, count):
    """words first .. first + count of the fill pattern"""
    return np.arange(first, first + count, dtype=U64) | U64(PATTERN)


def round_up(x, m):
    return -(-x // m) * m


class NumpyMemory:
    """`words` 64-bit words of host memory"""

    def __init__(self, words):
        self.array = np.zeros(words, dtype=U64)
        self.base = self.array.ctypes.data

    def write(self, offset, arr):
        raw = np.ascontiguousarray(arr).view(np.uint8).reshape(-1)
        self.array.view(np.uint8)[offset:offset + raw.size] = raw

    def read(self):
        return self.array.copy()

    def free(self):
        pass


class DeviceMemory:
    """`words` 64-bit words from gl_dev_alloc on `ctx` (a plonky2_demo_amd Context)"""

    def __init__(self, ctx, words):
        from plonky2_demo_amd._lib import check, lib
        self._check, self._lib, self.ctx, self.words = check, lib, ctx, words
        p = ctypes.c_void_p()
        check(lib.gl_dev_alloc(ctx.handle, words * 8, ctypes.byref(p)))
        self.base = p.value

    def write(self, offset, arr):
        raw = np.ascontiguousarray(arr)
        self._check(self._lib.gl_copy_h2d(self.ctx.handle, self.base + offset, raw.ctypes.data_as(ctypes.c_void_p), raw.nbytes))

    def read(self):
        out = np.empty(self.words, dtype=U64)
        self._check(self._lib.gl_copy_d2h(self.ctx.handle, out.ctypes.data_as(ctypes.c_void_p), self.base, out.nbytes))      # synchronises
        return out

    def free(self):
        if self.base:
            self._check(self._lib.gl_dev_free(self.ctx.handle, self.base))
            self.base = None


def _bytes_of(a):
    """any array (or bytes) -> its bytes as a flat uint8 array; integers without a dtype are 64-bit words"""
    if isinstance(a, (bytes, bytearray)):
        return np.frombuffer(bytes(a), dtype=np.uint8)
    a = np.ascontiguousarray(a) if isinstance(a, np.ndarray) else np.ascontiguousarray(a, dtype=U64)
    return a.reshape(-1).view(np.uint8)


class Region:
    """name, role, and the size in 64-bit words (or `nbytes` for a byte buffer whose length is no multiple of 8: it occupies whole words
    and the bytes past its end belong to it as pattern).  `item` is one polynomial, row, state or column of it, in words.  `data` is
    what an in / inout region is uploaded with, `expected` what an out / inout region must hold afterwards (set it with
    Arena.expect where it is only known later)."""

    def __init__(self, name, role, words=None, item=1, data=None, expected=None, nbytes=None):
        assert role in ("in", "out", "inout"), role
        self.name, self.role, self.item = name, role, int(item)
        self.data = None if data is None else _bytes_of(data)
        self.expected = None if expected is None else _bytes_of(expected)
        if nbytes is None:
            if words is not None:
                nbytes = int(words) * 8
            else:
                nbytes = (self.data if self.data is not None else self.expected).size
        self.nbytes = int(nbytes)
        self.words = -(-self.nbytes // 8)
        assert self.words >= 1 and self.item >= 1
        assert (self.data is not None) == (role != "out"), "%s: in / inout regions are uploaded, out regions are not" % name
        assert role != "in" or self.expected is None
        for a in (self.data, self.expected):
            assert a is None or a.size == self.nbytes, "%s: %d bytes given for a region of %d" % (name, a.size, self.nbytes)
        self.start = None


class Violation:
    """One guard or region that is not what it must be: `kind` "guard" / "in" / "out" / "inout", `name` the region (for a guard the
    regions on its two sides, `after` and `before`, None at the arena's ends), `offset` the first offending word counted from the
    start of the region (guard), `count` how many words are wrong.  For a guard `past` = words past the end of `after` and `short`
    = words before the start of `before`, which say how far from the region the write went and whether that is a multiple of an item."""

    def __init__(self, kind, name, offset, count, got, want, after=None, before=None, past=None, short=None):
        self.kind, self.name, self.offset, self.count, self.got, self.want = kind, name, int(offset), int(count), int(got), int(want)
        self.after, self.before, self.past, self.short = after, before, past, short

    def __str__(self):
        where = "%s region %s" % (self.kind, self.name) if self.kind != "guard" else "guard between %s and %s" % (self.after, self.before)
        s = "%s: %d word(s) wrong, first at offset %d (holds %#018x, must hold %#018x)" % (where, self.count, self.offset, self.got, self.want)
        if self.kind == "guard":
            s += "; %s word(s) past the end of %s, %s before the start of %s" % (self.past, self.after, self.short, self.before)
        return s

    __repr__ = __str__


class Arena:
    """regions: Region objects in the caller's order; `order` puts the out / inout regions before the in regions ("outputs-first") or
    after them ("inputs-first"), keeping the order within each kind, so that an underrun hits a guard in one order and an input in the
    other.  make_memory(words) -> a memory object.  Use as a context manager: the memory is freed on exit."""

    def __init__(self, make_memory, regions, order=ORDERS[0]):
        assert order in ORDERS, order
        regions = list(regions)
        assert len({r.name for r in regions}) == len(regions), "region names are unique"
        outs, ins = [r for r in regions if r.role != "in"], [r for r in regions if r.role == "in"]
        self.regions = outs + ins if order == ORDERS[0] else ins + outs
        self.by_name = {r.name: r for r in self.regions}
        self.guards = []                                             # (start, words, region before it or None, region after it or None)
        at = 0
        for k in range(len(self.regions) + 1):
            before, after = self.regions[k - 1] if k else None, self.regions[k] if k < len(self.regions) else None
            g = round_up(max([MIN_GUARD] + [r.item for r in (before, after) if r is not None]), 32)
            self.guards.append((at, g, before, after))
            at += g
            if after is not None:
                after.start = at
                at += round_up(after.words, 32)                      # the slack up to the next multiple of 32 words is guard as well
        self.words = at
        assert self.words < MAX_WORDS
        self.memory = make_memory(self.words)
        self.base = self.memory.base
        self.uploaded = False

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        if self.memory is not None:
            self.memory.free()
            self.memory = None

    def ptr(self, name, word=0):
        """the address of word `word` of region `name`"""
        return self.base + 8 * (self.by_name[name].start + word)

    def expect(self, name, expected):
        r = self.by_name[name]
        assert r.role != "in"
        r.expected = _bytes_of(expected)
        assert r.expected.size == r.nbytes, "%s: %d bytes expected of a region of %d" % (name, r.expected.size, r.nbytes)

    def _image(self, what):
        """the whole arena as it is uploaded (what = "data") or as it must be afterwards (what = "expected")"""
        img = pattern(0, self.words)
        raw = img.view(np.uint8)
        for r in self.regions:
            a = r.data
            if what == "expected" and r.role != "in":
                assert r.expected is not None, "region %s has no expected array" % r.name
                a = r.expected
            if a is not None:
                raw[8 * r.start:8 * r.start + a.size] = a
        return img

    def assert_unwritten_words_would_show(self):
        """No word of an expected array equals the pattern at its position: else a word the call never wrote would pass."""
        for r in self.regions:
            if r.role != "in" and r.expected is not None:
                fill = pattern(r.start, r.words)
                want = fill.copy()
                want.view(np.uint8)[:r.expected.size] = r.expected
                same = np.flatnonzero(want == fill)
                assert same.size == 0, "region %s: word %d equals the fill pattern, an unwritten word would not show" % (r.name, same[0])

    def upload(self):
        self.assert_unwritten_words_would_show()
        self.memory.write(0, self._image("data"))
        self.uploaded = True
        return self

    def violations(self):
        """downloads the whole arena once -> [Violation], guards and regions in address order"""
        assert self.uploaded
        self.assert_unwritten_words_would_show()
        got, want = self.memory.read(), self._image("expected")
        self.last = got
        out = []

        def look(lo, hi, make):
            bad = np.flatnonzero(got[lo:hi] != want[lo:hi])
            if bad.size:
                out.append(make(int(bad[0]), bad.size, got[lo + bad[0]], want[lo + bad[0]]))
        for k, (start, words, before, after) in enumerate(self.guards):
            lo = start if before is None else before.start + before.words      # with the slack behind the region
            hi = start + words
            look(lo, hi, lambda off, cnt, g, w, lo=lo, hi=hi, before=before, after=after: Violation(
                "guard", "guard %d" % k, off, cnt, g, w, after=before.name if before else None, before=after.name if after else None,
                past=off if before else None, short=hi - lo - off if after else None))
            if after is not None:
                look(after.start, after.start + after.words, lambda off, cnt, g, w, r=after: Violation(r.role, r.name, off, cnt, g, w))
        return out

    def check(self):
        """guards unchanged, in regions unchanged, out / inout regions equal to their expected arrays"""
        bad = self.violations()
        assert not bad, "\n".join(str(v) for v in bad)

    def check_untouched(self):
        """nothing at all has been written since the upload (a call that only reads, or that sets up a later write)"""
        assert self.uploaded
        bad = np.flatnonzero(self.memory.read() != self._image("data"))
        assert bad.size == 0, "%d word(s) changed since the upload, first at arena word %d" % (bad.size, bad[0])

    def region_words(self, name):
        """region `name` as the last download held it (violations() or check() first), whole words"""
        r = self.by_name[name]
        return self.last[r.start:r.start + r.words].copy()


def device_arena(ctx, regions, order):
    """an uploaded Arena in gl_dev_alloc memory of `ctx`"""
    return Arena(lambda words: DeviceMemory(ctx, words), regions, order).upload()


def host_arena(regions, order=ORDERS[0]):
    """an uploaded Arena in host memory: ptr(name) is an interior pointer into a numpy array with guards on both sides"""
    return Arena(NumpyMemory, regions, order).upload()


def host_out(name="out", words=None, nbytes=None, item=1, expected=None):
    """a guarded host output buffer of exactly `words` words (or `nbytes` bytes, or the length of `expected`)"""
    return host_arena([Region(name, "out", words=words, nbytes=nbytes, item=item, expected=expected)])

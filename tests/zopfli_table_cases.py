"""The Zopfli match table (d4g_debug_zopfli_table: k_zf_match_sorted or, with D4G_ZF_TABLE=scan, k_zf_match, plus the tail
tables of a block end inside the input) against the oracle's zopf_match_table, position by position and length by length:
shared by the emulator test (test_hostsim.py), the oracle-only test of the cases' conditions (test_zopfli_oracle.py) and
the GPU test (test_gpu_zopfli_table.py).  Every input is valid data made from a seed; each is the smallest at which the
edge it is named after exists, and says so with a condition on the oracle's output alone."""
import functools
import random

import numpy as np

import synth
import zopf_lib as ZF

WSIZE = 32768
BUILDS = ("sorted", "scan")         # D4G_ZF_TABLE; anything but "scan" is the default build


# ---- the two sides ----
class Oracle:
    """zopf_match_table of data[:end]: ol / od (longest length and its distance), osl[i, l] (distance of length l),
    cap_breaks (searches the 8192-hit cap ended)."""

    def __init__(self, data, end=0):
        e = end or len(data)
        self.end = e
        self.ol, self.od = np.zeros(e, np.uint16), np.zeros(e, np.uint16)
        self.osl = np.zeros((e, 259), np.uint16)
        ZF.lib().zopf_cap_breaks_reset()
        ZF.lib().zopf_match_table(data, 0, e, self.ol.ctypes.data, self.od.ctypes.data, self.osl.ctypes.data)
        self.cap_breaks = ZF.lib().zopf_cap_breaks()

    def change_points(self):
        """per position: the (length, distance) records of length >= 3, i.e. the runs of equal distance in osl[i, 3:len+1]"""
        cols = np.arange(3, 258)[None, :]
        step = (self.osl[:, 3:258] != self.osl[:, 4:259]) & (cols < self.ol[:, None])
        return step.sum(axis=1) + (self.ol >= 3)

    def stats(self):
        won = self.ol >= 3
        return {"cap_breaks": int(self.cap_breaks), "max_change_points": int(self.change_points().max(initial=0)),
                "max_dist": int(self.od[won].max(initial=0)), "max_len": int(self.ol.max(initial=0)),
                "dist_ge_32700": int((self.od[won] >= 32700).sum())}


def device_table(L, data, end=0):
    n, e = len(data), end or len(data)
    l16, d16 = np.zeros(n, np.uint16), np.zeros(n, np.uint16)
    sl = np.zeros((n, 259), np.uint16)
    rc = L.d4g_debug_zopfli_table(data, n, end, l16.ctypes.data, d16.ctypes.data, sl.ctypes.data)
    assert rc == 0, "d4g_debug_zopfli_table: %d %s" % (rc, L.d4g_last_error())
    return l16[:e], d16[:e], sl[:e]


def _around(data, i):
    lo = max(0, i - 8)
    return "bytes [%d, %d) = %s" % (lo, min(len(data), i + 8), data[lo:i + 8].hex(" "))


def compare(data, ora, dev, what=""):
    """len16 / dist16 / sublen of every position below the end; a failure names the first differing position and length,
    both values and the input around it."""
    l16, d16, sl = dev
    wl = np.where(ora.ol >= 3, ora.ol, 0)
    wd = np.where(ora.ol >= 3, ora.od, 0)
    for name, got, want in (("len16", l16, wl), ("dist16", d16, wd)):
        if not np.array_equal(got, want):
            i = int(np.flatnonzero(got != want)[0])
            raise AssertionError("%s %s[%d]: device %d, oracle %d (oracle length %d, distance %d; end %d of %d); %s"
                                 % (what, name, i, got[i], want[i], ora.ol[i], ora.od[i], ora.end, len(data), _around(data, i)))
    cols = np.arange(259)[None, :]
    inside = (cols >= 3) & (cols <= wl[:, None])
    want = np.where(inside, ora.osl, 0)
    # (the hook writes nothing above a position's last change point: a table that runs past `best` shows as a non-zero there)
    if not np.array_equal(sl, want):
        i, l = (int(x) for x in np.argwhere(sl != want)[0])
        raise AssertionError("%s sublen[%d, %d]: device %d, oracle %d (oracle length %d, distance %d, %d change points; end %d of %d); %s"
                             % (what, i, l, sl[i, l], want[i, l], ora.ol[i], ora.od[i], ora.change_points()[i], ora.end, len(data),
                                _around(data, i)))


def check(L, data, end=0, ora=None, what=""):
    ora = ora or Oracle(data, end)
    compare(data, ora, device_table(L, data, end), what)
    return ora


# ---- the inputs ----
def _cap():
    """Two parity classes, the top bit set on a tenth of the bytes: the 3-byte hash drops the top bit of its first byte, so most
    of a class shares one bucket (about 12 K nodes per window) while matches stay short — the walk ends at the hit cap."""
    rng = random.Random(2)
    return bytes((i & 1) | (0x80 if rng.random() < 0.10 else 0) for i in range(50000))


def _two():
    """A fair coin over {0x00, 0x80}: four buckets of about 8192 nodes per window (the cap's borderline: with this seed one
    search of 70000 ends at it), with byte runs, so the second hash and the switch between the chains are in play."""
    rng = random.Random(8)
    return bytes(rng.choice((0x00, 0x80)) for _ in range(70000))


EDGE_B, EDGE_C = 300, 10000


def _edge():
    """Block B at 0; B[:299] and a differing byte at 32767 (longest match at distance 32767 exactly, across the first sort-block
    seam); all of B at 65534 (distance 32767 from that copy, 65534 from B itself, across the second seam).  Block C at 10000 and
    again at 10000 + 32768: its only earlier occurrence is one byte out of the window."""
    rng = random.Random(11)
    B = bytes(rng.randrange(256) for _ in range(EDGE_B))
    Cb = bytes(rng.randrange(256) for _ in range(EDGE_B))
    d = bytearray(rng.randrange(256) for _ in range(2 * (WSIZE - 1) + EDGE_B))
    d[0:EDGE_B] = B
    d[WSIZE - 1:WSIZE - 1 + EDGE_B] = B[:-1] + bytes([B[-1] ^ 0x55])
    d[2 * (WSIZE - 1):] = B
    d[EDGE_C:EDGE_C + EDGE_B] = Cb
    d[EDGE_C + WSIZE:EDGE_C + WSIZE + EDGE_B] = Cb
    return bytes(d)


def _longrun():
    return b"x" * 70000 + b"y" + b"x" * 3000


def _ladder_group():
    S = synth.reptext(200, 1)
    return b"".join(S[:k] for k in range(200, 2, -1)) + S


def ladder():
    """the head of test_change_point_pool_grows_instead_of_failing's group S[:200], S[:199], ..., S[:3], S as that test cuts it"""
    return _ladder_group()[:6000]


def ladder_end(n=6000):
    """the same group's end, where its record-setting matches are: S after S[:3], S[:4], ... meets a longer match at every
    greater distance, so its positions carry up to a hundred change points and the pool is what holds them"""
    return _ladder_group()[-n:]


def _reptext():
    return synth.reptext(70000, 5)


SMALL = {"empty": b"", "one": b"a", "two_bytes": b"ab", "three": b"abc", "four": b"abca", "abcabc": b"abc" * 2}


class Case:
    def __init__(self, name, make, env=None, ends=None, match=None, cond=None):
        self.name, self.make, self.env, self.ends, self.match, self.cond = name, make, env or {}, ends or {}, match, cond

    @property
    def data(self):
        return _data(self.name)

    def end_keys(self):
        """"0" is the whole input; the named ends are the case's own"""
        return ["0"] + ([str(e) for e in FIXED_ENDS] + ["run", "match", "n-1"] if self.ends else [])

    def end(self, key):
        return len(self.data) - 1 if key == "n-1" else self.ends[key] if key in self.ends else int(key)

    def check_condition(self, ora):
        """what the case is for, asked of the oracle's whole-input table alone"""
        if self.cond:
            self.cond(ora)

    def check_ends(self):
        """`run`: a byte run crosses the end.  `match`: the end lies inside the match (position, distance, length) of the whole
        input, 100 bytes in (half way where the input has no match that long).  Properties of the input, asserted on it."""
        d = self.data
        e = self.ends["run"]
        assert 0 < e < len(d) and d[e - 1] == d[e]
        p, dist, ln = self.match
        assert 0 < dist <= p and ln >= 16 and d[p:p + ln] == d[p - dist:p - dist + ln]
        assert p < self.ends["match"] < p + ln <= len(d)


def pool_words(o):
    """words of the change-point pool the table of this input needs (an entry holds 8 points; beyond that 7 and a chain)"""
    c = o.change_points()
    return int((c[c > 8] - 7 + 1).sum())


def _cond_cap(o):
    assert o.cap_breaks >= 1000, o.cap_breaks
    assert o.change_points().max() > 7


def _cond_two(o):
    assert o.change_points().max() > 7


def _cond_edge(o):
    assert ((o.od == 32767) & (o.ol == 258)).any()
    assert o.od.max() == 32767
    # the copy of C: nothing of it is found one byte out of the window
    assert o.ol[EDGE_C + WSIZE:EDGE_C + WSIZE + EDGE_B - 8].max() < 8


def _cond_longrun(o):
    assert o.change_points().max() >= 200


def _cond_ladder_end(o):
    assert o.change_points().max() > 7
    assert pool_words(o) > 4 * LADDER_POOL      # the pool has to grow, more than once


FIXED_ENDS = (1, 2, 3, 511, 512, 513, 32767, 32768, 32769)
LADDER_POOL = 256

CASES = [
    Case("cap", _cap, cond=_cond_cap),
    Case("two", _two, cond=_cond_two, ends={"run": 35014, "match": 64865}, match=(64852, 332, 27)),
    Case("edge", _edge, cond=_cond_edge),
    Case("longrun", _longrun, cond=_cond_longrun, ends={"run": 68000, "match": 70102}, match=(70002, 1, 258)),
    Case("ladder", ladder, env={"D4G_ZF_POOL_WORDS": str(LADDER_POOL)}),
    Case("ladder_end", ladder_end, env={"D4G_ZF_POOL_WORDS": str(LADDER_POOL)}, cond=_cond_ladder_end),
    Case("reptext", _reptext, ends={"run": 35016, "match": 35148}, match=(35048, 10156, 258)),
] + [Case(k, (lambda v: lambda: v)(v)) for k, v in SMALL.items()]
BY_NAME = {c.name: c for c in CASES}


@functools.lru_cache(maxsize=None)
def _data(name):
    return BY_NAME[name].make()


@functools.lru_cache(maxsize=2)
def oracle(name, end):
    """the oracle's table of a case, kept for the next test that asks for the same one (the two table builds in turn)"""
    return Oracle(BY_NAME[name].data, end)


# the emulator's share (test_hostsim.py): the pool chain and its growth at a size a CPU walks in a moment
EMU_LADDER, EMU_LADDER_POOL = 800, 64

"""The pair table of the round-trip verification tests (test_verify_hostsim.py in the emulator, test_gpu_verify.py on the
GPU).  Every expected verdict comes from the oracle's inflate of both sides, never from the library under test."""
import zlib

import oracle_lib as O
import synth

OK, SKIPPED, PARSE, SIZE, LENGTH, BYTES = 0, 1, -1, -2, -3, -4
TILE = 128 * 1024          # bytes per workgroup of the compare kernel (D4G_CSUM_TILE)
STEP = 256 * 4 * 16        # bytes per unrolled step of a workgroup: 256 lanes x 4 loads x 16 bytes


def deflate(x, level=9, strategy=zlib.Z_DEFAULT_STRATEGY):
    c = zlib.compressobj(level, zlib.DEFLATED, -15, 8, strategy)
    return c.compress(x) + c.flush()


def oracle_verdict(a, b):
    """What d4g_verify_streams must say about (a, b), by the oracle alone."""
    ua, _ = O.inflate(a)
    if ua is None:
        return SKIPPED, -1
    ub, _ = O.inflate(b)
    if ub is None:
        return PARSE, -1
    common = min(len(ua), len(ub))
    for k in range(common):
        if ua[k] != ub[k]:
            return BYTES, k
    if len(ua) != len(ub):
        return LENGTH, common
    return OK, -1


def flip(x, k):
    y = bytearray(x)
    y[k] ^= 0x5A
    return bytes(y)


def pair_table(big=200000):
    """-> list of (name, a, b, decoded length of a).  `big` is the length of the main text: beyond one compare tile."""
    x = synth.reptext(big, 21)
    assert len(x) > TILE + STEP
    a9 = deflate(x, 9)
    t = [("same data, levels 9 and 1", a9, deflate(x, 1), len(x))]
    for k in (0, 1, 15, 16, 17, len(x) - 1, TILE + 4133):
        t.append(("one byte differs at %d" % k, a9, deflate(flip(x, k), 1), len(x)))
    t.append(("b one byte longer", a9, deflate(x + b"z"), len(x)))
    t.append(("b one byte shorter", a9, deflate(x[:-1]), len(x)))
    t.append(("b longer and an earlier byte differs", a9, deflate(flip(x, 77) + b"z"), len(x)))
    t.append(("b truncated", a9, a9[:len(a9) // 2], len(x)))
    t.append(("b garbage", a9, b"\x07garbage", len(x)))
    t.append(("a garbage", b"\x07garbage", a9, 0))
    t.append(("a truncated", a9[:len(a9) // 2], a9, 0))
    t.append(("empty and empty", deflate(b""), deflate(b"", 1), 0))
    t.append(("one byte and one byte", deflate(b"q"), deflate(b"q", 1), 1))
    t.append(("one byte and another byte", deflate(b"q"), deflate(b"r", 1), 1))
    t.append(("stored only and dynamic", deflate(x[:70000], 0), deflate(x[:70000], 9), 70000))
    # lengths around the kernel's paths: only a tail (< 16 bytes), whole vectors only, vectors and a tail, exactly one
    # unrolled step, a step and a remainder, last byte of each
    for n in (5, 16, 48, 1000, STEP, STEP + 16, STEP + 16 * 300 + 7, 2 * STEP + 9):
        y = synth.reptext(n, 100 + n)
        t.append(("%d bytes, equal" % n, deflate(y, 6), deflate(y, 1, zlib.Z_FIXED), n))
        t.append(("%d bytes, last differs" % n, deflate(y, 6), deflate(flip(y, n - 1), 1), n))
    return t


def check_table_covers_the_kernel_paths(t):
    """Asserted from the table itself: tail-only pairs, whole-vector pairs, pairs with an unrolled step, with a remainder
    after it, and one pair beyond a tile."""
    lens = [n for _, _, _, n in t]
    assert any(0 < n < 16 for n in lens)
    assert any(n >= 16 and n % 16 == 0 and n < STEP for n in lens)
    assert any(n >= 16 and n % 16 != 0 and n < STEP for n in lens)
    assert any(n == STEP for n in lens)
    assert any(n > STEP and (n % STEP) >= 16 and n % 16 != 0 for n in lens)
    assert any(n > TILE for n in lens)
    assert any(n == 0 for n in lens)

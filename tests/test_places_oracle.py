"""tests/places_oracle.py against a plain-Python scalar restatement of the specification, and what the
specification promises: the turn convention, the tie rules, empty scans."""
import functools
import math

import numpy as np

from tests.places_oracle import TURNS, describe, dilate, match_places, scores, sectors, to_bits, to_words

M64 = (1 << 64) - 1


def rotl(x, s):
    s &= 63
    return ((x << s) | (x >> (64 - s))) & M64 if s else x


def describe_scalar(row, angles, R, lo, hi):
    words, used = [0] * R, 0
    per_m = float(R) / hi
    for r, a in zip(row, angles):
        r = float(r)
        if not (lo < r and r < hi):
            continue
        used += 1
        ring = min(int(math.floor(r * per_m)), R - 1)
        words[ring] |= 1 << (int(math.floor(float(a) * (32.0 / math.pi))) & 63)
    return words, used, sum(bin(w).count("1") for w in words)


def field_scalar(D):
    R = len(D)
    out = []
    for g in range(R):
        w = 0
        for h in (g - 1, g, g + 1):
            if 0 <= h < R:
                w |= D[h] | rotl(D[h], 1) | rotl(D[h], 63)
        out.append(w)
    return out, sum(bin(w).count("1") for w in D) + sum(bin(w).count("1") for w in out)


def match_scalar(Qs, Ds, limit, k):
    out = []
    for q, Q in enumerate(Qs):
        cand = []
        for r, D in enumerate(Ds):
            if limit is not None and r >= limit[q]:
                continue
            P, w = field_scalar(D)
            best = None
            for s in range(64):
                v = sum(bin(Q[g] & rotl(D[g], s)).count("1") + bin(Q[g] & rotl(P[g], s)).count("1") for g in range(len(Q)))
                key = (-v, min(s, 64 - s), s)
                if best is None or key < best:
                    best = key
            if w > 0 and best[0] < 0:
                cand.append((r, best[2], -best[0], w))

        def order(a, b):
            l, r = a[2] * a[2] * b[3], b[2] * b[2] * a[3]
            return -1 if l > r or (l == r and a[0] < b[0]) else 1
        cand.sort(key=functools.cmp_to_key(order))
        out.append(cand[:k])
    return out


def test_words_and_bits_round_trip():
    rng = np.random.Generator(np.random.PCG64(1))
    d = rng.integers(0, 1 << 63, (5, 7), dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, (5, 7), dtype=np.uint64)
    assert np.array_equal(to_words(to_bits(d)), d) and to_bits(d).shape == (5, 7, 64)
    assert to_bits(np.array([[1 << 63]], dtype=np.uint64))[0, 0].tolist() == [False] * 63 + [True]
    assert TURNS[:6].tolist() == [0, 1, 63, 2, 62, 3] and TURNS[-1] == 32


def test_the_oracle_equals_the_scalar_restatement():
    rng = np.random.Generator(np.random.PCG64(2))
    ang = np.concatenate([np.linspace(-0.75 * math.pi, 0.75 * math.pi, 41), [-4.0, 7.0, -1e-9, 2.0 * math.pi]])
    rg = rng.uniform(0.0, 13.0, (9, len(ang)))
    rg[0, :8] = [np.nan, np.inf, -np.inf, 0.0, -2.0, 0.3, 12.0, np.nextafter(12.0, 0.0)]
    rg[3] = np.nan
    rg[4] = rg[1]
    for R in (1, 5, 24):
        desc, info = describe(rg, ang, R, 0.3, 12.0)
        rows = [describe_scalar(row, ang, R, 0.3, 12.0) for row in rg]
        assert desc.tolist() == [r[0] for r in rows] and info.tolist() == [[r[1], r[2]] for r in rows]
        assert info[3].tolist() == [0, 0] and rows[0][1] == 1 + sum(0.3 < r < 12.0 for r in rg[0, 8:])
        assert (int(desc[0, R - 1]) >> int(sectors(ang)[7])) & 1                     # nextafter(12, 0) is used, in ring R - 1
        P = to_words(dilate(to_bits(desc)))
        assert P.tolist() == [field_scalar(r[0])[0] for r in rows]
        limit = np.array([9, 9, 0, 9, 4, 5, 9, 2, 9])
        out4, out2 = match_places(desc[:, :], desc, limit, 3)
        want = match_scalar([r[0] for r in rows], [r[0] for r in rows], limit, 3)
        for q in range(9):
            got = [tuple(int(x) for x in row) for row in out4[q] if row[0] >= 0]
            assert got == want[q] and out2[q].tolist() == [rows[q][2], len(want[q])], (R, q)
            assert all(tuple(row) == (-1, 0, 0, 0) for row in out4[q, len(want[q]):].tolist())
        assert out2[2, 1] == 0 and out2[3, 1] == 0 and 3 not in out4[:, :, 0]           # no reference admitted; an empty scan
        assert out4[4, 0].tolist()[:2] == [1, 0] and out4[8, 0, 0] == 8                  # scan 4 is scan 1; a scan finds itself
        sc = scores(desc, desc)
        assert sc.max() <= 2 * info[:, 1].max() and np.all(sc[np.arange(9), np.arange(9), 0] == 2 * info[:, 1])


def test_the_turn_is_the_difference_of_the_headings():
    """One place seen at headings h * 2 pi / 64: 256 beams all round, four a sector, the range a function of the world
    direction alone.  The query's heading is the reference's minus shift sectors."""
    rng = np.random.Generator(np.random.PCG64(3))
    world = rng.uniform(0.5, 11.5, 256)
    ang = (np.arange(256) + 0.5) * (2.0 * math.pi / 256) - math.pi
    heads = [0, 1, 5, 31, 32, 33, 63]
    scans = np.stack([np.roll(world, -4 * h) for h in heads])                        # beam b looks along world direction b + 4 h
    desc, info = describe(scans, ang, 24, 0.3, 12.0)
    out4, _ = match_places(desc, desc, None, len(heads))
    for a, hq in enumerate(heads):
        for row in out4[a]:
            assert row[1] == (heads[row[0]] - hq) % 64 and row[2] == 2 * info[a, 1]


def test_tie_rules():
    one = np.uint64(0x0101010101010101)
    per = np.full((1, 4), one, dtype=np.uint64)                                      # periodic in the sector: eight turns tie
    turned = to_words(np.roll(to_bits(per), 3, axis=-1))
    refs = np.concatenate([per, turned, per, np.zeros((1, 4), np.uint64)])
    out4, out2 = match_places(per, refs, None, 4)
    # s = 0 wins among 0, 8, .. 56; the copy turned by 3 needs s = 61 (min(s, 64 - s) = 3) before 5, 13, ..; r 0 before r 2
    assert out4[0].tolist() == [[0, 0, 64, 32 + 96], [1, 61, 64, 128], [2, 0, 64, 128], [-1, 0, 0, 0]] and out2[0].tolist() == [32, 3]
    half = np.array([[0x00000001_00000001]], dtype=np.uint64)                        # s = 32 ties with s = 0
    assert match_places(half, half, None, 1)[0][0, 0].tolist() == [0, 0, 4, 2 + 6]
    # rank by v^2 / w, not by v: a small reference that the query covers beats a large one with more hits
    q = np.array([[0b0111]], dtype=np.uint64)
    small, large = np.array([[0b0011]], dtype=np.uint64), np.array([[0x00FF_FF07]], dtype=np.uint64)
    out4, _ = match_places(q, np.concatenate([large, small]), None, 2)
    assert out4[0, :, 0].tolist() == [1, 0] and out4[0, 0, 2] ** 2 * out4[0, 1, 3] > out4[0, 1, 2] ** 2 * out4[0, 0, 3]
    assert out4[0, 1, 2] > out4[0, 0, 2]


def test_empty_scans():
    ang = np.linspace(-2.0, 2.0, 30)
    rg = np.full((3, 30), 5.0)
    rg[1] = 0.1                                                                        # nothing in (0.3, 12)
    desc, info = describe(rg, ang, 8, 0.3, 12.0)
    assert info[1].tolist() == [0, 0] and not desc[1].any() and info[0, 0] == 30
    out4, out2 = match_places(desc, desc, None, 2)
    assert out4[1].tolist() == [[-1, 0, 0, 0]] * 2 and out2[1].tolist() == [0, 0]      # an empty query finds nothing
    assert out4[0, :, 0].tolist() == [0, 2] and out2[0, 1] == 2                        # and nobody finds an empty reference
    assert match_places(desc[:1], desc[1:2], None, 1)[1][0].tolist() == [int(info[0, 1]), 0]

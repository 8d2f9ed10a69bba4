"""Helpers of tests/test_gpu_absorb.py and tests/test_gpu_encode_session.py (a plain module): the
shapes, the sets of body ranges that cover [0, L) exactly once, and the expected parity rows after
any set of feeds -- by GF(2) linearity the C oracle's Encode of the body with every byte not yet
fed set to zero. Needs no device."""
import numpy as np

from oracle import cref

T = 4096  # columns of one interval per block
SIZES = (1, 5, 15, 16, 17, 40, 1023, T - 1, T, T + 1, T + 16, 2 * T + 83)
OTHER_PROFILES = ((1, 3), (3, 2), (4, 2), (16, 4), (10, 8), (20, 12), (64, 16))
PATTERNS = ("whole", "per-shard", "bytes", "cycle", "shuffled", "three", "two")


def body_len(k, S):
    """L = k * S - 7 whenever that is positive and still gives this S, else k * S."""
    L = k * S - 7
    return L if L > 0 and -(-L // k) == S else k * S


def cover(L, sizes, special=None):
    """Ranges (off, len) that cover [0, L) exactly once, in ascending order: `special` (clipped to
    L) and pieces whose sizes cycle through `sizes` over the rest."""
    out, q = [], 0
    s0, s1 = (min(special[0], L), min(special[0] + special[1], L)) if special else (L, L)
    for lo, hi in ((0, s0), (s1, L)):
        at = lo
        while at < hi:
            n = min(sizes[q % len(sizes)], hi - at)
            out.append((at, n))
            at += n
            q += 1
        if lo == 0 and s1 > s0:
            out.append((s0, s1 - s0))
    return sorted(out)


def ranges(pattern, S, L, rng):
    """One set of ranges of `pattern`, or None where the shape has none."""
    if pattern == "whole":
        return [(0, L)]
    if pattern == "per-shard":
        return cover(L, [S])
    if pattern == "bytes":
        return cover(L, [1]) if S <= 17 else None
    if pattern == "cycle":  # pieces of 7, 16, 100 and S + 3 bytes in order
        return cover(L, [7, 16, 100, S + 3])
    if pattern == "shuffled":  # consecutive pieces put their cut at every residue
        r = cover(L, [S + 3])
        return [r[i] for i in rng.permutation(len(r))]
    if pattern == "three":  # 2 S + 5 bytes from column S - 2: three intervals from S = 6 on
        if S < 2:
            return None
        r = cover(L, [S + 3], (S - 2, 2 * S + 5))
        return [r[i] for i in rng.permutation(len(r))]
    if pattern == "two":  # S - 1 bytes from column S - 3: two shards, the middle interval empty
        if S < 5:
            return None
        r = cover(L, [S + 3], (S - 3, S - 1))
        return [r[i] for i in rng.permutation(len(r))]
    raise ValueError(pattern)


def shards_of(body, k, S):
    """Split: the k data shards of S bytes, zero padded."""
    flat = np.zeros(k * S, dtype=np.uint8)
    flat[:len(body)] = body
    return flat.reshape(k, S)


def parity_of(body, k, m, S):
    """[m][S]: the oracle's Encode of the body."""
    sh = shards_of(body, k, S)
    return np.stack([np.asarray(p, dtype=np.uint8) for p in cref.encode([sh[i] for i in range(k)], k, m)])


class Masked:
    """The body with every byte not yet fed set to zero, and the oracle's parity of it."""

    def __init__(self, body, k, m, S):
        self.body, self.k, self.m, self.S = body, k, m, S
        self.fed = np.zeros(len(body), dtype=np.uint8)

    def feed(self, off, n):
        assert not self.fed[off:off + n].any() and off + n <= len(self.body)
        self.fed[off:off + n] = self.body[off:off + n]
        return self.parity()

    def parity(self):
        return parity_of(self.fed, self.k, self.m, self.S)


def random_body(L, rng):
    """L nonzero bytes: every fed byte changes every row (P has no zero entry)."""
    return rng.integers(1, 256, L, dtype=np.uint8)

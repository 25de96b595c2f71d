"""CPU restatement of the throughput-mode sampler, written from the published definitions.

  * Philox4x32-10: J. Salmon, M. Moraes, R. Dror, D. Shaw, "Parallel random numbers: as easy as
    1, 2, 3" (SC 2011) and the Random123 library: ten rounds of
        (c0, c1, c2, c3) <- (hi(M1 c2) ^ c1 ^ k0, lo(M1 c2), hi(M0 c0) ^ c3 ^ k1, lo(M0 c0))
    with M0 = 0xD2511F53, M1 = 0xCD9E8D57, the key raised by the Weyl constants
    (0x9E3779B9, 0xBB67AE85) between rounds.
  * Bounded draw: D. Lemire, "Fast random integer generation in an interval" (TOMACS 2019):
    m = x s, l = m mod 2^32; if l < s, reject while l < (2^32 - s) mod s; the draw is m >> 32.
  * Subsets: R. Floyd's algorithm (Bentley & Floyd, "Programming pearls: a sample of brilliance",
    CACM 1987): for j = n - k .. n - 1 draw t in [0, j] and take j if t is already taken, else t.

How the project keys it: hypothesis h of stream `seed` reads the blocks
of counters (h & 0xffffffff, h >> 32, c, 0x5a17), c = 0, 1, ..., under the key
(seed & 0xffffffff, seed >> 32); the words of a block are used in order and block c + 1 follows
every fourth word.  numpy only; h and seed wrap modulo 2^64 as the device's uint64 does.
"""
from __future__ import annotations

import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
DOMAIN = 0x5A17
MASK32 = 0xFFFFFFFF
MASK64 = 0xFFFFFFFFFFFFFFFF


# ------------------------------------------------------------------------------------------
# scalar (Python int) version
# ------------------------------------------------------------------------------------------
def philox4x32_10(counter, key):
    """One block: counter (c0, c1, c2, c3), key (k0, k1), all 32-bit -> four 32-bit words."""
    c0, c1, c2, c3 = (int(v) & MASK32 for v in counter)
    k0, k1 = (int(v) & MASK32 for v in key)
    for _ in range(10):
        p0, p1 = M0 * c0, M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & MASK32, (p0 >> 32) ^ c3 ^ k1, p0 & MASK32
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return c0, c1, c2, c3


def floyd_tuple(seed, h, n, k):
    """The k-subset of [0, n) of hypothesis h, in draw order, and the words it consumed."""
    seed, h = int(seed) & MASK64, int(h) & MASK64
    if not 0 < k <= n:
        raise ValueError("need 0 < k <= n")
    key = (seed & MASK32, seed >> 32)
    words = 0
    block = None

    def word():
        nonlocal words, block
        if words % 4 == 0:
            block = philox4x32_10((h & MASK32, h >> 32, words // 4, DOMAIN), key)
        w = block[words % 4]
        words += 1
        return w

    out = []
    for m in range(k):
        j = n - k + m
        s = j + 1
        prod = word() * s
        if (prod & MASK32) < s:
            thresh = ((1 << 32) - s) % s
            while (prod & MASK32) < thresh:
                prod = word() * s
        t = prod >> 32
        out.append(j if t in out else t)
    return out, words


# ------------------------------------------------------------------------------------------
# vectorised over hypotheses
# ------------------------------------------------------------------------------------------
def philox_blocks(h, c, seed):
    """Blocks of hypotheses h (uint64 array) at block index c (int): uint64 (len(h), 4), each
    entry a 32-bit word."""
    h = np.asarray(h, dtype=np.uint64)
    seed = int(seed) & MASK64
    m32 = np.uint64(MASK32)
    s32 = np.uint64(32)
    c0, c1 = h & m32, h >> s32
    c2 = np.full(h.shape, int(c) & MASK32, dtype=np.uint64)
    c3 = np.full(h.shape, DOMAIN, dtype=np.uint64)
    k0, k1 = seed & MASK32, seed >> 32
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c0, np.uint64(M1) * c2   # 32 x 32 bits: no overflow in 64
        c0, c1, c2, c3 = ((p1 >> s32) ^ c1 ^ np.uint64(k0), p1 & m32,
                          (p0 >> s32) ^ c3 ^ np.uint64(k1), p0 & m32)
        k0, k1 = (k0 + W0) & MASK32, (k1 + W1) & MASK32
    return np.stack([c0, c1, c2, c3], axis=1)


def _floyd(seed, h0, H, n, k):
    """(tuples int32 (H, k), words consumed int64 (H,), edge bool (H,)) of hypotheses h0 ..
    h0 + H - 1; edge: a draw was accepted with l equal to the rejection threshold (the case
    that tells "l < threshold" from "l <= threshold")."""
    H, n, k = int(H), int(n), int(k)
    if not 0 < k <= n or n > 1 << 31:
        raise ValueError("need 0 < k <= n <= 2^31")
    h = (np.arange(H, dtype=np.uint64) + np.uint64(int(h0) & MASK64))  # wraps modulo 2^64
    blocks = []                       # blocks[c]: (H, 4), made when first needed
    used = np.zeros(H, dtype=np.int64)
    rows = np.arange(H)

    def words(sel):
        """The next word of the hypotheses sel (index array)."""
        pos = used[sel]
        while len(blocks) <= int(pos.max(initial=0)) // 4:
            blocks.append(philox_blocks(h, len(blocks), seed))
        w = np.empty(len(sel), dtype=np.uint64)
        for c in np.unique(pos // 4):
            q = pos // 4 == c
            w[q] = blocks[c][sel[q], pos[q] % 4]
        used[sel] += 1
        return w

    out = np.empty((H, k), dtype=np.int64)
    edge = np.zeros(H, dtype=bool)
    m32 = np.uint64(MASK32)
    for m in range(k):
        j = n - k + m
        s = np.uint64(j + 1)
        prod = words(rows) * s
        thresh = np.uint64(((1 << 32) - (j + 1)) % (j + 1))
        # (l < s is implied by l < thresh, as thresh < s: Lemire's first test is a short cut)
        again = np.flatnonzero((prod & m32) < thresh)
        while len(again):
            prod[again] = words(again) * s
            again = again[(prod[again] & m32) < thresh]
        edge |= (prod & m32) == thresh
        t = (prod >> np.uint64(32)).astype(np.int64)
        dup = (out[:, :m] == t[:, None]).any(axis=1)
        out[:, m] = np.where(dup, j, t)
    return out.astype(np.int32), used, edge


def floyd_tuples(seed, h0, H, n, k):
    """int32 (H, k): the k-subsets of [0, n) of hypotheses h0 .. h0 + H - 1 of stream seed."""
    return _floyd(seed, h0, H, n, k)[0]


def rejecting_hypotheses(seed, h0, H, n, k, chunk=1 << 18):
    """The hypotheses of the window h0 .. h0 + H - 1 in which a bounded draw was rejected:
    (h int64 array, words consumed by each, > k)."""
    hs, ws = [], []
    for lo in range(0, int(H), chunk):
        cnt = min(chunk, int(H) - lo)
        _, used, _ = _floyd(seed, int(h0) + lo, cnt, n, k)
        r = np.flatnonzero(used > k)
        hs.append(r + int(h0) + lo)
        ws.append(used[r])
    return np.concatenate(hs).astype(np.int64), np.concatenate(ws)


def edge_hypotheses(seed, h0, H, n, k, chunk=1 << 18):
    """The hypotheses of the window that accept a draw with l exactly equal to the rejection
    threshold: a sampler that rejects on "l <= threshold" draws another tuple there.  For a
    range that is a power of two the threshold is 0 and l = 0 once in 2^32 / range words, so
    such hypotheses can be found (for any other range: once in 2^32)."""
    hs = []
    for lo in range(0, int(H), chunk):
        cnt = min(chunk, int(H) - lo)
        hs.append(np.flatnonzero(_floyd(seed, int(h0) + lo, cnt, n, k)[2]) + int(h0) + lo)
    return np.concatenate(hs).astype(np.int64)


# Hypotheses of stream REJECT_SEED at n = REJECT_N, k = 8 that reject a draw (all of
# rejecting_hypotheses over [0, 2^17) below 50 000): each consumes a ninth word, so a third
# block.  EDGE_H8 / EDGE_H5: hypotheses of the same stream at n = EDGE_N (the last draw's range
# is 2^16) whose last draw has l = threshold = 0, for k = 8 and k = 5 (the first of
# edge_hypotheses over [0, 2^20)).  tests/test_philox_ref_cpu.py keeps all of them honest.
REJECT_SEED, REJECT_N = 20240611, 100003
REJECT_H = (6953, 28401, 42002, 42881)
EDGE_N = 65536
EDGE_H8 = (13725, 30738, 49725)
EDGE_H5 = (37592, 96026)

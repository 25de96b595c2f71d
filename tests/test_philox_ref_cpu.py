"""The numpy restatement of the throughput-mode sampler (tests/philox_ref.py) against the
published known answers of Philox4x32-10, against its own scalar version, and for what the
sampler promises: k distinct indices, every k-subset equally likely, Lemire's rejection taken
where it must be.  The GPU side is tests/test_gpu_philox.py."""
from itertools import combinations

import numpy as np
import pytest
from scipy import stats

import philox_ref as pr

HIGH_SEED = 0x9E3779B97F4A7C15


@pytest.mark.parametrize("counter, key, out", [
    ((0, 0, 0, 0), (0, 0), "6627e8d5 e169c58d bc57ac4c 9b00dbd8"),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, "408f276d 41c83b0e a20bc7c6 6d5451fd"),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0),
     "d16cfe09 94fdcceb 5001e420 24126ea1"),
])
def test_philox4x32_10_known_answers(counter, key, out):
    assert " ".join(f"{w:08x}" for w in pr.philox4x32_10(counter, key)) == out


def test_vectorised_blocks_equal_scalar_blocks():
    """The numpy block function on the project's counter layout, h on both sides of 2^32."""
    for seed in (0, 1234, HIGH_SEED):
        h = np.array([0, 1, 2**32 - 1, 2**32, 2**40 + 7, 2**64 - 1], dtype=np.uint64)
        for c in (0, 1, 2):
            got = pr.philox_blocks(h, c, seed)
            for i, hh in enumerate(h.tolist()):
                want = pr.philox4x32_10((hh & pr.MASK32, hh >> 32, c, pr.DOMAIN),
                                        (seed & pr.MASK32, seed >> 32))
                assert tuple(got[i].tolist()) == want


@pytest.mark.parametrize("seed, h0, H, n, k", [
    (0, 0, 700, 8, 8),                       # n = k: permutations
    (1234, 1, 700, 9, 8),
    (HIGH_SEED, 2**32 - 350, 700, 37, 8),    # h crosses into the high counter word
    (HIGH_SEED, 2**40 + 7, 500, 2000, 8),
    (1, 2**64 - 5, 10, 100, 5),              # h wraps as the device's uint64
    (7, 0, 500, 5, 5),
    (2**32 + 3, 2**32, 500, 120, 5),
    (3, 0, 500, 3, 3),
    (HIGH_SEED, 5, 500, 6, 6),
    (11, 0, 500, 500, 6),
    (13, 0, 500, 4, 3),
    (pr.REJECT_SEED, pr.REJECT_H[0] - 32, 64, pr.REJECT_N, 8),   # through a rejected draw
    (pr.REJECT_SEED, pr.EDGE_H8[0] - 32, 64, pr.EDGE_N, 8),
])
def test_vectorised_tuples_equal_scalar_tuples(seed, h0, H, n, k):
    tup, used, _ = pr._floyd(seed, h0, H, n, k)
    assert tup.dtype == np.int32 and tup.shape == (H, k)
    assert np.array_equal(tup, pr.floyd_tuples(seed, h0, H, n, k))
    for i in range(H):
        want, words = pr.floyd_tuple(seed, h0 + i, n, k)
        assert tup[i].tolist() == want and used[i] == words, (i, tup[i], want)
    # k distinct indices in [0, n)
    assert tup.min() >= 0 and tup.max() < n
    s = np.sort(tup, axis=1)
    assert (s[:, 1:] > s[:, :-1]).all()
    if n == k:
        assert (s == np.arange(k)).all()


def test_seed_and_hypothesis_words_all_matter():
    """Dropping the high word of the seed or of h, or the block index, changes the tuples."""
    base = pr.floyd_tuples(HIGH_SEED, 2**40 + 7, 64, 2000, 8)
    assert not np.array_equal(base, pr.floyd_tuples(HIGH_SEED & pr.MASK32, 2**40 + 7, 64, 2000, 8))
    assert not np.array_equal(base, pr.floyd_tuples(HIGH_SEED, 7, 64, 2000, 8))
    # words 0-3 and 4-7 of a hypothesis come from different blocks
    b0 = pr.philox_blocks(np.arange(64, dtype=np.uint64), 0, 1234)
    b1 = pr.philox_blocks(np.arange(64, dtype=np.uint64), 1, 1234)
    assert not (b0 == b1).any()


@pytest.mark.parametrize("n, k, per_subset", [(7, 3, 1200), (9, 8, 2000)])
def test_subsets_are_uniform(n, k, per_subset):
    """Chi-square of the subset counts over a fixed window (deterministic: fixed seed)."""
    subsets = list(combinations(range(n), k))
    H = per_subset * len(subsets)
    tup = pr.floyd_tuples(2024, 0, H, n, k)
    code = (1 << tup.astype(np.int64)).sum(axis=1)
    want = np.array([sum(1 << i for i in s) for s in subsets])
    counts = np.array([(code == w).sum() for w in want])
    assert counts.sum() == H            # every tuple is one of the k-subsets
    chi2 = ((counts - per_subset) ** 2 / per_subset).sum()
    bound = stats.chi2.ppf(1 - 1e-3, len(subsets) - 1)
    print(f"\n(n, k) = ({n}, {k}): chi2 {chi2:.1f} < {bound:.1f} over {len(subsets)} subsets")
    assert chi2 < bound


def test_rejection_path_constants():
    """At n = 100 003, k = 8 about one hypothesis in 10^4 rejects a draw; the recorded ones are
    what the finder lists, and each reads a ninth word (a third block)."""
    hs, words = pr.rejecting_hypotheses(pr.REJECT_SEED, 0, 1 << 17, pr.REJECT_N, 8)
    print(f"\nrejecting hypotheses in [0, 2^17): {hs.tolist()} words {words.tolist()}")
    assert len(hs) >= 3 and (words >= 9).any()
    assert tuple(hs[hs < 50000].tolist()) == pr.REJECT_H
    for h in pr.REJECT_H:
        tup, w = pr.floyd_tuple(pr.REJECT_SEED, h, pr.REJECT_N, 8)
        assert w >= 9 and len(set(tup)) == 8


def test_threshold_edge_constants():
    """The recorded hypotheses whose last draw sits exactly on Lemire's threshold (range 2^16,
    threshold 0, l = 0): accepted by "l < threshold", drawn again by "l <= threshold"."""
    for k, want in ((8, pr.EDGE_H8), (5, pr.EDGE_H5)):
        hs = pr.edge_hypotheses(pr.REJECT_SEED, 0, 100000, pr.EDGE_N, k)
        assert tuple(hs[:len(want)].tolist()) == want
        for h in want:
            c, q = divmod(k - 1, 4)
            w = pr.philox4x32_10((h, 0, c, pr.DOMAIN), (pr.REJECT_SEED, 0))[q]
            assert (w * pr.EDGE_N) % 2**32 == 0 == (2**32 - pr.EDGE_N) % pr.EDGE_N
            tup, words = pr.floyd_tuple(pr.REJECT_SEED, h, pr.EDGE_N, k)
            assert words == k and tup[-1] in (w >> 16, pr.EDGE_N - 1)

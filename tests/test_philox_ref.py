"""CPU: tests/philox_ref.py against the published Philox4x32-10 known-answer vectors (Random123 kat_vectors), and the
properties of mask_reference that tests/test_gpu_step_tail.py relies on."""
import numpy as np
import pytest

from tests import philox_ref as P

# counter[4], key[2] -> output[4]
KAT = [
    ((0x00000000, 0x00000000, 0x00000000, 0x00000000), (0x00000000, 0x00000000),
     (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff, 0xffffffff, 0xffffffff, 0xffffffff), (0xffffffff, 0xffffffff),
     (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


def _scalar_philox(ctr, key):
    """The same definition once more in plain Python integers (no NumPy): guards the vectorised form against a
    wrap-around or dtype slip that the three vectors alone might miss."""
    c0, c1, c2, c3 = ctr
    k0, k1 = key
    for _ in range(10):
        p0, p1 = P.M0 * c0, P.M1 * c2
        c0, c1, c2, c3 = (p1 >> 32) ^ c1 ^ k0, p1 & 0xFFFFFFFF, (p0 >> 32) ^ c3 ^ k1, p0 & 0xFFFFFFFF
        k0, k1 = (k0 + P.W0) & 0xFFFFFFFF, (k1 + P.W1) & 0xFFFFFFFF
    return c0, c1, c2, c3


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_known_answer_vectors(ctr, key, want):
    got = P.philox4x32_10(ctr, key)
    assert tuple(int(w[0]) for w in got) == want
    assert _scalar_philox(ctr, key) == want


def test_vectorised_over_the_counter_matches_the_scalar_form():
    # all three vectors in one call (different counters, one key each is the API: so vary the counter under one key)
    rng = np.random.default_rng(0)
    ctr = rng.integers(0, 2 ** 32, (4, 257), dtype=np.uint64)
    ctr[:, 0] = 0xFFFFFFFF  # products at the top of the range
    key = (0xA4093822, 0x299F31D0)
    got = np.stack(P.philox4x32_10(tuple(ctr), key), axis=1)
    for j in range(ctr.shape[1]):
        assert tuple(int(x) for x in got[j]) == _scalar_philox(tuple(int(x) for x in ctr[:, j]), key)
    assert got.dtype == np.uint32


def test_mask_reference_contract():
    seed, step = (1234 + 1000003 * 7) * 1000003 + 3, 2 ** 40 + 7  # both high words live
    assert seed >> 32 and step >> 32
    n = 4097
    w = P.uniform_words(n, seed, step)
    # element i = word i % 4 of the block with counter (i // 4, 0, step_lo, step_hi), key (seed_lo, seed_hi)
    for i in (0, 1, 2, 3, 4, 5, 4095, 4096):
        blk = _scalar_philox((i // 4, 0, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
        assert int(w[i]) == blk[i % 4]
    # a prefix of a longer mask is the shorter mask (the tail group draws like any other group)
    for n_short in (1, 3, 4, 5, 1023):
        np.testing.assert_array_equal(P.uniform_words(n_short, seed, step), w[:n_short])
    # strict `<`: u takes multiples of 2^-24 in [0, 1): at keep = 1 everything is kept, and the element whose u equals
    # float32(keep) exactly is dropped
    assert P.mask_reference(n, 1.0, seed, step).all()
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    assert float(u.max()) < 1.0 and float(u.min()) >= 0.0
    k = float(u[17])
    m = P.mask_reference(n, k, seed, step)
    assert not m[17] and np.array_equal(m, u < np.float32(k))
    # every one of the four words, and both high words, matter
    assert len({int(x) for x in w[:4]}) == 4
    assert not np.array_equal(w, P.uniform_words(n, seed & 0xFFFFFFFF, step))
    assert not np.array_equal(w, P.uniform_words(n, seed, step & 0xFFFFFFFF))


def test_seed_formulas_match_the_product():
    """layer_seed / rank_seed restate hypelcnn_amd/plan.py (dropout launch) and runtime._rank_seed; held to the source
    text so that a change there is noticed here."""
    import inspect

    from hypelcnn_amd import plan, runtime
    assert "int(self.seed * 1000003 + idx)" in inspect.getsource(plan)
    assert "self.seed + (1000003 * self.dist[1]" in inspect.getsource(runtime)
    assert P.layer_seed(1234, 3) == 1234 * 1000003 + 3
    assert P.layer_seed(1234, 3, rank=7) == (1234 + 1000003 * 7) * 1000003 + 3 > 2 ** 32


def test_product_streams_are_independent_in_the_reference():
    """The bound the device test asserts, met by mask_reference alone for the exact seeds chosen.

    Two independent Bernoulli(p) masks agree at an element with probability a = p^2 + (1-p)^2 (0.58 at p = 0.3); over
    n = 2^20 elements the agreement rate has standard deviation sqrt(a(1-a)/n) = 4.82e-4 <= 4.9e-4, so
    |rate - a| <= 3e-3 is a six-sigma band (2e-9 per pair).  Derived, not measured."""
    n, keep = P.INDEP_N, P.INDEP_KEEP
    a = P.independent_agreement(keep)
    sigma = np.sqrt(a * (1 - a) / n)
    assert sigma <= 4.9e-4 and 6 * sigma <= P.INDEP_BOUND
    for name, (s0, t0), (s1, t1) in P.INDEP_PAIRS:
        m0, m1 = P.mask_reference(n, keep, s0, t0), P.mask_reference(n, keep, s1, t1)
        rate = float((m0 == m1).mean())
        print(f"{name}: agreement {rate:.6f} (independent: {a:.6f}, sigma {sigma:.2e})")
        assert abs(rate - a) <= P.INDEP_BOUND, name
        assert abs(float(m0.mean()) - keep) <= 6 * np.sqrt(keep * (1 - keep) / n), name

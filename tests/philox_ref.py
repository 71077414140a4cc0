"""Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1, 2, 3", SC'11), restated from the
paper's definition in NumPy, and the contract of hypel_dropout_mask stated on top of it.  Independent of the kernel
source on purpose: tests/test_philox_ref.py pins it to the published known-answer vectors, and
tests/test_gpu_step_tail.py compares the device masks with it bit for bit.

One round of the 4x32 bijection, with counter words (c0, c1, c2, c3) and round key (k0, k1):

    (hi0, lo0) = M0 * c0          (32 x 32 -> 64 bit product)
    (hi1, lo1) = M1 * c2
    (c0, c1, c2, c3) <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0)

Ten rounds; the key is bumped by the Weyl constants (W0, W1) BETWEEN rounds, so round r uses key + r * W."""
import numpy as np

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
ROUNDS = 10
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32_10(counter, key):
    """counter: four arrays (or ints) of 32-bit words, broadcast against each other; key: two ints.
    Returns four uint32 arrays: the output block of every counter."""
    c = [np.atleast_1d(np.asarray(w, dtype=np.uint64)) & _LO for w in counter]
    c = [w.copy() for w in np.broadcast_arrays(*c)]
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for r in range(ROUNDS):
        rk0 = np.uint64((k0 + r * W0) & 0xFFFFFFFF)
        rk1 = np.uint64((k1 + r * W1) & 0xFFFFFFFF)
        p0 = np.uint64(M0) * c[0]  # < 2^64: both factors are below 2^32
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> _S32) ^ c[1] ^ rk0, p1 & _LO, (p0 >> _S32) ^ c[3] ^ rk1, p0 & _LO]
    return tuple(w.astype(np.uint32) for w in c)


def uniform_words(count, seed, step):
    """The 32-bit word element i of a mask draws: word i % 4 of the block whose counter is
    (g_lo, g_hi, step_lo, step_hi), g = i // 4, under the key (seed_lo, seed_hi)."""
    count, seed, step = int(count), int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    groups = (count + 3) // 4
    g = np.arange(groups, dtype=np.uint64)
    out = philox4x32_10((g & _LO, g >> _S32, step & 0xFFFFFFFF, step >> 32), (seed & 0xFFFFFFFF, seed >> 32))
    return np.stack(out, axis=1).reshape(-1)[:count]


def mask_reference(count, keep, seed, step):
    """Boolean keep pattern of hypel_dropout_mask(count, keep, seed, *step): u = float32(word >> 8) * 2^-24 (exact: 24
    bits), kept iff u < float32(keep)."""
    w = uniform_words(count, seed, step)
    u = (w >> np.uint32(8)).astype(np.float32) * np.float32(2.0 ** -24)
    return u < np.float32(keep)


# --- the product's own seed formulas (hypelcnn_amd/plan.py dropout launch, hypelcnn_amd/runtime.py _rank_seed) ----------
SEED_PRIME = 1000003


def rank_seed(seed, rank):
    return seed + SEED_PRIME * rank


def layer_seed(seed, idx, rank=0):
    return rank_seed(seed, rank) * SEED_PRIME + idx


# The stream pairs whose independence both the CPU test (on mask_reference alone) and the device test check:
# (name, (seed, step) of the first mask, (seed, step) of the second).  Base seed 1234, layer 3, rank 7, step 41.
INDEP_N, INDEP_KEEP = 1 << 20, 0.3
INDEP_PAIRS = [
    ("layer idx / idx+1", (layer_seed(1234, 3), 41), (layer_seed(1234, 4), 41)),
    ("step s / s+1", (layer_seed(1234, 3), 41), (layer_seed(1234, 3), 42)),
    ("rank r / r+1", (layer_seed(1234, 3, rank=7), 41), (layer_seed(1234, 3, rank=8), 41)),
]
INDEP_BOUND = 3e-3


def independent_agreement(keep):
    """P(two independent masks agree at an element) = p^2 + (1-p)^2 (u is a multiple of 2^-24: P(u < keep) differs from
    keep by less than 2^-24, far below the bound)."""
    p = float(keep)
    return p * p + (1.0 - p) * (1.0 - p)

"""Inputs and references of the K24 tests (tests/test_hamming_index_cpu.py, test_hamming_index_gpu.py,
test_hamming_index_components_gpu.py, test_hamming_index_pool_fill_gpu.py): the block-index rule of polyfuzz_amd/csrc/k24_core.h restated
in numpy, the counts it gives on K23's cases and on a list of 4 096 fingerprints with planted near-copies as constants, pairs built by
hand against the rule's edges, and the lists whose block shapes can go wrong."""
import functools

import numpy as np

from tests import hamming_join_cases as HJ

MAX_BLOCKS = 256

# ---- the rule, in numpy ----------------------------------------------------------------------------------------------------------


def indexable(d, hmax):
    return 1 <= d < 1 << 24 and 0 <= hmax and hmax + 1 <= min(d, MAX_BLOCKS)


def bounds(d, hmax):
    """the m + 1 borders of the m = hmax + 1 blocks"""
    m = hmax + 1
    return [(b * d) // m for b in range(m + 1)]


def block_keys(x, d, hmax):
    """packed uint8 [n, B] -> uint64 [n, m]: the first min(width, 32) bits of every block, first bit most significant"""
    bits = np.unpackbits(x, axis=1)[:, :d]
    bd = bounds(d, hmax)
    out = np.zeros((len(x), hmax + 1), np.uint64)
    for b in range(hmax + 1):
        lo, hi = bd[b], min(bd[b + 1], bd[b] + 32)
        v = np.zeros(len(x), np.uint64)
        for k in range(lo, hi):
            v = (v << np.uint64(1)) | bits[:, k].astype(np.uint64)
        out[:, b] = v
    return out


def first_block(ka, kb, b):
    """the first-block rule on two key rows: no block before b has equal keys"""
    return not any(ka[q] == kb[q] for q in range(b))


def rule(x, y, d, hmax):
    """(checks, [(row, col, block)] of the hits) of the rule; y None: the self-join"""
    kx = block_keys(x, d, hmax)
    ky = kx if y is None else block_keys(y, d, hmax)
    h = HJ.distances_of(x, y)
    checks, hits = 0, []
    seen = np.zeros(h.shape, bool)          # a pair that agreed on an earlier block
    for b in range(hmax + 1):
        eq = kx[:, b][:, None] == ky[:, b][None, :]
        if y is None:
            eq = np.triu(eq, 1)
        checks += int(eq.sum())
        r, c = np.nonzero(eq & ~seen & (h <= hmax))
        hits += [(int(i), int(j), b) for i, j in zip(r, c)]
        seen |= eq
    return checks, hits


def oracle(x, y, hmax):
    """(rows, cols, distances) of the XOR / popcount oracle, row-major"""
    return HJ.oracle_pairs(HJ.distances_of(x, y), hmax)


def all_pairs(x, y):
    return len(x) * (len(x) - 1) // 2 if y is None else len(x) * len(y)


# ---- the rule's counts on K23's cases, measured with the numpy above -------------------------------------------------------------
CHECKS = {
    "300x96": {0.9: 1133, 0.8: 6153, 0.6: 50561},
    "257x64": {0.9: 1587, 0.8: 5473, 0.6: 26368},
    "200x1000": {0.9: 57034, 0.8: 307665, 0.6: 1866548},
    "130x4104": {0.9: 47927},                     # m = 206; 0.8 and 0.6 give m = 411 and 821: no index
}
ALL_PAIRS = {"300x96": 44850, "257x64": 32896, "200x1000": 200000, "130x4104": 8385}
INDEXABLE = [(name, t) for name in HJ.CASES for t in HJ.THRESHOLDS if t in CHECKS[name]]
NOT_INDEXABLE = [("130x4104", 0.8), ("130x4104", 0.6)]


# ---- 4 096 fingerprints of 64 bits with 1 024 planted near-copies, hmax = 3 -----------------------------------------------------
PLANTED = {"n": 4096, "d": 64, "hmax": 3, "checks": 3075, "all": 8386560, "hits": 750, "at_cutoff": 186, "one_beyond": 218}


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(24)
    x = rng.integers(0, 256, (4096, 8), dtype=np.uint8)
    src = rng.integers(0, 2048, 1024)
    for k, s in enumerate(src):
        row = np.unpackbits(x[s]).copy()
        f = rng.choice(64, rng.integers(0, 6), replace=False)      # 0 .. 5 flips: some beyond hmax
        row[f] ^= 1
        x[2048 + k] = np.packbits(row)
    x.setflags(write=False)
    return x


# ---- pairs built by hand ----------------------------------------------------------------------------------------------------------

def _flip(row, positions):
    bits = np.unpackbits(row).copy()
    bits[list(positions)] ^= 1
    return np.packbits(bits)


def adversarial64():
    """d = 64, hmax = 3 (blocks of 16 bits): rows 2 k, 2 k + 1 are pairs; returns (codes [12, 8], what each pair is there for)"""
    rng = np.random.default_rng(64)
    rows, why = [], []
    for keep in range(4):             # exactly ONE agreeing block: one flipped bit in each of the three others (h = 3)
        a = rng.integers(0, 256, 8, dtype=np.uint8)
        rows += [a, _flip(a, [16 * b + 5 + b for b in range(4) if b != keep])]
        why.append(("only block %d agrees" % keep, 3, keep))
    a = rng.integers(0, 256, 8, dtype=np.uint8)
    rows += [a, _flip(a, [3, 16 + 15, 32, 48 + 8])]      # one bit in EVERY block: h = 4, a candidate nowhere
    why.append(("a bit in every block", 4, None))
    a = rng.integers(0, 256, 8, dtype=np.uint8)
    rows += [a, a.copy()]                                # equal codes: agree on all four, reported in block 0
    why.append(("equal codes", 0, 0))
    return np.stack(rows), why


def adversarial768():
    """d = 768, hmax = 3 (blocks of 192 bits, keys of 32): a pair that agrees on block 1's key and differs only in that block's tail"""
    rng = np.random.default_rng(768)
    a = rng.integers(0, 256, 96, dtype=np.uint8)
    return np.stack([a, _flip(a, [192 + 32, 192 + 100, 192 + 191])])      # h = 3, every key equal


# ---- block shapes that can go wrong: 512 rows each ------------------------------------------------------------------------------

def _near_copies(rng, n, d, hmax, beyond_bit=None):
    """n rows of d bits (packed, zero padded): half random, half copies of them with 0 .. hmax + 2 flipped bits"""
    bits = rng.integers(0, 2, (n, d), dtype=np.uint8)
    for k in range(n // 2, n):
        bits[k] = bits[rng.integers(0, n // 2)]
        flips = rng.choice(d, rng.integers(0, min(hmax + 3, d + 1)), replace=False)
        if beyond_bit is not None:
            flips = flips[(flips % beyond_bit[0]) >= beyond_bit[1]]      # only behind the first bits of a block
        bits[k, flips] ^= 1
    return bits


@functools.lru_cache(maxsize=None)
def shape(name):
    """name -> (codes, d, hmax); codes packed uint8, or a float array for '100f'"""
    rng = np.random.default_rng(sum(map(ord, name)))
    if name == "96":
        d, hmax, out = 96, 4, np.packbits(_near_copies(rng, 512, 96, 4), axis=1)
    elif name == "100f":                        # d no multiple of 8: only a float array has such a width
        d, hmax = 100, 6
        out = np.where(_near_copies(rng, 512, 100, 6) > 0, 1.0, -1.0).astype(np.float32)
    elif name == "64w1":                        # blocks of ONE bit
        d, hmax, out = 64, 63, np.packbits(_near_copies(rng, 512, 64, 63), axis=1)
    elif name == "64h0":                        # one block wider than a key; 40 % repeated rows
        d, hmax = 64, 0
        bits = rng.integers(0, 2, (512, 64), dtype=np.uint8)
        rep = rng.choice(512, 205, replace=False)
        bits[rep] = bits[rng.integers(0, 40, 205)]
        bits[5, 40] ^= 1                        # and rows that differ from a repeated one behind the key's 32 bits
        bits[6] = bits[rep[0]]
        bits[6, 63] ^= 1
        out = np.packbits(bits, axis=1)
    elif name == "768":                         # blocks of 192 bits: planted pairs that differ only beyond a block's first 32
        d, hmax, out = 768, 3, np.packbits(_near_copies(rng, 512, 768, 3, beyond_bit=(192, 32)), axis=1)
    elif name == "4104":
        d, hmax, out = 4104, 205, np.packbits(_near_copies(rng, 512, 4104, 205), axis=1)
    elif name == "adversarial":                 # the hand-built pairs among random rows
        d, hmax = 64, 3
        out = rng.integers(0, 256, (512, 8), dtype=np.uint8)
        adv, _ = adversarial64()
        out[rng.choice(512, len(adv), replace=False)] = adv
    else:
        raise KeyError(name)
    out.setflags(write=False)
    return out, d, hmax


SHAPES = ("96", "100f", "64w1", "64h0", "768", "4104", "adversarial")


def packed(codes):
    """what the device makes of a float array: bit = x > 0, np.packbits order, zero padded"""
    return codes if codes.dtype == np.uint8 else np.packbits(codes > 0, axis=1)


@functools.lru_cache(maxsize=None)
def heavy():
    """700 copies of one code among 1 300 random ones, shuffled: d = 64, hmax = 3; 244 650 pairs among the copies alone"""
    rng = np.random.default_rng(700)
    x = rng.integers(0, 256, (2000, 8), dtype=np.uint8)
    x[rng.choice(2000, 700, replace=False)] = x[0]
    x.setflags(write=False)
    return x

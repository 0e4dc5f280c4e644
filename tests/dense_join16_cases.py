"""What the K22 tests share (tests/test_dense_join16_cpu.py, tests/test_dense_join16_gpu.py): the search copy of a row emulated in
numpy -- round16(x[k] * inv32), to nearest even -- the margin formula restated, and the rows the rounding term is held on."""
import math

import numpy as np

DTYPES = ("bfloat16", "float16")
U = {"bfloat16": 2.0 ** -8, "float16": 2.0 ** -11}
CHUNK = 64                     # the 16-bit k-chunk: a handle's width is padded to a multiple of it


def padded(dim):
    return -(-dim // CHUNK) * CHUNK


def rounding_term(dtype, ld):
    """the first term of eps: what rounding the two unit vectors to 16 bits can move their cosine by"""
    return 2.0 * math.asin(U[dtype] + 2.0 ** -24 + math.sqrt(ld) * 2.0 ** -25)


def accumulation_term(ld):
    """the second term of eps: the fp32 accumulation of the matrix core (an assumption), the two row factors, the last rounding"""
    return (ld + 8) * 2.0 ** -23


def margin(dtype, ld):
    return rounding_term(dtype, ld) + accumulation_term(ld)


def round_bf16(a):
    """float32 -> bfloat16 to nearest even by bit arithmetic, back as float32 (finite input)"""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
    return r.astype(np.uint32).view(np.float32)


def round16(a, dtype):
    return round_bf16(a) if dtype == "bfloat16" else np.asarray(a, np.float32).astype(np.float16).astype(np.float32)


def inv_norm32(x):
    """1 / ||row|| as the device keeps it: a float64 sum of squares, the reciprocal root rounded to float32 (0 for a row of zeros)"""
    ss = (np.asarray(x, np.float64) ** 2).sum(axis=1)
    return np.where(ss > 0, 1.0 / np.sqrt(np.where(ss > 0, ss, 1.0)), 0.0).astype(np.float32)


def search_copy(x, dtype):
    """the rows of the 16-bit search copy of float32 rows x, as float32: round16(x[k] * inv32), the product in float32"""
    x = np.asarray(x, np.float32)
    return round16(x * inv_norm32(x)[:, None], dtype)


def cosines64(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    na, nb = np.sqrt((a * a).sum(1)), np.sqrt((b * b).sum(1))
    return (a @ b.T) / np.outer(np.where(na > 0, na, 1.0), np.where(nb > 0, nb, 1.0))


def gaussian_rows(n, d, seed, tiny=0):
    """n Gaussian rows; the last `tiny` columns scaled by 2^-13, so that the unit vector's values there lie below float16's 2^-14"""
    x = np.random.default_rng(seed).standard_normal((n, d))
    if tiny:
        x[:, d - tiny:] *= 2.0 ** -13
    return x.astype(np.float32)


def decaying_rows(n, d, seed, decay=0.7):
    """n Gaussian rows whose column k is scaled by decay^k: the energy of a row sits in a few columns, so its cosines move with the
    rounding of a few values and come much nearer the rounding term than those of plain Gaussian rows of the same width"""
    return (np.random.default_rng(seed).standard_normal((n, d)) * decay ** np.arange(d)).astype(np.float32)


def half_ulp_rows(n, d, dtype, seed, tiny=0):
    """Adversarial unit rows: every value of the pre-scaled row lies half a 16-bit ulp above (in magnitude) a value the type holds,
    where rounding costs the most.  Columns 0 .. d - 2 are snapped to such points on a vector of norm sqrt(1 - 0.15^2); the last
    column closes the norm and is snapped too, which leaves the norm within 1e-4 of 1 and so every value within a few hundredths
    of an ulp of its half-way point."""
    p, emin = (7, -126) if dtype == "bfloat16" else (10, -14)

    def snap(y):
        m = np.abs(y)
        e = np.maximum(np.floor(np.log2(np.where(m > 0, m, 1.0))), emin)
        ulp = 2.0 ** (e - p)
        return np.sign(y) * (np.floor(m / ulp) + 0.5) * ulp
    g = np.random.default_rng(seed).standard_normal((n, d - 1))
    if tiny:
        g[:, :tiny] *= 2.0 ** -13
    g *= math.sqrt(1.0 - 0.15 ** 2) / np.sqrt((g * g).sum(1, keepdims=True))
    y = snap(g)
    last = snap(np.sqrt(1.0 - (y * y).sum(1)))
    out = np.concatenate([y, last[:, None]], axis=1)
    assert np.array_equal(out.astype(np.float32).astype(np.float64), out)          # the half-way points are float32 values
    return out.astype(np.float32)

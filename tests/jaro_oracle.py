"""The definition K8 is held to: jellyfish's jaro_similarity / jaro_winkler_similarity with their default arguments,
restated on Unicode code points in plain Python (float64, the definition's order of operations).  PARITY UNPINNED:
jellyfish is not importable where this was written; tests/test_jaro_cpu.py compares with it wherever it is.
Test code only -- the package never imports this module."""
import numpy as np


def _jaro(a, b, winkler):
    la, lb = len(a), len(b)
    if la == 0 or lb == 0:
        return 0.0                                  # also when both are empty
    r = max(max(la, lb) // 2 - 1, 0)
    flag_a, flag_b = [False] * la, [False] * lb
    m = 0
    for i in range(la):
        for j in range(max(0, i - r), min(i + r, lb - 1) + 1):
            if not flag_b[j] and b[j] == a[i]:
                flag_a[i] = flag_b[j] = True
                m += 1
                break
    if m == 0:
        return 0.0
    fa = [a[i] for i in range(la) if flag_a[i]]
    fb = [b[j] for j in range(lb) if flag_b[j]]
    t = sum(x != y for x, y in zip(fa, fb)) // 2
    w = (m / la + m / lb + (m - t) / m) / 3
    if winkler and w > 0.7:
        l = 0
        while l < min(la, lb, 4) and a[l] == b[l]:
            l += 1
        w = w + (l * 0.1) * (1.0 - w)
    return w


def jaro_similarity(a, b):
    return _jaro(a, b, False)


def jaro_winkler_similarity(a, b):
    return _jaro(a, b, True)


SCORERS = {"jaro": jaro_similarity, "jaro_winkler": jaro_winkler_similarity}


def matrix(from_list, to_list, scorer):
    """every score, float64 [len(from_list), len(to_list)]; equal strings are scored once"""
    f = SCORERS[scorer]
    memo = {}
    out = np.empty((len(from_list), len(to_list)), np.float64)
    for i, a in enumerate(from_list):
        for j, b in enumerate(to_list):
            k = (a, b)
            if k not in memo:
                memo[k] = f(a, b)
            out[i, j] = memo[k]
    return out


def left_out(choice, skip):
    """the skip codes of the best-choice kernels: skip >= 0 leaves that choice out, skip <= -2 every choice up to -2 - skip"""
    return choice == skip or choice <= -2 - skip


def argmax(m, skip=None):
    """(first arg-max int32[n], score float64[n]) of a score matrix as np.argmax gives it (reference _distance.py:97-100) over
    the choices `skip` leaves in; a row without a choice gets -1 / 0.0"""
    idx, score = np.full(len(m), -1, np.int32), np.zeros(len(m))
    for i, row in enumerate(m):
        keep = [j for j in range(len(row)) if skip is None or not left_out(j, int(skip[i]))]
        if keep:
            k = int(np.argmax(row[keep]))
            idx[i], score[i] = keep[k], row[keep[k]]
    return idx, score

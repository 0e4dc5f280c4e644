"""The lists of K25's GPU tests (tests/test_simhash_gpu.py, tests/test_simhash_pool_fill_gpu.py) and the numpy helpers they share."""
import functools

import numpy as np

from polyfuzz_amd.models._tfidf import _clean_string

PUNCT = "!?.,;:-_()[]{}#*+/&%$'\""


def cleaned_to(length, seed):
    """a raw string with capitals, punctuation and runs of spaces whose cleaned form has exactly `length` symbols"""
    rng = np.random.default_rng(seed)
    core = ""
    while len(core) < length:
        core += "".join(rng.choice(list("abcdefghij0123"), int(rng.integers(1, 9)))) + " "
    core = core[:length]
    if core.endswith(" "):
        core = core[:-1] + "z"
    raw = ""
    for ch in core:
        raw += ch.upper() if rng.random() < 0.2 else ch
        if rng.random() < 0.15:
            raw += str(rng.choice(list(PUNCT)))
        if ch == " " and rng.random() < 0.5:
            raw += "  "
    raw = "  ." + raw + "! "
    assert len(_clean_string(raw)) == length and _clean_string(raw) == core
    return raw


@functools.lru_cache(maxsize=None)
def edge_strings():
    out = ["", " ", "ab", "abc", "!!!", "Apple  Inc.", "abcabc"]
    out += [cleaned_to(n, 100 + n) for n in (63, 64, 65, 66, 127, 128, 129, 300)]
    out += ["a" * 62 + "bcd",                       # windows that straddle a 64-character step
            "x" + " " * 70 + "y z",                 # a pending space carried across a step
            (PUNCT * 9)[:200],                      # long raw, empty cleaned
            (PUNCT * 5)[:100] + "abc"]
    assert len(out[-2]) == 200 and _clean_string(out[-2]) == "" and _clean_string(out[-1]) == "abc"
    return tuple(out)


@functools.lru_cache(maxsize=None)
def boundary_strings():
    """a space pending at a step's border in front of a step that is full of kept characters and single spaces: the step then holds one
    symbol more than it has units.  Built for borders at 62 .. 65 units, whatever the step's size is; then text without punctuation"""
    out = []
    for size in (62, 63, 64, 65):
        first = "x" + " " * (size - 1) + "a" * size
        out += [first, first + " tail of more text", first + " " + "b" * size + " c",
                "x" * (size - 1) + " " + ("a b " * 40)[:size] + "cd", "x" + " " * (size - 1) + ("ab " * 40)[:size] + "x" * 70]
    out += [("the quick brown fox jumps over the lazy dog " * 6)[:n] for n in (126, 127, 128, 129, 190, 256)]
    rng = np.random.default_rng(65)
    out += ["".join(rng.choice(list("ab "), int(n))) for n in rng.integers(120, 330, 60)]
    out += ["a" * 300, " " * 130 + "abc", "abc" + " " * 130, "a" + " " * 62 + "b" + " " * 62 + "c" + " " * 62 + "def"]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def names(n=3000):
    from polyfuzz_amd import datasets
    return tuple(datasets.load_company_names()[:n])


@functools.lru_cache(maxsize=None)
def list257():
    """the edge strings, then company names, the last string without a window: 64 full workgroups and one of a single wave"""
    out = list(edge_strings()) + list(names(257 - len(edge_strings()) - 1)) + ["a."]
    assert len(out) == 257
    return tuple(out)


# windowless strings at the start, in the middle and at the end; every string and none; one, three, four and five strings: the last
# workgroup holds one to four waves with a string
SMALL_LISTS = {
    "one": ("abcd",),
    "one_windowless": ("ab",),
    "start": ("", "abcd", "abce"),
    "middle": ("abcd", "a b", "abce", "abcf"),
    "end": ("abcd", "abce", "abcf", "abcg", "!!!"),
    "all_windowless": ("", " ", "ab", "!!!", "a"),
    "none_windowless": ("abcd", "abce", "abcf", "Apple  Inc."),
    "empty": (),
}

WIDE = ("Zażółć gęślą", "Ελληνικά γράμματα και άλλα", "日本語のテキスト", "ab", "", "żó", "naïve café Ω",
        "Ω" * 63 + "αβγ", "ж" * 64 + "abc", ("дом " * 40).strip(), "x" + " " * 70 + "ÿ ż")


def popcounts(x, y):
    """int64 [len(x), len(y)] Hamming distances of packed uint8 rows"""
    table = np.array([bin(v).count("1") for v in range(256)], np.int64)
    out = np.empty((len(x), len(y)), np.int64)
    for r0 in range(0, len(x), 256):
        out[r0:r0 + 256] = table[x[r0:r0 + 256, None, :] ^ y[None, :, :]].sum(axis=2)
    return out


def union_find_labels(n, rows, cols):
    """label[i] = the smallest member of i's component under the edges (rows[p], cols[p])"""
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a
    for a, b in zip(rows.tolist(), cols.tolist()):
        ra, rb = find(a), find(b)
        if ra != rb:
            parent[max(ra, rb)] = min(ra, rb)
    return np.array([find(i) for i in range(n)], np.int32)

"""Interface parity with the reference package, held against its recorded interface (tests/golden/reference_interface.json,
made by tests/golden/make_golden_interface.py from a PolyFuzz v0.4.3 checkout, with the two absent third-party modules stubbed
exactly as tests/golden/make_golden.py does).

The mirrors are imported in a child process and compared with the record: constructor / match() signatures (names, order,
defaults), the public attributes of a default-constructed matcher, the function signatures of cosine_similarity /
single_linkage / precision_recall_curve, the Embeddings signatures as the reference's source states them, and the plug-in
relation the facade tests with isinstance (polyfuzz/polyfuzz.py:141-152): the BaseMatcher the matchers subclass is the
reference's ABC (same abstract methods, same signatures), the facade's own check accepts them (tests/facade_standin.py), and
the record holds what the real facade did with them when it was made.  No device call is made.
"""
import json
import os
import subprocess
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(REPO, "tests", "golden", "reference_interface.json")


def sig(f):
    """[name, kind, default] per parameter; a callable default by its name"""
    import inspect
    out = []
    for name, p in inspect.signature(f).parameters.items():
        d = p.default
        if d is inspect.Parameter.empty:
            d = "<required>"
        elif callable(d):
            d = "callable:" + getattr(d, "__name__", "?")
        out.append([name, str(p.kind), repr(d) if not isinstance(d, str) else d])
    return out


def base_info(cls):
    """what a plug-in matcher is held to: the ABC's abstract methods and its two signatures"""
    return {"abstract": sorted(cls.__abstractmethods__), "init": sig(cls.__init__), "match": sig(cls.match)}


CHILD = r"""
import json, sys
sys.path.insert(0, %(repo)r)
import polyfuzz_amd.models as ours
from polyfuzz_amd.models import cosine_similarity as our_cos
from polyfuzz_amd.linkage import single_linkage as our_link
from polyfuzz_amd.metrics import precision_recall_curve as our_pr
from tests.facade_standin import FacadeStandIn
from tests.test_reference_interface_cpu import sig, base_info

res = {"sig": {}, "rel": {}}
for cls in ("TFIDF", "EditDistance", "RapidFuzz", "Embeddings"):
    o = getattr(ours, cls)
    res["sig"][cls + ".__init__"] = sig(o.__init__)
    res["sig"][cls + ".match"] = sig(o.match)
    res["rel"][cls + " is a BaseMatcher"] = issubclass(o, ours.BaseMatcher)
res["sig"]["cosine_similarity"] = sig(our_cos)
res["sig"]["single_linkage"] = sig(our_link)
res["sig"]["precision_recall_curve"] = sig(our_pr)
m = ours.TFIDF(n_gram_range=(3, 3), min_similarity=0, top_n=2, model_id="hip")
res["rel"]["the facade's check keeps the instance"] = FacadeStandIn(m).method is m
res["base"] = base_info(ours.BaseMatcher)
res["attrs"] = {c: sorted(k for k in dir(getattr(ours, c)()) if not k.startswith("_"))     # (properties included, not evaluated)
                for c in ("TFIDF", "EditDistance", "RapidFuzz")}
print("RESULT" + json.dumps(res))
"""


@pytest.fixture(scope="module")
def recorded():
    with open(GOLDEN) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def report():
    env = dict(os.environ, PYTHONPATH="")
    p = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO}], capture_output=True, text=True, env=env, timeout=300,
                       cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1]
    return json.loads(line[len("RESULT"):])


def _names(sig):
    return [(n, k) for n, k, _ in sig]


def test_matchers_plug_into_the_reference_facade(report, recorded):
    for what, ok in recorded["rel"].items():          # what the real facade did with the mirrors when the record was made
        assert ok, what
    for what, ok in report["rel"].items():
        assert ok, what
    assert report["base"] == recorded["base"], (report["base"], recorded["base"])


@pytest.mark.parametrize("cls", ["TFIDF", "EditDistance", "RapidFuzz"])
def test_constructor_and_match_signatures_equal_the_reference(report, recorded, cls):
    ref_init, our_init = recorded["sig"][cls + ".__init__"], report["sig"][cls + ".__init__"]
    assert _names(ref_init) == _names(our_init), (ref_init, our_init)
    for (n, _, d_ref), (_, _, d_our) in zip(ref_init, our_init):
        if n == "scorer":
            # documented deviation: the default is the NAME of the reference's default callable (rapidfuzz is not a
            # dependency of this package); both resolve to the same device scorer
            assert (cls, d_ref, d_our) in (("EditDistance", "callable:ratio", "ratio"),
                                           ("RapidFuzz", "callable:WRatio", "None")), (cls, d_ref, d_our)
        else:
            assert d_ref == d_our, (cls, n, d_ref, d_our)
    ref_match, our_match = recorded["sig"][cls + ".match"], report["sig"][cls + ".match"]
    assert _names(ref_match) == _names(our_match), (ref_match, our_match)
    assert [d for _, _, d in ref_match] == [d for _, _, d in our_match]
    # every public attribute the reference's instance carries is there (equal_lists is internal state of its loops)
    missing = set(recorded["ref_attrs"][cls]) - set(report["attrs"][cls]) - {"equal_lists"}
    assert not missing, missing


@pytest.mark.parametrize("fn", ["cosine_similarity", "single_linkage", "precision_recall_curve"])
def test_function_signatures_equal_the_reference(report, recorded, fn):
    ref_sig, our_sig = recorded["sig"][fn], report["sig"][fn]
    assert _names(ref_sig) == _names(our_sig), (ref_sig, our_sig)
    assert [d for _, _, d in ref_sig] == [d for _, _, d in our_sig], (ref_sig, our_sig)


def test_embeddings_signature_equals_the_reference_source(report, recorded):
    """polyfuzz.models.Embeddings needs flair (absent): its signatures were read from the source when the record was made."""
    for fn_name in ("__init__", "match"):
        names, defaults = recorded["embeddings"][fn_name]["names"], recorded["embeddings"][fn_name]["defaults"]
        ours = report["sig"]["Embeddings." + fn_name]
        assert names == [n for n, _, _ in ours], (names, ours)
        our_defaults = [d for _, _, d in ours if d != "<required>"]
        assert defaults == our_defaults, (defaults, our_defaults)

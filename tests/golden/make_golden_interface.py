"""
Record the reference package's public interface into tests/golden/reference_interface.json, so that
tests/test_reference_interface_cpu.py holds the mirrors against it wherever the tests run:

    python tests/golden/make_golden_interface.py <path of a PolyFuzz v0.4.3 checkout>

What is recorded is data: the parameter lists (name, kind, default) of the matchers' constructors and match(), of
cosine_similarity / single_linkage / precision_recall_curve and of the BaseMatcher ABC, the public attributes a
default-constructed matcher carries, the Embeddings signatures as its source states them (it needs flair to import), and the
facade relations observed with the real package (our matchers imported AFTER it subclass its BaseMatcher and PolyFuzz keeps
them as custom models, polyfuzz/polyfuzz.py:141-152).  The two absent third-party modules are stubbed as make_golden.py does.
"""
import ast
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_interface.json")

CHILD = r"""
import inspect, json, sys, types
sys.path.insert(0, %(repo)r)
from tests.test_reference_interface_cpu import sig, base_info    # (before the checkout's own tests/ is on the path)
sys.path.insert(0, %(ref)r)
sns = types.ModuleType("seaborn"); sys.modules["seaborn"] = sns
rf = types.ModuleType("rapidfuzz"); fuzz = types.ModuleType("rapidfuzz.fuzz"); process = types.ModuleType("rapidfuzz.process")
def ratio(a, b, **kw): return 0.0
def WRatio(a, b, **kw): return 0.0
ratio.__module__ = WRatio.__module__ = "rapidfuzz.fuzz"
fuzz.ratio, fuzz.WRatio = ratio, WRatio
process.extractOne = lambda *a, **k: None
rf.fuzz, rf.process = fuzz, process
sys.modules.update({"rapidfuzz": rf, "rapidfuzz.fuzz": fuzz, "rapidfuzz.process": process})

import polyfuzz                                   # the reference, first
from polyfuzz import PolyFuzz
import polyfuzz.models as ref
from polyfuzz.models._utils import cosine_similarity as ref_cos
from polyfuzz.linkage import single_linkage as ref_link
from polyfuzz.metrics import precision_recall_curve as ref_pr
import polyfuzz_amd.models as ours

res = {"sig": {}, "rel": {}}
for cls in ("TFIDF", "EditDistance", "RapidFuzz"):
    r, o = getattr(ref, cls), getattr(ours, cls)
    res["sig"][cls + ".__init__"] = sig(r.__init__)
    res["sig"][cls + ".match"] = sig(r.match)
    res["rel"][cls + " is a reference BaseMatcher"] = issubclass(o, ref.BaseMatcher)
res["rel"]["Embeddings is a reference BaseMatcher"] = issubclass(ours.Embeddings, ref.BaseMatcher)
res["rel"]["BaseMatcher is the reference's"] = ours.BaseMatcher is ref.BaseMatcher
res["sig"]["cosine_similarity"] = sig(ref_cos)
res["sig"]["single_linkage"] = sig(ref_link)
res["sig"]["precision_recall_curve"] = sig(ref_pr)
m = ours.TFIDF(n_gram_range=(3, 3), min_similarity=0, top_n=2, model_id="hip")
pf = PolyFuzz(m)
res["rel"]["PolyFuzz(TFIDF) keeps the instance"] = pf.method is m and isinstance(pf.method, ref.BaseMatcher)
res["rel"]["PolyFuzz([...]) keeps the instances"] = all(
    isinstance(x, ref.BaseMatcher) for x in PolyFuzz([ours.TFIDF(model_id="a"), ours.EditDistance(model_id="b"),
                                                       ours.RapidFuzz(model_id="c")]).method)
res["base"] = base_info(ref.BaseMatcher)
res["ref_attrs"] = {c: sorted(k for k in vars(getattr(ref, c)()).keys() if not k.startswith("_"))
                    for c in ("TFIDF", "EditDistance", "RapidFuzz")}
print("RESULT" + json.dumps(res))
"""


def embeddings_signatures(ref):
    """polyfuzz.models.Embeddings needs flair: its parameter names and defaults as the source states them"""
    with open(os.path.join(ref, "polyfuzz", "models", "_embeddings.py")) as f:
        tree = ast.parse(f.read())
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "Embeddings")
    out = {}
    for fn_name in ("__init__", "match"):
        fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == fn_name)
        defaults = [ast.literal_eval(d) for d in fn.args.defaults]
        out[fn_name] = {"names": [a.arg for a in fn.args.args],
                        "defaults": [repr(d) if not isinstance(d, str) else d for d in defaults]}
    return out


def main(ref):
    env = dict(os.environ, PYTHONPATH="")
    p = subprocess.run([sys.executable, "-c", CHILD % {"repo": REPO, "ref": ref}], capture_output=True, text=True, env=env,
                       timeout=300, cwd=REPO)
    assert p.returncode == 0, p.stderr[-3000:]
    res = json.loads([ln for ln in p.stdout.splitlines() if ln.startswith("RESULT")][-1][len("RESULT"):])
    res["embeddings"] = embeddings_signatures(ref)
    res = {"reference": "MaartenGr/PolyFuzz v0.4.3, recorded by tests/golden/make_golden_interface.py", **res}
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", OUT)


if __name__ == "__main__":
    if len(sys.argv) != 2 or not os.path.isdir(os.path.join(sys.argv[1], "polyfuzz")):
        raise SystemExit("usage: python tests/golden/make_golden_interface.py <path of a PolyFuzz v0.4.3 checkout>")
    main(os.path.abspath(sys.argv[1]))

"""pfz_pool_fill without a GPU: the entry in header, library and ctypes table with its three patterns and its blind spot stated,
the modes named beside the binding, the allocator's promise in DESIGN.md, and polyfuzz_amd/csrc/pool_class.h -- the size classes
the fill is written over -- compiled for the host as a stand-alone program (tests/pool_class_host.cpp) and run, once plain and once
under the host's address and undefined-behaviour sanitizers."""
import ctypes
import os
import re
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
PATTERNS = {1: ("ZERO", 0x0000000000000000), 2: ("ONE64", 0x0000000000000001), 3: ("ONE32", 0x0000000100000001)}


def _read(*parts):
    with open(os.path.join(REPO, *parts), encoding="utf-8") as f:
        return f.read()


def test_the_entry_is_declared_with_its_patterns_and_its_blind_spot():
    header = _read("include", "polyfuzz_hip.h")
    m = re.search(r"/\*((?:(?!\*/).)*?)\*/\s*int pfz_pool_fill\(pfz_ctx \*ctx, int32_t mode\);", header, flags=re.S)
    assert m, "pfz_pool_fill is not declared behind a comment of its own"
    text = " ".join(m.group(1).replace("*", " ").split())
    for mode, (name, word) in PATTERNS.items():
        assert re.search(rf"\b{mode} {name} 0x{word:016x}\b", text), (mode, name)
    for phrase in ("UNSPECIFIED", "does not clear", "one branch per allocation", "BLIND SPOT", "denormals",
                   "float accumulator that is not cleared is NOT detected", "PFZ_ERR_INVALID", "pinned staging buffers"):
        assert phrase in text, phrase


def test_the_entry_is_bound_and_exported_and_the_modes_are_named():
    from polyfuzz_amd import _build, _lib
    if _build.is_stale():
        _build.build()
    assert _lib.SIGNATURES["pfz_pool_fill"] == (ctypes.c_int, [ctypes.c_void_p, ctypes.c_int32])
    assert hasattr(ctypes.CDLL(_lib.lib_path()), "pfz_pool_fill")
    from tests.test_abi_cpu import _declared_symbols
    assert "pfz_pool_fill" in _declared_symbols() and sorted(_lib.SIGNATURES) == _declared_symbols()
    c = _lib.Context
    assert (c.POOL_FILL_OFF, c.POOL_FILL_ZERO, c.POOL_FILL_ONE64, c.POOL_FILL_ONE32) == (0, 1, 2, 3)
    assert c.POOL_FILL_WORDS == {mode: word for mode, (_, word) in PATTERNS.items()}
    assert callable(c.pool_fill)
    from tests import pool_fill_cases as cases
    assert cases.FILLS == tuple((name, mode) for mode, (name, _) in PATTERNS.items())
    # a NULL context is refused before any device call, like every entry
    lib = _lib.load()
    assert lib.pfz_pool_fill(None, 1) == -1 and b"pfz_pool_fill" in lib.pfz_last_error()


def test_there_is_no_environment_knob_and_one_choke_point():
    """the fill is per context and switched at run time; it is applied where every block is handed out, and nowhere else"""
    knobs = _read("polyfuzz_amd", "csrc", "pfz_knobs.h")
    assert "POOL_FILL" not in knobs.upper().replace("POOL_FILL_MODE", "")
    api = _read("polyfuzz_amd", "csrc", "pfz_api.hip")
    assert api.count("pool_fill_block(") == 2                      # its definition and the one call in pool_alloc_raw
    body = api[api.index("int pool_alloc_raw("):api.index("void pool_free(")]
    assert "pool_fill_block(" in body and "g_pool_mu" not in body    # (the lock is pool_take's: released before the fill waits)
    assert "hipStreamSynchronize(ctx->stream)" in api[api.index("static int pool_fill_block("):api.index("static int pool_take(")]
    csrc = os.path.join(REPO, "polyfuzz_amd", "csrc")
    users = [f for f in sorted(os.listdir(csrc)) if f.endswith((".hip", ".h")) and re.search(r"\bpool_fill_mode\b", _read("polyfuzz_amd", "csrc", f))]
    assert users == ["pfz_api.hip", "pfz_internal.h"], users


def test_design_states_the_promise_the_patterns_and_what_was_found():
    design = _read("DESIGN.md")
    at = design.index("## The allocator's promise and the pool fill mode")
    section = design[at:]
    nxt = re.search(r"^## ", section[3:], flags=re.M)
    section = section[:nxt.start() + 3] if nxt else section
    flat = " ".join(section.split())
    assert "contents are unspecified; mode 0 does not clear" in flat
    for mode, (name, word) in PATTERNS.items():
        assert name in flat and f"0x{word:016x}" in flat
    assert "float accumulator" in flat and "denormal" in flat
    assert re.search(r"^\| *site *\| *symptom *\| *fix *\|", section, flags=re.M | re.I) or "none found" in flat


# ---- pool_class.h on the host ----------------------------------------------------------------------------------------------------

def _host_program(tag, flags):
    exe = os.path.join(REPO, "oracle", "_build", f"pool_class_host_{tag}")
    src = [os.path.join(HERE, "pool_class_host.cpp"), os.path.join(REPO, "polyfuzz_amd", "csrc", "pool_class.h")]
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    if not os.path.exists(exe) or any(os.path.getmtime(s) > os.path.getmtime(exe) for s in src):
        subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + [src[0], "-o", exe])
    return exe


def _run_host_program(exe):
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stdout + out.stderr
    words = out.stdout.split()
    assert words[:2] == ["pool_class_host", "ok"] and int(words[2]) > 260_000 and int(words[3]) > 140, out.stdout


def test_size_classes_are_multiples_of_8_and_cover_the_request():
    _run_host_program(_host_program("plain", ["-O2"]))


def test_the_same_program_under_the_host_sanitizers():
    try:
        exe = _host_program("san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"])
    except subprocess.CalledProcessError:
        pytest.skip("this g++ cannot link -fsanitize=address,undefined")
    _run_host_program(exe)

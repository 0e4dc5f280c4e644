"""Registers, LDS and scratch of every gfx950 kernel in the built library (the code objects' own metadata).
usage: python tools/kernel_budget.py [libpolyfuzz_hip.so] [name filter]
       python tools/kernel_budget.py --digest [libpolyfuzz_hip.so]     one sha256 of the device code per translation unit
       python tools/kernel_budget.py --digest [libpolyfuzz_hip.so] k8_jaro.hip     one sha256 per kernel of that unit, by name:
                                                                       the same lines when only the kernels' order in the unit moved

Why: round 3 found K7 and K3 sitting ON occupancy steps -- 256 B of LDS more cost K7 a workgroup per CU and 5 %, K3 4.4 %
(DESIGN.md, K7 / "What comes next") -- and nothing but this metadata says when an edit crosses one.
tests/test_kernel_budget_cpu.py holds the budgets of the kernels where it matters."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"
TARGET = "hipv4-amdgcn-amd-amdhsa--gfx950"


def code_objects(lib, d):
    """the gfx950 code objects of the linked library, unbundled into directory d: one path per translation unit, in link order"""
    fat = os.path.join(d, "fat.bin")
    subprocess.check_call([f"{LLVM}/llvm-objcopy", "--dump-section", f".hip_fatbin={fat}", lib, os.path.join(d, "copy.so")])
    blob = open(fat, "rb").read()
    # one offload bundle per translation unit, back to back
    starts = [m.start() for m in re.finditer(re.escape(b"__CLANG_OFFLOAD_BUNDLE__"), blob)]
    out = []
    for k, a in enumerate(starts):
        piece, co = os.path.join(d, f"b{k}.bin"), os.path.join(d, f"b{k}.co")
        with open(piece, "wb") as f:
            f.write(blob[a:starts[k + 1] if k + 1 < len(starts) else len(blob)])
        r = subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={piece}", f"--targets={TARGET}",
                            f"--output={co}"], capture_output=True)
        if r.returncode or not os.path.exists(co) or os.path.getsize(co) == 0:
            continue
        out.append(co)
    return out


def kernel_metadata(lib):
    """{mangled kernel name: {vgpr, sgpr, lds (static bytes), scratch (bytes per lane)}}"""
    out = {}
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
            cur = {}
            for line in notes.splitlines():
                m = re.match(r"\s*-?\s*\.(\w+):\s*(.*)$", line)
                if not m:
                    continue
                key, val = m.group(1), m.group(2).strip().strip("'")
                if key in ("group_segment_fixed_size", "private_segment_fixed_size", "sgpr_count", "vgpr_count", "agpr_count"):
                    # (vgpr_count is the lane's whole unified register file, the accumulation registers included; agpr_count
                    # says how many of them are accumulation registers)
                    cur[{"group_segment_fixed_size": "lds", "private_segment_fixed_size": "scratch", "sgpr_count": "sgpr",
                         "vgpr_count": "vgpr", "agpr_count": "agpr"}[key]] = int(val)
                elif key == "name":
                    cur["name"] = val
                elif key == "wavefront_size":           # (the last key of a kernel's record)
                    if "name" in cur:
                        out[cur.pop("name")] = cur
                    cur = {}
    return out


def device_digests(lib):
    """one sha256 per translation unit over its code object's .text, .rodata and kernel metadata (llvm-readelf --notes): a
    change of host code alone leaves every line as it was"""
    import hashlib
    out = []
    with tempfile.TemporaryDirectory() as d:
        for co in code_objects(lib, d):
            h = hashlib.sha256()
            for sec in (".text", ".rodata"):
                dump = co + sec
                subprocess.run([f"{LLVM}/llvm-objcopy", "--dump-section", f"{sec}={dump}", co, co + ".copy"], capture_output=True)
                h.update(open(dump, "rb").read() if os.path.exists(dump) else b"")
            h.update(subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True).stdout)
            out.append(h.hexdigest())
    return out


def kernel_digests(lib, unit_index):
    """{kernel symbol: sha256 of its disassembly, addresses and encodings left out} of one translation unit: the order in which a
    unit's templates are instantiated (host code decides it) moves its kernels and the unit's digest, not these"""
    import hashlib
    out, cur = {}, None
    with tempfile.TemporaryDirectory() as d:
        co = code_objects(lib, d)[unit_index]
        dis = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", "--no-leading-addr", co], capture_output=True, text=True).stdout
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]* ?<(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), hashlib.sha256())
        elif cur is not None:
            cur.update(re.sub(r"//.*$", "", line).strip().encode() + b"\n")
    return {k: h.hexdigest() for k, h in out.items()}


def demangled(names):
    import shutil
    exe = shutil.which("c++filt")
    if not exe:
        return list(names)
    r = subprocess.run([exe], input="\n".join(names), capture_output=True, text=True)
    return r.stdout.splitlines() if r.returncode == 0 else list(names)


if __name__ == "__main__":
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from polyfuzz_amd import _build
    args = [a for a in sys.argv[1:] if a != "--digest"]
    lib = args[0] if args and args[0].endswith(".so") else _build.LIB_PATH
    flt = [a for a in args if not a.endswith(".so")]
    if "--digest" in sys.argv[1:]:
        units = [os.path.basename(p) for p in _build.sources()]      # (link order)
        if flt:
            per_kernel = kernel_digests(lib, units.index(flt[0]))
            for pretty, n in sorted(zip(demangled(list(per_kernel)), per_kernel)):
                print(per_kernel[n], pretty[:110])
            sys.exit(0)
        for k, h in enumerate(device_digests(lib)):
            print(h, units[k] if k < len(units) else f"unit{k}")
        sys.exit(0)
    md = kernel_metadata(lib)
    names = sorted(md)
    print(f"{'vgpr':>5} {'agpr':>5} {'sgpr':>5} {'lds B':>7} {'scratch':>7}  kernel")
    for n, pretty in zip(names, demangled(names)):
        if flt and not any(f in pretty for f in flt):
            continue
        v = md[n]
        print(f"{v.get('vgpr', -1):5d} {v.get('agpr', 0):5d} {v.get('sgpr', -1):5d} {v.get('lds', -1):7d} {v.get('scratch', -1):7d}  {pretty[:110]}")

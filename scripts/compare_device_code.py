#!/usr/bin/env python3
"""Compare the gfx950 device code of two builds of the library, object by object:

    python scripts/compare_device_code.py <parent>/build/csrc build/csrc [OLD=NEW ...]     (and .../csrc_nofma for the other form)

An object whose code object (the gfx950 entry of its .hip_fatbin section) is byte-identical says so.  Otherwise every symbol of the
code object is compared by name: a kernel's machine code and its 64-byte kernel descriptor (VGPRs, AGPRs, SGPRs, scratch, LDS and
the other occupancy-relevant fields) as raw bytes, so kernels may stand in another order but none may differ, appear or vanish.
Exit status 1 if any symbol differs."""
import hashlib
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("LLVM_BIN", "/opt/rocm/llvm/bin")
def sh(*a): return subprocess.run(a, check=True, capture_output=True, text=True).stdout
def code_object(obj, tmp):
    fb = os.path.join(tmp, "fb"); co = os.path.join(tmp, "co")
    sh(f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb)
    sh(f"{LLVM}/clang-offload-bundler", "--type=o", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--unbundle", f"--input={fb}", f"--output={co}")
    return open(co, "rb").read(), co
def symbols(co):
    secs = {}
    for l in sh(f"{LLVM}/llvm-readelf", "-S", "-W", co).splitlines():
        m = re.match(r"\s*\[\s*(\d+)\]\s+(\S+)\s+\S+\s+([0-9a-f]+)\s+([0-9a-f]+)\s+([0-9a-f]+)", l)
        if m: secs[int(m[1])] = (m[2], int(m[3], 16), int(m[4], 16))
    out = {}
    for l in sh(f"{LLVM}/llvm-readelf", "-s", "-W", co).splitlines():
        f = l.split()
        if len(f) == 8 and f[3] in ("FUNC", "OBJECT") and f[6].isdigit():
            name, addr, size, (sec, saddr, soff) = f[7], int(f[1], 16), int(f[2]), secs[int(f[6])]
            out[name] = (f[3], sec, soff + addr - saddr, size)
    return out
def digest(obj):
    with tempfile.TemporaryDirectory() as tmp:
        raw, co = code_object(obj, tmp)
        syms = symbols(co)
        # a descriptor's bytes 16..23 are the distance from the descriptor to its code (kernel_code_entry_byte_offset): it moves when
        # kernels are emitted in another order and is left out; a __hip_cuid_<hash of the source> symbol is a 1-byte tag, not code
        def body(n, off, size):
            b = raw[off:off + size]
            return b[:16] + b[24:] if n.endswith(".kd") else b
        d = {n: (t, sec, size, hashlib.sha256(body(n, off, size)).hexdigest()) for n, (t, sec, off, size) in syms.items() if not n.startswith("__hip_cuid_")}
        return hashlib.sha256(raw).hexdigest(), d
a, b = sys.argv[1], sys.argv[2]
# further arguments OLD=NEW: substrings of the second build's symbol names rewritten before the comparison, for a change that renames a
# template argument and nothing else (e.g. NS_9MemPolicyILy69905EEE=Lb1E: the policy type where the parent had `bool NT = true`)
renames = [r.split("=", 1) for r in sys.argv[3:]]
def renamed(d):
    out = {}
    for n, v in d.items():
        for old, new in renames: n = n.replace(old, new)
        out[n] = v
    return out
bad = 0
for f in sorted(os.listdir(a)):
    if not f.endswith(".o") or f == "resources.o": continue
    pa, pb = os.path.join(a, f), os.path.join(b, f)
    try: ha, da = digest(pa)
    except subprocess.CalledProcessError: 
        print(f"{f}: no device code"); continue
    hb, db = digest(pb)
    db = renamed(db)
    if ha == hb:
        print(f"{f}: code object byte-identical ({len([n for n in da if n.endswith('.kd')])} kernels)"); continue
    ka, kb = {n for n in da if n.endswith(".kd")}, {n for n in db if n.endswith(".kd")}
    diff = [n for n in sorted(set(da) | set(db)) if da.get(n) != db.get(n)]
    print(f"{f}: code object differs; kernels {len(ka)} vs {len(kb)}, same set: {ka == kb}; symbols that differ: {diff if diff else 'none (code and descriptors equal symbol by symbol)'}")
    bad += bool(diff) or ka != kb
sys.exit(1 if bad else 0)

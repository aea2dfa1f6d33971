#!/usr/bin/env python3
"""Build a libsfmi variant with extra compiler flags into build/abl/ (for tools/ab.py):
    python tools/variant.py NAME [-DSF_MROWS=2 ...] [--only SOURCE FLAG ...]   ->  build/abl/libsfmi_NAME.so
Flags behind `--only SOURCE` go to that one translation unit (e.g. --only sf_kernels.hip -mllvm -amdgpu-sched-strategy=max-ilp);
the others apply to every source."""
import os, subprocess, sys, tempfile
from concurrent.futures import ThreadPoolExecutor
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from spacefortress_amd import build as B
name, rest = sys.argv[1], sys.argv[2:]
only_src, only = None, []
if "--only" in rest:
    k = rest.index("--only")
    only_src, only, rest = rest[k + 1], rest[k + 2:], rest[:k]
    assert only_src in B.SOURCES, only_src
out = os.path.join(ROOT, "build", "abl", "libsfmi_%s.so" % name)
os.makedirs(os.path.dirname(out), exist_ok=True)
cflags = [f for f in B.FLAGS if f != "-shared"] + rest
with tempfile.TemporaryDirectory() as td:
    objs = [os.path.join(td, os.path.splitext(s)[0] + ".o") for s in B.SOURCES]
    one = lambda j: subprocess.check_call(["/opt/rocm/bin/hipcc"] + cflags + (only if j[0] == only_src else []) +
                                          ["-x", "hip", "-c", os.path.join(B.CSRC, j[0]), "-o", j[1]])
    with ThreadPoolExecutor(max_workers=6) as ex:
        list(ex.map(one, zip(B.SOURCES, objs)))
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=" + B.offload_arch(cflags), "-fPIC", "-shared", "--hip-link"] + objs + ["-o", out])
bare = B.scan_wide_store_hazard(B.device_disassembly(out))
assert not bare, ("wide buffer stores without their wait state", bare[:3])
print(out)

#!/usr/bin/env python3
"""The identity of a built library's device code:  python tools/device_code_id.py [lib]
One line per gfx950 code object (one per .hip source, in the build's order): sha256 of its bytes, sha256 of its
disassembly, then one resource line per kernel (as tools/kernel_resources.py prints them).  Two builds whose lines are
equal run the same device code: what a "no device change" claim is checked with (profiles/closed_switches.md)."""
import hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import build as B

llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
lib = sys.argv[1] if len(sys.argv) > 1 else B.LIB
hips = [s for s in B.SOURCES if s.endswith(".hip")]
for n, co in enumerate(B.device_code_objects(lib)):
    dis = B.disassemble_code_object(co)
    dis = dis[dis.index("\n", dis.index("file format")):]  # (the first line names the temporary file)
    print("%-22s bytes %s disasm %s" % (hips[n] if n < len(hips) else "#%d" % n, hashlib.sha256(co).hexdigest(), hashlib.sha256(dis.encode()).hexdigest()))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "code.co")
        open(path, "wb").write(co)
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", path], text=True)
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        print("  %-70s vgpr %4s agpr %4s sgpr %4s scratch %6s lds %6s spill_v %s" % (g("name")[:70], g("vgpr_count"), blk.split()[1], g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), g("vgpr_spill_count")))

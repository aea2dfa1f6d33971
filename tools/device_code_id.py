#!/usr/bin/env python3
"""The identity of a built library's device code:  python tools/device_code_id.py [--kernels] [lib]
One line per gfx950 code object (one per .hip source, in the build's order): sha256 of its bytes, sha256 of its
disassembly, then one resource line per kernel (as tools/kernel_resources.py prints them).  Two builds whose lines are
equal run the same device code: what a "no device change" claim is checked with (profiles/closed_switches.md).
--kernels: each resource line also carries the sha256 (16 digits) of that kernel's instruction text alone, the address and
encoding comments stripped and the pc-relative literals that address another symbol masked (`pcrel` counts them) -- equal
for a kernel that moved inside its code object or to another one (profiles/state_ops_split.md); the per-object hashes are
left out."""
import hashlib, os, re, subprocess, sys, tempfile
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from spacefortress_amd import build as B


def kernel_texts(dis):
    """llvm-objdump -d text -> {symbol: its instructions, one per line, without the '// address: encoding' comments}"""
    out, name = {}, None
    for line in dis.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            ins = line.split("//")[0].strip()
            # s_getpc_b64 s[N:N+1]; s_add_u32 sN, sN, <literal>: the distance from here to another symbol (a constant
            # table), which is where the linker put things, not what the kernel does: masked, and counted in `pcrel`
            if out[name] and out[name][-1].startswith("s_getpc_b64") and re.match(r"s_add_u32 (s\d+), \1, 0x[0-9a-f]+$", ins):
                ins = ins.rsplit(" ", 1)[0] + " <pcrel>"
            out[name].append(ins)
    for v in out.values():  # (the padding between one symbol's end and the next one's alignment)
        while v and v[-1] in ("s_nop 0", "s_code_end", "..."):
            v.pop()
    return {k: "\n".join(v) for k, v in out.items()}


argv = [x for x in sys.argv[1:] if x != "--kernels"]
per_kernel = "--kernels" in sys.argv[1:]
llvm = os.environ.get("ROCM_LLVM_BIN", "/opt/rocm/lib/llvm/bin")
lib = argv[0] if argv else B.LIB
hips = [s for s in B.SOURCES if s.endswith(".hip")]
for n, co in enumerate(B.device_code_objects(lib)):
    dis = B.disassemble_code_object(co)
    dis = dis[dis.index("\n", dis.index("file format")):]  # (the first line names the temporary file)
    src = hips[n] if n < len(hips) else "#%d" % n
    if per_kernel:
        print(src)
        texts = kernel_texts(dis)
    else:
        print("%-22s bytes %s disasm %s" % (src, hashlib.sha256(co).hexdigest(), hashlib.sha256(dis.encode()).hexdigest()))
    with tempfile.TemporaryDirectory() as td:
        path = os.path.join(td, "code.co")
        open(path, "wb").write(co)
        notes = subprocess.check_output([os.path.join(llvm, "llvm-readelf"), "--notes", path], text=True)
    for blk in notes.split("- .agpr_count")[1:]:
        g = lambda k: (re.search(r"\." + k + r":\s+(\S+)", blk) or [None, "?"])[1]
        code = " code %s pcrel %d" % (hashlib.sha256(texts[g("name")].encode()).hexdigest()[:16], texts[g("name")].count("<pcrel>")) if per_kernel else ""
        print("  %-70s vgpr %4s agpr %4s sgpr %4s scratch %6s lds %6s spill_v %s%s" % (g("name")[:70], g("vgpr_count"), blk.split()[1], g("sgpr_count"), g("private_segment_fixed_size"), g("group_segment_fixed_size"), g("vgpr_spill_count"), code))

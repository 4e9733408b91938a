"""Per-kernel instruction counts of two builds of librp_amd.so, from their gfx950 code objects (no GPU needed): which kernels'
opcode multisets differ, by how much, and in which opcodes.  Resource usage from the code objects' metadata alongside.
usage: python profiles/isa_diff.py <before.so> <after.so>"""
import collections
import os
import re
import subprocess
import sys
import tempfile

LLVM = "/opt/rocm/lib/llvm/bin"


def kernels(so):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "dev.co")
        subprocess.run([f"{LLVM}/llvm-objcopy", "-O", "binary", "--only-section=.hip_fatbin", so, fat], check=True)
        subprocess.run([f"{LLVM}/clang-offload-bundler", "--unbundle", "--type=o", f"--input={fat}", "--targets=hipv4-amdgcn-amd-amdhsa--gfx950",
                        f"--output={co}"], check=True)
        asm = subprocess.run([f"{LLVM}/llvm-objdump", "-d", "--no-show-raw-insn", co], capture_output=True, text=True, check=True).stdout
        notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", co], capture_output=True, text=True).stdout
    ops, name = {}, None
    for line in asm.splitlines():
        m = re.match(r"^[0-9a-f]+ <(\S+)>:", line)
        if m:
            name = m.group(1) if not m.group(1).startswith("L") and "$" not in m.group(1) else name
            if name is not None:
                ops.setdefault(name, collections.Counter())
            continue
        t = line.split()
        if name is not None and len(t) >= 1 and line.startswith(("\t", " ")) and re.match(r"^[a-z_0-9]+$", t[0]):
            ops[name][t[0]] += 1
    res = {n: (int(lds), int(scr), int(sg), int(ss), int(vg), int(vs)) for lds, n, scr, sg, ss, vg, vs in re.findall(
        r"\.group_segment_fixed_size: (\d+).*?\.name:\s+(\S+).*?\.private_segment_fixed_size: (\d+).*?\.sgpr_count:\s+(\d+).*?\.sgpr_spill_count: (\d+)"
        r".*?\.vgpr_count:\s+(\d+).*?\.vgpr_spill_count: (\d+)", notes, re.S)}
    return ops, res


a_ops, a_res = kernels(sys.argv[1])
b_ops, b_res = kernels(sys.argv[2])
names = sorted(n for n in set(a_ops) | set(b_ops) if n in a_res or n in b_res)
same = 0
print(f"{len(names)} kernels; (LDS, scratch, SGPRs, SGPR spills, VGPRs, VGPR spills) where they differ")
for n in names:
    a, b = a_ops.get(n), b_ops.get(n)
    if a is None or b is None:
        print(n, "only in", "before" if b is None else "after")
        continue
    d = {k: b[k] - a[k] for k in set(a) | set(b) if b[k] != a[k]}
    r = "" if a_res.get(n) == b_res.get(n) else f"  resources {a_res.get(n)} -> {b_res.get(n)}"
    if not d and not r:
        same += 1
        continue
    na, nb = sum(a.values()), sum(b.values())
    print(f"{n} {na} -> {nb} ({(nb - na) / na * 100:+.3f}%) {dict(sorted(d.items()))}{r}")
print(f"{same} kernels with the same opcode multiset and resources")

#!/usr/bin/env python3
"""Per-kernel register / LDS / scratch figures of the gfx950 code objects inside the built objects (no GPU needed):

    python tools/kernel_resources.py [csv-out]
    python tools/kernel_resources.py --isa-digest [csrc-dir] > digest.txt
    python tools/kernel_resources.py --isa-histogram before-csrc-dir [csrc-dir]

--isa-digest: one line per kernel, sorted by name -- file, kernel, the figures above, and a SHA-256 of the kernel's disassembled
body (llvm-objdump -d, addresses and comments stripped) -- so that the device code of two builds (say, before and after a change
that touches host code only) is compared with `diff`: the order kernels are emitted in does not matter, anything else shows.

--isa-histogram: for every kernel whose disassembled body differs between the two builds, the mnemonics whose counts differ
(mnemonic before -> after) -- whether a device-code refactor moved arithmetic or only address computation and waits.

For every csrc/*.o: the .hip_fatbin section is unbundled (clang-offload-bundler) and the AMDGPU metadata note of the code
object read (llvm-readelf --notes): .vgpr_count, .agpr_count, .sgpr_count, .vgpr_spill_count, .sgpr_spill_count,
.private_segment_fixed_size (scratch bytes per lane), .group_segment_fixed_size (static LDS).  What profiles/README.md quotes.
"""
import collections
import glob
import hashlib
import os
import re
import subprocess
import sys
import tempfile

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LLVM = "/opt/rocm/lib/llvm/bin"
KEYS = (".vgpr_count", ".agpr_count", ".sgpr_count", ".vgpr_spill_count", ".sgpr_spill_count",
        ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout
    return out.splitlines()


def short(n):
    n = n.replace("(anonymous namespace)::", "")
    m = re.match(r"(?:void )?([\w:]+(?:<[^(]*>)?)\(", n)
    return m.group(1) if m else n[:80]


def bodies_of(co):
    """symbol -> its instructions, without addresses, encodings and comments, and without the padding behind its last
    instruction (s_nop / s_code_end / elided zeros up to the next symbol or the end of the section: that depends on the kernel's neighbours)"""
    dis = subprocess.run([os.path.join(LLVM, "llvm-objdump"), "-d", "--no-show-raw-insn", co], capture_output=True, text=True,
                         check=True).stdout
    out, cur = {}, None
    for line in dis.splitlines():
        m = re.match(r"[0-9a-f]+ <(.+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
        elif cur is not None and line.strip():
            cur.append(re.sub(r"\s+", " ", line.split("//")[0]).strip())
    for body in out.values():
        while body and body[-1] in ("s_nop 0", "s_code_end", "..."):
            body.pop()
    return out


def kernels_of(obj, isa=False):
    with tempfile.TemporaryDirectory() as d:
        fat, co = os.path.join(d, "fat.bin"), os.path.join(d, "k.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fat])
        if os.path.getsize(fat) == 0:
            return []
        subprocess.check_call([os.path.join(LLVM, "clang-offload-bundler"), "--type=o", "--input=" + fat,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co, "--unbundle"])
        notes = subprocess.run([os.path.join(LLVM, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
        bodies = bodies_of(co) if isa else {}
    ks, cur = [], None
    for line in notes.splitlines():
        m = re.match(r"\s*-?\s*(\.[a-z_]+):\s*(.*)$", line)
        if not m:
            continue
        k, v = m.group(1), m.group(2).strip()
        if k == ".agpr_count":          # first key of a kernel's map in the note (alphabetical)
            cur = {}
            ks.append(cur)
        if cur is not None and (k in KEYS or k == ".name"):
            cur[k] = v.strip("'\"")
    ks = [k for k in ks if ".name" in k]
    for k, dn in zip(ks, demangle([k[".name"] for k in ks])):
        k["kernel"] = short(dn)
        if isa:
            k["isa"] = hashlib.sha256("\n".join(bodies[k[".name"]]).encode()).hexdigest()
            k["mnemonics"] = collections.Counter(line.split()[0] for line in bodies[k[".name"]])
    return ks


def isa_digest(csrc):
    lines = []
    for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))):
        for k in kernels_of(obj, isa=True):
            lines.append(" ".join([os.path.basename(obj)[:-2], k["kernel"].replace(" ", "")] + [str(k.get(x, "")) for x in KEYS] + [k["isa"]]))
    sys.stdout.write("\n".join(sorted(lines)) + "\n")


def isa_histogram(before, after):
    def load(csrc):
        return {(os.path.basename(obj)[:-2], k["kernel"].replace(" ", "")): k
                for obj in sorted(glob.glob(os.path.join(csrc, "*.o"))) for k in kernels_of(obj, isa=True)}
    a, b = load(before), load(after)
    for key in sorted(set(a) & set(b)):
        if a[key]["isa"] != b[key]["isa"]:
            ma, mb = a[key]["mnemonics"], b[key]["mnemonics"]
            diff = ["%s %d -> %d" % (m, ma[m], mb[m]) for m in sorted(set(ma) | set(mb)) if ma[m] != mb[m]]
            print("%s %s: %d -> %d instructions; %s" % (key[0], key[1], sum(ma.values()), sum(mb.values()),
                                                        ", ".join(diff) or "same mnemonic counts (order / registers only)"))


def main():
    here = os.path.join(REPO, "fly_bproject_amd", "csrc")
    if len(sys.argv) > 1 and sys.argv[1] == "--isa-digest":
        return isa_digest(sys.argv[2] if len(sys.argv) > 2 else here)
    if len(sys.argv) > 2 and sys.argv[1] == "--isa-histogram":
        return isa_histogram(sys.argv[2], sys.argv[3] if len(sys.argv) > 3 else here)
    rows = []
    for obj in sorted(glob.glob(os.path.join(REPO, "fly_bproject_amd", "csrc", "*.o"))):
        for k in kernels_of(obj):
            rows.append((os.path.basename(obj)[:-2], k))
    hdr = ["file", "kernel", "vgpr", "agpr", "sgpr", "vgpr_spill", "sgpr_spill", "scratch_bytes_per_lane", "static_lds_bytes"]
    lines = [",".join(hdr)]
    for f, k in rows:
        lines.append(",".join([f, '"%s"' % k["kernel"]] + [str(k.get(x, "")) for x in KEYS]))
    text = "\n".join(lines) + "\n"
    if len(sys.argv) > 1:
        open(sys.argv[1], "w").write(text)
    sys.stdout.write(text)


if __name__ == "__main__":
    main()

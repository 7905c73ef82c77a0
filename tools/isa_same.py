#!/usr/bin/env python3
"""isa_same.py <objects A> <objects B> -- are the gfx950 kernels of two builds the same machine code?

Each argument is a directory of hipcc -c outputs (oceantransportmatrixbuilder.jl_amd/lib of two checkouts).  Every object is unbundled
(as tools/isa_stats.sh does), every kernel disassembled; addresses and symbol annotations are dropped, mnemonics, operands and instruction
ENCODINGS are kept.  A kernel may live in another object of the other build (a text move between translation units): kernels are matched
by name across all objects.  Prints one line per kernel -- same | DIFFERS, instructions, VGPRs / SGPRs / LDS / scratch of both builds -- and
exits 1 if any kernel differs or exists in one build only.  Evidence for "a refactor did not touch the hot kernels"."""
import os
import re
import subprocess
import sys
import tempfile

LLVM = os.environ.get("OTMB_LLVM_BIN", "/opt/rocm/lib/llvm/bin")


def kernels(objdir):
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        for o in sorted(f for f in os.listdir(objdir) if f.endswith(".o")):
            fat, dev = os.path.join(tmp, "fat.bin"), os.path.join(tmp, "dev.o")
            if subprocess.run([f"{LLVM}/llvm-objcopy", f"--dump-section=.hip_fatbin={fat}", os.path.join(objdir, o)], capture_output=True).returncode:
                continue  # (host code only: no device section)
            subprocess.check_call([f"{LLVM}/clang-offload-bundler", "--type=o", "--unbundle", f"--input={fat}",
                                   "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", f"--output={dev}"])
            notes = subprocess.run([f"{LLVM}/llvm-readelf", "--notes", dev], capture_output=True, text=True).stdout
            res = {}
            for blk in re.split(r"^\s+- \.agpr_count:", notes, flags=re.M)[1:]:  # one block per kernel (its keys are sorted: .agpr_count first)
                g = lambda k: (re.search(r"^\s+\." + k + r":\s+(\d+)", blk, re.M) or [None, "?"])[1]
                sym = re.search(r"^\s+\.symbol:\s+(\S+)\.kd", blk, re.M).group(1)
                res[sym] = (g("vgpr_count"), g("sgpr_count"), g("group_segment_fixed_size"), g("private_segment_fixed_size"))
            cur = None
            for line in subprocess.run([f"{LLVM}/llvm-objdump", "-d", dev], capture_output=True, text=True, errors="replace").stdout.splitlines():
                m = re.match(r"^[0-9a-f]+ <(.+)>:", line)
                if m:
                    cur = m.group(1) if m.group(1) in res else None
                    if cur:
                        out[cur] = {"obj": o, "res": res[cur], "text": []}
                    continue
                m = re.match(r"^\s+(\S.*?)\s*//\s*[0-9A-Fa-f]+:((?: [0-9A-Fa-f]{8})+)", line)
                if cur and m:
                    out[cur]["text"].append(m.group(1) + " |" + m.group(2))
    for k in out.values():  # (the padding behind a kernel, which depends on what follows it in its object: s_nop 0 after the last instruction)
        while k["text"] and k["text"][-1].startswith("s_nop 0 |"):
            k["text"].pop()
    return out


def main():
    a, b = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for k in sorted(set(a) | set(b)):
        name = subprocess.run(["c++filt", k], capture_output=True, text=True).stdout.strip().replace("(TmParams)", "")[:64]
        if k not in a or k not in b:
            print(f"{name:64s} ONLY IN {'A' if k in a else 'B'} ({(a.get(k) or b.get(k))['obj']})")
            bad += 1
            continue
        same = a[k]["text"] == b[k]["text"] and a[k]["res"] == b[k]["res"]
        bad += not same
        r = lambda x: "vgpr %s sgpr %s lds %s scratch %s" % x["res"]
        print(f"{name:64s} {'same   ' if same else 'DIFFERS'} insns {len(a[k]['text']):5d} / {len(b[k]['text']):5d}  {r(a[k])} / {r(b[k])}  {a[k]['obj']} -> {b[k]['obj']}")
    print(f"{len(set(a) | set(b))} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())

#!/usr/bin/env python
"""Static instruction counts per kernel and instruction class, read off the gfx950 ISA by mnemonic prefix -- no GPU needed.
  python tools/isa_count.py [pattern] [--asm FILE]
Without --asm, ctrl-vio_amd/csrc/ctvio.hip is compiled to device assembly first (~25 s).  `pattern` selects kernels by a substring of
the demangled name (default: k_assemble_vis_mfma).  Classes: mfma, valu (every other v_*), salu (s_* except waits, nops and branches),
lds (ds_*, with the ds_add_f64 and ds_bpermute counts beside it), vmem (global_ / flat_ / buffer_ / scratch_), wait (s_waitcnt, s_nop,
s_barrier), branch (s_branch, s_cbranch_*)."""
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLASSES = ["total", "valu", "salu", "mfma", "lds", "ds_add_f64", "ds_bpermute", "vmem", "wait", "branch"]


def classes(op):
    if op.startswith("v_mfma"): return ["mfma"]
    if op.startswith("v_"): return ["valu"]
    if op.startswith("ds_"): return ["lds"] + [c for c in ("ds_add_f64", "ds_bpermute") if op.startswith(c)]
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")): return ["vmem"]
    if op.startswith(("s_waitcnt", "s_nop", "s_barrier")): return ["wait"]
    if op.startswith(("s_branch", "s_cbranch")): return ["branch"]
    if op.startswith("s_"): return ["salu"]
    return ["other"]


def count(asm, pattern):
    rows = []
    for m in re.finditer(r"^(_Z\w+):\s*; @\1\n(.*?)^\.Lfunc_end", asm, re.S | re.M):
        name = subprocess.run(["c++filt", m.group(1)], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"ctv::|^void |\(.*", "", name)
        if pattern not in name:
            continue
        c = Counter()
        for line in m.group(2).split("\n"):
            line = line.strip()
            if not line or line.startswith((";", ".", "//")) or line.split(";")[0].strip().endswith(":"):
                continue
            c["total"] += 1
            for k in classes(line.split()[0]):
                c[k] += 1
        rows.append((name, c))
    return rows


def main():
    args = sys.argv[1:]
    asm_path = None
    if "--asm" in args:
        i = args.index("--asm")
        asm_path = args[i + 1]
        del args[i:i + 2]
    pattern = args[0] if args else "k_assemble_vis_mfma"
    if asm_path is None:
        asm_path = os.path.join(tempfile.mkdtemp(), "ctvio.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "-munsafe-fp-atomics", "-fno-slp-vectorize", "-S", "--cuda-device-only",
                               "-o", asm_path, os.path.join(ROOT, "ctrl-vio_amd", "csrc", "ctvio.hip")], stderr=subprocess.DEVNULL)
    rows = count(open(asm_path).read(), pattern)
    print(f"{'kernel':44s}" + "".join(f"{c:>12s}" for c in CLASSES))
    for name, c in rows:
        print(f"{name[:44]:44s}" + "".join(f"{c[k]:12d}" for k in CLASSES))


if __name__ == "__main__":
    main()

#!/usr/bin/env python3
"""Instruction streams of the gfx950 kernels of two builds of one object, kernel by kernel:
    python tools/isa_compare.py PARENT.o TREE.o
Unbundles the code objects (as tools/kernel_meta.py does), disassembles them and compares opcodes and operands; addresses,
encodings and branch targets are left out.  Prints "identical" or how many instructions differ and where in the stream."""
import difflib
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from kernel_meta import LLVM, demangle  # noqa: E402


def streams(obj):
    with tempfile.TemporaryDirectory() as td:
        fb, co = os.path.join(td, "a.fatbin"), os.path.join(td, "a.co")
        subprocess.check_call(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", obj, fb])
        subprocess.check_call([LLVM + "/clang-offload-bundler", "--unbundle", "--type=o", "--input=" + fb,
                               "--targets=hipv4-amdgcn-amd-amdhsa--gfx950", "--output=" + co])
        txt = subprocess.check_output([LLVM + "/llvm-objdump", "-d", "--no-show-raw-insn", co], text=True)
    out, cur = {}, None
    for line in txt.split("\n"):
        m = re.match(r"^[0-9a-f]+ <(\S+)>:$", line)
        if m:
            cur = out.setdefault(m.group(1), [])
            continue
        ins = line.split("//")[0].strip()
        if cur is None or not ins:
            continue
        if re.match(r"s_(c?branch|call)", ins):
            ins = ins.split()[0]
        cur.append(ins)
    return out


def main(parent, tree):
    a, b = streams(parent), streams(tree)
    for name in sorted(set(a) | set(b), key=demangle):
        short = demangle(name)[-60:]
        if name not in a or name not in b:
            print("%-60s only in the %s" % (short, "parent" if name in a else "tree"))
            continue
        x, y = a[name], b[name]
        if x == y:
            print("%-60s identical (%d instructions)" % (short, len(x)))
            continue
        ops = [o for o in difflib.SequenceMatcher(None, x, y, autojunk=False).get_opcodes() if o[0] != "equal"]
        gone = sum(o[2] - o[1] for o in ops)
        new = sum(o[4] - o[3] for o in ops)
        print("%-60s parent %d, tree %d instructions: %d of the parent's replaced by %d, in %d places between instruction %d and %d"
              % (short, len(x), len(y), gone, new, len(ops), ops[0][1], ops[-1][2]))


if __name__ == "__main__":
    main(sys.argv[1], sys.argv[2])

#!/usr/bin/env python3
"""Do two builds of one source hold the same kernels?   usage: tools/compare_kernel_isa.py OLD.o NEW.o

Extracts the gfx950 device code of both objects (llvm-objdump --offloading), disassembles it and looks, for every
kernel of OLD, for a kernel of NEW with the same instruction stream (symbol names left out: a template that gained a
defaulted parameter changes the mangled name of every instantiation and nothing else).  Prints one line per kernel and
exits 1 when a kernel of OLD has no identical counterpart.

What it is for: profiles/traffic.json carries a fingerprint of csrc/spmm.hip + plan.hip + common.h, because its counter
figures belong to the kernels they were collected on.  When those sources gain NEW instantiations only, this shows that
the kernels the bench launches did not change, and the record may keep its figures under the new fingerprint (say so in
the record: `fingerprint_note`)."""
import os
import re
import shutil
import subprocess
import sys
import tempfile


def kernels(obj):
    objdump = shutil.which("llvm-objdump") or "/opt/rocm/lib/llvm/bin/llvm-objdump"
    with tempfile.TemporaryDirectory() as d:
        local = os.path.join(d, "k.o")
        shutil.copy(obj, local)
        subprocess.run([objdump, "--offloading", local], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, cwd=d, check=True)
        code = [f for f in os.listdir(d) if "gfx950" in f]
        if not code:
            sys.exit(f"{obj}: no gfx950 bundle")
        text = subprocess.run([objdump, "-d", "--no-show-raw-insn", os.path.join(d, code[0])], stdout=subprocess.PIPE,
                              text=True, check=True).stdout
    out, name = {}, None
    for line in text.splitlines():
        m = re.match(r"^[0-9a-f]+ <(.+)>:$", line)
        if m:
            name = m.group(1)
            out[name] = []
        elif name and line.strip():
            out[name].append(re.sub(r"<[^>]*>", "", line.split("//")[0]).strip())
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bodies = {}
    for k, v in new.items():
        bodies.setdefault(tuple(v), []).append(k)
    missing = 0
    for k, v in old.items():
        hit = bodies.get(tuple(v))
        missing += hit is None
        print(("identical    " if hit else "NO COUNTERPART") + f" {len(v):5d} instructions  {k}" + (f"  ->  {hit[0]}" if hit and hit[0] != k else ""))
    print(f"{len(old)} kernels in {sys.argv[1]}, {len(old) - missing} with an identical instruction stream in {sys.argv[2]} "
          f"({len(new)} kernels)")
    sys.exit(1 if missing else 0)


if __name__ == "__main__":
    main()

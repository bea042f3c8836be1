#!/usr/bin/env python3
"""Are two builds' gfx950 device code the same, instruction for instruction?

    python tools/code_identity.py A B

A and B are libraries (libm3s_gn.so: the first code object of the bundle, which
is m3s_gn.hip's) or device objects (hipcc --cuda-device-only
--no-gpu-bundle-output -c). Compared: the disassembly with its addresses, the
kernel metadata notes (register counts, LDS, scratch, arguments) and the symbol
tables. The __hip_cuid_<hash> symbol is ignored: hipcc derives it from the
source path. Prints the first difference, or `identical: <n> functions`; the
exit status is non-zero on a difference. CPU only. The proof that a change which
only moves source text (between csrc/m3s_gn.hip and its parts in csrc/gn/, or
within the order rule that opens csrc/m3s_gn.hip) left the device code
alone."""
import os
import subprocess
import sys
import tempfile

ROOT = os.path.abspath(os.path.join(os.path.dirname(__file__), ".."))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from test_isa import OBJDUMP, code_object  # noqa: E402

READELF = os.path.join(os.path.dirname(OBJDUMP), "llvm-readelf")


def views(path, tmp):
    """The three texts compared for one build, as lists of lines."""
    data = open(path, "rb").read()
    co = os.path.join(tmp, "code.co")
    with open(co, "wb") as f:  # a device object is the code object itself
        f.write(code_object(path) if b"__CLANG_OFFLOAD_BUNDLE__" in data else data)

    def run(*cmd):
        return subprocess.run(cmd + (co,), check=True, capture_output=True, text=True).stdout.splitlines()

    dis = run(OBJDUMP, "-d", "--no-show-raw-insn")[2:]  # after the file-name line
    syms = sorted(" ".join(ln.split()[1:]) for ln in run(READELF, "--symbols", "-W")
                  if ln.split(":")[0].strip().isdigit() and "__hip_cuid_" not in ln)
    return {"disassembly": dis, "notes": run(READELF, "--notes"), "symbols": syms}


def main(a, b):
    with tempfile.TemporaryDirectory() as ta, tempfile.TemporaryDirectory() as tb:
        va, vb = views(a, ta), views(b, tb)
    for what in ("symbols", "notes", "disassembly"):
        la, lb = va[what], vb[what]
        for k in range(max(len(la), len(lb))):
            xa, xb = (la[k] if k < len(la) else "<end>"), (lb[k] if k < len(lb) else "<end>")
            if xa != xb:
                print(f"{what} differ at line {k + 1}:\n  {a}: {xa}\n  {b}: {xb}")
                return 1
    n = sum(1 for ln in va["disassembly"] if ln.endswith(">:") and not ln.startswith((" ", "\t")))
    print(f"identical: {n} functions")
    return 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))

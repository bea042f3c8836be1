"""The C side of the ABI tests (tests/test_*abi.py): what gcc says about the
public headers, to hold the ctypes mirrors and the export lists against."""
import ctypes
import os
import re
import subprocess
import tempfile

INCLUDE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "include")


def probe(headers, mirrors, macros=()):
    """Compile and run one C program over ``headers`` (file names under
    include/) and assert that every mirror of ``mirrors`` ({C struct name:
    ctypes class}) has the C struct's size and, for every field its ``_fields_``
    names, the C offset. Returns {name: value} of the integer ``macros``."""
    lines = [f'printf("{m} %lld\\n", (long long)({m}));' for m in macros]
    for struct, cls in mirrors.items():
        lines.append(f'printf("{struct} %zu\\n", sizeof({struct}));')
        lines += [f'printf("{struct}.{f} %zu\\n", offsetof({struct}, {f}));' for f, *_ in cls._fields_]
    source = ("#include <stdio.h>\n#include <stddef.h>\n" + "".join(f'#include "{h}"\n' for h in headers)
              + "int main(void) {\n  " + "\n  ".join(lines) + "\n  return 0;\n}\n")
    with tempfile.TemporaryDirectory() as tmp:
        c, exe = os.path.join(tmp, "probe.c"), os.path.join(tmp, "probe")
        with open(c, "w") as f:
            f.write(source)
        subprocess.check_call(["gcc", "-std=c11", "-I", INCLUDE, c, "-o", exe])
        got = {k: int(v) for k, v in (l.split() for l in subprocess.check_output([exe]).decode().splitlines())}
    for struct, cls in mirrors.items():
        assert cls._fields_, struct
        assert got.pop(struct) == ctypes.sizeof(cls), struct
        for f, *_ in cls._fields_:
            assert got.pop(f"{struct}.{f}") == getattr(cls, f).offset, f"{struct}.{f}"
    assert set(got) == set(macros)  # every line of the probe was looked at
    return got


def declared_symbols(header):
    """The ``m3s_*`` functions ``header`` (a file name under include/)
    declares, comments left out."""
    with open(os.path.join(INCLUDE, header)) as f:
        text = re.sub(r"/\*.*?\*/|//[^\n]*", "", f.read(), flags=re.S)
    return set(re.findall(r"\b(m3s_\w+)\s*\(", text))

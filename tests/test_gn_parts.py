"""CPU check of csrc/m3s_gn.hip's layout: the files under csrc/gn/ are parts of
that one translation unit. Each is included by m3s_gn.hip exactly once and
includes nothing itself; an orphaned part would be dead code that looks alive.
Each part opens by naming itself. m3s_gn.hip itself holds no device code, and
the launch map in its opening comment names the part that defines each kernel."""
import os
import re

CSRC = os.path.join(os.path.dirname(__file__), "..", "mast3r-slam-ysh_amd", "csrc")


def test_every_part_is_included_once():
    main = open(os.path.join(CSRC, "m3s_gn.hip")).read()
    included = re.findall(r'^\s*#\s*include\s+"gn/([^"]+)"', main, re.M)
    parts = sorted(os.listdir(os.path.join(CSRC, "gn")))
    assert parts and sorted(included) == parts  # a list: a part named twice fails too
    for p in parts:
        text = open(os.path.join(CSRC, "gn", p)).read()
        assert not re.search(r"^\s*#\s*include\b", text, re.M), p


def test_every_part_opens_by_naming_itself():
    parts = sorted(os.listdir(os.path.join(CSRC, "gn")))
    assert parts
    for p in parts:
        first = open(os.path.join(CSRC, "gn", p), encoding="utf-8").readline()
        assert first.startswith(f"// gn/{p} — part of the m3s_gn.hip translation unit"), p


def _code(text):
    """text without its // and /* */ comments"""
    return re.sub(r"//[^\n]*|/\*.*?\*/", "", text, flags=re.S)


def test_main_file_holds_no_device_code():
    code = _code(open(os.path.join(CSRC, "m3s_gn.hip"), encoding="utf-8").read())
    assert "#include" in code and 'extern "C"' in code  # the strip left the file's own text
    assert "__global__" not in code and "__device__" not in code


def test_launch_map_names_the_part_of_every_kernel():
    main = open(os.path.join(CSRC, "m3s_gn.hip"), encoding="utf-8").read()
    head = re.match(r"(?://[^\n]*\n)+", main).group(0)  # the opening comment
    head = " ".join(line[2:].strip() for line in head.splitlines())
    homes = {}  # kernel -> the parts that define it
    for p in sorted(os.listdir(os.path.join(CSRC, "gn"))):
        code = _code(open(os.path.join(CSRC, "gn", p), encoding="utf-8").read())
        for m in re.finditer(r"__global__\s+void\s+(?:__launch_bounds__\s*\([^;{]*?\)\s+)?(\w+)\s*\(", code):
            homes.setdefault(m.group(1), []).append(p)
    assert len(homes) > 20 and all(k.endswith("_kernel") for k in homes), homes
    # a mention: the name, template arguments if any ("<1> / <2>"), and "(gn/<part>.h" where the map gives the part
    mentions = re.findall(r"\b(\w+_kernel)\b((?:\s*/?\s*<[^>]*>)*)(?:\s*\(gn/(\w+\.h))?", head)
    assert mentions
    first = {}
    for name, _, part in mentions:
        assert len(homes.get(name, [])) == 1, (name, homes.get(name))
        if part:
            assert homes[name] == [part], (name, part, homes[name])
        first.setdefault(name, part)
    assert all(first.values()), [k for k, v in first.items() if not v]  # every first mention carries its part
    assert set(first) == set(homes), set(homes) ^ set(first)  # and the map leaves no kernel out

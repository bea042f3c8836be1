"""CPU check of csrc/m3s_gn.hip's layout: the files under csrc/gn/ are parts of
that one translation unit. Each is included by m3s_gn.hip exactly once and
includes nothing itself; an orphaned part would be dead code that looks alive.
Each part opens by naming itself."""
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

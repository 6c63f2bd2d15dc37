"""Writes tests/golden/option_defaults.json, the fixture of tests/test_options_table.py: the names and defaults of the options of
oicc_problem ("spline") and oicc_ba ("ba") as the constructors of a commit set them, opt["name"] = value, before the options moved
into csrc/oicc_options.def and csrc/oicc_ba_options.def.  The fixture in the tree was written from ba13ebb, the last such commit:

    python scripts/make_option_defaults_golden.py ba13ebb [output.json]
"""
import json
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "openimucameracalibrator_amd/csrc/"
SOURCES = {"spline": (CSRC + "oicc_problem.h", 56), "ba": (CSRC + "oicc_ba.hip", 17)}

commit = sys.argv[1]
out_path = sys.argv[2] if len(sys.argv) > 2 else os.path.join(ROOT, "tests", "golden", "option_defaults.json")
tables = {}
for which, (path, count) in SOURCES.items():
    text = subprocess.check_output(["git", "-C", ROOT, "show", "%s:%s" % (commit, path)], text=True)
    pairs = re.findall(r'\bopt\["(\w+)"\]\s*=\s*([^;]+);', text)
    tables[which] = {name: float(value) for name, value in pairs}   # (a chained assignment would fail here: float("opt[...] = 0"))
    assert len(pairs) == len(tables[which]) == count, (which, len(pairs), len(tables[which]))
    print("%-6s %d options from %s:%s" % (which, count, commit, path))
with open(out_path, "w") as f:
    json.dump(tables, f, indent=1)
    f.write("\n")
print("wrote %s (%d bytes)" % (out_path, os.path.getsize(out_path)))

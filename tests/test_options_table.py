"""The options of oicc_problem and oicc_ba are members of two plain structs, generated with their defaults and their name lookup from
csrc/oicc_options.def and csrc/oicc_ba_options.def (csrc/oicc_options.h).  These tests hold the two tables to the names and defaults
the constructors set before the options moved there (tests/golden/option_defaults.json, scripts/make_option_defaults_golden.py), and
the setters and getters to one member per name: every name is written with a value of its own and read back, an unknown name is
refused by both and stays unknown.  The spline problem is a host-only object (oicc_debug_create_host_only); an oicc_ba needs the device."""
import ctypes as C
import json
import os
import re

import pytest

from openimucameracalibrator_amd import _abi, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "option_defaults.json")) as f:
    GOLDEN = json.load(f)
ERR_INVALID_ARG = -1   # OICC_ERR_INVALID_ARG, include/oicc_hip.h


def _table(which):
    fn = _abi.bind_option_debug(_lib.load().lib, "oicc_debug_option_table")
    name = C.c_char_p(); default = C.c_double()
    n = fn(which, -1, C.byref(name), C.byref(default))
    out = []
    for i in range(n):
        assert fn(which, i, C.byref(name), C.byref(default)) == n
        out.append((name.value.decode(), default.value))
    return out


def _round_trip(names, set_option, get_option, last_error):
    """set_option / get_option(name[, value]) -> status (the value read lands in get_option.value)"""
    for i, name in enumerate(names):
        assert set_option(name, 1000.5 + i) == 0, name
    for i, name in enumerate(names):
        assert get_option(name) == 0 and get_option.value == 1000.5 + i, (name, get_option.value)
    for call in (lambda: get_option("no_such_option"), lambda: set_option("no_such_option", 1.0), lambda: get_option("no_such_option")):
        assert call() == ERR_INVALID_ARG
        assert "unknown option no_such_option" in last_error()


def _getter(fn, handle):
    def get(name):
        v = C.c_double(float("nan")); rc = fn(handle, name.encode(), C.byref(v)); get.value = v.value
        return rc
    return get


@pytest.mark.parametrize("which,key", [(0, "spline"), (1, "ba")])
def test_the_tables_hold_the_names_and_defaults_the_constructors_set(which, key):
    table = _table(which)
    assert len(table) == len(GOLDEN[key]) == (56, 17)[which]
    assert len({name for name, _ in table}) == len(table)   # no name twice
    assert dict(table) == GOLDEN[key]                        # the same names, defaults equal as doubles
    assert _abi.bind_option_debug(_lib.load().lib, "oicc_debug_option_table")(2, 0, None, None) == 0   # there is no third table


class _HostOnlyProblem:
    def __init__(self):
        self.b = _lib.load(); raw = self.b.lib
        raw.oicc_debug_create_host_only.restype = C.c_int
        raw.oicc_debug_create_host_only.argtypes = [C.POINTER(_abi.H)]
        raw.oicc_debug_destroy_host_only.restype = None
        raw.oicc_debug_destroy_host_only.argtypes = [_abi.H]
        self.h = _abi.H()
        assert raw.oicc_debug_create_host_only(C.byref(self.h)) == 0
        self.get = _getter(_abi.bind_option_debug(raw, "oicc_debug_get_option"), self.h)

    def set(self, name, value):
        return self.b.set_option(self.h, name.encode(), float(value))

    def last_error(self):
        return self.b.last_error(self.h).decode()

    def __del__(self):
        self.b.lib.oicc_debug_destroy_host_only(self.h)


def test_every_option_of_the_spline_problem_is_a_member_of_its_own():
    p = _HostOnlyProblem()
    for name, default in GOLDEN["spline"].items():
        assert p.get(name) == 0 and p.get.value == default, name
    _round_trip(list(GOLDEN["spline"]), p.set, p.get, p.last_error)
    fresh = _HostOnlyProblem()
    for name, default in GOLDEN["spline"].items():
        assert fresh.get(name) == 0 and fresh.get.value == default, name


def test_the_integration_guide_names_only_options_that_exist():
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text[text.index("## Options a maintainer should know"):]
    rows = [line for line in section.split("\n## ")[0].splitlines() if line.startswith("| `")]
    named = [name for line in rows for name in re.findall(r"`(\w+)`", line.split("|")[1])]
    assert len(rows) >= 10 and len(named) >= len(rows)
    assert [name for name in named if name not in GOLDEN["spline"]] == []


@pytest.mark.gpu
def test_every_option_of_the_view_bundle_adjustment_is_a_member_of_its_own():
    from openimucameracalibrator_amd import camera_calibrator as CC
    ba = CC.ViewBundleAdjuster()
    get = _getter(_abi.bind_option_debug(ba.b.lib, "oicc_debug_ba_get_option"), ba.h)
    for name, default in GOLDEN["ba"].items():
        assert get(name) == 0 and get.value == default, name
    _round_trip(list(GOLDEN["ba"]), lambda name, value: ba.b.set_option(ba.h, name.encode(), float(value)), get,
                lambda: ba.b.last_error(ba.h).decode())

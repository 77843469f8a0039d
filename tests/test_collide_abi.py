"""CPU side of the collision forms: option "collide" (include/hns.h) round-trips as host code, and the plan query hns_sim_substep_plan is
declared in the header, exported by the library and bound in hnanosolver_amd/_lib.py."""
import os
import re
import subprocess

import pytest

from hnanosolver_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture
def collide_default():
    yield
    _lib.set_option("collide", None)


def test_collide_option_round_trips(collide_default):
    assert _lib.get_option("collide") == "auto"
    for word in ("generic", "auto", "generic"):
        _lib.set_option("collide", word)
        assert _lib.get_option("collide") == word
    _lib.set_option("collide", None)
    assert _lib.get_option("collide") == "auto"


@pytest.mark.parametrize("start", ["auto", "generic"])
@pytest.mark.parametrize("bad", ["1", "0", "Generic", "narrow", ""])
def test_collide_refuses_a_bad_word_and_changes_nothing(collide_default, start, bad):
    _lib.set_option("collide", start)
    others = {n: _lib.get_option(n) for n in ("advect", "fuse", "lookahead")}
    with pytest.raises(_lib.HNSError) as e:
        _lib.set_option("collide", bad)
    assert e.value.code == _lib.HNS_ERR_INVALID_ARGUMENT and "collide" in str(e.value)
    assert _lib.get_option("collide") == start
    assert {n: _lib.get_option(n) for n in others} == others


def test_collide_is_independent_of_advect(collide_default):
    _lib.set_option("collide", "generic")
    assert _lib.get_option("advect") == "auto"
    _lib.set_option("advect", "generic")
    _lib.set_option("advect", None)
    assert _lib.get_option("collide") == "generic"


def test_substep_plan_is_declared_exported_and_bound():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "hns.h")).read(), flags=re.S)
    decl = re.search(r"int\s+hns_sim_substep_plan\s*\(([^)]*)\)\s*;", src)
    assert decl, "hns_sim_substep_plan is not declared in include/hns.h"
    args = [a.strip() for a in decl.group(1).split(",")]
    assert len(args) == 5 and args[0].startswith("hns_sim") and "hns_combustion_params" in args[1] and args[2].startswith("int") and args[3].startswith("char") and "uint64_t" in args[4]
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T hns_sim_substep_plan$", out, re.M), "libhns.so does not export hns_sim_substep_plan"
    res, argtypes = _lib.SIGNATURES["hns_sim_substep_plan"]
    assert len(argtypes) == 5
    lib = _lib.load_library()
    assert lib.hns_sim_substep_plan.argtypes is not None and len(lib.hns_sim_substep_plan.argtypes) == 5
    # a null sim is refused with the function's name, and nothing is written
    import ctypes as C

    buf = C.create_string_buffer(b"untouched", 64)
    assert lib.hns_sim_substep_plan(None, None, 0, buf, 64) == _lib.HNS_ERR_INVALID_ARGUMENT
    assert b"hns_sim_substep_plan" in lib.hns_last_error() and buf.value == b"untouched"


def test_header_lists_the_option():
    src = open(os.path.join(ROOT, "include", "hns.h")).read()
    assert "Fifteen names" in src and re.search(r'"collide"\s+auto \| generic', src)

"""The options a library context is created with (csrc/options.h, options.hip): one table-driven reader of the MTV_* environment, the override
record of the mtv_debug_* setters laid over it, both visible through mtv_debug_options_dump(NULL, ...) = "what a context created now would
get".  Host only: no device is touched.  Every test restores os.environ and the overrides."""
import contextlib
import ctypes
import os
import re

import pytest

from conftest import ROOT
from moditalker_amd import _lib

DEFAULTS = """\
MTV_FORCE_TILE=0
MTV_FORCE_WIN=0
MTV_FORCE_PW=0
MTV_FORCE_B3=0
MTV_FORCE_LDS=0
MTV_FORCE_WIN_XM=0
MTV_WIN_PACKED=1
MTV_WIN_XM=-1
MTV_PW_XM=-1
MTV_AUTOTUNE=1
MTV_TUNE_SAMPLES=5
MTV_TUNE_CACHE=
MTV_GEO=1
MTV_STAMPS=0
MTV_DEEP=1
MTV_DEEP_POOL_FOLD=1
MTV_DEEP_NO_ATTN=0
MTV_DEEP_NO_BLOCK=0
MTV_DEEP_BLOCK_ALL=0
MTV_DEEP_FIN_PASS=0
MTV_DEEP_XM=1
MTV_DEEP_ATTN_QT=1
MTV_DEEP_ATTN_HPW=0
MTV_BLOCK_CL=0
MTV_BLOCK_RQ=0
MTV_BLOCK_MAX_L=32
MTV_BLOCK_MAX_LC=32768
MTV_RESIDENT_CUS=0
MTV_ATT_QW=0
MTV_ATT_KBX=2
MTV_ATT_QB=-1
MTV_STEPS_PER_GRAPH=8
MTV_AE_NO_GEGLU_FUSION=0
"""

# variable -> (text in the environment, value the dump then shows)
CASES = {
    "MTV_FORCE_TILE": ("2,4,8,2", "2,4,8,2"),
    "MTV_FORCE_WIN": ("1,2", "1,2,1"),
    "MTV_FORCE_PW": ("2,1,6", "2,1,6"),
    "MTV_FORCE_B3": ("4,2,4", "4,2,4"),
    "MTV_FORCE_LDS": ("4,8", "4,8,1"),
    "MTV_FORCE_WIN_XM": ("1", "1"),
    "MTV_WIN_PACKED": ("0", "0"),
    "MTV_WIN_XM": ("1", "1"),
    "MTV_PW_XM": ("2", "2"),
    "MTV_AUTOTUNE": ("0", "0"),
    "MTV_TUNE_SAMPLES": ("99", "15"),
    "MTV_TUNE_CACHE": ("tune_raw.txt", "tune_raw.txt"),
    "MTV_GEO": ("0", "0"),
    "MTV_STAMPS": ("1", "1"),
    "MTV_DEEP": ("0", "0"),
    "MTV_DEEP_POOL_FOLD": ("0", "0"),
    "MTV_DEEP_NO_ATTN": ("1", "1"),
    "MTV_DEEP_NO_BLOCK": ("1", "1"),
    "MTV_DEEP_BLOCK_ALL": ("1", "1"),
    "MTV_DEEP_FIN_PASS": ("1", "1"),
    "MTV_DEEP_XM": ("0", "0"),
    "MTV_DEEP_ATTN_QT": ("2", "2"),
    "MTV_DEEP_ATTN_HPW": ("2", "2"),
    "MTV_BLOCK_CL": ("4", "4"),
    "MTV_BLOCK_RQ": ("2", "2"),
    "MTV_BLOCK_MAX_L": ("128", "128"),
    "MTV_BLOCK_MAX_LC": ("65536", "65536"),
    "MTV_RESIDENT_CUS": ("48", "48"),
    "MTV_ATT_QW": ("2", "2"),
    "MTV_ATT_KBX": ("1", "1"),
    "MTV_ATT_QB": ("0", "0"),
    "MTV_STEPS_PER_GRAPH": ("5", "4"),
    "MTV_AE_NO_GEGLU_FUSION": ("1", "1"),
}


def _dump(lib, ctx=None):
    buf = ctypes.create_string_buffer(4096)
    _lib.check(lib.mtv_debug_options_dump(ctx, buf, len(buf)), "mtv_debug_options_dump")
    return buf.value.decode()


def _lines(text):
    return dict(line.split("=", 1) for line in text.splitlines())


def _clear_overrides(lib):
    lib.mtv_debug_deep(-1)
    lib.mtv_debug_deep_options(-1)
    lib.mtv_debug_deep_attn_form(-1)
    lib.mtv_debug_attention_qb(-1)
    lib.mtv_debug_resident_cus(0)
    for off in (lib.mtv_debug_force_win, lib.mtv_debug_force_pw, lib.mtv_debug_force_lds):
        off(0, 0)
    lib.mtv_debug_force_b3(0, 0, 1)


@contextlib.contextmanager
def _clean(**env):
    """No MTV_* variable but `env`, no override; everything as it was afterwards.  (MTV_LIB and the other Python-side variables are read by Python alone.)"""
    lib = _lib.load()
    saved = dict(os.environ)
    try:
        for k in [k for k in os.environ if k.startswith("MTV_")]:
            del os.environ[k]
        os.environ.update(env)
        _clear_overrides(lib)
        yield lib
    finally:
        _clear_overrides(lib)
        os.environ.clear()
        os.environ.update(saved)


def test_defaults():
    with _clean() as lib:
        assert _dump(lib) == DEFAULTS


def test_table_covers_every_row():
    assert list(CASES) == [line.split("=")[0] for line in DEFAULTS.splitlines()]


@pytest.mark.parametrize("name", list(CASES))
def test_each_variable_changes_its_own_line_only(name):
    text, shown = CASES[name]
    want = _lines(DEFAULTS)
    assert want[name] != shown, "the case shows nothing"
    want[name] = shown
    with _clean(**{name: text}) as lib:
        assert _lines(_dump(lib)) == want


@pytest.mark.parametrize("name,text", [("MTV_FORCE_WIN", "4,4"), ("MTV_FORCE_WIN", "1,2,3"), ("MTV_FORCE_WIN", "1"), ("MTV_FORCE_WIN", "x"),
                                       ("MTV_FORCE_PW", "1,2,6"), ("MTV_FORCE_PW", "3,1"), ("MTV_FORCE_B3", "3,3"), ("MTV_FORCE_B3", "4,2,3"),
                                       ("MTV_FORCE_LDS", "1,1"), ("MTV_FORCE_LDS", "-2,4"), ("MTV_FORCE_TILE", "2,4"), ("MTV_FORCE_TILE", "")])
def test_malformed_or_missing_forced_tiles_stay_off(name, text):
    """A forced tile from the environment goes through the rule of the mtv_debug_force_* arguments (conv_tile_exists): a tile no kernel
    has leaves the family off, and so does the setter, which reports it."""
    with _clean(**{name: text}) as lib:
        assert _dump(lib) == DEFAULTS
    with _clean() as lib:
        assert lib.mtv_debug_force_win(4, 4) < 0 and lib.mtv_debug_force_pw_waves(1, 2, 6) < 0 and lib.mtv_debug_force_b3(3, 3, 1) < 0
        assert lib.mtv_debug_force_lds(1, 1) < 0 and lib.mtv_last_error()
        assert _dump(lib) == DEFAULTS


def test_override_then_environment_then_default():
    with _clean(MTV_FORCE_WIN="1,2", MTV_DEEP="0", MTV_RESIDENT_CUS="64", MTV_ATT_QB="0", MTV_DEEP_NO_BLOCK="1", MTV_DEEP_ATTN_HPW="2") as lib:
        _lib.check(lib.mtv_debug_force_win_ks(2, 4, 2), "mtv_debug_force_win_ks")
        assert _lines(_dump(lib))["MTV_FORCE_WIN"] == "2,4,2"
        _lib.check(lib.mtv_debug_force_win(0, 0), "mtv_debug_force_win")
        assert _lines(_dump(lib))["MTV_FORCE_WIN"] == "1,2,1"          # the "off" call clears the override: the variable counts again
        for setter, arg, off, name, over, env in ((lib.mtv_debug_deep, 1, -1, "MTV_DEEP", "1", "0"), (lib.mtv_debug_resident_cus, 48, 0, "MTV_RESIDENT_CUS", "48", "64"),
                                                  (lib.mtv_debug_attention_qb, 1, -1, "MTV_ATT_QB", "1", "0"), (lib.mtv_debug_deep_attn_form, 1, -1, "MTV_DEEP_ATTN_HPW", "1", "2")):
            _lib.check(setter(arg), name)
            assert _lines(_dump(lib))[name] == over, name
            _lib.check(setter(off), name)
            assert _lines(_dump(lib))[name] == env, name
        _lib.check(lib.mtv_debug_deep_options(8 | 64), "mtv_debug_deep_options")          # a mask sets all four, also the ones the environment has on
        got = _lines(_dump(lib))
        assert [got[k] for k in ("MTV_DEEP_NO_ATTN", "MTV_DEEP_NO_BLOCK", "MTV_DEEP_BLOCK_ALL", "MTV_DEEP_FIN_PASS")] == ["1", "0", "0", "1"]
        _lib.check(lib.mtv_debug_deep_options(-1), "mtv_debug_deep_options")
        got = _lines(_dump(lib))
        assert [got[k] for k in ("MTV_DEEP_NO_ATTN", "MTV_DEEP_NO_BLOCK", "MTV_DEEP_BLOCK_ALL", "MTV_DEEP_FIN_PASS")] == ["0", "1", "0", "0"]
        _lib.check(lib.mtv_debug_force_pw_waves(1, 1, 8), "mtv_debug_force_pw_waves")     # (8 waves = all = the tile code 1)
        assert _lines(_dump(lib))["MTV_FORCE_PW"] == "1,1,1"


def test_retired_deep_option_bits_leave_the_override_unchanged():
    with _clean() as lib:
        _lib.check(lib.mtv_debug_deep_options(16), "mtv_debug_deep_options")
        before = _dump(lib)
        for mask in (1, 2, 4, 16 | 1, 128, -2):
            assert lib.mtv_debug_deep_options(mask) < 0 and lib.mtv_last_error(), mask
            assert _dump(lib) == before
        assert _lines(before)["MTV_DEEP_NO_BLOCK"] == "1"


def test_dump_reports_a_short_buffer():
    with _clean() as lib:
        buf = ctypes.create_string_buffer(16)
        assert lib.mtv_debug_options_dump(None, buf, len(buf)) < 0 and b"needed" in lib.mtv_last_error()


def test_readme_table_lists_exactly_the_variables_of_the_dump():
    readme = open(os.path.join(ROOT, "README.md")).read()
    section = readme[readme.index("### Run-time switches"):readme.index("Python-side variables")]
    names = {re.match(r"\| `(MTV_[A-Z0-9_]+)", line).group(1) for line in section.splitlines() if line.startswith("| `")}
    assert names == set(CASES), names ^ set(CASES)

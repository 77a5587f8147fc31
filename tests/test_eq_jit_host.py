"""Host side of the per-shape equality scan (csrc/eqs_jit.hip): its getter and tunings, its source string (no GPU calls)."""
import ctypes
import os
import re

from conftest import ROOT


def test_getter_is_declared_and_exported():
    from pinot_amd import _lib as L
    src = open(os.path.join(ROOT, "include", "pinot_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    assert re.search(r"\bint32_t\s+pa_query_eq_jit\s*\(\s*const\s+pa_query\s*\*\s*q\s*\)\s*;", src)
    assert "pa_query_eq_jit" in L.EXPORTED
    assert L.lib().pa_query_eq_jit(None) == -1  # (not prepared)
    assert L.ABI_VERSION == 5 and L.lib().pa_abi_version() == 5


def test_tunings_are_known():
    """eq_jit takes -1 (the planner decides), 0 and 1; eqs_dbg = 1 skips kernel work, so it marks the results invalid."""
    from pinot_amd import _lib as L
    lib = L.lib()
    spec = L.QuerySpec()
    spec.num_aggs = 1
    spec.aggs[0].type = L.PA_AGG_COUNT
    q = L.check_ptr(lib.pa_query_create(ctypes.byref(spec), 0), "pa_query_create")
    try:
        for v in (-1, 0, 1):
            assert lib.pa_query_set_tuning(q, b"eq_jit", v) == 0
        assert lib.pa_query_set_tuning(q, b"eq_jit", 2) == -1
        assert b"eq_jit" in lib.pa_last_error()
        assert lib.pa_query_results_invalid(q) == 0
        assert lib.pa_query_set_tuning(q, b"eqs_dbg", 1) == 0
        assert lib.pa_query_results_invalid(q) == 1
        assert lib.pa_query_set_tuning(q, b"eqs_dbg", 0) == 0
        assert lib.pa_query_results_invalid(q) == 0
    finally:
        lib.pa_query_destroy(q)


def test_source_string_is_self_contained():
    """build.py pastes the descriptors into the kernel's source string; the kernel defines no copy of its own."""
    from pinot_amd import build
    assert "eqs_jit.hip" in build.JIT_SOURCES
    raw = open(os.path.join(ROOT, "pinot_amd", "csrc", "eqs_jit.hip")).read()
    for st in ("struct EqsSeg", "struct EqsHdr", "struct JitArgs"):
        assert st not in raw, st
    text = build.jit_source_text("eqs_jit.hip")
    assert "struct EqsSeg" in text and '#include "' not in text

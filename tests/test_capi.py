"""The C-ABI library builds, loads and exports every entry point include/pinot_amd.h declares (no GPU calls)."""
import ctypes
import os
import re

from conftest import ROOT


def _declared():
    src = open(os.path.join(ROOT, "include", "pinot_amd.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    return sorted(set(re.findall(r"\b(pa_[a-z_0-9]+)\s*\(", src)))


def test_header_matches_binding():
    from pinot_amd import _lib
    assert _declared() == sorted(_lib.EXPORTED)


def test_library_exports_every_symbol():
    from pinot_amd import build, _lib
    path = build.build()
    lib = ctypes.CDLL(path)
    missing = [s for s in _declared() if not hasattr(lib, s)]
    assert not missing, missing
    assert _lib.lib().pa_abi_version() == _lib.ABI_VERSION


def test_struct_layout_matches_header():
    """ctypes mirrors of the C structs have the sizes the compiled library expects."""
    from pinot_amd import _lib as L
    # pa_query_spec: 4 + 16*8 + 4 + 48*4 + 4 + 8*4 (+4 pad) + 8*8 + 4 (+4 pad) + 16*24 + 4 + 4
    assert ctypes.sizeof(L.LeafSpec) == 8
    assert ctypes.sizeof(L.AggSpec) == 24
    assert ctypes.sizeof(L.LeafParams) == 72  # (+ RAW_SET values, num_values: ABI 4)
    assert ctypes.sizeof(L.QuerySpec) == 848  # (+ flags2, reserved2)


def test_no_stray_environment_reads():
    """The library's plans and results do not depend on the process environment: every getenv of csrc (the hiprtc kernel
    sources included) lies in pa_host.h and reads one of the two variables that only log. Overrides are tunings carried
    by the query (pa_tuning.h, pa_query_set_tuning)."""
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    seen = []
    for f in sorted(os.listdir(csrc)):
        if not f.endswith((".hip", ".h")):
            continue
        text = open(os.path.join(csrc, f)).read()
        for m in re.finditer(r"getenv", text):
            assert f == "pa_host.h", (f, text.count("\n", 0, m.start()) + 1)
            arg = re.match(r'getenv\(\s*"([^"]*)"\s*\)', text[m.start():])
            assert arg and arg.group(1) in ("PA_DEBUG_PLAN", "PA_JIT_LOG"), text[m.start():m.start() + 60]
            seen.append(arg.group(1))
    assert sorted(set(seen)) == ["PA_DEBUG_PLAN", "PA_JIT_LOG"]


def test_tuning_calls():
    """pa_query_set_tuning / pa_query_results_invalid on a query of zero segments (pa_query_create binds nothing and
    touches no device): a known name with a value in its range is taken; an unknown name and a value outside the range
    fail with a message; a tuning that skips kernel work marks the results invalid."""
    from pinot_amd import _lib as L
    lib = L.lib()
    spec = L.QuerySpec()
    spec.num_aggs = 1
    spec.aggs[0].type = L.PA_AGG_COUNT
    q = L.check_ptr(lib.pa_query_create(ctypes.byref(spec), 0), "pa_query_create")
    try:
        assert lib.pa_query_results_invalid(q) == 0
        assert lib.pa_query_set_tuning(q, b"gdl_nd", 8) == 0
        assert lib.pa_query_set_tuning(q, b"gdl_nd", -1) == 0  # (back to the planner's choice)
        assert lib.pa_query_set_tuning(q, b"no_such_tuning", 1) == -1  # PA_EINVAL
        assert b"no_such_tuning" in lib.pa_last_error()
        assert lib.pa_query_set_tuning(q, b"gdl_ring", 5) == -1
        assert b"gdl_ring" in lib.pa_last_error()
        assert lib.pa_query_set_tuning(q, b"gdl_dbg", 4) == -1
        assert lib.pa_query_set_tuning(None, b"gdl_nd", 8) == -1
        assert lib.pa_query_results_invalid(q) == 0
        assert lib.pa_query_set_tuning(q, b"gdl_dbg", 1) == 0
        assert lib.pa_query_results_invalid(q) == 1
        assert lib.pa_query_set_tuning(q, b"gdl_dbg", 0) == 0
        assert lib.pa_query_results_invalid(q) == 0
    finally:
        lib.pa_query_destroy(q)
    assert lib.pa_query_results_invalid(None) == -1


def test_product_path_does_not_import_oracle():
    """The oracle is a checker only: nothing under pinot_amd/ may import, link or execute it."""
    for dirpath, _, files in os.walk(os.path.join(ROOT, "pinot_amd")):
        for f in files:
            if f.endswith((".py", ".hip", ".h", ".cpp")):
                text = open(os.path.join(dirpath, f)).read()
                assert "import oracle" not in text and "from oracle" not in text and "liboracle" not in text, f


def test_jit_descriptors_have_one_definition():
    """The hiprtc kernels' descriptors (JitSeg, JitArgs, PveSeg, PveArgs) have one definition, pa_jit_abi.h, with its
    layout static_asserts: the host includes it and build.py pastes it into the kernels' source strings, so no kernel
    source defines a copy of its own (round 5 kept hand-mirrored host structs)."""
    from pinot_amd import build
    csrc = os.path.join(ROOT, "pinot_amd", "csrc")
    abi = open(os.path.join(csrc, build.JIT_ABI)).read()
    assert "static_assert(sizeof(JitSeg)" in abi and "static_assert(sizeof(PveSeg)" in abi
    for name in build.JIT_SOURCES:
        raw = open(os.path.join(csrc, name)).read()
        assert '#include "%s"' % build.JIT_ABI in raw, name
        for st in ("struct JitSeg", "struct JitArgs", "struct PveSeg", "struct PveArgs"):
            assert st not in raw, (name, st)
        text = build.jit_source_text(name)
        assert abi.replace("#pragma once\n", "") in text and '#include "' not in text, name
    assert '#include "%s"' % build.JIT_ABI in open(os.path.join(csrc, "pa_host.h")).read()

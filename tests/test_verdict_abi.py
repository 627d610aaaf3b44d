"""CPU: the verdict ABI (include/maxcover.h mac_verdict, mac_cons_explain_f64, mac_verdict_read,
MAC_OPT_VERDICTS): the record's layout, the symbols, and the errors that need no context. The size
and N > 2048 errors are reported after the null-context check, so they need a context and sit with
the GPU tests (tests/test_gpu_verdicts.py test_matrix_errors)."""
import ctypes
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ("mac_cons_explain_f64", "mac_verdict_read")


def test_record_layout(pkg):
    V, dt = pkg._lib.Verdict, pkg._lib.VERDICT_DTYPE
    assert ctypes.sizeof(V) == 64 and dt.itemsize == 64
    want = {"reasons": 0, "pairs": 4, "n_uav": 8, "first_uav": 32, "reserved": 56}
    for name, off in want.items():
        assert getattr(V, name).offset == off, name
        assert dt.fields[name][1] == off, name
    assert dt["n_uav"].shape == dt["first_uav"].shape == (6,) and dt["reserved"].shape == (2,)
    assert pkg._lib.MAC_VERDICT_KINDS == 6
    assert pkg._lib.VERDICT_KINDS == ("cons3", "cons8", "cons7", "cons4", "cons5", "cons6")
    # a ctypes record and a numpy record are the same bytes
    v = V(0x22, 3, (ctypes.c_int32 * 6)(0, 2, 0, 0, 0, 1), (ctypes.c_int32 * 6)(-1, 4, -1, -1, -1, 7))
    r = np.frombuffer(bytes(v), dtype=dt)[0]
    assert int(r["reasons"]) == 0x22 and int(r["pairs"]) == 3
    assert r["n_uav"].tolist() == [0, 2, 0, 0, 0, 1] and r["first_uav"].tolist() == [-1, 4, -1, -1, -1, 7]


def test_header_constants(pkg):
    src = open(os.path.join(ROOT, "include", "maxcover.h")).read()
    defs = dict(re.findall(r"#define\s+(MAC_\w+)\s+(0x[0-9a-fA-F]+u?|\d+)", src))
    assert int(defs["MAC_VERDICT_KINDS"]) == 6 and int(defs["MAC_OPT_VERDICTS"]) == 8
    assert int(defs["MAC_PROF_ROLES"]) == 12   # the verdict launches take no role
    for q, k in enumerate(pkg._lib.VERDICT_KINDS):
        assert int(defs["MAC_REJ_" + k.upper()].rstrip("u"), 16) == 1 << q
        assert getattr(pkg._lib, "MAC_REJ_" + k.upper()) == 1 << q
    assert pkg._lib.MAC_OPT_VERDICTS == 8


def test_symbols_declared_and_exported(pkg):
    L = pkg.load_library()
    src = open(os.path.join(ROOT, "include", "maxcover.h")).read()
    src = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    declared = set(re.findall(r"\b(mac_\w+)\s*\(", src))
    for s in SYMBOLS:
        assert s in declared and s in pkg._lib.EXPORTS and hasattr(L, s), s
    assert declared == set(pkg._lib.EXPORTS)
    assert "mac_verdict" in re.findall(r"}\s*(mac_\w+);", src)


def test_null_context_errors(pkg):
    L = pkg.load_library()
    INVAL = pkg._lib.MAC_E_INVAL
    assert L.mac_set_option(None, pkg._lib.MAC_OPT_VERDICTS, 1) == INVAL
    out = np.zeros(2, dtype=pkg._lib.VERDICT_DTYPE)
    c = np.zeros((2, 6))
    dp = ctypes.POINTER(ctypes.c_double)
    rc = L.mac_cons_explain_f64(None, c.ctypes.data_as(dp), 6, 2, None, None, 1.0, None, None,
                                out.ctypes.data_as(ctypes.POINTER(pkg._lib.Verdict)))
    assert rc == INVAL and "null" in L.mac_last_error().decode()
    # (the null context wins over a bad size)
    rc = L.mac_cons_explain_f64(None, c.ctypes.data_as(dp), 7, 2, None, None, 1.0, None, None,
                                out.ctypes.data_as(ctypes.POINTER(pkg._lib.Verdict)))
    assert rc == INVAL
    n = ctypes.c_int64(5)
    assert L.mac_verdict_read(None, ctypes.byref(n), None, None, None, 0) == INVAL
    assert n.value == 5
    assert not out.view(np.uint8).any()   # nothing was written

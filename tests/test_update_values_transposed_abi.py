"""CPU tier of update_values for transposed handles (include/spmv_mi355x.h "new values for an existing handle", TRANSPOSED HANDLES):
spmv_mi355x_update_values_prepare_transposed and spmv_mi355x_update_values_count are declared, exported and bound, and what can be
refused without a handle is refused with the entry's name in last_error — in a child process that sees no device at all, so the
refusal provably comes before a device is touched."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np

import spmv_mi355x as E

from conftest import ROOT

NAMES = ("spmv_mi355x_update_values_prepare_transposed", "spmv_mi355x_update_values_count")


def test_both_symbols_are_declared_exported_and_bound():
    header = open(os.path.join(ROOT, "include", "spmv_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert re.search(r"\bint\s+spmv_mi355x_update_values_prepare_transposed\s*\(\s*spmv_mi355x_matrix\s*\*\s*At\s*,\s*long\s+m\s*,\s*long\s+n\s*,"
                     r"\s*const\s+int32_t\s*\*\s*row_ptr\s*,\s*const\s+int32_t\s*\*\s*col_idx\s*\)\s*;", code)
    assert re.search(r"\blong\s+spmv_mi355x_update_values_count\s*\(\s*const\s+spmv_mi355x_matrix\s*\*\s*A\s*\)\s*;", code)
    assert "left to a later change" not in header
    lib = E.lib()
    for name in NAMES:
        assert name in E.SYMBOLS and hasattr(lib, name), name
    assert lib.spmv_mi355x_update_values_count.restype is C.c_long
    assert callable(E.Matrix.update_values_prepare_transposed) and callable(E.Matrix.update_values_count)


def test_count_of_a_null_handle():
    assert E.lib().spmv_mi355x_update_values_count(None) == -1


def test_prepare_transposed_refuses_a_null_handle():
    lib = E.lib()
    rp = np.array([0, 1, 2, 3], np.int32)
    ci = np.array([0, 1, 2], np.int32)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    for arrays in ((p(rp), p(ci)), (None, p(ci)), (p(rp), None), (None, None)):
        assert lib.spmv_mi355x_update_values_prepare_transposed(None, C.c_long(3), C.c_long(3), *arrays) == 1
        msg = lib.spmv_mi355x_last_error()
        assert b"update_values_prepare_transposed" in msg and b"NULL" in msg, msg
    assert rp.tolist() == [0, 1, 2, 3] and ci.tolist() == [0, 1, 2]


def test_matrix_update_values_checks_against_the_count():
    """Matrix.update_values sizes its argument by update_values_count(), not by nnz"""

    class Handle:
        nnz, h = 3, None
        update_values_count = lambda self: 7

    try:
        E.Matrix.update_values(Handle(), np.ones(3))
    except ValueError as e:
        assert "7 entries" in str(e)
    else:
        raise AssertionError("a value array of nnz entries passed the length check of a handle whose updates read 7")


CHILD = r"""
import ctypes as C, json
import numpy as np
import spmv_mi355x as E

L = E.lib()
rp = np.array([0, 1, 2, 3], np.int32)
ci = np.array([0, 1, 2], np.int32)
p = lambda a: a.ctypes.data_as(C.c_void_p)
rc = L.spmv_mi355x_update_values_prepare_transposed(None, C.c_long(3), C.c_long(3), p(rp), p(ci))
print("RESULT " + json.dumps(dict(devices=E.device_count(), rc=rc, err=L.spmv_mi355x_last_error().decode(),
                                  count=L.spmv_mi355x_update_values_count(None))))
"""


def test_the_null_refusal_needs_no_device():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "spmv-research_amd", "python")] + [q for q in env.get("PYTHONPATH", "").split(os.pathsep) if q])
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    got = json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])
    assert got["devices"] == 0, "the child was meant to see no device"
    assert got["rc"] == 1 and "update_values_prepare_transposed" in got["err"] and "NULL handle" in got["err"], got
    assert got["count"] == -1

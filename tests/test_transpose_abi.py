"""opts.transpose (include/spmv_mi355x.h "transposed handles") at the C ABI, without a GPU: the field is the last of the options and
defaults to 0, a struct_size that ends before it hides it, the getter takes a NULL handle, and every request that can be refused from
the arguments alone is refused with a message that names the field — in a child process that sees no device at all, so the refusals
provably come before a device is touched."""
import ctypes as C
import json
import os
import subprocess
import sys

import spmv_mi355x as E

from conftest import ROOT


def test_transpose_is_the_last_option_and_defaults_to_zero(tmp_path):
    """the header's field against the binding's mirror of it (a property over the bytes behind value_storage: the field took the
    struct's tail padding, and Opts._fields_ is pinned by the ABI tests of the earlier options): same offset, same size, last"""
    src = tmp_path / "layout.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "spmv_mi355x.h"\nint main(void) {\n'
                   'spmv_mi355x_opts o; printf("%zu %zu %zu\\n", offsetof(spmv_mi355x_opts, transpose), sizeof(o.transpose), sizeof(o));\nreturn 0; }\n')
    exe = tmp_path / "layout"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    off, size, total = map(int, subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split())
    assert (off, size, total) == (E.OPTS_TRANSPOSE_OFFSET, C.sizeof(C.c_int), C.sizeof(E.Opts))
    assert off + size == total, "transpose is not the last field of spmv_mi355x_opts"
    assert all(getattr(E.Opts, name).offset + getattr(E.Opts, name).size <= off for name, _ in E.Opts._fields_)
    o = E._make_opts({})
    assert o.transpose == 0
    o = E._make_opts({"transpose": 1, "value_storage": 1})
    assert (o.transpose, o.value_storage) == (1, 1)
    assert bytes(o)[off:off + 4] == (1).to_bytes(4, sys.byteorder) and o.struct_size == total


def test_getter_is_exported_and_takes_a_null_handle():
    assert "spmv_mi355x_transposed" in E.SYMBOLS
    fn = E.lib().spmv_mi355x_transposed
    fn.restype = C.c_int
    assert fn(None) == -1


CHILD = r"""
import ctypes as C, json, sys
import numpy as np
import spmv_mi355x as E

L = E.lib()
RP = np.array([0, 1, 2, 3], np.int32)
CI = np.array([0, 1, 2], np.int32)
VA = np.array([0.1, 0.3, 0.7])
p = lambda a: a.ctypes.data_as(C.c_void_p)


def create(struct_size=None, **opts):
    o = E._make_opts(opts)
    if struct_size is not None:
        o.struct_size = struct_size
    h = C.c_void_p()
    rc = L.spmv_mi355x_create(C.byref(h), C.c_int(E.CSR_VECTOR), C.c_int(E.F64), C.c_long(3), C.c_long(3), C.c_long(3), p(RP), p(CI), p(VA), C.byref(o))
    return rc, L.spmv_mi355x_last_error().decode()


def partitioned(**opts):
    o = E._make_opts(opts)
    h = C.c_void_p()
    rc = L.spmv_mi355x_create_partitioned(C.byref(h), C.c_int(2), None, C.c_int(0), C.c_int(E.SELL_C_SIGMA), C.c_int(E.F64), C.c_long(3), C.c_long(3),
                                          C.c_long(3), p(RP), p(CI), p(VA), C.byref(o))
    return rc, L.spmv_mi355x_last_error().decode()


out = dict(devices=E.device_count(),
           two=create(transpose=2), minus=create(transpose=-1), symmetric=create(transpose=1, symmetric_input=1),
           partitioned=partitioned(transpose=1), partitioned_two=partitioned(transpose=2),
           plain=create(), asked=create(transpose=1),
           short=create(struct_size=E.OPTS_TRANSPOSE_OFFSET, transpose=2))
print("RESULT " + json.dumps(out))
"""


def _child():
    env = dict(os.environ, HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="", CUDA_VISIBLE_DEVICES="")
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "spmv-research_amd", "python")] + [q for q in env.get("PYTHONPATH", "").split(os.pathsep) if q])
    r = subprocess.run([sys.executable, "-c", CHILD], capture_output=True, text=True, timeout=120, env=env, cwd=ROOT)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads([l for l in r.stdout.splitlines() if l.startswith("RESULT ")][0][7:])


def test_refusals_without_a_device():
    got = _child()
    assert got["devices"] == 0, "the child was meant to see no device"
    for case in ("two", "minus", "symmetric", "partitioned", "partitioned_two"):
        rc, err = got[case]
        assert rc == 1 and "transpose" in err, (case, rc, err)
    assert "symmetric" in got["symmetric"][1]
    # what the field allows gets past the check: the no-device error, never a message about transpose
    for case in ("plain", "asked"):
        rc, err = got[case]
        assert rc == 1 and "transpose" not in err and "no HIP device" in err, (case, rc, err)
    # a caller whose struct_size ends before the field gets transpose = 0, whatever the bytes behind its struct hold
    rc, err = got["short"]
    assert rc == 1 and "transpose" not in err and "no HIP device" in err, (rc, err)

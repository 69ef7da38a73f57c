"""opts.value_storage (fp32-stored values under fp64 vectors; include/spmv_mi355x.h "mixed precision") at the C ABI, without a GPU:
the field is the last of the options, the query is exported and takes a NULL handle, and every request the SELL delta layout
cannot serve is refused by spmv_mi355x_create with a message that names the field — before a device is looked for, so the
refusals are the same on a machine without one."""
import ctypes as C

import numpy as np
import pytest

import spmv_mi355x as E

RP = np.array([0, 1, 2], np.int32)
CI = np.array([0, 1], np.int32)
VA = np.array([0.1, 0.3])


def _create(fmt, precision, **opts):
    o = E.Opts()
    o.struct_size = C.sizeof(E.Opts)
    o.device = -1
    for k, v in opts.items():
        setattr(o, k, v)
    h = C.c_void_p()
    rc = E.lib().spmv_mi355x_create(C.byref(h), C.c_int(fmt), C.c_int(precision), C.c_long(2), C.c_long(2), C.c_long(2),
                                    RP.ctypes.data_as(C.c_void_p), CI.ctypes.data_as(C.c_void_p), VA.ctypes.data_as(C.c_void_p), C.byref(o))
    err = E.lib().spmv_mi355x_last_error().decode()
    if rc == 0:
        E.lib().spmv_mi355x_destroy(h)
    return rc, err


def test_value_storage_is_the_last_option():
    assert E.Opts._fields_[-1] == ("value_storage", C.c_int)
    assert E.Opts.value_storage.offset + C.sizeof(C.c_int) <= C.sizeof(E.Opts)
    assert all(getattr(E.Opts, name).offset < E.Opts.value_storage.offset for name, _ in E.Opts._fields_[:-1])


def test_query_is_exported_and_takes_a_null_handle():
    assert "spmv_mi355x_value_storage" in E.SYMBOLS
    fn = E.lib().spmv_mi355x_value_storage
    fn.restype = C.c_int
    assert fn(None) not in (E.F64, E.F32)


CONTRADICTIONS = [
    ("csr_scalar", E.CSR_SCALAR, {}), ("csr_vector", E.CSR_VECTOR, {}), ("csr_merge", E.CSR_MERGE, {}), ("coo", E.COO, {}),
    ("csr_stream", E.CSR_STREAM, {}),
    ("sell_window_on", E.SELL_C_SIGMA, {"sell_window": 1}),
    ("sell_delta_off", E.SELL_C_SIGMA, {"sell_delta": 2}),
    ("sell_c_16", E.SELL_C_SIGMA, {"sell_c": 16}), ("sell_c_32", E.SELL_C_SIGMA, {"sell_c": 32}), ("sell_c_256", E.SELL_C_SIGMA, {"sell_c": 256}),
    ("sell_values_on", E.SELL_C_SIGMA, {"sell_values": 1}),
]


@pytest.mark.parametrize("name,fmt,opts", CONTRADICTIONS, ids=[c[0] for c in CONTRADICTIONS])
def test_requests_the_delta_layout_cannot_serve_are_refused(name, fmt, opts):
    rc, err = _create(fmt, E.F64, value_storage=1, **opts)
    assert rc == 1 and "value_storage" in err, (rc, err)


@pytest.mark.parametrize("value", (2, -1, 7))
@pytest.mark.parametrize("precision", (E.F64, E.F32))
def test_unknown_value_storage_is_refused(value, precision):
    rc, err = _create(E.SELL_C_SIGMA, precision, value_storage=value)
    assert rc == 1 and "value_storage" in err, (rc, err)


def test_accepted_requests_get_past_the_check():
    """what the field allows reaches the next stage of create(): a handle on a machine with a GPU, the no-device error without one —
    never a message about value_storage"""
    for precision, opts in ((E.F64, {}), (E.F64, {"sell_c": 64, "sell_delta": 1, "sell_values": 2, "sell_window": 2}),
                            (E.F32, {}), (E.F32, {"sell_c": 16})):
        rc, err = _create(E.SELL_C_SIGMA, precision, value_storage=1, **opts)
        assert rc == 0 or "value_storage" not in err, (precision, opts, err)
    rc, err = _create(E.CSR_VECTOR, E.F32, value_storage=1)         # fp32 vectors: the field changes nothing, whatever the format
    assert rc == 0 or "value_storage" not in err, err

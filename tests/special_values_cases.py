"""Inputs and expectations of the special-value tests (test_special_values_cases.py on the CPU, test_gpu_special_values.py on the GPU):
matrices with ragged rows and empty rows in every 64-row slice, x vectors that hold ONE Inf or NaN, and x vectors whose every product
is subnormal. Nothing here touches the engine; everything is computed once (lru_cache) and handed out read-only.

The contract these pin (include/spmv_mi355x.h, "special values"): y[i] of y = A x is non-finite exactly for the rows i that store an
entry in a column j with non-finite x[j]; beta = 0 overwrites whatever y held; subnormal products are not flushed."""
import functools

import numpy as np

M = 1000                                           # 15 full slices of 64 rows and one of 40
SHAPES = ((150, 1200), (5000, 70_000), (2_000_000, 2_000_000))       # (span, n)
NAMES = tuple(f"span{span}-n{n}" for span, n in SHAPES)
INT32_ONLY = NAMES[2]                              # exists to reach the int32 index mode: SELL variants only
NNZ = 5623
POISON = (np.inf, -np.inf, np.nan)
MAX_READER_SHARE = 0.05                            # of the rows, per poisoned column
SUBNORMAL_SCALE = {np.float32: -130, np.float64: -1040}              # x = uniform(-1, 1) * 2**scale
SUBNORMAL_UNIT = {np.float32: 2.0 ** -149, np.float64: 2.0 ** -1074}


def _readonly(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


def row_lengths():
    i = np.arange(M)
    lens = np.where(i % 7 == 3, 0, 1 + (37 * i) % 12)
    lens[[100, 700]] = 40
    lens[M - 1] = 0
    return lens


@functools.lru_cache(maxsize=None)
def ragged(span, n):
    """The CSR of an M x n matrix: row i is empty when i % 7 == 3 (and the last row is), else holds 1 + (37 i) % 12 entries, rows 100
    and 700 hold 40; its columns are a sorted random subset of the `span` consecutive columns that start at
    min(i * ((n - span) // M), n - span), the first and the last of them left out (so that no row stores column 0 or column n - 1);
    values uniform(-1, 1), none of them 0."""
    rng = np.random.default_rng(1000 + span)
    lens = row_lengths()
    rp = np.zeros(M + 1, np.int32)
    np.cumsum(lens, out=rp[1:])
    ci = np.empty(int(rp[M]), np.int32)
    stride = (n - span) // M
    for i in np.nonzero(lens)[0]:
        start = min(int(i) * stride, n - span)
        ci[rp[i]:rp[i + 1]] = start + 1 + np.sort(rng.choice(span - 2, int(lens[i]), replace=False))
    va = rng.uniform(-1, 1, int(rp[M]))
    va[va == 0] = 0.5
    rp, ci, va, lens = _readonly(rp, ci, va, lens)
    case = dict(name=f"span{span}-n{n}", span=span, n=n, m=M, rp=rp, ci=ci, va=va, lens=lens)
    # ---- what the tests rely on
    assert int(rp[M]) == NNZ and ci.min() > 0 and ci.max() < n - 1 and np.all(va != 0)
    for s in range(0, M, 64):
        assert (lens[s:s + 64] == 0).any() and (lens[s:s + 64] > 0).any(), f"slice {s // 64} does not mix empty and non-empty rows"
    return case


def step_spread(case):
    """The widest spread of the columns that the rows of one UNSORTED slice (64 consecutive rows) hold at one step: what decides between
    8-bit deltas (< 256), 16-bit deltas (< 65 536) and int32 indices when the rows stay where they are (sell_sigma = 64 keeps every row
    in its slice)."""
    rp, ci, lens = case["rp"], case["ci"], case["lens"]
    widest = 0
    for s in range(0, M, 64):
        rows = np.arange(s, min(M, s + 64))
        for k in range(int(lens[rows].max())):
            c = ci[rp[rows[lens[rows] > k]] + k]
            widest = max(widest, int(c.max() - c.min()))
    return widest


def readers(case, column):
    """mask of the rows that store an entry in `column`"""
    rows = np.repeat(np.arange(M), case["lens"])
    out = np.zeros(M, bool)
    out[rows[case["ci"] == column]] = True
    return out


@functools.lru_cache(maxsize=None)
def _base_x(span, n):
    return _readonly(np.random.default_rng(2000 + span).uniform(-1, 1, n))[0]


def poisoned(case, column, kind):
    """the case's finite x, uniform(-1, 1), with entry `column` replaced by POISON[kind % 3] (a fresh array)"""
    x = _base_x(case["span"], case["n"]).copy()
    x[column] = POISON[kind % 3]
    return x


@functools.lru_cache(maxsize=None)
def _poison(span, n):
    case = ragged(span, n)
    rng = np.random.default_rng(2500 + span)
    drawn = []
    while len(drawn) < 6:                                       # six distinct stored columns
        c = int(case["ci"][rng.integers(0, NNZ)])
        if c not in drawn:
            drawn.append(c)
    columns = (0, n - 1) + tuple(drawn)
    vectors = []
    for k, c in enumerate(columns):
        share = readers(case, c).mean()
        assert share <= MAX_READER_SHARE, f"column {c} is read by {share:.1%} of the rows"
        assert (share > 0) == (k >= 2), f"column {c}: {share:.1%} of the rows read it"
        vectors.append(_readonly(poisoned(case, c, k))[0])
    return columns, tuple(vectors)


def poison_vectors(case):
    """(columns, vectors): eight copies of one finite x, uniform(-1, 1), each with ONE entry replaced, cycling +Inf, -Inf, NaN: column
    0, column n - 1 (no row stores either: every y must stay finite) and six columns drawn from col_idx, each read by at least one row
    and by at most 5 % of them. Vector k is poisoned(case, columns[k], k)."""
    return _poison(case["span"], case["n"])


def _oracle():
    import oracle as orc
    orc.build()
    return orc


@functools.lru_cache(maxsize=256)
def _expectation(span, n, column, kind, dtype):
    case = ragged(span, n)
    orc = _oracle()
    x = poisoned(case, column, kind)
    y_ref = orc.csr_spmv(case["rp"], case["ci"], case["va"], x, dtype)
    finite = np.isfinite(y_ref)
    # a stored value (none is 0, none can overflow: |a|, |x| < 1) times Inf or NaN is never finite
    np.testing.assert_array_equal(finite, ~readers(case, column), err_msg=f"{case['name']}: the oracle's finite rows, column {column}")
    x[column] = 0.0
    absrow = orc.csr_spmv(case["rp"], case["ci"], np.abs(case["va"]), np.abs(x))
    return _readonly(y_ref, finite, absrow)


def expectation_at(case, column, kind, dtype):
    """For x = poisoned(case, column, kind) in precision `dtype`: (the oracle's csr_spmv, its isfinite mask — asserted to be "the row
    does not store `column`" —, absrow = sum_j |a_ij x_j| over the finite entries of x, in fp64)."""
    return _expectation(case["span"], case["n"], int(column), int(kind) % 3, np.dtype(dtype).type)


def expectation(case, k, dtype):
    """expectation_at for poison vector k"""
    return expectation_at(case, poison_vectors(case)[0][k], k, dtype)


@functools.lru_cache(maxsize=None)
def _subnormal(span, n, dtype):
    case = ragged(span, n)
    orc = _oracle()
    x = (np.random.default_rng(3000 + span).uniform(-1, 1, n) * 2.0 ** SUBNORMAL_SCALE[dtype]).astype(dtype)
    assert np.all(np.abs(x) < np.finfo(dtype).tiny) and np.count_nonzero(x) > 0.99 * n
    y_ref = orc.csr_spmv(case["rp"], case["ci"], case["va"], x, dtype)
    absrow = orc.csr_spmv(case["rp"], case["ci"], np.abs(case["va"]), np.abs(x.astype(np.float64)))
    filled = case["lens"] > 0
    share = np.count_nonzero(y_ref[filled]) / filled.sum()
    assert share >= 0.9, f"{case['name']} {np.dtype(dtype).name}: the oracle's y is non-zero in {share:.1%} of the non-empty rows"
    return _readonly(x, y_ref, absrow)


def subnormal(case, dtype):
    """(x, y_ref, absrow): x = uniform(-1, 1) * 2^-130 (fp32) / 2^-1040 (fp64) in precision `dtype`, so that every product a_ij x_j is
    subnormal — 2^18 / 2^33 or more units of its precision for all but the smallest factors — with the oracle's y (non-zero in at least
    90 % of the non-empty rows) and absrow in fp64."""
    return _subnormal(case["span"], case["n"], np.dtype(dtype).type)


def subnormal_bound(case, absrow, dtype, tol, unit=None):
    """|y - y_ref| allowed for a kernel that reorders a row's sum: tol * absrow for the order, plus one rounding of at most one unit per
    product (sums of subnormals are exact). `unit`: SUBNORMAL_UNIT[dtype] unless a layout is recorded as flushing."""
    unit = SUBNORMAL_UNIT[np.dtype(dtype).type] if unit is None else unit
    return tol * absrow + case["lens"] * unit


def cases():
    return tuple(ragged(span, n) for span, n in SHAPES)

"""CPU tier of the special-value tests: the conditions special_values_cases.py promises to the GPU tier (test_gpu_special_values.py),
checked without the engine — the slice mix, the index modes the three shapes land in, the reader caps of the poisoned columns, the
reader masks against a scipy restatement, and the subnormal inputs. Prints the counts."""
import numpy as np
import pytest
import scipy.sparse as sp

import special_values_cases as sv


@pytest.fixture(scope="module", params=range(len(sv.SHAPES)), ids=sv.NAMES)
def case(request):
    return sv.ragged(*sv.SHAPES[request.param])


def _scipy(case):
    return sp.csr_matrix((case["va"], case["ci"], case["rp"]), shape=(case["m"], case["n"]))


def test_rows_and_slices(case):
    lens = case["lens"]
    assert case["m"] == 1000 and lens.sum() == sv.NNZ == 5623 and lens[100] == lens[700] == 40 and lens[-1] == 0
    assert np.all(lens[np.arange(1000) % 7 == 3] == 0) and lens.max() == 40
    assert np.all(np.diff(case["rp"]) == lens)
    mixed = 0
    for s in range(0, 1000, 64):
        part = lens[s:s + 64]
        assert (part == 0).any() and (part > 0).any()
        mixed += 1
        for i in range(s, min(1000, s + 64)):
            c = case["ci"][case["rp"][i]:case["rp"][i + 1]]
            assert np.all(np.diff(c) > 0), f"row {i}: columns not strictly ascending"
    assert mixed == 16
    A = _scipy(case)
    assert A.has_sorted_indices and A.nnz == 5623
    # no row stores the first or the last column: poisoning them must leave every y finite
    assert A[:, 0].nnz == 0 and A[:, case["n"] - 1].nnz == 0
    assert np.all(case["va"] != 0) and np.all(np.abs(case["va"]) < 1)
    print(f"{case['name']}: 16 slices, each with empty and non-empty rows; {int((lens == 0).sum())} empty rows, {A.nnz} entries")


def test_shapes_reach_the_three_index_modes():
    spread = [sv.step_spread(sv.ragged(*s)) for s in sv.SHAPES]
    print("widest per-step column spread of an unsorted slice:", dict(zip(sv.NAMES, spread)))
    assert spread[0] < 256, "8-bit deltas"
    assert 256 <= spread[1] < 65536, "16-bit deltas"
    assert spread[2] >= 65536, "int32 indices"


def test_poison_vectors(case):
    columns, vectors = sv.poison_vectors(case)
    n = case["n"]
    assert len(columns) == len(vectors) == 8 and columns[:2] == (0, n - 1) and len(set(columns)) == 8
    A = _scipy(case)
    base = vectors[0].copy()
    base[0] = vectors[1][0]
    assert np.all(np.isfinite(base)) and np.all(np.abs(base) < 1)
    shares = []
    for k, (c, x) in enumerate(zip(columns, vectors)):
        bad = np.nonzero(~np.isfinite(x))[0]
        assert bad.tolist() == [c], f"vector {k}: exactly one poisoned entry"
        want = sv.POISON[k % 3]
        assert (np.isnan(x[c]) and np.isnan(want)) or x[c] == want
        keep = np.arange(n) != c
        np.testing.assert_array_equal(x[keep], base[keep])
        assert not x.flags.writeable
        # the reader mask against scipy's column
        mask = np.zeros(case["m"], bool)
        mask[A[:, c].nonzero()[0]] = True
        np.testing.assert_array_equal(sv.readers(case, c), mask)
        shares.append(mask.mean())
        assert mask.mean() <= sv.MAX_READER_SHARE
        assert mask.any() == (k >= 2)
    print(f"{case['name']}: poisoned columns {columns}, share of the rows that read them {[f'{s:.1%}' for s in shares]}")


def test_expectation_masks(case, oracle):
    columns, vectors = sv.poison_vectors(case)
    A = _scipy(case)
    for dtype in (np.float64, np.float32):
        for k, c in enumerate(columns):
            y_ref, finite, absrow = sv.expectation(case, k, dtype)
            assert y_ref.dtype == np.dtype(dtype) and absrow.dtype == np.float64 and not y_ref.flags.writeable
            np.testing.assert_array_equal(finite, ~sv.readers(case, c))
            assert np.all(np.isfinite(absrow))
            # the finite rows against scipy on the cleaned vector (a reached row would differ: it lost a term)
            clean = np.nan_to_num(vectors[k], nan=0.0, posinf=0.0, neginf=0.0)
            want = A @ clean
            tol = 1e-12 if dtype == np.float64 else 1e-5
            assert np.all(np.abs(y_ref[finite].astype(np.float64) - want[finite]) <= tol * absrow[finite] + 1e-300)
            np.testing.assert_allclose(absrow, abs(A) @ np.abs(clean), rtol=1e-13, atol=0)
        print(f"{case['name']} {np.dtype(dtype).name}: non-finite rows per vector "
              f"{[int((~sv.expectation(case, k, dtype)[1]).sum()) for k in range(8)]}")


def test_subnormal_inputs(case, oracle):
    for dtype in (np.float32, np.float64):
        x, y_ref, absrow = sv.subnormal(case, dtype)
        tiny = np.finfo(dtype).tiny
        assert x.dtype == np.dtype(dtype) and np.all(np.abs(x) < tiny) and np.all(np.isfinite(y_ref))
        filled = case["lens"] > 0
        share = np.count_nonzero(y_ref[filled]) / filled.sum()
        assert share >= 0.9 and np.all(y_ref[~filled] == 0)
        # every product is subnormal, and most of them many units large
        prod = np.abs(case["va"] * x[case["ci"]].astype(np.float64))
        unit = sv.SUBNORMAL_UNIT[dtype]
        assert prod.max() < tiny
        big = np.mean(prod >= 2.0 ** 10 * unit)
        assert big > 0.95
        # a kernel that flushes misses the bound by a wide margin: zeros against the reference
        bound = sv.subnormal_bound(case, absrow, dtype, 1e-12 if dtype == np.float64 else 1e-5)
        missed = np.abs(y_ref.astype(np.float64))[filled] > bound[filled]
        assert missed.mean() >= 0.9
        print(f"{case['name']} {np.dtype(dtype).name}: y non-zero in {share:.1%} of the non-empty rows, {big:.1%} of the products hold "
              f"2^10 units or more, median |y| / bound = {np.median(np.abs(y_ref.astype(np.float64))[filled] / bound[filled]):.3g}")

// SpGEMM plans (include/spmv_mi355x.h "SpGEMM"): the checks of spgemm_create in the header's order, the symbolic phase (the products
// per row, the bins, the COUNT launches, the scan, the FILL launches), the numeric launches and the C ABI. The row kernel is in
// kernels_spgemm.hip, the mapping in spgemm.hpp.

#include <algorithm>
#include <chrono>
#include <cstring>
#include <vector>

#include <hipcub/hipcub.hpp>

#include "handle.hpp"
#include "solvers_common.hpp"
#include "spgemm.hpp"

namespace spmv {

static_assert(SPGEMM_BINS == SPMV_MI355X_SPGEMM_BINS, "the header's rows-per-bin arrays and spgemm.hpp disagree");

// row_ptr from 0 and monotone, columns in [0, cols)
static int
spgemm_check_csr(const char * what, const char * name, long rows, long cols, const int32_t * rp, const int32_t * ci)
{
	if (rp[0] != 0)
	{
		set_error("%s: %s_row_ptr must start at 0 (got %d)", what, name, rp[0]);
		return 1;
	}
	for (long i = 0; i < rows; i++)
		if (rp[i + 1] < rp[i])
		{
			set_error("%s: %s_row_ptr is not monotone at row %ld", what, name, i);
			return 1;
		}
	if (rp[rows] > 0 && !ci)
	{
		set_error("%s: NULL argument ( %s_col_idx )", what, name);
		return 1;
	}
	for (long j = 0; j < rp[rows]; j++)
		if (ci[j] < 0 || ci[j] >= cols)
		{
			set_error("%s: column index %d of %s out of range [0,%ld) at entry %ld", what, ci[j], name, cols, j);
			return 1;
		}
	return 0;
}

// a column twice in a row of B: the products of one step would land on one entry. A sorted copy of each row, no array of n.
static int
spgemm_check_b_duplicates(const char * what, long k, const int32_t * rp, const int32_t * ci)
{
	std::vector<int32_t> row;
	for (long i = 0; i < k; i++)
	{
		if (rp[i + 1] - rp[i] < 2)
			continue;
		row.assign(ci + rp[i], ci + rp[i + 1]);
		std::sort(row.begin(), row.end());
		for (size_t t = 1; t < row.size(); t++)
			if (row[t] == row[t - 1])
			{
				set_error("%s: row %ld of B stores column %d twice: the products of one entry of A must land on distinct entries of C",
						what, i, row[t]);
				return 1;
			}
	}
	return 0;
}

static void
spgemm_free(spmv_mi355x_spgemm * P)
{
	for (void * p : P->owned)
		if (p)
			(void) hipFree(p);
	delete P;
}

static double
seconds_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// device allocations that die with the scope unless they are handed to the plan
struct SpgemmOwner {
	std::vector<void *> ptrs;
	size_t bytes = 0;
	~SpgemmOwner()
	{
		for (void * p : ptrs)
			(void) hipFree(p);
	}
	template <typename T>
	int up(const T * src, size_t count, T ** out)
	{
		if (upload_bytes(src, count * sizeof(T), 0, (void **) out))
			return 1;
		ptrs.push_back(*out);
		bytes += std::max<size_t>(count * sizeof(T), 8);
		return 0;
	}
	template <typename T>
	int alloc(size_t count, T ** out)
	{
		if (dev_alloc_bytes((void **) out, count * sizeof(T)))
			return 1;
		ptrs.push_back(*out);
		bytes += std::max<size_t>(count * sizeof(T), 8);
		return 0;
	}
	void hand_over(spmv_mi355x_spgemm * P)
	{
		P->owned.insert(P->owned.end(), ptrs.begin(), ptrs.end());
		P->device_bytes += bytes;
		ptrs.clear();
		bytes = 0;
	}
};

// the rows of every bin, the slab's table size and the grids, from w[i] = the bound of row i's width
struct SpgemmBins {
	std::vector<int32_t> rows[SPGEMM_BINS];
	int grid[SPGEMM_BINS] = {};
	long slab_t = 0;

	template <typename W>
	void build(long m, W width_of, size_t slab_entry_bytes)
	{
		long widest = 0;
		for (long i = 0; i < m; i++)
		{
			const long w = width_of(i);
			const int b = spgemm_bin_of(w);
			rows[b].push_back((int32_t) i);
			if (b == SPGEMM_BINS - 1)
				widest = std::max(widest, w);
		}
		for (int b = 0; b < SPGEMM_BINS; b++)
		{
			const long groups = ((long) rows[b].size() + SPGEMM_BIN_ROWS[b] - 1) / SPGEMM_BIN_ROWS[b];
			grid[b] = (int) std::min<long>(groups, b == SPGEMM_BINS - 1 ? SPGEMM_GLOBAL_GRID : SPGEMM_MAX_GRID);
		}
		if (widest > 0)
		{
			slab_t = (long) 1 << spgemm_log_table(widest);
			int & g = grid[SPGEMM_BINS - 1];
			while (g > 1 && (size_t) g * (size_t) slab_t * slab_entry_bytes > SPGEMM_SLAB_BYTES)
				g = (g + 1) / 2;
		}
	}
};

static int
spgemm_error_word(const char * what, const spmv_mi355x_spgemm * P)
{
	int word = 0;
	HIP_TRY(hipMemcpy(&word, P->d_error, sizeof(int), hipMemcpyDeviceToHost));
	if (word)
	{
		set_error("%s: spgemm: internal: table overflow in row %d", what, word - 1);
		return 1;
	}
	return 0;
}

// the device part of create: everything from the upload of the patterns to C's pattern and the numeric bins
static int
spgemm_symbolic(const char * what, spmv_mi355x_spgemm * P, const int32_t * a_rp, const int32_t * a_ci, const int32_t * b_rp,
		const int32_t * b_ci)
{
	const long m = P->m;
	SpgemmOwner keep, tmp;
	if (keep.up(a_rp, (size_t) m + 1, &P->d_a_rp) || keep.up(a_ci, (size_t) P->nnz_a, &P->d_a_ci) ||
	    keep.up(b_rp, (size_t) P->k + 1, &P->d_b_rp) || keep.up(b_ci, (size_t) P->nnz_b, &P->d_b_ci) ||
	    keep.alloc((size_t) m, &P->d_products) || keep.alloc(1, &P->d_error))
		return 1;
	HIP_TRY(hipMemset(P->d_error, 0, sizeof(int)));
	// the products per row, and the bins on min(products, n)
	if (launch_spgemm_products(m, P->d_a_rp, P->d_a_ci, P->d_b_rp, P->d_products, nullptr))
		return 1;
	std::vector<long> products((size_t) m);
	if (m > 0)
		HIP_TRY(hipMemcpy(products.data(), P->d_products, (size_t) m * sizeof(long), hipMemcpyDeviceToHost));
	for (long i = 0; i < m; i++)
	{
		P->products += products[i];
		P->max_row_products = std::max(P->max_row_products, products[i]);
	}
	SpgemmBins sym;
	sym.build(m, [&](long i) { return std::min(products[i], P->n); }, sizeof(int));
	int * d_sym[SPGEMM_BINS], * d_probes, * d_slab;
	long * d_width, * d_offsets;
	for (int b = 0; b < SPGEMM_BINS; b++)
	{
		P->symbolic_bin_rows[b] = (long) sym.rows[b].size();
		if (tmp.up(sym.rows[b].data(), sym.rows[b].size(), &d_sym[b]))
			return 1;
	}
	if (tmp.alloc((size_t) m + 1, &d_width) || tmp.alloc((size_t) m + 1, &d_offsets) || tmp.alloc((size_t) m, &d_probes) ||
	    tmp.alloc((size_t) sym.grid[SPGEMM_BINS - 1] * (size_t) sym.slab_t, &d_slab))
		return 1;
	HIP_TRY(hipMemset(d_width, 0, ((size_t) m + 1) * sizeof(long)));
	HIP_TRY(hipMemset(d_probes, 0, std::max<size_t>((size_t) m * sizeof(int), 8)));
	SpgemmArrays arr;
	memset(&arr, 0, sizeof(arr));
	arr.a_rp = P->d_a_rp;
	arr.a_ci = P->d_a_ci;
	arr.b_rp = P->d_b_rp;
	arr.b_ci = P->d_b_ci;
	arr.n = P->n;
	arr.products = P->d_products;
	arr.width = d_width;
	arr.probes = d_probes;
	arr.slab_keys = d_slab;
	arr.slab_t = sym.slab_t;
	arr.error = P->d_error;
	for (int b = 0; b < SPGEMM_BINS; b++)
		if (launch_spgemm_rows(SPGEMM_COUNT, b, arr, d_sym[b], (long) sym.rows[b].size(), sym.grid[b], nullptr))
			return 1;
	// c_row_ptr: an exclusive scan in 64 bits, so that a product beyond the int32 range is seen before C is allocated
	{
		size_t bytes = 0;
		char * scan_tmp = nullptr;
		HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, d_width, d_offsets, (int) (m + 1), (hipStream_t) 0));
		if (tmp.alloc(bytes, &scan_tmp))
			return 1;
		HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, bytes, d_width, d_offsets, (int) (m + 1), (hipStream_t) 0));
	}
	long nnz_c = 0;
	HIP_TRY(hipMemcpy(&nnz_c, d_offsets + m, sizeof(long), hipMemcpyDeviceToHost));
	if (spgemm_error_word(what, P))
		return 1;
	if (nnz_c >= 0x80000000L)
	{
		set_error("%s: symbolic: C has %ld entries, beyond the int32 index range (nnz(C) must stay below 2^31)", what, nnz_c);
		return 1;
	}
	P->nnz_c = nnz_c;
	std::vector<int> probes((size_t) m);
	if (m > 0)
		HIP_TRY(hipMemcpy(probes.data(), d_probes, (size_t) m * sizeof(int), hipMemcpyDeviceToHost));
	for (long i = 0; i < m; i++)
		P->symbolic_probes += probes[i];
	if (keep.alloc((size_t) m + 1, &P->d_c_rp) || keep.alloc((size_t) nnz_c, &P->d_c_ci))
		return 1;
	if (launch_spgemm_narrow(d_offsets, P->d_c_rp, m + 1, nullptr))
		return 1;
	P->c_rp.assign((size_t) m + 1, 0);
	HIP_TRY(hipMemcpy(P->c_rp.data(), P->d_c_rp, ((size_t) m + 1) * sizeof(int), hipMemcpyDeviceToHost));
	// the bins on the true width of C's rows: the columns are written from tables of that size, and the numeric pass keeps them
	SpgemmBins num;
	num.build(m, [&](long i) { return (long) P->c_rp[i + 1] - P->c_rp[i]; }, sizeof(int) + sizeof(double));
	for (long i = 0; i < m; i++)
		P->max_row_c = std::max<long>(P->max_row_c, P->c_rp[i + 1] - P->c_rp[i]);
	for (int b = 0; b < SPGEMM_BINS; b++)
	{
		P->numeric_bin_rows[b] = (long) num.rows[b].size();
		P->grid[b] = num.grid[b];
		if (keep.up(num.rows[b].data(), num.rows[b].size(), &P->d_bin[b]))
			return 1;
	}
	P->slab_t = num.slab_t;
	const size_t slab = (size_t) num.grid[SPGEMM_BINS - 1] * (size_t) num.slab_t;
	if (keep.alloc(slab, &P->d_slab_keys) || keep.alloc(slab, &P->d_slab_vals))
		return 1;
	arr.c_rp = P->d_c_rp;
	arr.c_ci = P->d_c_ci;
	arr.slab_keys = P->d_slab_keys;
	arr.slab_t = P->slab_t;
	for (int b = 0; b < SPGEMM_BINS; b++)
		if (launch_spgemm_rows(SPGEMM_FILL, b, arr, P->d_bin[b], P->numeric_bin_rows[b], P->grid[b], nullptr))
			return 1;
	HIP_TRY(hipDeviceSynchronize());
	if (spgemm_error_word(what, P))
		return 1;
	keep.hand_over(P);
	return 0;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int
spmv_mi355x_spgemm_create(spmv_mi355x_spgemm ** out, int device, long m, long k, long n, const int32_t * a_row_ptr,
		const int32_t * a_col_idx, const int32_t * b_row_ptr, const int32_t * b_col_idx)
{
	const char * what = "spgemm_create";
	if (out)
		*out = nullptr;
	// 1. the sizes
	const long dims[3] = {m, k, n};
	for (int d = 0; d < 3; d++)
		if (dims[d] < 0 || dims[d] >= 0x7fffffffL)
		{
			set_error("%s: %c = %ld out of range [0, 2^31 - 1)", what, "mkn"[d], dims[d]);
			return 1;
		}
	// 2. NULL pointers (a col_idx may be NULL where its matrix has no entries: checked with the pattern)
	if (!out || !a_row_ptr || !b_row_ptr)
	{
		set_error("%s: NULL argument (%s%s%s )", what, !out ? " out" : "", !a_row_ptr ? " a_row_ptr" : "", !b_row_ptr ? " b_row_ptr" : "");
		return 1;
	}
	// 3. the two patterns, 4. B stores no column twice in a row
	if (spgemm_check_csr(what, "a", m, k, a_row_ptr, a_col_idx) || spgemm_check_csr(what, "b", k, n, b_row_ptr, b_col_idx) ||
	    spgemm_check_b_duplicates(what, k, b_row_ptr, b_col_idx))
		return 1;
	// 5. the device
	int ndev = 0;
	spmv_mi355x_device_count(&ndev);
	if (ndev < 1)
	{
		set_error("%s: no HIP device available: this engine has no CPU fallback", what);
		return 1;
	}
	if (device < 0)
		HIP_TRY(hipGetDevice(&device));
	if (device >= ndev)
	{
		set_error("%s: device %d out of range (%d devices)", what, device, ndev);
		return 1;
	}
	HIP_TRY(hipSetDevice(device));
	spmv_mi355x_spgemm * P = new spmv_mi355x_spgemm();
	P->device = device;
	P->m = m;
	P->k = k;
	P->n = n;
	P->nnz_a = a_row_ptr[m];
	P->nnz_b = b_row_ptr[k];
	// 6. the symbolic phase: nnz(C) >= 2^31 is refused there
	const auto t0 = std::chrono::steady_clock::now();
	if (spgemm_symbolic(what, P, a_row_ptr, a_col_idx, b_row_ptr, b_col_idx))
	{
		spgemm_free(P);
		return 1;
	}
	P->symbolic_seconds = seconds_since(t0);
	*out = P;
	return 0;
}

int
spmv_mi355x_spgemm_destroy(spmv_mi355x_spgemm * P)
{
	if (!P)
		return 0;
	(void) hipSetDevice(P->device);
	spgemm_free(P);
	return 0;
}

int
spmv_mi355x_spgemm_pattern(const spmv_mi355x_spgemm * P, int32_t * c_row_ptr_out, int32_t * c_col_idx_out)
{
	if (!P || !c_row_ptr_out || (P->nnz_c > 0 && !c_col_idx_out))
	{
		set_error("spgemm_pattern: NULL argument (%s%s%s )", !P ? " P" : "", !c_row_ptr_out ? " c_row_ptr_out" : "",
				P && P->nnz_c > 0 && !c_col_idx_out ? " c_col_idx_out" : "");
		return 1;
	}
	memcpy(c_row_ptr_out, P->c_rp.data(), P->c_rp.size() * sizeof(int32_t));
	if (P->nnz_c > 0)
	{
		HIP_TRY(hipSetDevice(P->device));
		HIP_TRY(hipMemcpy(c_col_idx_out, P->d_c_ci, (size_t) P->nnz_c * sizeof(int32_t), hipMemcpyDeviceToHost));
	}
	return 0;
}

int
spmv_mi355x_spgemm_multiply_device_async(spmv_mi355x_spgemm * P, const double * a_values_dev, const double * b_values_dev,
		double * c_values_dev, void * hip_stream)
{
	const bool work = P && P->nnz_c > 0;
	if (!P || (work && (!a_values_dev || !b_values_dev || !c_values_dev)))
	{
		set_error("spgemm_multiply: NULL argument (%s%s%s%s )", !P ? " P" : "", work && !a_values_dev ? " a_values" : "",
				work && !b_values_dev ? " b_values" : "", work && !c_values_dev ? " c_values" : "");
		return 1;
	}
	if (!work)                                        // C has no entries: nothing is read and nothing is written
		return 0;
	HIP_TRY(hipSetDevice(P->device));
	SpgemmArrays arr;
	memset(&arr, 0, sizeof(arr));
	arr.a_rp = P->d_a_rp;
	arr.a_ci = P->d_a_ci;
	arr.b_rp = P->d_b_rp;
	arr.b_ci = P->d_b_ci;
	arr.n = P->n;
	arr.products = P->d_products;
	arr.c_rp = P->d_c_rp;
	arr.c_ci = P->d_c_ci;
	arr.a_va = a_values_dev;
	arr.b_va = b_values_dev;
	arr.c_va = c_values_dev;
	arr.slab_keys = P->d_slab_keys;
	arr.slab_vals = P->d_slab_vals;
	arr.slab_t = P->slab_t;
	arr.error = P->d_error;
	for (int b = 0; b < SPGEMM_BINS; b++)
		if (launch_spgemm_rows(SPGEMM_NUMERIC, b, arr, P->d_bin[b], P->numeric_bin_rows[b], P->grid[b], (hipStream_t) hip_stream))
			return 1;
	return 0;
}

int
spmv_mi355x_spgemm_multiply(spmv_mi355x_spgemm * P, const double * a_values, const double * b_values, double * c_values_out)
{
	const char * what = "spgemm_multiply";
	const bool work = P && P->nnz_c > 0;
	if (!P || (work && (!a_values || !b_values || !c_values_out)))
	{
		set_error("%s: NULL argument (%s%s%s%s )", what, !P ? " P" : "", work && !a_values ? " a_values" : "",
				work && !b_values ? " b_values" : "", work && !c_values_out ? " c_values_out" : "");
		return 1;
	}
	P->multiply_seconds = 0;
	if (!work)
		return 0;
	HIP_TRY(hipSetDevice(P->device));
	// the values are staged for this call only: the plan holds patterns, never values
	SpgemmOwner tmp;
	double * d_a, * d_b, * d_c;
	if (tmp.up(a_values, (size_t) P->nnz_a, &d_a) || tmp.up(b_values, (size_t) P->nnz_b, &d_b) || tmp.alloc((size_t) P->nnz_c, &d_c))
		return 1;
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	HIP_TRY(hipEventCreate(&e1));
	int rc = hipEventRecord(e0, nullptr) != hipSuccess;
	rc = rc || spmv_mi355x_spgemm_multiply_device_async(P, d_a, d_b, d_c, nullptr);
	if (!rc && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess)
	{
		float ms = 0;
		(void) hipEventElapsedTime(&ms, e0, e1);
		P->multiply_seconds = ms * 1e-3;
	}
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	if (rc)
		return 1;
	HIP_TRY(hipMemcpy(c_values_out, d_c, (size_t) P->nnz_c * sizeof(double), hipMemcpyDeviceToHost));
	return spgemm_error_word(what, P);
}

int
spmv_mi355x_spgemm_info(const spmv_mi355x_spgemm * P, spmv_mi355x_spgemm_stats * info)
{
	const char * what = "spgemm_info";
	if (!P || !info)
	{
		set_error("%s: NULL argument (%s%s )", what, !P ? " P" : "", !info ? " info" : "");
		return 1;
	}
	if (!info_size_ok(what, info))
		return 1;
	spmv_mi355x_spgemm_stats s;
	memset(&s, 0, sizeof(s));
	s.m = P->m;
	s.k = P->k;
	s.n = P->n;
	s.nnz_a = P->nnz_a;
	s.nnz_b = P->nnz_b;
	s.nnz_c = P->nnz_c;
	s.products = P->products;
	s.max_row_products = P->max_row_products;
	s.max_row_c = P->max_row_c;
	for (int b = 0; b < SPGEMM_BINS; b++)
	{
		s.symbolic_bin_rows[b] = P->symbolic_bin_rows[b];
		s.numeric_bin_rows[b] = P->numeric_bin_rows[b];
	}
	s.symbolic_probes = P->symbolic_probes;
	s.symbolic_seconds = P->symbolic_seconds;
	s.multiply_seconds = P->multiply_seconds;
	s.device_bytes = (double) P->device_bytes;
	put_info(info, info->struct_size, s);
	return 0;
}

}  // extern "C"

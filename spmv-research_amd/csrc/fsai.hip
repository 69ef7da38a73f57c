// Factorized sparse approximate inverse handles (include/spmv_mi355x.h "FSAI"): the host pattern routine, the checks of
// fsai_create in the header's order, the setup (upload, the row kernel of kernels_fsai.hip bin by bin, download, the two
// spmv_mi355x_create calls) and the C ABI. Applying the handle is two SpMVs over G and G^t with one scratch vector between them.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "handle.hpp"
#include "fsai.hpp"

namespace spmv {

// row_ptr from 0 and monotone, columns in [0, n): the checks and the messages of spmv_mi355x_create
static int
fsai_check_csr(const char * what, long n, const int32_t * rp, const int32_t * ci)
{
	if (rp[0] != 0)
	{
		set_error("%s: row_ptr must start at 0 (got %d)", what, rp[0]);
		return 1;
	}
	for (long i = 0; i < n; i++)
		if (rp[i + 1] < rp[i])
		{
			set_error("%s: row_ptr is not monotone at row %ld", what, i);
			return 1;
		}
	for (long j = 0; j < rp[n]; j++)
		if (ci[j] < 0 || ci[j] >= n)
		{
			set_error("%s: column index %d out of range [0,%ld) at entry %ld", what, ci[j], n, j);
			return 1;
		}
	return 0;
}

// The pattern of tril(A~)^power, A~ = the lower triangle of A's pattern with the diagonal added; columns ascending. One marker array:
// row i of the next power is the union of the rows of tril(A~) that row i of this power names. The CSR has been checked.
static void
fsai_power_pattern(long n, const int32_t * rp, const int32_t * ci, int power, std::vector<int32_t> & out_rp, std::vector<int32_t> & out_ci)
{
	std::vector<int32_t> mark((size_t) n, -1);
	std::vector<int32_t> l_rp((size_t) n + 1, 0), l_ci;
	for (long i = 0; i < n; i++)
	{
		mark[i] = (int32_t) i;
		l_ci.push_back((int32_t) i);
		for (long j = rp[i]; j < rp[i + 1]; j++)
			if (ci[j] < i && mark[ci[j]] != i)
			{
				mark[ci[j]] = (int32_t) i;
				l_ci.push_back(ci[j]);
			}
		l_rp[i + 1] = (int32_t) l_ci.size();
	}
	std::vector<int32_t> cur_rp = l_rp, cur_ci = l_ci;
	for (int t = 2; t <= power; t++)
	{
		std::vector<int32_t> nx_rp((size_t) n + 1, 0), nx_ci;
		std::fill(mark.begin(), mark.end(), -1);
		for (long i = 0; i < n; i++)
		{
			for (long j = cur_rp[i]; j < cur_rp[i + 1]; j++)
				for (long e = l_rp[cur_ci[j]]; e < l_rp[cur_ci[j] + 1]; e++)
					if (mark[l_ci[e]] != i)
					{
						mark[l_ci[e]] = (int32_t) i;
						nx_ci.push_back(l_ci[e]);
					}
			nx_rp[i + 1] = (int32_t) nx_ci.size();
		}
		cur_rp.swap(nx_rp);
		cur_ci.swap(nx_ci);
	}
	for (long i = 0; i < n; i++)
		std::sort(cur_ci.begin() + cur_rp[i], cur_ci.begin() + cur_rp[i + 1]);
	out_rp.swap(cur_rp);
	out_ci.swap(cur_ci);
}

static bool
fsai_scalars_ok(const char * what, int format, int precision, long n, const spmv_mi355x_opts & o)
{
	if (precision != SPMV_MI355X_F64 && precision != SPMV_MI355X_F32)
		set_error("%s: unknown precision %d", what, precision);
	else if (format < 0 || format >= SPMV_MI355X_NUM_FORMATS)
		set_error("%s: unknown format %d", what, format);
	else if (n < 0 || n >= 0x7fffffffL)
		set_error("%s: n = %ld out of range [0, 2^31 - 1)", what, n);
	else if (o.transpose)
		set_error("%s: opts->transpose = %d: the library sets it itself, 0 for the handle of G and 1 for that of G^t", what, o.transpose);
	else if (o.symmetric_input)
		set_error("%s: opts->symmetric_input = %d: G is triangular, its handles are built from G's own CSR", what, o.symmetric_input);
	else if (o.row_begin || o.row_end || o.col_filter_mode)
		set_error("%s: opts name a row block or a column filter (row_begin %ld, row_end %ld, col_filter_mode %d): the "
				"row-partitioned form is not built", what, o.row_begin, o.row_end, o.col_filter_mode);
	else if (value_storage_check(what, o, format, precision))
		;                                     // create's own rule and message for opts->value_storage
	else
		return true;
	return false;
}

// 4. a column stored twice among the entries of a row with column <= row
static int
fsai_check_duplicates(const char * what, long n, const int32_t * rp, const int32_t * ci)
{
	std::vector<int32_t> mark((size_t) n, -1);
	for (long i = 0; i < n; i++)
		for (long j = rp[i]; j < rp[i + 1]; j++)
			if (ci[j] <= i)
			{
				if (mark[ci[j]] == i)
				{
					set_error("%s: row %ld of A stores column %d twice in its lower triangle: which value A(%ld, %d) has is not defined",
							what, i, ci[j], i, ci[j]);
					return 1;
				}
				mark[ci[j]] = (int32_t) i;
			}
	return 0;
}

// 5. the pattern of G
static int
fsai_check_pattern(const char * what, long n, const int32_t * rp, const int32_t * ci)
{
	if (rp[0] != 0)
	{
		set_error("%s: pat_row_ptr must start at 0 (got %d)", what, rp[0]);
		return 1;
	}
	for (long i = 0; i < n; i++)
		if (rp[i + 1] < rp[i])
		{
			set_error("%s: pat_row_ptr is not monotone at row %ld", what, i);
			return 1;
		}
	for (long i = 0; i < n; i++)
	{
		const long s = (long) rp[i + 1] - rp[i];
		for (long j = rp[i]; j < rp[i + 1]; j++)
		{
			if (ci[j] < 0 || ci[j] > i)
			{
				set_error("%s: the pattern's row %ld holds column %d: every column must lie in [0, row] (entries above the diagonal "
						"are not built)", what, i, ci[j]);
				return 1;
			}
			if (j > rp[i] && ci[j] <= ci[j - 1])
			{
				set_error("%s: the pattern's row %ld is not strictly ascending (column %d after %d)", what, i, ci[j], ci[j - 1]);
				return 1;
			}
		}
		if (s == 0 || ci[rp[i + 1] - 1] != i)
		{
			set_error("%s: the pattern's row %ld does not end with its diagonal entry (column %ld)", what, i, i);
			return 1;
		}
		if (s > SPMV_MI355X_FSAI_MAX_ROW)
		{
			set_error("%s: the pattern's row %ld has %ld entries, more than SPMV_MI355X_FSAI_MAX_ROW = %d", what, i, s,
					SPMV_MI355X_FSAI_MAX_ROW);
			return 1;
		}
	}
	return 0;
}

// 6. the diagonal of A: the first stored entry with column i
static int
fsai_check_diagonal(const char * what, long n, const int32_t * rp, const int32_t * ci, const double * va)
{
	for (long i = 0; i < n; i++)
	{
		long at = -1;
		for (long j = rp[i]; j < rp[i + 1] && at < 0; j++)
			if (ci[j] == i)
				at = j;
		if (at < 0)
		{
			set_error("%s: row %ld of A has no diagonal entry", what, i);
			return 1;
		}
		if (!std::isfinite(va[at]) || !(va[at] > 0))
		{
			set_error("%s: the diagonal of row %ld of A is %g: it must be finite and > 0", what, i, va[at]);
			return 1;
		}
	}
	return 0;
}

static void
fsai_free(spmv_mi355x_fsai * F)
{
	if (F->G)
		spmv_mi355x_destroy(F->G);
	if (F->Gt)
		spmv_mi355x_destroy(F->Gt);
	for (void * p : {F->d_scratch, F->d_in, F->d_out, F->d_scratch_multi, F->d_in_multi, F->d_out_multi})
		if (p)
			(void) hipFree(p);
	delete F;
}

static double
seconds_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

// the device part of the setup: G's values and the rows that fell back
static int
fsai_compute(spmv_mi355x_fsai * F, const int32_t * rp, const int32_t * ci, const double * va, const int32_t * prp, const int32_t * pci)
{
	const long n = F->n, nnz_a = rp[n], nnz = F->nnz;
	std::vector<int32_t> bins[FSAI_BINS];
	for (long i = 0; i < n; i++)
		bins[fsai_bin_of(prp[i + 1] - prp[i])].push_back((int32_t) i);
	struct Owner {
		std::vector<void *> ptrs;
		~Owner()
		{
			for (void * p : ptrs)
				(void) hipFree(p);
		}
		int up(const void * src, size_t bytes, void ** out)
		{
			if (upload_bytes(src, bytes, 0, out))
				return 1;
			ptrs.push_back(*out);
			return 0;
		}
		int alloc(size_t bytes, void ** out)
		{
			if (dev_alloc_bytes(out, bytes))
				return 1;
			ptrs.push_back(*out);
			return 0;
		}
	} own;
	void * d_rp, * d_ci, * d_va, * d_prp, * d_pci, * d_g, * d_fb, * d_bin[FSAI_BINS];
	if (own.up(rp, (size_t) (n + 1) * 4, &d_rp) || own.up(ci, (size_t) nnz_a * 4, &d_ci) || own.up(va, (size_t) nnz_a * 8, &d_va) ||
	    own.up(prp, (size_t) (n + 1) * 4, &d_prp) || own.up(pci, (size_t) nnz * 4, &d_pci) || own.alloc((size_t) nnz * 8, &d_g) ||
	    own.alloc((size_t) n * 4, &d_fb))
		return 1;
	for (int b = 0; b < FSAI_BINS; b++)
		if (own.up(bins[b].data(), bins[b].size() * 4, &d_bin[b]))
			return 1;
	const FsaiArrays arr = {(const int *) d_rp, (const int *) d_ci, (const double *) d_va, (const int *) d_prp, (const int *) d_pci,
	                        (double *) d_g, (int *) d_fb};
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	HIP_TRY(hipEventCreate(&e1));
	HIP_TRY(hipEventRecord(e0, nullptr));
	int rc = 0;
	for (int b = 0; b < FSAI_BINS && !rc; b++)
		rc = launch_fsai_rows(b, arr, (const int *) d_bin[b], (long) bins[b].size(), nullptr);
	if (!rc && hipEventRecord(e1, nullptr) == hipSuccess && hipEventSynchronize(e1) == hipSuccess)
	{
		float ms = 0;
		(void) hipEventElapsedTime(&ms, e0, e1);
		F->kernel_seconds = ms * 1e-3;
	}
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	if (rc)
		return 1;
	const auto t_down = std::chrono::steady_clock::now();
	F->values.assign((size_t) nnz, 0.0);
	std::vector<int32_t> fb((size_t) n, 0);
	HIP_TRY(hipMemcpy(F->values.data(), d_g, (size_t) nnz * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(fb.data(), d_fb, (size_t) n * 4, hipMemcpyDeviceToHost));
	F->download_seconds = seconds_since(t_down);
	F->fallback_rows = 0;
	for (long i = 0; i < n; i++)
		F->fallback_rows += fb[i] != 0;
	return 0;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int
spmv_mi355x_fsai_pattern(long n, const int32_t * row_ptr, const int32_t * col_idx, int power, int32_t ** row_ptr_out,
		int32_t ** col_idx_out)
{
	const char * what = "fsai_pattern";
	if (row_ptr_out)
		*row_ptr_out = nullptr;
	if (col_idx_out)
		*col_idx_out = nullptr;
	if (n < 0 || n >= 0x7fffffffL)
	{
		set_error("%s: n = %ld out of range [0, 2^31 - 1)", what, n);
		return 1;
	}
	if (power < 1 || power > 3)
	{
		set_error("%s: power must be 1, 2 or 3 (got %d)", what, power);
		return 1;
	}
	if (!row_ptr || (!col_idx && row_ptr[n] > 0) || !row_ptr_out || !col_idx_out)
	{
		set_error("%s: NULL argument (%s%s%s%s )", what, !row_ptr ? " row_ptr" : "", row_ptr && !col_idx ? " col_idx" : "",
				!row_ptr_out ? " row_ptr_out" : "", !col_idx_out ? " col_idx_out" : "");
		return 1;
	}
	if (fsai_check_csr(what, n, row_ptr, col_idx))
		return 1;
	std::vector<int32_t> rp, ci;
	fsai_power_pattern(n, row_ptr, col_idx, power, rp, ci);
	if (ci.size() >= 0x7fffffffUL)
	{
		set_error("%s: the pattern has %zu entries, beyond the int32 index range", what, ci.size());
		return 1;
	}
	int32_t * rp_out = (int32_t *) malloc(rp.size() * sizeof(int32_t));
	int32_t * ci_out = (int32_t *) malloc(std::max<size_t>(ci.size(), 1) * sizeof(int32_t));
	if (!rp_out || !ci_out)
	{
		free(rp_out);
		free(ci_out);
		set_error("%s: out of host memory (%zu entries)", what, ci.size());
		return 1;
	}
	memcpy(rp_out, rp.data(), rp.size() * sizeof(int32_t));
	if (!ci.empty())
		memcpy(ci_out, ci.data(), ci.size() * sizeof(int32_t));
	*row_ptr_out = rp_out;
	*col_idx_out = ci_out;
	return 0;
}

int
spmv_mi355x_fsai_create(spmv_mi355x_fsai ** out, int format, int precision, long n, const int32_t * row_ptr, const int32_t * col_idx,
		const double * values, const int32_t * pat_row_ptr, const int32_t * pat_col_idx, const spmv_mi355x_opts * opts_in)
{
	const char * what = "fsai_create";
	const auto t_start = std::chrono::steady_clock::now();
	if (out)
		*out = nullptr;
	// 1. the scalars
	spmv_mi355x_opts o;
	memset(&o, 0, sizeof(o));
	o.device = -1;
	if (opts_in)
	{
		const size_t sz = std::min<size_t>(sizeof(o), (size_t) std::max(opts_in->struct_size, 0));
		if (sz < 8)
		{
			set_error("%s: opts->struct_size not set", what);
			return 1;
		}
		memcpy(&o, opts_in, sz);
	}
	o.struct_size = (int) sizeof(o);
	if (!fsai_scalars_ok(what, format, precision, n, o))
		return 1;
	// 2. NULL pointers: the pattern comes as both arrays or as neither
	const bool entries = row_ptr && row_ptr[n] > 0;
	const bool pat_half = !pat_row_ptr != !pat_col_idx && !(pat_row_ptr && n == 0);
	if (!out || !row_ptr || (entries && (!col_idx || !values)) || pat_half)
	{
		set_error("%s: NULL argument (%s%s%s%s%s )", what, !out ? " out" : "", !row_ptr ? " row_ptr" : "",
				entries && !col_idx ? " col_idx" : "", entries && !values ? " values" : "",
				pat_half ? (!pat_row_ptr ? " pat_row_ptr" : " pat_col_idx") : "");
		return 1;
	}
	// 3. A's pattern, 4. its lower triangle stores no column twice
	if (fsai_check_csr(what, n, row_ptr, col_idx) || fsai_check_duplicates(what, n, row_ptr, col_idx))
		return 1;
	// 5. the pattern of G; NULL = the lower triangle of A's own, each row sorted (a missing diagonal is added here and refused in 6.)
	std::vector<int32_t> own_rp, own_ci;
	if (!pat_row_ptr)
	{
		fsai_power_pattern(n, row_ptr, col_idx, 1, own_rp, own_ci);
		pat_row_ptr = own_rp.data();
		pat_col_idx = own_ci.data();
	}
	if (fsai_check_pattern(what, n, pat_row_ptr, pat_col_idx))
		return 1;
	// 6. the diagonal of A
	if (fsai_check_diagonal(what, n, row_ptr, col_idx, values))
		return 1;
	// 7. the device
	int ndev = 0;
	spmv_mi355x_device_count(&ndev);
	if (ndev < 1)
	{
		set_error("%s: no HIP device available: this engine has no CPU fallback", what);
		return 1;
	}
	int device = o.device;
	if (device < 0)
		HIP_TRY(hipGetDevice(&device));
	if (device >= ndev)
	{
		set_error("%s: device %d out of range (%d devices)", what, device, ndev);
		return 1;
	}
	HIP_TRY(hipSetDevice(device));
	o.device = device;

	spmv_mi355x_fsai * F = new spmv_mi355x_fsai();
	F->precision = precision;
	F->f32 = precision == SPMV_MI355X_F32;
	F->device = device;
	F->format = format;
	F->n = n;
	F->nnz = pat_row_ptr[n];
	for (long i = 0; i < n; i++)
		F->max_row = std::max<long>(F->max_row, pat_row_ptr[i + 1] - pat_row_ptr[i]);
	if (n > 0)
	{
		if (fsai_compute(F, row_ptr, col_idx, values, pat_row_ptr, pat_col_idx))
		{
			fsai_free(F);
			return 1;
		}
		// the two handles, values narrowed as create narrows them; a refusal of create keeps its own message
		auto t0 = std::chrono::steady_clock::now();
		int rc = spmv_mi355x_create(&F->G, format, precision, n, n, F->nnz, pat_row_ptr, pat_col_idx, F->values.data(), &o);
		F->create_g_seconds = seconds_since(t0);
		if (!rc)
		{
			o.transpose = 1;
			t0 = std::chrono::steady_clock::now();
			rc = spmv_mi355x_create(&F->Gt, format, precision, n, n, F->nnz, pat_row_ptr, pat_col_idx, F->values.data(), &o);
			F->create_gt_seconds = seconds_since(t0);
		}
		if (rc || dev_alloc_bytes(&F->d_scratch, (size_t) n * (F->f32 ? 4 : 8)))
		{
			std::string msg = spmv_mi355x_last_error();
			fsai_free(F);
			if (msg.rfind("fsai_create:", 0) != 0)
				set_error("%s: %s", what, msg.c_str());
			return 1;
		}
	}
	F->setup_seconds = seconds_since(t_start);
	*out = F;
	return 0;
}

int
spmv_mi355x_fsai_destroy(spmv_mi355x_fsai * F)
{
	if (!F)
		return 0;
	(void) hipSetDevice(F->device);
	fsai_free(F);
	return 0;
}

int
spmv_mi355x_fsai_apply_device_async(spmv_mi355x_fsai * F, const void * in_dev, void * out_dev, void * hip_stream)
{
	if (!F || (F->n > 0 && (!in_dev || !out_dev)))
	{
		set_error("fsai_apply: NULL argument (%s%s%s )", !F ? " F" : "", F && !in_dev ? " in" : "", F && !out_dev ? " out" : "");
		return 1;
	}
	if (F->n == 0)
		return 0;
	// the first product has left `in` behind when the second one writes `out`: in == out is legal
	if (spmv_mi355x_spmv_device_async(F->G, in_dev, F->d_scratch, 0, hip_stream))
		return 1;
	return spmv_mi355x_spmv_device_async(F->Gt, F->d_scratch, out_dev, 0, hip_stream);
}

int
spmv_mi355x_fsai_apply(spmv_mi355x_fsai * F, const void * in_host, void * out_host)
{
	if (!F || (F->n > 0 && (!in_host || !out_host)))
	{
		set_error("fsai_apply: NULL argument (%s%s%s )", !F ? " F" : "", F && !in_host ? " in" : "", F && !out_host ? " out" : "");
		return 1;
	}
	if (F->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(F->device));
	const size_t bytes = (size_t) F->n * (F->f32 ? 4 : 8);
	if (!F->d_in && (dev_alloc_bytes(&F->d_in, bytes) || dev_alloc_bytes(&F->d_out, bytes)))
		return 1;
	HIP_TRY(hipMemcpyAsync(F->d_in, in_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_fsai_apply_device_async(F, F->d_in, F->d_out, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(out_host, F->d_out, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

// in == out with equal ld is legal as in the single apply: the first SpMM has left `in` behind when the second writes `out`
int
spmv_mi355x_fsai_apply_multi_device_async(spmv_mi355x_fsai * F, int k, const void * in_dev, long ldin, void * out_dev, long ldout,
		void * hip_stream)
{
	if (!F || (F->n > 0 && (!in_dev || !out_dev)))
	{
		set_error("fsai_apply_multi: NULL argument (%s%s%s )", !F ? " F" : "", F && !in_dev ? " in" : "", F && !out_dev ? " out" : "");
		return 1;
	}
	if (k < 1)
	{
		set_error("fsai_apply_multi: k = %d: at least one column is needed", k);
		return 1;
	}
	if (ldin < k || ldout < k)
	{
		set_error("fsai_apply_multi: ldin = %ld, ldout = %ld: both must be >= k = %d", ldin, ldout, k);
		return 1;
	}
	if (in_dev == out_dev && ldin != ldout)
	{
		set_error("fsai_apply_multi: in == out needs ldin == ldout (got %ld and %ld)", ldin, ldout);
		return 1;
	}
	if (F->n == 0)
		return 0;
	if (k > F->multi_k)
	{
		// growing waits for whatever still reads the smaller block
		HIP_TRY(hipDeviceSynchronize());
		if (F->d_scratch_multi)
			(void) hipFree(F->d_scratch_multi);
		F->d_scratch_multi = nullptr;
		F->multi_k = 0;
		if (dev_alloc_bytes(&F->d_scratch_multi, (size_t) F->n * (size_t) k * (F->f32 ? 4 : 8)))
			return 1;
		F->multi_k = k;
	}
	if (spmv_mi355x_spmm_device_async(F->G, k, in_dev, ldin, F->d_scratch_multi, k, 0, hip_stream))
		return 1;
	return spmv_mi355x_spmm_device_async(F->Gt, k, F->d_scratch_multi, k, out_dev, ldout, 0, hip_stream);
}

int
spmv_mi355x_fsai_apply_multi(spmv_mi355x_fsai * F, int k, const void * in_host, void * out_host)
{
	if (!F || (F->n > 0 && (!in_host || !out_host)))
	{
		set_error("fsai_apply_multi: NULL argument (%s%s%s )", !F ? " F" : "", F && !in_host ? " in" : "", F && !out_host ? " out" : "");
		return 1;
	}
	if (k < 1)
	{
		set_error("fsai_apply_multi: k = %d: at least one column is needed", k);
		return 1;
	}
	if (F->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(F->device));
	const size_t bytes = (size_t) F->n * (size_t) k * (F->f32 ? 4 : 8);
	if (k > F->multi_host_k)
	{
		HIP_TRY(hipDeviceSynchronize());
		for (void ** p : {&F->d_in_multi, &F->d_out_multi})
		{
			if (*p)
				(void) hipFree(*p);
			*p = nullptr;
		}
		F->multi_host_k = 0;
		if (dev_alloc_bytes(&F->d_in_multi, bytes) || dev_alloc_bytes(&F->d_out_multi, bytes))
			return 1;
		F->multi_host_k = k;
	}
	HIP_TRY(hipMemcpyAsync(F->d_in_multi, in_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_fsai_apply_multi_device_async(F, k, F->d_in_multi, k, F->d_out_multi, k, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(out_host, F->d_out_multi, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

int
spmv_mi355x_fsai_values(const spmv_mi355x_fsai * F, double * out)
{
	if (!F || (F->nnz > 0 && !out))
	{
		set_error("fsai_values: NULL %s", !F ? "handle" : "out");
		return 1;
	}
	if (F->nnz > 0)
		memcpy(out, F->values.data(), (size_t) F->nnz * sizeof(double));
	return 0;
}

int
spmv_mi355x_fsai_matrices(const spmv_mi355x_fsai * F, spmv_mi355x_matrix ** G_out, spmv_mi355x_matrix ** Gt_out)
{
	if (!F)
	{
		set_error("fsai_matrices: NULL handle");
		return 1;
	}
	if (G_out)
		*G_out = F->G;
	if (Gt_out)
		*Gt_out = F->Gt;
	return 0;
}

int
spmv_mi355x_fsai_info(const spmv_mi355x_fsai * F, long * n_out, long * nnz_out, long * max_row_out, long * fallback_rows_out,
		double * kernel_seconds_out, double * setup_seconds_out)
{
	if (!F)
	{
		set_error("fsai_info: NULL handle");
		return 1;
	}
	if (n_out)
		*n_out = F->n;
	if (nnz_out)
		*nnz_out = F->nnz;
	if (max_row_out)
		*max_row_out = F->max_row;
	if (fallback_rows_out)
		*fallback_rows_out = F->fallback_rows;
	if (kernel_seconds_out)
		*kernel_seconds_out = F->kernel_seconds;
	if (setup_seconds_out)
		*setup_seconds_out = F->setup_seconds;
	return 0;
}

int
spmv_mi355x_fsai_setup_split(const spmv_mi355x_fsai * F, double * kernel_out, double * download_out, double * create_g_out,
		double * create_gt_out)
{
	if (!F)
	{
		set_error("fsai_setup_split: NULL handle");
		return 1;
	}
	if (kernel_out)
		*kernel_out = F->kernel_seconds;
	if (download_out)
		*download_out = F->download_seconds;
	if (create_g_out)
		*create_g_out = F->create_g_seconds;
	if (create_gt_out)
		*create_gt_out = F->create_gt_seconds;
	return 0;
}

double
spmv_mi355x_fsai_mem_footprint(const spmv_mi355x_fsai * F)
{
	if (!F || F->n == 0)
		return 0;
	return spmv_mi355x_mem_footprint(F->G) + spmv_mi355x_mem_footprint(F->Gt) + (double) F->n * (F->f32 ? 4 : 8);
}

}  // extern "C"

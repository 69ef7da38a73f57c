// ILU(0) handles (include/spmv_mi355x.h "ILU(0)"): the host checks, the analysis and the C ABI. Host code only; the
// kernels are in kernels_ilu0.hip.
//
// THE SCHEDULE. Row i needs the finished rows k of every stored k < i of row i: the level rule of trsv_analysis(LOWER) on A's
// pattern, and the levels are taken from there (trsv_analysis_blocked for a blocked handle, where the level WITHIN the block is the
// launch index, so all blocks run in the same launches). Level 0 has no k step and gets no launch; every later level is one launch.
// The order of the launches on the stream is the only ordering between levels.

#include <cmath>
#include <cstring>
#include <vector>

#include "handle.hpp"
#include "ilu0.hpp"
#include "trsv.hpp"

using namespace spmv;

namespace spmv {

constexpr unsigned ILU0_NO_BREAKDOWN = 0xffffffffu;

static void
ilu0_free(spmv_mi355x_ilu0 * F)
{
	for (void * p : F->owned)
		if (p)
			(void) hipFree(p);
	delete F;
}

// The checks 4 and 5 of the header: columns strictly ascending in every row, a stored diagonal in every row. dia receives the
// position of each diagonal.
static int
ilu0_check_rows(long n, const int32_t * rp, const int32_t * ci, std::vector<int32_t> & dia)
{
	long unsorted = n, missing = n;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(min : unsorted, missing) schedule(static, 4096)
	for (long i = 0; i < n; i++)
	{
		int32_t at = -1;
		for (long j = rp[i]; j < rp[i + 1]; j++)
		{
			if (j > rp[i] && ci[j] <= ci[j - 1])
				unsorted = std::min(unsorted, i);
			if (ci[j] == i)
				at = (int32_t) j;
		}
		dia[i] = at;
		if (at < 0)
			missing = std::min(missing, i);
	}
	if (unsorted < n)
	{
		for (long j = rp[unsorted] + 1; j < rp[unsorted + 1]; j++)
			if (ci[j] <= ci[j - 1])
			{
				set_error("ilu0_create: row %ld: column %d follows column %d: the columns of a row must be strictly ascending", unsorted,
						ci[j], ci[j - 1]);
				break;
			}
		return 1;
	}
	if (missing < n)
	{
		set_error("ilu0_create: row %ld has no diagonal entry (ILU(0) needs a stored diagonal in every row)", missing);
		return 1;
	}
	return 0;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_ilu0_create(spmv_mi355x_ilu0 ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, long block_rows, int device)
{
	if (out)
		*out = nullptr;
	// 1. scalars, 2. NULL pointers, 3. the pattern, 4. sorted rows, 5. the diagonal: all on the host; 6. the device
	if (n < 0 || n >= 0x7fffffffL)
	{
		set_error("ilu0_create: n = %ld out of range [0, 2^31 - 1)", n);
		return 1;
	}
	if (block_rows < -1 || block_rows > TRSV_BLOCK_ROWS_MAX)
	{
		set_error("ilu0_create: block_rows must be -1 (global), 0 (the default) or 1 .. %d (got %ld)", TRSV_BLOCK_ROWS_MAX, block_rows);
		return 1;
	}
	if (!out || !row_ptr || (!col_idx && row_ptr[n] > 0))
	{
		set_error("ilu0_create: NULL argument (%s%s%s )", !out ? " out" : "", !row_ptr ? " row_ptr" : "",
				row_ptr && !col_idx ? " col_idx" : "");
		return 1;
	}
	if (trsv_check_pattern("ilu0_create", n, row_ptr, col_idx))
		return 1;
	std::vector<int32_t> dia((size_t) n);
	if (ilu0_check_rows(n, row_ptr, col_idx, dia))
		return 1;
	int ndev = 0;
	spmv_mi355x_device_count(&ndev);
	if (ndev < 1)
	{
		set_error("ilu0_create: no HIP device available: this engine has no CPU fallback");
		return 1;
	}
	if (device < 0)
		HIP_TRY(hipGetDevice(&device));
	if (device >= ndev)
	{
		set_error("ilu0_create: device %d out of range (%d devices)", device, ndev);
		return 1;
	}
	HIP_TRY(hipSetDevice(device));

	const bool blocked = block_rows >= 0;
	TrsvAnalysis an;
	if (blocked)
		trsv_analysis_blocked(SPMV_MI355X_LOWER, n, row_ptr, col_idx, block_rows, an);
	else
		trsv_analysis(SPMV_MI355X_LOWER, n, row_ptr, col_idx, 0, an);
	spmv_mi355x_ilu0 * F = new spmv_mi355x_ilu0();
	F->device = device;
	F->n = n;
	F->nnz = row_ptr[n];
	F->block_rows = an.block_rows;
	F->blocks = an.blocks;
	F->levels = blocked ? an.max_block_levels : an.levels;
	const long B = an.block_rows;

	// the run of every row inside its block (the whole row for a global handle); columns ascend, so it is one run
	std::vector<int32_t> beg((size_t) n), end((size_t) n), level((size_t) n);
	long kept = 0;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(+ : kept) schedule(static, 4096)
	for (long i = 0; i < n; i++)
	{
		long b = row_ptr[i], e = row_ptr[i + 1];
		if (B)
		{
			const long c0 = i / B * B, c1 = c0 + B;
			while (col_idx[b] < c0)
				b++;
			while (col_idx[e - 1] >= c1)
				e--;
		}
		beg[i] = (int32_t) b;
		end[i] = (int32_t) e;
		kept += e - b;
		level[i] = an.level_of_row[i] - (B ? an.block_level[i / B] : 0);
	}
	F->nnz_dropped = F->nnz - kept;
	// rows by (level, row): the level WITHIN the block is the launch index
	F->level_ptr.assign((size_t) F->levels + 1, 0);
	for (long i = 0; i < n; i++)
		F->level_ptr[level[i] + 1]++;
	for (long l = 0; l < F->levels; l++)
	{
		F->max_level_rows = std::max<long>(F->max_level_rows, F->level_ptr[l + 1]);
		F->level_ptr[l + 1] += F->level_ptr[l];
	}
	std::vector<int32_t> rows((size_t) n);
	{
		std::vector<int32_t> next(F->level_ptr.begin(), F->level_ptr.end());
		for (long i = 0; i < n; i++)
			rows[next[level[i]]++] = (int32_t) i;
	}
	// lanes per row of each level, from the mean width of the level's rows, as csr_vector chooses them
	F->level_lanes.assign((size_t) F->levels, 4);
	for (long l = 0; l < F->levels; l++)
	{
		long width = 0;
		for (long t = F->level_ptr[l]; t < F->level_ptr[l + 1]; t++)
			width += end[rows[t]] - beg[rows[t]];
		F->level_lanes[l] = pick_lanes_per_row((double) width / (double) (F->level_ptr[l + 1] - F->level_ptr[l]));
	}

	const size_t nb = (size_t) n * sizeof(int32_t);
	struct Up { const void * src; size_t bytes; } ups[5] = {
		{col_idx, (size_t) F->nnz * sizeof(int32_t)}, {beg.data(), nb}, {dia.data(), nb}, {end.data(), nb}, {rows.data(), nb}};
	for (int k = 0; k < 5; k++)
	{
		if (upload_bytes(ups[k].src, ups[k].bytes, 0, &F->owned[k]))
		{
			ilu0_free(F);
			return 1;
		}
		F->mem_footprint += (double) ups[k].bytes;
	}
	// the breakdown word sits in a 16-byte block of its own, which is what a factor call resets
	if (dev_alloc_bytes(&F->owned[5], (size_t) F->nnz * sizeof(double)) || dev_alloc_bytes(&F->owned[6], 16)
			|| hipMemset(F->owned[6], 0xff, 16) != hipSuccess)
	{
		set_error("ilu0_create: out of device memory (%ld values)", F->nnz);
		ilu0_free(F);
		return 1;
	}
	F->mem_footprint += (double) F->nnz * sizeof(double) + 16;
	F->arr.col = (const int *) F->owned[0];
	F->arr.beg = (const int *) F->owned[1];
	F->arr.dia = (const int *) F->owned[2];
	F->arr.end = (const int *) F->owned[3];
	F->arr.rows = (const int *) F->owned[4];
	F->arr.f = (double *) F->owned[5];
	F->arr.breakdown = (unsigned *) F->owned[6];
	*out = F;
	return 0;
}

int
spmv_mi355x_ilu0_factor_device_async(spmv_mi355x_ilu0 * F, const double * values_dev, void * hip_stream)
{
	if (!F || (F->nnz > 0 && !values_dev))
	{
		set_error("ilu0_factor: NULL argument (%s%s )", !F ? " F" : "", F && !values_dev ? " values" : "");
		return 1;
	}
	F->factorizations++;
	if (F->n == 0)
		return 0;
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != F->device)
		HIP_TRY(hipSetDevice(F->device));
	hipStream_t st = (hipStream_t) hip_stream;
	HIP_TRY(hipMemsetAsync(F->arr.breakdown, 0xff, 16, st));
	if (launch_ilu0_begin(F->arr, F->nnz, values_dev, F->level_ptr[1], st))
		return 1;
	for (long l = 1; l < F->levels; l++)
		if (launch_ilu0_level(F->arr, F->level_ptr[l], F->level_ptr[l + 1] - F->level_ptr[l], F->level_lanes[l], st))
			return 1;
	return 0;
}

int
spmv_mi355x_ilu0_factor(spmv_mi355x_ilu0 * F, const double * values_host)
{
	if (!F || (F->nnz > 0 && !values_host))
	{
		set_error("ilu0_factor: NULL argument (%s%s )", !F ? " F" : "", F && !values_host ? " values" : "");
		return 1;
	}
	if (F->n == 0)
	{
		F->factorizations++;
		return 0;
	}
	HIP_TRY(hipSetDevice(F->device));
	// the values go straight into f; the first kernel then finds source and destination equal and only checks the pivots of level 0
	HIP_TRY(hipMemcpyAsync(F->arr.f, values_host, (size_t) F->nnz * sizeof(double), hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_ilu0_factor_device_async(F, F->arr.f, nullptr))
		return 1;
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

int
spmv_mi355x_ilu0_values_device(spmv_mi355x_ilu0 * F, const double ** f_dev_out)
{
	if (!F || !f_dev_out)
	{
		set_error("ilu0_values: NULL argument (%s%s )", !F ? " F" : "", !f_dev_out ? " out" : "");
		return 1;
	}
	if (F->factorizations == 0)
	{
		set_error("ilu0_values: the handle has not been factorized yet (call spmv_mi355x_ilu0_factor first)");
		return 1;
	}
	*f_dev_out = F->arr.f;
	return 0;
}

int
spmv_mi355x_ilu0_values(spmv_mi355x_ilu0 * F, double * out_host)
{
	if (!F || (F->nnz > 0 && !out_host))
	{
		set_error("ilu0_values: NULL argument (%s%s )", !F ? " F" : "", F && !out_host ? " out" : "");
		return 1;
	}
	if (F->factorizations == 0)
	{
		set_error("ilu0_values: the handle has not been factorized yet (call spmv_mi355x_ilu0_factor first)");
		return 1;
	}
	if (F->nnz == 0)
		return 0;
	HIP_TRY(hipSetDevice(F->device));
	HIP_TRY(hipDeviceSynchronize());      // a factorization may be in flight on any stream
	HIP_TRY(hipMemcpy(out_host, F->arr.f, (size_t) F->nnz * sizeof(double), hipMemcpyDeviceToHost));
	return 0;
}

int
spmv_mi355x_ilu0_get_info(spmv_mi355x_ilu0 * F, spmv_mi355x_ilu0_info * info)
{
	if (!F || !info)
	{
		set_error("ilu0_get_info: NULL argument (%s%s )", !F ? " F" : "", !info ? " info" : "");
		return 1;
	}
	if (info->struct_size < sizeof(size_t))
	{
		set_error("ilu0_get_info: info->struct_size not set");
		return 1;
	}
	spmv_mi355x_ilu0_info r;
	memset(&r, 0, sizeof(r));
	r.n = F->n;
	r.nnz = F->nnz;
	r.nnz_dropped = F->nnz_dropped;
	r.levels = F->levels;
	r.launches = F->levels > 0 ? F->levels - 1 : 0;
	r.max_level_rows = F->max_level_rows;
	r.block_rows = F->block_rows;
	r.blocks = F->blocks;
	r.breakdown_row = -1;
	r.factorizations = F->factorizations;
	if (F->n > 0 && F->factorizations > 0)
	{
		unsigned word = ILU0_NO_BREAKDOWN;
		HIP_TRY(hipSetDevice(F->device));
		HIP_TRY(hipDeviceSynchronize());
		HIP_TRY(hipMemcpy(&word, F->arr.breakdown, sizeof(word), hipMemcpyDeviceToHost));
		if (word != ILU0_NO_BREAKDOWN)
			r.breakdown_row = (long) word;
	}
	const size_t bytes = std::min(info->struct_size, sizeof(r));
	r.struct_size = bytes;
	memcpy(info, &r, bytes);
	return 0;
}

double
spmv_mi355x_ilu0_mem_footprint(const spmv_mi355x_ilu0 * F)
{
	return F ? F->mem_footprint : 0;
}

int
spmv_mi355x_ilu0_destroy(spmv_mi355x_ilu0 * F)
{
	if (!F)
		return 0;
	(void) hipSetDevice(F->device);
	ilu0_free(F);
	return 0;
}

}  // extern "C"

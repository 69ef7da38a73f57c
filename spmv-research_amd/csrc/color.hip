// Multicolour ordering handles (include/spmv_mi355x.h "multicolour ordering"): the host checks, the loop of rounds, the
// derived arrays, the permuted matrix and the C ABI. Host code only; the kernels are in kernels_color.hip, the graph, the rule and the
// mapping in color.hpp.

#include <chrono>
#include <cstring>
#include <vector>

#include "handle.hpp"
#include "color.hpp"
#include "solvers_common.hpp"
#include "trsv.hpp"

using namespace spmv;

namespace spmv {

static double
color_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

static void
color_free(spmv_mi355x_color * C)
{
	for (void * p : {(void *) C->d_rp, (void *) C->d_ci, (void *) C->d_perm, (void *) C->d_rank, (void *) C->d_rp_b, (void *) C->d_ci_b, (void *) C->d_map})
		if (p)
			(void) hipFree(p);
	delete C;
}

// The colouring and what is derived from it, for a handle whose pattern is on the device. Everything runs on the null stream.
static int
color_build(spmv_mi355x_color * C, int round_cap)
{
	const long n = C->n, nnz = C->nnz;
	if (n == 0)
	{
		C->color_ptr.assign(1, 0);
		C->symmetric = 1;
		return 0;
	}
	DeviceBuffers buf;
	// the pattern of A^t, and whether it is A's own (then one walk serves)
	auto t0 = std::chrono::steady_clock::now();
	int * d_rpt = nullptr, * d_cit = nullptr, * d_flag;
	unsigned * d_ids = nullptr;
	ABI_TRY(transpose_pattern_device(n, n, nnz, C->d_rp, C->d_ci, &d_rpt, &d_cit, &d_ids));
	buf.ptrs.push_back(d_rpt);
	buf.ptrs.push_back(d_cit);
	buf.ptrs.push_back(d_ids);
	ABI_TRY(buf.alloc(&d_flag, 16));
	HIP_TRY(hipMemsetAsync(d_flag, 0, 16, nullptr));
	ABI_TRY(launch_color_differ(C->d_rp, d_rpt, n + 1, d_flag, nullptr));
	ABI_TRY(launch_color_differ(C->d_ci, d_cit, nnz, d_flag, nullptr));
	int differ = 0;
	HIP_TRY(hipMemcpy(&differ, d_flag, 4, hipMemcpyDeviceToHost));
	C->symmetric = !differ;
	C->transpose_seconds = color_since(t0);

	// the rounds: one counter each
	t0 = std::chrono::steady_clock::now();
	ColorGraph g = {C->d_rp, C->d_ci, differ ? d_rpt : nullptr, differ ? d_cit : nullptr, n};
	int * d_color[2], * d_count;
	ABI_TRY(buf.alloc(&d_color[0], (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_color[1], (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_count, (size_t) round_cap * 4));
	HIP_TRY(hipMemsetAsync(d_color[0], 0xff, (size_t) n * 4, nullptr));      // -1: uncoloured
	HIP_TRY(hipMemsetAsync(d_count, 0, (size_t) round_cap * 4, nullptr));
	int left = 1, cur = 0;
	while (left > 0)
	{
		if (C->rounds == round_cap)
		{
			set_error("color_create: %d rows are still uncoloured after %d rounds (the cap; a clique of m rows needs m rounds)", left, round_cap);
			return 1;
		}
		ABI_TRY(launch_color_round(g, d_color[cur], d_color[cur ^ 1], d_count + C->rounds, nullptr));
		HIP_TRY(hipMemcpy(&left, d_count + C->rounds, 4, hipMemcpyDeviceToHost));
		cur ^= 1;
		C->rounds++;
	}
	const int * d_colors = d_color[cur];
	C->round_seconds = color_since(t0);

	// the largest colour, the rows by (colour, row), the inverse, the first position of every colour
	t0 = std::chrono::steady_clock::now();
	const size_t max_bytes = color_max_bytes(n);
	void * d_tmp;
	int * d_iota, * d_sorted, * d_ptr;
	ABI_TRY(buf.alloc(&d_tmp, max_bytes));
	ABI_TRY(buf.alloc(&d_iota, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_sorted, (size_t) n * 4));
	ABI_TRY(dev_alloc_bytes((void **) &C->d_perm, (size_t) n * 4));
	ABI_TRY(dev_alloc_bytes((void **) &C->d_rank, (size_t) n * 4));
	ABI_TRY(launch_color_max(n, d_colors, d_flag, d_tmp, max_bytes, nullptr));
	int max_color = -1;
	HIP_TRY(hipMemcpy(&max_color, d_flag, 4, hipMemcpyDeviceToHost));
	if (max_color < 0 || max_color >= n)
	{
		set_error("color_create: internal: the largest colour is %d of %ld rows", max_color, n);
		return 1;
	}
	const size_t tmp_bytes = color_sort_bytes(n, max_color);
	ABI_TRY(buf.alloc(&d_tmp, tmp_bytes));
	C->num_colors = (long) max_color + 1;
	ABI_TRY(launch_color_sort(n, d_colors, max_color, d_iota, d_sorted, C->d_perm, C->d_rank, d_tmp, tmp_bytes, nullptr));
	ABI_TRY(buf.alloc(&d_ptr, (size_t) (C->num_colors + 1) * 4));
	ABI_TRY(launch_color_start(n, d_sorted, C->num_colors, d_ptr, nullptr));
	C->colors.resize((size_t) n);
	C->perm.resize((size_t) n);
	C->rank.resize((size_t) n);
	C->color_ptr.resize((size_t) C->num_colors + 1);
	HIP_TRY(hipMemcpy(C->colors.data(), d_colors, (size_t) n * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(C->perm.data(), C->d_perm, (size_t) n * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(C->rank.data(), C->d_rank, (size_t) n * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(C->color_ptr.data(), d_ptr, (size_t) (C->num_colors + 1) * 4, hipMemcpyDeviceToHost));
	C->sort_seconds = color_since(t0);
	C->max_class = 0;
	C->min_class = n;
	for (long c = 0; c < C->num_colors; c++)
	{
		const long rows = (long) C->color_ptr[c + 1] - C->color_ptr[c];
		C->max_class = std::max(C->max_class, rows);
		C->min_class = std::min(C->min_class, rows);
	}
	C->mem_footprint += 2.0 * (double) n * 4;
	return 0;
}

// B = P A P^t and the entry map, on the device, at the first call that asks for them; A's own pattern is dropped afterwards
static int
color_form_permuted(spmv_mi355x_color * C)
{
	if (C->permuted)
		return 0;
	HIP_TRY(hipSetDevice(C->device));
	const long n = C->n, nnz = C->nnz;
	auto t0 = std::chrono::steady_clock::now();
	if (n == 0)
	{
		ABI_TRY(dev_alloc_bytes((void **) &C->d_rp_b, 4));
		HIP_TRY(hipMemset(C->d_rp_b, 0, 4));
		C->permuted = true;
		return 0;
	}
	DeviceBuffers buf;
	int * d_lab, * d_rp1 = nullptr, * d_ci1 = nullptr, * d_rp2 = nullptr, * d_ci2 = nullptr;
	unsigned * d_ids1 = nullptr, * d_ids2 = nullptr;
	ABI_TRY(buf.alloc(&d_lab, (size_t) nnz * 4));
	// the columns in the new numbering, transposed: rows = new columns, each in ascending old row
	ABI_TRY(launch_color_relabel(nnz, C->d_ci, C->d_rank, d_lab, nullptr));
	ABI_TRY(transpose_pattern_device(n, n, nnz, C->d_rp, d_lab, &d_rp1, &d_ci1, &d_ids1));
	buf.ptrs.push_back(d_rp1);
	buf.ptrs.push_back(d_ci1);
	buf.ptrs.push_back(d_ids1);
	// the old rows in the new numbering, transposed again: rows = new rows, each in ascending new column, equal columns as stored
	ABI_TRY(launch_color_relabel(nnz, d_ci1, C->d_rank, d_lab, nullptr));
	ABI_TRY(transpose_pattern_device(n, n, nnz, d_rp1, d_lab, &d_rp2, &d_ci2, &d_ids2));
	buf.ptrs.push_back(d_ids2);
	C->d_rp_b = d_rp2;
	C->d_ci_b = d_ci2;
	ABI_TRY(dev_alloc_bytes((void **) &C->d_map, (size_t) nnz * 4));
	ABI_TRY(launch_color_compose(nnz, d_ids1, d_ids2, C->d_map, nullptr));
	HIP_TRY(hipDeviceSynchronize());
	(void) hipFree(C->d_rp);
	(void) hipFree(C->d_ci);
	C->d_rp = C->d_ci = nullptr;
	C->mem_footprint += (double) nnz * 4;                     // the pattern of B replaces A's; the map is new
	C->permute_seconds = color_since(t0);
	C->permuted = true;
	return 0;
}

int
color_create_capped(spmv_mi355x_color ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, int device, int round_cap)
{
	if (out)
		*out = nullptr;
	// 1. scalars, 2. NULL pointers, 3. the pattern: all on the host; 4. the device
	if (n < 0 || n >= 0x7fffffffL)
	{
		set_error("color_create: n = %ld out of range [0, 2^31 - 1)", n);
		return 1;
	}
	if (round_cap < 1 || round_cap > COLOR_ROUND_CAP)
	{
		set_error("color_create: round cap %d out of range [1, %d]", round_cap, COLOR_ROUND_CAP);
		return 1;
	}
	if (!out || !row_ptr || (!col_idx && row_ptr[n] > 0))
	{
		set_error("color_create: NULL argument (%s%s%s )", !out ? " out" : "", !row_ptr ? " row_ptr" : "", row_ptr && !col_idx ? " col_idx" : "");
		return 1;
	}
	if (trsv_check_pattern("color_create", n, row_ptr, col_idx))
		return 1;
	const long nnz = row_ptr[n];
	if (n + nnz >= 0x7fffffffL)
	{
		set_error("color_create: n + nnz = %ld out of range [0, 2^31 - 1) (the device transposition's limit)", n + nnz);
		return 1;
	}
	int ndev = 0;
	spmv_mi355x_device_count(&ndev);
	if (ndev < 1)
	{
		set_error("color_create: no HIP device available: this engine has no CPU fallback");
		return 1;
	}
	if (device < 0)
		HIP_TRY(hipGetDevice(&device));
	if (device >= ndev)
	{
		set_error("color_create: device %d out of range (%d devices)", device, ndev);
		return 1;
	}
	HIP_TRY(hipSetDevice(device));
	spmv_mi355x_color * C = new spmv_mi355x_color();
	C->device = device;
	C->n = n;
	C->nnz = nnz;
	if (n > 0)
	{
		if (upload_bytes(row_ptr, (size_t) (n + 1) * 4, 0, (void **) &C->d_rp) || upload_bytes(col_idx, (size_t) nnz * 4, 0, (void **) &C->d_ci))
		{
			color_free(C);
			return 1;
		}
		C->mem_footprint = (double) (n + 1) * 4 + (double) nnz * 4;
	}
	if (color_build(C, round_cap))
	{
		color_free(C);
		return 1;
	}
	*out = C;
	return 0;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_color_create(spmv_mi355x_color ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, int device)
{
	return color_create_capped(out, n, row_ptr, col_idx, device, COLOR_ROUND_CAP);
}

// not in the header: spmv_mi355x_color_create with a lower round cap, so that the tests reach the refusal without a clique of 4097 rows
int
spmv_mi355x_color_create_capped_for_tests(spmv_mi355x_color ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, int device, int round_cap)
{
	return color_create_capped(out, n, row_ptr, col_idx, device, round_cap);
}

int
spmv_mi355x_color_destroy(spmv_mi355x_color * C)
{
	if (!C)
		return 0;
	(void) hipSetDevice(C->device);
	color_free(C);
	return 0;
}

int
spmv_mi355x_color_info(const spmv_mi355x_color * C, spmv_mi355x_color_stats * stats)
{
	if (!C || !stats)
	{
		set_error("color_info: NULL argument (%s%s )", !C ? " C" : "", !stats ? " stats" : "");
		return 1;
	}
	if (stats->struct_size < sizeof(size_t))
	{
		set_error("color_info: stats->struct_size not set");
		return 1;
	}
	spmv_mi355x_color_stats r;
	memset(&r, 0, sizeof(r));
	r.n = C->n;
	r.nnz = C->nnz;
	r.symmetric = C->symmetric;
	r.num_colors = C->num_colors;
	r.rounds = C->rounds;
	r.max_class = C->max_class;
	r.min_class = C->min_class;
	r.transpose_seconds = C->transpose_seconds;
	r.round_seconds = C->round_seconds;
	r.sort_seconds = C->sort_seconds;
	r.permute_seconds = C->permute_seconds;
	const size_t bytes = std::min(stats->struct_size, sizeof(r));
	r.struct_size = bytes;
	memcpy(stats, &r, bytes);
	return 0;
}

int
spmv_mi355x_color_colors(const spmv_mi355x_color * C, int32_t * colors_host)
{
	if (!C || (C->n > 0 && !colors_host))
	{
		set_error("color_colors: NULL argument (%s%s )", !C ? " C" : "", C && !colors_host ? " colors" : "");
		return 1;
	}
	if (C->n > 0)
		memcpy(colors_host, C->colors.data(), (size_t) C->n * 4);
	return 0;
}

int
spmv_mi355x_color_perm(const spmv_mi355x_color * C, int32_t * perm_host, int32_t * rank_host)
{
	if (!C)
	{
		set_error("color_perm: NULL argument ( C )");
		return 1;
	}
	if (C->n > 0 && perm_host)
		memcpy(perm_host, C->perm.data(), (size_t) C->n * 4);
	if (C->n > 0 && rank_host)
		memcpy(rank_host, C->rank.data(), (size_t) C->n * 4);
	return 0;
}

int
spmv_mi355x_color_color_ptr(const spmv_mi355x_color * C, int32_t * color_ptr_host)
{
	if (!C || !color_ptr_host)
	{
		set_error("color_color_ptr: NULL argument (%s%s )", !C ? " C" : "", !color_ptr_host ? " color_ptr" : "");
		return 1;
	}
	memcpy(color_ptr_host, C->color_ptr.data(), C->color_ptr.size() * 4);
	return 0;
}

double
spmv_mi355x_color_mem_footprint(const spmv_mi355x_color * C)
{
	return C ? C->mem_footprint : 0;
}

int
spmv_mi355x_color_permute_csr_device(spmv_mi355x_color * C, const int32_t ** row_ptr_dev_out, const int32_t ** col_idx_dev_out,
		const int32_t ** entry_map_dev_out)
{
	if (!C || !row_ptr_dev_out || !col_idx_dev_out || !entry_map_dev_out)
	{
		set_error("color_permute_csr: NULL argument (%s%s%s%s )", !C ? " C" : "", !row_ptr_dev_out ? " row_ptr" : "", !col_idx_dev_out ? " col_idx" : "",
				!entry_map_dev_out ? " entry_map" : "");
		return 1;
	}
	ABI_TRY(color_form_permuted(C));
	*row_ptr_dev_out = C->d_rp_b;
	*col_idx_dev_out = C->d_ci_b;
	*entry_map_dev_out = C->d_map;
	return 0;
}

int
spmv_mi355x_color_permute_values_device_async(spmv_mi355x_color * C, const double * values_dev, double * values_out_dev, void * hip_stream)
{
	if (!C || (C->nnz > 0 && (!values_dev || !values_out_dev)))
	{
		set_error("color_permute_values: NULL argument (%s%s%s )", !C ? " C" : "", C && !values_dev ? " values" : "", C && !values_out_dev ? " out" : "");
		return 1;
	}
	if (C->nnz > 0 && values_dev == values_out_dev)
	{
		set_error("color_permute_values: values and out are the same array (the gather cannot run in place)");
		return 1;
	}
	ABI_TRY(color_form_permuted(C));
	if (C->nnz == 0)
		return 0;
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != C->device)
		HIP_TRY(hipSetDevice(C->device));
	return launch_color_gather_values(C->nnz, C->d_map, values_dev, values_out_dev, (hipStream_t) hip_stream);
}

int
spmv_mi355x_color_permute_values(spmv_mi355x_color * C, const double * values_host, double * values_out_host)
{
	if (!C || (C->nnz > 0 && (!values_host || !values_out_host)))
	{
		set_error("color_permute_values: NULL argument (%s%s%s )", !C ? " C" : "", C && !values_host ? " values" : "", C && !values_out_host ? " out" : "");
		return 1;
	}
	ABI_TRY(color_form_permuted(C));
	if (C->nnz == 0)
		return 0;
	DeviceBuffers buf;
	double * d_in, * d_out;
	const size_t bytes = (size_t) C->nnz * sizeof(double);
	ABI_TRY(buf.alloc(&d_in, bytes));
	ABI_TRY(buf.alloc(&d_out, bytes));
	HIP_TRY(hipMemcpy(d_in, values_host, bytes, hipMemcpyHostToDevice));
	ABI_TRY(launch_color_gather_values(C->nnz, C->d_map, d_in, d_out, nullptr));
	HIP_TRY(hipMemcpy(values_out_host, d_out, bytes, hipMemcpyDeviceToHost));
	return 0;
}

int
spmv_mi355x_color_permute_csr(spmv_mi355x_color * C, const double * values_host, int32_t * row_ptr_out, int32_t * col_idx_out, double * values_out,
		int32_t * entry_map_out)
{
	if (!C || !row_ptr_out || (C->nnz > 0 && (!col_idx_out || !entry_map_out)) || (C->nnz > 0 && values_host && !values_out))
	{
		set_error("color_permute_csr: NULL argument (%s%s%s%s%s )", !C ? " C" : "", !row_ptr_out ? " row_ptr" : "", C && !col_idx_out ? " col_idx" : "",
				C && !entry_map_out ? " entry_map" : "", C && values_host && !values_out ? " values_out" : "");
		return 1;
	}
	ABI_TRY(color_form_permuted(C));
	HIP_TRY(hipMemcpy(row_ptr_out, C->d_rp_b, (size_t) (C->n + 1) * 4, hipMemcpyDeviceToHost));
	if (C->nnz == 0)
		return 0;
	HIP_TRY(hipMemcpy(col_idx_out, C->d_ci_b, (size_t) C->nnz * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(entry_map_out, C->d_map, (size_t) C->nnz * 4, hipMemcpyDeviceToHost));
	if (values_host)
		return spmv_mi355x_color_permute_values(C, values_host, values_out);
	return 0;
}

static int
color_vectors_check(const spmv_mi355x_color * C, int direction, int precision, int k, const void * in, long ldin, const void * out, long ldout)
{
	if (direction != SPMV_MI355X_COLOR_FORWARD && direction != SPMV_MI355X_COLOR_BACKWARD)
	{
		set_error("color_permute_vectors: direction must be 0 (forward) or 1 (backward) (got %d)", direction);
		return 1;
	}
	if (precision != 0 && precision != 1)
	{
		set_error("color_permute_vectors: precision must be 0 (fp64) or 1 (fp32) (got %d)", precision);
		return 1;
	}
	if (k < 1 || ldin < k || ldout < k)
	{
		set_error("color_permute_vectors: need k >= 1, ldin >= k and ldout >= k (got k=%d ldin=%ld ldout=%ld)", k, ldin, ldout);
		return 1;
	}
	if (!C || (C->n > 0 && (!in || !out)))
	{
		set_error("color_permute_vectors: NULL argument (%s%s%s )", !C ? " C" : "", C && !in ? " in" : "", C && !out ? " out" : "");
		return 1;
	}
	if (C->n > 0 && in == out)
	{
		set_error("color_permute_vectors: in and out are the same block (a permutation cannot run in place)");
		return 1;
	}
	return 0;
}

int
spmv_mi355x_color_permute_vectors_device_async(spmv_mi355x_color * C, int direction, int precision, int k, const void * in_dev, long ldin, void * out_dev,
		long ldout, void * hip_stream)
{
	ABI_TRY(color_vectors_check(C, direction, precision, k, in_dev, ldin, out_dev, ldout));
	if (C->n == 0)
		return 0;
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != C->device)
		HIP_TRY(hipSetDevice(C->device));
	return launch_color_gather_rows(precision == 1, k, direction == SPMV_MI355X_COLOR_FORWARD ? C->d_perm : C->d_rank, in_dev, ldin, out_dev, ldout, C->n,
			(hipStream_t) hip_stream);
}

int
spmv_mi355x_color_permute_vectors(spmv_mi355x_color * C, int direction, int precision, int k, const void * in_host, long ldin, void * out_host, long ldout)
{
	ABI_TRY(color_vectors_check(C, direction, precision, k, in_host, ldin, out_host, ldout));
	if (C->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(C->device));
	const size_t w = precision == 1 ? sizeof(float) : sizeof(double);
	// whole rows travel, so that what lies between k and ld in the caller's out comes back as it went
	const size_t in_bytes = ((size_t) (C->n - 1) * ldin + k) * w, out_bytes = ((size_t) (C->n - 1) * ldout + k) * w;
	DeviceBuffers buf;
	void * d_in, * d_out;
	ABI_TRY(buf.alloc(&d_in, in_bytes));
	ABI_TRY(buf.alloc(&d_out, out_bytes));
	HIP_TRY(hipMemcpy(d_in, in_host, in_bytes, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_out, out_host, out_bytes, hipMemcpyHostToDevice));
	ABI_TRY(spmv_mi355x_color_permute_vectors_device_async(C, direction, precision, k, d_in, ldin, d_out, ldout, nullptr));
	HIP_TRY(hipMemcpy(out_host, d_out, out_bytes, hipMemcpyDeviceToHost));
	return 0;
}

}  // extern "C"

// Smoothed-aggregation AMG handles (include/spmv_mi355x.h "AMG"): the checks of amg_create in the header's order, the hierarchy
// level by level (upload A_l, steps 1 to 5 on the device with kernels_amg.hip, the products through SpGEMM plans whose values never
// leave the device, R by the device transposition, downloads for the handles that spmv_mi355x_create builds from host arrays), the
// dense factor of the last level, the cycle and the C ABI. New values for a hierarchy (amg_update_values*): prepare builds the three
// plans of every coarsened level once more and keeps them with the aggregates, the entry map P -> R and the value arrays; an update
// redoes steps 1, 5 and 6 and the factor on the device and refreshes every handle in place. amg_create_with (a caller's near-null
// vector, filtered prolongator smoothing) replaces step 5 by amg_prolongator_with; with its defaults it is amg_create.

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "handle.hpp"
#include "amg.hpp"
#include "spgemm.hpp"
#include "solvers_common.hpp"

namespace spmv {

static double
amg_since(std::chrono::steady_clock::time_point t0)
{
	return std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
}

static bool
amg_scalars_ok(const char * what, int format, int precision, long n, const spmv_mi355x_opts & o, const spmv_mi355x_amg_opts & a)
{
	if (precision != SPMV_MI355X_F64 && precision != SPMV_MI355X_F32)
		set_error("%s: unknown precision %d", what, precision);
	else if (format < 0 || format >= SPMV_MI355X_NUM_FORMATS)
		set_error("%s: unknown format %d", what, format);
	else if (n < 0 || n >= 0x7fffffffL)
		set_error("%s: n = %ld out of range [0, 2^31 - 1)", what, n);
	else if (o.transpose)
		set_error("%s: opts->transpose = %d: the library builds R from the CSR of P^t itself", what, o.transpose);
	else if (o.symmetric_input)
		set_error("%s: opts->symmetric_input = %d: A comes with both triangles, P and R are not symmetric", what, o.symmetric_input);
	else if (o.row_begin || o.row_end || o.col_filter_mode)
		set_error("%s: opts name a row block or a column filter (row_begin %ld, row_end %ld, col_filter_mode %d): the "
				"row-partitioned form is not built", what, o.row_begin, o.row_end, o.col_filter_mode);
	else if (value_storage_check(what, o, format, precision))
		;                                     // create's own rule and message for opts->value_storage
	else if (!std::isfinite(a.theta) || a.theta < 0 || a.theta > 1)
		set_error("%s: amg_opts->theta = %g: it must be finite and lie in [0, 1]", what, a.theta);
	else if (a.max_levels < 1 || a.max_levels > SPMV_MI355X_AMG_MAX_LEVELS)
		set_error("%s: amg_opts->max_levels = %d out of range 1..%d", what, a.max_levels, SPMV_MI355X_AMG_MAX_LEVELS);
	else if (a.coarse_rows < 1 || a.coarse_rows > AMG_DENSE_MAX)
		set_error("%s: amg_opts->coarse_rows = %d out of range 1..%d", what, a.coarse_rows, AMG_DENSE_MAX);
	else if (a.sweeps < 1 || a.sweeps > 4)
		set_error("%s: amg_opts->sweeps = %d out of range 1..4", what, a.sweeps);
	else if (a.coarse_sweeps < 1 || a.coarse_sweeps > 64)
		set_error("%s: amg_opts->coarse_sweeps = %d out of range 1..64", what, a.coarse_sweeps);
	else
		return true;
	return false;
}

// 3. row_ptr from 0 and monotone, columns in [0, n); 4. no column twice in a row; 5. a stored, finite, positive diagonal
static int
amg_check_matrix(const char * what, long n, const int32_t * rp, const int32_t * ci, const double * va)
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
	std::vector<int32_t> mark((size_t) n, -1);
	for (long i = 0; i < n; i++)
		for (long j = rp[i]; j < rp[i + 1]; j++)
		{
			if (mark[ci[j]] == i)
			{
				set_error("%s: row %ld of A stores column %d twice: which value A(%ld, %d) has is not defined", what, i, ci[j], i, ci[j]);
				return 1;
			}
			mark[ci[j]] = (int32_t) i;
		}
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
amg_update_free(AmgUpdate * u)
{
	if (!u)
		return;
	for (AmgUpdateLevel & U : u->lev)
		for (spmv_mi355x_spgemm * p : {U.at, U.ap, U.ac})
			if (p)
				spmv_mi355x_spgemm_destroy(p);
	for (void * p : u->owned)
		(void) hipFree(p);
	delete u;
}

static void
amg_fold_free(spmv_mi355x_amg * M)
{
	if (!M->fold)
		return;
	for (void * p : M->fold->owned)
		(void) hipFree(p);
	delete M->fold;
	M->fold = nullptr;
}

// the first folded level; `levels` when nothing folds
static int
amg_fold_first(const spmv_mi355x_amg * M)
{
	return M->fold ? M->fold->first : M->levels;
}

// SpMVs and launches of one apply: the levels above the first folded one as ever, then one launch for the tail
static void
amg_count_launches(spmv_mi355x_amg * M)
{
	const int nu = M->opts.sweeps, cs = M->opts.coarse_sweeps, f = amg_fold_first(M);
	const bool dense = M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE;
	if (f < M->levels)
	{
		M->spmvs = (long) f * (2 * nu + 2);
		M->launches = M->spmvs + (long) f * (2 * nu + 1) + 1;
		return;
	}
	M->spmvs = (long) (M->levels - 1) * (2 * nu + 2) + (dense ? 0 : cs - 1);
	M->launches = M->spmvs + (long) (M->levels - 1) * (2 * nu + 1) + (dense ? 1 : cs);
}

static void
amg_free(spmv_mi355x_amg * M)
{
	amg_update_free(M->upd);
	M->upd = nullptr;
	amg_fold_free(M);
	for (AmgLevel & L : M->lev)
	{
		for (spmv_mi355x_matrix * h : {L.A, L.P, L.R})
			if (h)
				spmv_mi355x_destroy(h);
		for (void * p : {L.w, L.b, L.x, L.t})
			if (p)
				(void) hipFree(p);
	}
	for (void * p : {(void *) M->d_factor, M->d_in, M->d_out, M->d_in_multi, M->d_out_multi})
		if (p)
			(void) hipFree(p);
	for (const std::vector<void *> * v : {&M->mb, &M->mx, &M->mt})
		for (void * p : *v)
			if (p)
				(void) hipFree(p);
	delete M;
}

// the plan of a product and its values on the device: c = A B with a_va and b_va resident
struct AmgProduct {
	spmv_mi355x_spgemm * plan = nullptr;
	~AmgProduct()
	{
		if (plan)
			spmv_mi355x_spgemm_destroy(plan);
	}
	int run(int device, long m, long k, long n, const int32_t * a_rp, const int32_t * a_ci, const double * a_va_dev, const int32_t * b_rp,
			const int32_t * b_ci, const double * b_va_dev, DeviceBuffers & buf, double ** c_va_dev)
	{
		ABI_TRY(spmv_mi355x_spgemm_create(&plan, device, m, k, n, a_rp, a_ci, b_rp, b_ci));
		ABI_TRY(buf.alloc(c_va_dev, (size_t) std::max<long>(plan->nnz_c, 1) * 8));
		ABI_TRY(spmv_mi355x_spgemm_multiply_device_async(plan, a_va_dev, b_va_dev, *c_va_dev, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		return 0;
	}
	// C's pattern on the host
	int pattern(std::vector<int32_t> & rp, std::vector<int32_t> & ci) const
	{
		rp = plan->c_rp;
		ci.assign((size_t) std::max<long>(plan->nnz_c, 1), 0);
		return spmv_mi355x_spgemm_pattern(plan, rp.data(), ci.data());
	}
};

// Steps 5a to 5c of level l for a hierarchy of amg_create_with: A_F (filtered), t and the next level's vector (near_null), AT = A_F T
// in `at` and P's values in *d_p_out. a, d_d and d_agg are the level's on the device, d_ones n ones.
static int
amg_prolongator_with(spmv_mi355x_amg * M, int l, const AmgCsr & a, const double * d_d, const int * d_agg, double theta2,
		const std::vector<int32_t> & t_rp, const double * d_ones, DeviceBuffers & buf, AmgProduct & at, std::vector<double> & nrm, double ** d_p_out)
{
	AmgLevel & L = M->lev[(size_t) l];
	const long n = L.n, nc = L.aggregates;
	auto t0 = std::chrono::steady_clock::now();
	const int32_t * f_rp = L.rp.data(), * f_ci = L.ci.data();
	const double * d_fva = a.va, * d_df = d_d;
	L.nnz_f = L.nnz;
	L.omega_p = L.omega;
	L.rho_p = L.rho;
	if (M->filtered)
	{
		int * d_kept, * d_fb, * d_frp, * d_fci, * d_map;
		double * d_dfw, * d_fv, * d_part;
		void * d_scan;
		const size_t scan_bytes = amg_scan_bytes(n + 1);
		ABI_TRY(buf.alloc(&d_kept, (size_t) (n + 1) * 4));
		ABI_TRY(buf.alloc(&d_frp, (size_t) (n + 1) * 4));
		ABI_TRY(buf.alloc(&d_fb, (size_t) n * 4));
		ABI_TRY(buf.alloc(&d_dfw, (size_t) n * 8));
		ABI_TRY(buf.alloc(&d_part, (size_t) AMG_MAX_GRID * 8));
		ABI_TRY(buf.alloc(&d_scan, scan_bytes));
		HIP_TRY(hipMemsetAsync(d_kept, 0, (size_t) (n + 1) * 4, nullptr));
		ABI_TRY(launch_amg_filter_count(a, d_d, theta2, d_kept, d_fb, d_dfw, nullptr));
		ABI_TRY(launch_amg_offsets(n + 1, d_kept, d_frp, d_scan, scan_bytes, nullptr));
		L.f_rp.assign((size_t) n + 1, 0);
		L.f_fb.assign((size_t) n, 0);
		HIP_TRY(hipMemcpy(L.f_rp.data(), d_frp, (size_t) (n + 1) * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(L.f_fb.data(), d_fb, (size_t) n * 4, hipMemcpyDeviceToHost));
		L.nnz_f = L.f_rp[(size_t) n];
		if (L.nnz_f < n || L.nnz_f > L.nnz)
		{
			set_error("amg_create_with: internal: level %d: the filtered operator has %ld entries, A has %ld in %ld rows", l, L.nnz_f, L.nnz, n);
			return 1;
		}
		L.unfiltered_rows = 0;
		for (long i = 0; i < n; i++)
			L.unfiltered_rows += L.f_fb[(size_t) i] != 0;
		ABI_TRY(buf.alloc(&d_fci, (size_t) L.nnz_f * 4));
		ABI_TRY(buf.alloc(&d_fv, (size_t) L.nnz_f * 8));
		ABI_TRY(buf.alloc(&d_map, (size_t) L.nnz_f * 4));
		ABI_TRY(launch_amg_filter_fill(a, d_d, theta2, d_frp, d_fb, d_dfw, d_fci, d_fv, d_map, d_part, nullptr));
		L.f_ci.assign((size_t) L.nnz_f, 0);
		L.f_map.assign((size_t) L.nnz_f, 0);
		L.f_va.assign((size_t) L.nnz_f, 0.0);
		std::vector<double> part((size_t) amg_grid(n));
		HIP_TRY(hipMemcpy(L.f_ci.data(), d_fci, (size_t) L.nnz_f * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(L.f_map.data(), d_map, (size_t) L.nnz_f * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(L.f_va.data(), d_fv, (size_t) L.nnz_f * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost));
		L.rho_p = *std::max_element(part.begin(), part.end());
		if (!std::isfinite(L.rho_p) || !(L.rho_p > 0))
		{
			set_error("amg_create_with: level %d: max_i sum_j |aF_ij| / dF_i = %g is not a positive finite number", l, L.rho_p);
			return 1;
		}
		L.omega_p = 4.0 / (3.0 * L.rho_p);
		f_rp = L.f_rp.data();
		f_ci = L.f_ci.data();
		d_fva = d_fv;
		d_df = d_dfw;
	}
	M->coarsen_seconds += amg_since(t0);
	t0 = std::chrono::steady_clock::now();
	ABI_TRY(spmv_mi355x_spgemm_create(&at.plan, M->device, n, n, nc, f_rp, f_ci, t_rp.data(), L.agg.data()));
	M->spgemm_seconds += amg_since(t0);
	const double * d_t = d_ones;
	if (M->has_nn)
	{
		// the members of every aggregate in ascending order, with their b: the transposition of T's pattern
		t0 = std::chrono::steady_clock::now();
		double * d_b, * d_nrm, * d_tw, * d_mb = nullptr;
		int * d_mrp = nullptr, * d_mci = nullptr;
		ABI_TRY(buf.alloc(&d_b, (size_t) n * 8));
		ABI_TRY(buf.alloc(&d_nrm, (size_t) nc * 8));
		ABI_TRY(buf.alloc(&d_tw, (size_t) n * 8));
		HIP_TRY(hipMemcpy(d_b, L.nn.data(), (size_t) n * 8, hipMemcpyHostToDevice));
		ABI_TRY(transpose_csr_device(n, nc, n, at.plan->d_b_rp, at.plan->d_b_ci, d_b, &d_mrp, &d_mci, &d_mb));
		for (void * p : {(void *) d_mrp, (void *) d_mci, (void *) d_mb})
			buf.ptrs.push_back(p);
		ABI_TRY(launch_amg_agg_norm(nc, d_mrp, d_mb, d_nrm, nullptr));
		ABI_TRY(launch_amg_tentative(n, d_b, d_agg, d_nrm, d_tw, nullptr));
		nrm.assign((size_t) nc, 0.0);
		L.tv.assign((size_t) n, 0.0);
		HIP_TRY(hipMemcpy(nrm.data(), d_nrm, (size_t) nc * 8, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(L.tv.data(), d_tw, (size_t) n * 8, hipMemcpyDeviceToHost));
		for (long g = 0; g < nc; g++)
			if (!std::isfinite(nrm[(size_t) g]) || !(nrm[(size_t) g] > 0))
			{
				set_error("amg_create_with: level %d: the norm of the near-null vector over aggregate %ld is %g: it must be a positive finite "
						"number (b * b underflowed or overflowed)", l, g, nrm[(size_t) g]);
				return 1;
			}
		d_t = d_tw;
		M->coarsen_seconds += amg_since(t0);
	}
	t0 = std::chrono::steady_clock::now();
	double * d_at;
	ABI_TRY(buf.alloc(&d_at, (size_t) std::max<long>(at.plan->nnz_c, 1) * 8));
	ABI_TRY(spmv_mi355x_spgemm_multiply_device_async(at.plan, d_fva, d_t, d_at, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	M->spgemm_seconds += amg_since(t0);
	t0 = std::chrono::steady_clock::now();
	ABI_TRY(buf.alloc(d_p_out, (size_t) std::max<long>(at.plan->nnz_c, 1) * 8));
	ABI_TRY(launch_amg_prolong_t(n, at.plan->d_c_rp, at.plan->d_c_ci, d_at, d_agg, d_t, d_df, L.omega_p, *d_p_out, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	M->coarsen_seconds += amg_since(t0);
	return 0;
}

// Level l of M: steps 1 to 4, and unless the level turns out to be the last, steps 5 and 6, the handles of P and R and the CSR of
// level l + 1. *last_out says which.
static int
amg_build_level(spmv_mi355x_amg * M, int l, const spmv_mi355x_opts & o, bool * last_out)
{
	AmgLevel & L = M->lev[(size_t) l];
	const long n = L.n, nnz = L.nnz;
	const double theta2 = M->opts.theta * M->opts.theta;
	DeviceBuffers buf;
	int * d_rp, * d_ci, * d_state, * d_flag, * d_id, * d_agg1, * d_agg2, * d_count;
	double * d_va, * d_d, * d_part;
	unsigned long long * d_key[3];
	void * d_scan;

	auto t0 = std::chrono::steady_clock::now();
	ABI_TRY(buf.alloc(&d_rp, (size_t) (n + 1) * 4));
	ABI_TRY(buf.alloc(&d_ci, (size_t) std::max<long>(nnz, 1) * 4));
	ABI_TRY(buf.alloc(&d_va, (size_t) std::max<long>(nnz, 1) * 8));
	ABI_TRY(buf.alloc(&d_d, (size_t) n * 8));
	ABI_TRY(buf.alloc(&d_part, (size_t) AMG_MAX_GRID * 8));
	HIP_TRY(hipMemcpy(d_rp, L.rp.data(), (size_t) (n + 1) * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_ci, L.ci.data(), (size_t) nnz * 4, hipMemcpyHostToDevice));
	HIP_TRY(hipMemcpy(d_va, L.va.data(), (size_t) nnz * 8, hipMemcpyHostToDevice));
	const AmgCsr a = {d_rp, d_ci, d_va, n};

	// 1. the diagonal and the damping
	ABI_TRY(launch_amg_diag(a, d_d, d_part, nullptr));
	std::vector<double> d((size_t) n), part((size_t) amg_grid(n));
	HIP_TRY(hipMemcpy(d.data(), d_d, (size_t) n * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(part.data(), d_part, part.size() * 8, hipMemcpyDeviceToHost));
	for (long i = 0; i < n; i++)
		if (!std::isfinite(d[i]) || !(d[i] > 0))
		{
			set_error("amg_create: the diagonal of row %ld of level %d is %g: the matrix is not positive definite", i, l, d[i]);
			return 1;
		}
	L.rho = *std::max_element(part.begin(), part.end());
	if (!std::isfinite(L.rho) || !(L.rho > 0))
	{
		set_error("amg_create: level %d: max_i sum_j |a_ij| / a_ii = %g is not a positive finite number", l, L.rho);
		return 1;
	}
	L.omega = 4.0 / (3.0 * L.rho);
	const size_t vbytes = (size_t) n * (M->f32 ? 4 : 8);
	{
		std::vector<double> w8;
		std::vector<float> w4;
		if (M->f32)
		{
			w4.resize((size_t) n);
			for (long i = 0; i < n; i++)
				w4[i] = (float) (L.omega / d[i]);
		}
		else
		{
			w8.resize((size_t) n);
			for (long i = 0; i < n; i++)
				w8[i] = L.omega / d[i];
		}
		// level 0 solves into the caller's vector; its b is the copy of `in` that an apply in place works on
		for (void ** v : {&L.w, &L.b, &L.t, &L.x})
			if (l > 0 || v != &L.x)
			{
				ABI_TRY(dev_alloc_bytes(v, vbytes));
				M->vector_bytes += (double) vbytes;
			}
		HIP_TRY(hipMemcpy(L.w, M->f32 ? (const void *) w4.data() : (const void *) w8.data(), vbytes, hipMemcpyHostToDevice));
	}
	M->coarsen_seconds += amg_since(t0);

	bool last = n <= M->opts.coarse_rows || l + 1 == M->opts.max_levels;
	if (last)
	{
		*last_out = true;
		return 0;
	}

	// 3. the roots: rounds of two sweeps and the verdicts, one counter per round
	t0 = std::chrono::steady_clock::now();
	ABI_TRY(buf.alloc(&d_state, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_flag, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_id, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_agg1, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_agg2, (size_t) n * 4));
	ABI_TRY(buf.alloc(&d_count, (size_t) AMG_MIS_ROUND_CAP * 4));
	for (auto & k : d_key)
		ABI_TRY(buf.alloc(&k, (size_t) n * 8));
	const size_t scan_bytes = amg_scan_bytes(n);
	ABI_TRY(buf.alloc(&d_scan, scan_bytes));
	HIP_TRY(hipMemsetAsync(d_count, 0, (size_t) AMG_MIS_ROUND_CAP * 4, nullptr));
	ABI_TRY(launch_amg_mis_init(n, d_state, d_key[0], nullptr));
	int undecided = 1;
	while (undecided > 0)
	{
		if (L.mis_rounds == AMG_MIS_ROUND_CAP)
		{
			set_error("amg_create: internal: level %d: %d nodes are still undecided after %d rounds of the independent set", l, undecided,
					AMG_MIS_ROUND_CAP);
			return 1;
		}
		ABI_TRY(launch_amg_mis_sweep(a, d_d, theta2, d_key[0], d_key[1], nullptr));
		ABI_TRY(launch_amg_mis_sweep(a, d_d, theta2, d_key[1], d_key[2], nullptr));
		ABI_TRY(launch_amg_mis_decide(n, d_state, d_key[0], d_key[2], d_count + L.mis_rounds, nullptr));
		HIP_TRY(hipMemcpy(&undecided, d_count + L.mis_rounds, 4, hipMemcpyDeviceToHost));
		L.mis_rounds++;
	}
	// 4. the aggregates
	ABI_TRY(launch_amg_number_roots(n, d_state, d_flag, d_id, d_scan, scan_bytes, nullptr));
	ABI_TRY(launch_amg_agg_pass1(a, d_d, theta2, d_state, d_id, d_agg1, nullptr));
	ABI_TRY(launch_amg_agg_pass2(a, d_d, theta2, d_agg1, d_agg2, nullptr));
	int last_id = 0, last_flag = 0;
	HIP_TRY(hipMemcpy(&last_id, d_id + (n - 1), 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(&last_flag, d_flag + (n - 1), 4, hipMemcpyDeviceToHost));
	const long nc = (long) last_id + last_flag;
	L.aggregates = nc;
	L.agg.assign((size_t) n, 0);
	HIP_TRY(hipMemcpy(L.agg.data(), d_agg2, (size_t) n * 4, hipMemcpyDeviceToHost));
	M->coarsen_seconds += amg_since(t0);
	for (long i = 0; i < n; i++)
		if (L.agg[i] < 0 || L.agg[i] >= nc)
		{
			set_error("amg_create: internal: level %d: row %ld was left without an aggregate (%d of %ld)", l, i, L.agg[i], nc);
			return 1;
		}
	if ((double) nc > 0.9 * (double) n)
	{
		M->stalled = 1;
		*last_out = true;
		return 0;
	}

	// 5. A T on the device, then P's values on its pattern
	t0 = std::chrono::steady_clock::now();
	std::vector<int32_t> t_rp((size_t) n + 1);
	for (long i = 0; i <= n; i++)
		t_rp[i] = (int32_t) i;
	double * d_ones, * d_at, * d_p;
	{
		std::vector<double> ones((size_t) n, 1.0);
		ABI_TRY(buf.alloc(&d_ones, (size_t) n * 8));
		HIP_TRY(hipMemcpy(d_ones, ones.data(), (size_t) n * 8, hipMemcpyHostToDevice));
	}
	AmgProduct at;
	std::vector<double> nrm;                              // b_{l+1} of a near-null vector
	if (!M->filtered && !M->has_nn)
	{
		ABI_TRY(at.run(M->device, n, n, nc, L.rp.data(), L.ci.data(), d_va, t_rp.data(), L.agg.data(), d_ones, buf, &d_at));
		M->spgemm_seconds += amg_since(t0);
		t0 = std::chrono::steady_clock::now();
		ABI_TRY(buf.alloc(&d_p, (size_t) at.plan->nnz_c * 8));
		ABI_TRY(launch_amg_prolong(n, at.plan->d_c_rp, at.plan->d_c_ci, d_at, d_agg2, d_d, L.omega, d_p, nullptr));
		HIP_TRY(hipStreamSynchronize(nullptr));
		M->coarsen_seconds += amg_since(t0);
		L.nnz_f = nnz;
		L.omega_p = L.omega;
		L.rho_p = L.rho;
	}
	else
		ABI_TRY(amg_prolongator_with(M, l, a, d_d, d_agg2, theta2, t_rp, d_ones, buf, at, nrm, &d_p));
	const long nnz_p = at.plan->nnz_c;

	// 6. R = P^t on the device
	t0 = std::chrono::steady_clock::now();
	int * d_r_rp = nullptr, * d_r_ci = nullptr;
	double * d_r_va = nullptr;
	ABI_TRY(transpose_csr_device(n, nc, nnz_p, at.plan->d_c_rp, at.plan->d_c_ci, d_p, &d_r_rp, &d_r_ci, &d_r_va));
	for (void * p : {(void *) d_r_rp, (void *) d_r_ci, (void *) d_r_va})
		buf.ptrs.push_back(p);
	HIP_TRY(hipStreamSynchronize(nullptr));
	M->transpose_seconds += amg_since(t0);

	t0 = std::chrono::steady_clock::now();
	L.nnz_p = nnz_p;
	ABI_TRY(at.pattern(L.p_rp, L.p_ci));
	L.p_va.assign((size_t) nnz_p, 0.0);
	std::vector<int32_t> r_rp((size_t) nc + 1), r_ci((size_t) nnz_p);
	std::vector<double> r_va((size_t) nnz_p);
	HIP_TRY(hipMemcpy(L.p_va.data(), d_p, (size_t) nnz_p * 8, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(r_rp.data(), d_r_rp, (size_t) (nc + 1) * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(r_ci.data(), d_r_ci, (size_t) nnz_p * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(r_va.data(), d_r_va, (size_t) nnz_p * 8, hipMemcpyDeviceToHost));
	M->download_seconds += amg_since(t0);

	// A_{l+1} = R (A_l P)
	t0 = std::chrono::steady_clock::now();
	double * d_ap, * d_ac;
	AmgProduct ap, ac;
	ABI_TRY(ap.run(M->device, n, n, nc, L.rp.data(), L.ci.data(), d_va, L.p_rp.data(), L.p_ci.data(), d_p, buf, &d_ap));
	std::vector<int32_t> ap_rp, ap_ci;
	ABI_TRY(ap.pattern(ap_rp, ap_ci));
	ABI_TRY(ac.run(M->device, nc, n, nc, r_rp.data(), r_ci.data(), d_r_va, ap_rp.data(), ap_ci.data(), d_ap, buf, &d_ac));
	M->spgemm_seconds += amg_since(t0);
	t0 = std::chrono::steady_clock::now();
	M->lev.emplace_back();                            // reserved in amg_create: L stays valid
	AmgLevel & C = M->lev.back();
	C.n = nc;
	C.nn = nrm;
	C.nnz = ac.plan->nnz_c;
	ABI_TRY(ac.pattern(C.rp, C.ci));
	C.va.assign((size_t) std::max<long>(C.nnz, 1), 0.0);
	HIP_TRY(hipMemcpy(C.va.data(), d_ac, (size_t) C.nnz * 8, hipMemcpyDeviceToHost));
	M->download_seconds += amg_since(t0);

	// the handles of P and R, values narrowed as create narrows them
	t0 = std::chrono::steady_clock::now();
	ABI_TRY(spmv_mi355x_create(&L.P, M->format, M->precision, n, nc, nnz_p, L.p_rp.data(), L.p_ci.data(), L.p_va.data(), &o));
	ABI_TRY(spmv_mi355x_create(&L.R, M->format, M->precision, nc, n, nnz_p, r_rp.data(), r_ci.data(), r_va.data(), &o));
	M->create_seconds += amg_since(t0);
	*last_out = false;
	return 0;
}

// The packed factor of the last level, row-major lower triangle; false when a pivot is not positive.
static bool
amg_factor(const AmgLevel & L, std::vector<double> & F)
{
	const long n = L.n;
	std::vector<double> S((size_t) (n * (n + 1) / 2), 0.0);
	for (long i = 0; i < n; i++)
		for (long e = L.rp[i]; e < L.rp[i + 1]; e++)
			if (L.ci[e] <= i)
				S[(size_t) (i * (i + 1) / 2 + L.ci[e])] = L.va[e];
	F.assign(S.size(), 0.0);
	for (long k = 0; k < n; k++)
		for (long a = k; a < n; a++)
		{
			double s = S[(size_t) (a * (a + 1) / 2 + k)];
			for (long p = 0; p < k; p++)
				s = std::fma(-F[(size_t) (a * (a + 1) / 2 + p)], F[(size_t) (k * (k + 1) / 2 + p)], s);
			if (a == k)
			{
				if (!std::isfinite(s) || !(s > 0))
					return false;
				F[(size_t) (k * (k + 1) / 2 + k)] = std::sqrt(s);
			}
			else
				F[(size_t) (a * (a + 1) / 2 + k)] = s / F[(size_t) (k * (k + 1) / 2 + k)];
		}
	return true;
}

static int
amg_build(spmv_mi355x_amg * M, const spmv_mi355x_opts & o)
{
	for (int l = 0;; l++)
	{
		bool last = true;
		ABI_TRY(amg_build_level(M, l, o, &last));
		AmgLevel & L = M->lev[(size_t) l];
		const auto t0 = std::chrono::steady_clock::now();
		ABI_TRY(spmv_mi355x_create(&L.A, M->format, M->precision, L.n, L.n, L.nnz, L.rp.data(), L.ci.data(), L.va.data(), &o));
		M->create_seconds += amg_since(t0);
		if (last)
			break;
	}
	M->levels = (int) M->lev.size();
	const AmgLevel & Z = M->lev.back();
	M->coarse_kind = SPMV_MI355X_AMG_COARSE_SWEEPS;
	if (Z.n <= AMG_DENSE_MAX)
	{
		std::vector<double> F;
		if (amg_factor(Z, F))
		{
			M->coarse_kind = SPMV_MI355X_AMG_COARSE_DENSE;
			ABI_TRY(dev_alloc_bytes((void **) &M->d_factor, F.size() * 8));
			HIP_TRY(hipMemcpy(M->d_factor, F.data(), F.size() * 8, hipMemcpyHostToDevice));
			M->vector_bytes += (double) F.size() * 8;
		}
		else
			M->coarse_kind = SPMV_MI355X_AMG_COARSE_SWEEPS_AFTER_PIVOT;
	}
	amg_count_launches(M);
	return 0;
}

// ---- new values for a hierarchy ------------------------------------------------------------------------------------------------------

static const char * const AMG_OPERATOR_NAMES[3] = {"A", "P", "R"};

// 0 and an error "<what>: level l: X: <the handle's reason>" if a handle of the hierarchy takes no update, else 1
static int
amg_handles_updatable(const char * what, const spmv_mi355x_amg * M)
{
	for (int l = 0; l < M->levels; l++)
	{
		const AmgLevel & L = M->lev[(size_t) l];
		const spmv_mi355x_matrix * const h[3] = {L.A, L.P, L.R};
		for (int k = 0; k < 3; k++)
			if (h[k] && spmv_mi355x_update_values_state(h[k]) == 0)
			{
				const std::string why = spmv_mi355x_last_error();
				set_error("%s: level %d: %s: %s", what, l, AMG_OPERATOR_NAMES[k], why.c_str());
				return 0;
			}
	}
	return 1;
}

template <typename T>
static int
amg_keep(AmgUpdate * u, T ** out, size_t count, const T * host = nullptr)
{
	void * p = nullptr;
	const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
	ABI_TRY(dev_alloc_bytes(&p, bytes));
	u->owned.push_back(p);
	u->bytes += (double) bytes;
	*out = (T *) p;
	if (host && count)
		HIP_TRY(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
	return 0;
}

static int
amg_plan(AmgUpdate * u, spmv_mi355x_spgemm ** plan, int device, long m, long k, long n, const int32_t * a_rp, const int32_t * a_ci,
		const int32_t * b_rp, const int32_t * b_ci)
{
	ABI_TRY(spmv_mi355x_spgemm_create(plan, device, m, k, n, a_rp, a_ci, b_rp, b_ci));
	u->bytes += (double) (*plan)->device_bytes;
	return 0;
}

// what prepare keeps of level l (AmgUpdateLevel); u->lev has an entry per level already
static int
amg_prepare_level(spmv_mi355x_amg * M, AmgUpdate * u, int l)
{
	AmgLevel & L = M->lev[(size_t) l];
	AmgUpdateLevel & U = u->lev[(size_t) l];
	const long n = L.n;
	ABI_TRY(amg_keep(u, &U.d_va, (size_t) L.nnz));
	ABI_TRY(amg_keep(u, &U.d_d, (size_t) n));
	ABI_TRY(spmv_mi355x_update_values_prepare(L.A, L.rp.data()));
	if (!L.P)
	{
		int * d_rp, * d_ci;
		ABI_TRY(amg_keep(u, &d_rp, (size_t) n + 1, (const int *) L.rp.data()));
		ABI_TRY(amg_keep(u, &d_ci, (size_t) L.nnz, (const int *) L.ci.data()));
		U.d_rp = d_rp;
		U.d_ci = d_ci;
		return 0;
	}
	const long nc = L.aggregates, nnz_p = L.nnz_p;
	const AmgLevel & C = M->lev[(size_t) l + 1];
	// A T: its pattern is P's, its copy of A_l's pattern serves step 1
	std::vector<int32_t> t_rp((size_t) n + 1);
	for (long i = 0; i <= n; i++)
		t_rp[(size_t) i] = (int32_t) i;
	ABI_TRY(amg_plan(u, &U.at, M->device, n, n, nc, M->filtered ? L.f_rp.data() : L.rp.data(), M->filtered ? L.f_ci.data() : L.ci.data(),
			t_rp.data(), L.agg.data()));
	U.d_rp = U.at->d_a_rp;                                // filtered: A_F's pattern; A_l's own comes with the plan of A P below
	U.d_ci = U.at->d_a_ci;
	if (M->filtered)
	{
		U.d_f_rp = U.at->d_a_rp;
		ABI_TRY(amg_keep(u, &U.d_map, (size_t) L.nnz_f, (const int *) L.f_map.data()));
		ABI_TRY(amg_keep(u, &U.d_fb, (size_t) n, (const int *) L.f_fb.data()));
		ABI_TRY(amg_keep(u, &U.d_fva, (size_t) L.nnz_f));
		ABI_TRY(amg_keep(u, &U.d_df, (size_t) n));
	}
	if (M->has_nn)
		ABI_TRY(amg_keep(u, &U.d_t, (size_t) n, L.tv.data()));
	if (U.at->nnz_c != nnz_p || U.at->c_rp != L.p_rp)
	{
		set_error("amg_update_values_prepare: internal: level %d: the pattern of A T (%ld entries) is not that of P (%ld)", l, U.at->nnz_c, nnz_p);
		return 1;
	}
	{
		const std::vector<double> ones((size_t) n, 1.0);
		ABI_TRY(amg_keep(u, &U.d_ones, (size_t) n, ones.data()));
	}
	ABI_TRY(amg_keep(u, &U.d_agg, (size_t) n, (const int *) L.agg.data()));
	ABI_TRY(amg_keep(u, &U.d_at, (size_t) nnz_p));
	ABI_TRY(amg_keep(u, &U.d_p, (size_t) nnz_p));
	ABI_TRY(amg_keep(u, &U.d_r, (size_t) nnz_p));
	// the entry map P -> R and R's pattern, in the transposition's own order
	int * d_r_rp = nullptr;
	long lnnz = 0;
	ABI_TRY(transpose_entry_map(true, n, nc, nnz_p, L.p_rp.data(), L.p_ci.data(), 0, nc, &d_r_rp, &U.d_src, &lnnz));
	u->owned.push_back(d_r_rp);
	u->owned.push_back(U.d_src);
	u->bytes += (double) (nc + 1) * 4 + (double) std::max<long>(lnnz, 1) * 4;
	if (lnnz != nnz_p)
	{
		set_error("amg_update_values_prepare: internal: level %d: the transposition of P has %ld entries, P has %ld", l, lnnz, nnz_p);
		return 1;
	}
	std::vector<int32_t> r_rp((size_t) nc + 1), r_ci((size_t) std::max<long>(nnz_p, 1)), row_of((size_t) std::max<long>(nnz_p, 1));
	std::vector<unsigned> src((size_t) std::max<long>(nnz_p, 1));
	HIP_TRY(hipMemcpy(r_rp.data(), d_r_rp, (size_t) (nc + 1) * 4, hipMemcpyDeviceToHost));
	HIP_TRY(hipMemcpy(src.data(), U.d_src, (size_t) nnz_p * 4, hipMemcpyDeviceToHost));
	for (long i = 0; i < n; i++)
		for (long e = L.p_rp[(size_t) i]; e < L.p_rp[(size_t) i + 1]; e++)
			row_of[(size_t) e] = (int32_t) i;
	for (long e = 0; e < nnz_p; e++)
	{
		if ((long) src[(size_t) e] >= nnz_p)
		{
			set_error("amg_update_values_prepare: internal: level %d: entry %ld of the map P -> R is %u of %ld", l, e, src[(size_t) e], nnz_p);
			return 1;
		}
		r_ci[(size_t) e] = row_of[src[(size_t) e]];
	}
	// A P and R (A P): the second must come back with the pattern of level l + 1
	ABI_TRY(amg_plan(u, &U.ap, M->device, n, n, nc, L.rp.data(), L.ci.data(), L.p_rp.data(), L.p_ci.data()));
	if (M->filtered)
	{
		U.d_rp = U.ap->d_a_rp;
		U.d_ci = U.ap->d_a_ci;
	}
	std::vector<int32_t> ap_rp((size_t) n + 1), ap_ci((size_t) std::max<long>(U.ap->nnz_c, 1));
	ABI_TRY(spmv_mi355x_spgemm_pattern(U.ap, ap_rp.data(), ap_ci.data()));
	ABI_TRY(amg_keep(u, &U.d_ap, (size_t) U.ap->nnz_c));
	ABI_TRY(amg_plan(u, &U.ac, M->device, nc, n, nc, r_rp.data(), r_ci.data(), ap_rp.data(), ap_ci.data()));
	std::vector<int32_t> c_rp((size_t) nc + 1), c_ci((size_t) std::max<long>(U.ac->nnz_c, 1));
	ABI_TRY(spmv_mi355x_spgemm_pattern(U.ac, c_rp.data(), c_ci.data()));
	c_ci.resize((size_t) U.ac->nnz_c);
	if (U.ac->nnz_c != C.nnz || U.ac->c_rp != C.rp || !std::equal(c_ci.begin(), c_ci.end(), C.ci.begin()))
	{
		set_error("amg_update_values_prepare: internal: level %d: R (A P) has another pattern than level %d (%ld entries, %ld)", l, l + 1,
				U.ac->nnz_c, C.nnz);
		return 1;
	}
	ABI_TRY(spmv_mi355x_update_values_prepare(L.P, L.p_rp.data()));
	ABI_TRY(spmv_mi355x_update_values_prepare(L.R, r_rp.data()));
	return 0;
}

// the host copies level_csr returns, brought up to the device's after an update
static int
amg_refresh_host(spmv_mi355x_amg * M)
{
	AmgUpdate * u = M->upd;
	if (!u || !u->host_stale)
		return 0;
	HIP_TRY(hipSetDevice(M->device));
	for (int l = 0; l < M->levels; l++)
	{
		AmgLevel & L = M->lev[(size_t) l];
		const AmgUpdateLevel & U = u->lev[(size_t) l];
		if (L.nnz > 0)
			HIP_TRY(hipMemcpy(L.va.data(), U.d_va, (size_t) L.nnz * 8, hipMemcpyDeviceToHost));
		if (L.P && L.nnz_p > 0)
			HIP_TRY(hipMemcpy(L.p_va.data(), U.d_p, (size_t) L.nnz_p * 8, hipMemcpyDeviceToHost));
		if (L.P && M->filtered && L.nnz_f > 0)
			HIP_TRY(hipMemcpy(L.f_va.data(), U.d_fva, (size_t) L.nnz_f * 8, hipMemcpyDeviceToHost));
	}
	u->host_stale = false;
	return 0;
}

// step 1 of level l on `va`: d into the level's array; *bad_out = the bad diagonals, *rho_out = the largest partial
static int
amg_update_diag(spmv_mi355x_amg * M, int l, const double * va, hipStream_t st, int * bad_out, double * rho_out)
{
	AmgUpdate * u = M->upd;
	const AmgUpdateLevel & U = u->lev[(size_t) l];
	const long n = M->lev[(size_t) l].n;
	const AmgCsr a = {U.d_rp, U.d_ci, va, n};
	ABI_TRY(launch_amg_diag_check(a, U.d_d, u->d_part, u->d_count + l, st));
	double part[AMG_MAX_GRID];
	HIP_TRY(hipMemcpyAsync(bad_out, u->d_count + l, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(part, u->d_part, (size_t) amg_grid(n) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	*rho_out = *std::max_element(part, part + amg_grid(n));
	return 0;
}

// the first row of level l whose diagonal is not positive and finite (an error path: n doubles come to the host)
static int
amg_first_bad_row(spmv_mi355x_amg * M, int l, long * row_out, double * d_out)
{
	const long n = M->lev[(size_t) l].n;
	std::vector<double> d((size_t) n);
	HIP_TRY(hipMemcpy(d.data(), M->upd->lev[(size_t) l].d_d, (size_t) n * 8, hipMemcpyDeviceToHost));
	*row_out = -1;
	for (long i = 0; i < n && *row_out < 0; i++)
		if (!std::isfinite(d[(size_t) i]) || !(d[(size_t) i] > 0))
		{
			*row_out = i;
			*d_out = d[(size_t) i];
		}
	return 0;
}

// step 5a of the coarsened level l on `va` over the frozen kept pattern: dF into the level's array, A_F's values into f_va (NULL: the
// check alone); *bad_out = the rows filtered at create whose lumped diagonal is bad, *rho_out = the largest partial
static int
amg_update_filter(spmv_mi355x_amg * M, int l, const double * va, double * f_va, hipStream_t st, int * bad_out, double * rho_out)
{
	AmgUpdate * u = M->upd;
	const AmgUpdateLevel & U = u->lev[(size_t) l];
	const long n = M->lev[(size_t) l].n;
	const AmgCsr a = {U.d_rp, U.d_ci, va, n};
	int * d_bad = u->d_count + SPMV_MI355X_AMG_MAX_LEVELS + 1 + l;
	HIP_TRY(hipMemsetAsync(d_bad, 0, 4, st));
	ABI_TRY(launch_amg_filter_values(a, U.d_d, U.d_f_rp, U.d_map, U.d_fb, U.d_df, f_va, u->d_part, d_bad, st));
	double part[AMG_MAX_GRID];
	HIP_TRY(hipMemcpyAsync(bad_out, d_bad, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(part, u->d_part, (size_t) amg_grid(n) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	*rho_out = *std::max_element(part, part + amg_grid(n));
	return 0;
}

// the first row of level l that was filtered at create and whose lumped diagonal is not positive and finite (an error path)
static int
amg_first_bad_lump(spmv_mi355x_amg * M, int l, long * row_out, double * d_out)
{
	const AmgLevel & L = M->lev[(size_t) l];
	std::vector<double> d((size_t) L.n);
	HIP_TRY(hipMemcpy(d.data(), M->upd->lev[(size_t) l].d_df, (size_t) L.n * 8, hipMemcpyDeviceToHost));
	*row_out = -1;
	for (long i = 0; i < L.n && *row_out < 0; i++)
		if (!L.f_fb[(size_t) i] && (!std::isfinite(d[(size_t) i]) || !(d[(size_t) i] > 0)))
		{
			*row_out = i;
			*d_out = d[(size_t) i];
		}
	return 0;
}

// Levels 0, 1, ... from the values of level 0 in u->lev[0].d_va; level 0's step 1 has run and passed (rho0). 1 = error set: the
// hierarchy is partly rewritten.
static int
amg_update_levels(spmv_mi355x_amg * M, double rho0, hipStream_t st)
{
	AmgUpdate * u = M->upd;
	const bool f32 = M->f32;
	for (int l = 0; l < M->levels; l++)
	{
		AmgLevel & L = M->lev[(size_t) l];
		AmgUpdateLevel & U = u->lev[(size_t) l];
		const long n = L.n;
		double rho = rho0;
		if (l > 0)
		{
			int bad = 0;
			ABI_TRY(amg_update_diag(M, l, U.d_va, st, &bad, &rho));
			if (bad > 0)
			{
				long row = -1;
				double d = 0;
				ABI_TRY(amg_first_bad_row(M, l, &row, &d));
				set_error("amg_update_values: the diagonal of row %ld of level %d is %g: the matrix is not positive definite", row, l, d);
				return 1;
			}
			if (!std::isfinite(rho) || !(rho > 0))
			{
				set_error("amg_update_values: level %d: max_i sum_j |a_ij| / a_ii = %g is not a positive finite number", l, rho);
				return 1;
			}
		}
		L.rho = rho;
		L.omega = 4.0 / (3.0 * L.rho);
		ABI_TRY(launch_amg_weights(f32, n, U.d_d, L.omega, L.w, st));
		auto t0 = std::chrono::steady_clock::now();
		ABI_TRY(spmv_mi355x_update_values_device(L.A, U.d_va, st));
		u->handle_seconds += amg_since(t0);
		// a folded level: the tail's copy of A_l's values, narrowed as the handle's are (w is the level's own array)
		const bool folded = M->fold && l >= M->fold->first;
		if (folded)
			ABI_TRY(launch_amg_fold_values(f32, U.d_va, M->fold->va[(size_t) l], L.nnz, st));
		if (!L.P)
			continue;
		AmgUpdateLevel & C = u->lev[(size_t) l + 1];
		const bool with = M->filtered || M->has_nn;
		L.omega_p = L.omega;
		L.rho_p = L.rho;
		if (M->filtered)
		{
			int bad = 0;
			ABI_TRY(amg_update_filter(M, l, U.d_va, U.d_fva, st, &bad, &L.rho_p));
			if (bad > 0)
			{
				long row = -1;
				double d = 0;
				ABI_TRY(amg_first_bad_lump(M, l, &row, &d));
				set_error("amg_update_values: the lumped diagonal of row %ld of level %d is %g: the row was filtered at create and cannot "
						"fall back now", row, l, d);
				return 1;
			}
			if (!std::isfinite(L.rho_p) || !(L.rho_p > 0))
			{
				set_error("amg_update_values: level %d: max_i sum_j |aF_ij| / dF_i = %g is not a positive finite number", l, L.rho_p);
				return 1;
			}
			L.omega_p = 4.0 / (3.0 * L.rho_p);
		}
		t0 = std::chrono::steady_clock::now();
		ABI_TRY(spmv_mi355x_spgemm_multiply_device_async(U.at, M->filtered ? U.d_fva : U.d_va, M->has_nn ? U.d_t : U.d_ones, U.d_at, st));
		HIP_TRY(hipStreamSynchronize(st));
		u->spgemm_seconds += amg_since(t0);
		if (with)
			ABI_TRY(launch_amg_prolong_t(n, U.at->d_c_rp, U.at->d_c_ci, U.d_at, U.d_agg, M->has_nn ? U.d_t : U.d_ones,
					M->filtered ? U.d_df : U.d_d, L.omega_p, U.d_p, st));
		else
			ABI_TRY(launch_amg_prolong(n, U.at->d_c_rp, U.at->d_c_ci, U.d_at, U.d_agg, U.d_d, L.omega, U.d_p, st));
		ABI_TRY(transpose_gather_values(U.d_src, U.d_p, L.nnz_p, U.d_r, st));
		if (folded)
		{
			ABI_TRY(launch_amg_fold_values(f32, U.d_p, M->fold->p_va[(size_t) l], L.nnz_p, st));
			ABI_TRY(launch_amg_fold_values(f32, U.d_r, M->fold->r_va[(size_t) l], L.nnz_p, st));
		}
		HIP_TRY(hipStreamSynchronize(st));
		t0 = std::chrono::steady_clock::now();
		ABI_TRY(spmv_mi355x_spgemm_multiply_device_async(U.ap, U.d_va, U.d_p, U.d_ap, st));
		ABI_TRY(spmv_mi355x_spgemm_multiply_device_async(U.ac, U.d_r, U.d_ap, C.d_va, st));
		HIP_TRY(hipStreamSynchronize(st));
		u->spgemm_seconds += amg_since(t0);
		t0 = std::chrono::steady_clock::now();
		ABI_TRY(spmv_mi355x_update_values_device(L.P, U.d_p, st));
		ABI_TRY(spmv_mi355x_update_values_device(L.R, U.d_r, st));
		u->handle_seconds += amg_since(t0);
	}
	// the last level: its factor, if it is small enough to have one
	const AmgLevel & Z = M->lev.back();
	const AmgUpdateLevel & UZ = u->lev.back();
	if (Z.n <= AMG_DENSE_MAX)
	{
		int * d_failed = u->d_count + M->levels;
		int failed = 0;
		const size_t fbytes = (size_t) (Z.n * (Z.n + 1) / 2) * 8;
		const AmgCsr a = {UZ.d_rp, UZ.d_ci, UZ.d_va, Z.n};
		ABI_TRY(launch_amg_dense_factor(a, u->d_factor, d_failed, st));
		HIP_TRY(hipMemcpyAsync(&failed, d_failed, 4, hipMemcpyDeviceToHost, st));
		HIP_TRY(hipStreamSynchronize(st));
		if (failed)
		{
			// as create leaves it: no factor, the level takes the sweeps
			if (M->d_factor)
			{
				(void) hipFree(M->d_factor);
				M->d_factor = nullptr;
				M->vector_bytes -= (double) fbytes;
			}
			M->coarse_kind = SPMV_MI355X_AMG_COARSE_SWEEPS_AFTER_PIVOT;
		}
		else
		{
			if (!M->d_factor)
			{
				ABI_TRY(dev_alloc_bytes((void **) &M->d_factor, fbytes));
				M->vector_bytes += (double) fbytes;
			}
			HIP_TRY(hipMemcpyAsync(M->d_factor, u->d_factor, fbytes, hipMemcpyDeviceToDevice, st));
			HIP_TRY(hipStreamSynchronize(st));
			M->coarse_kind = SPMV_MI355X_AMG_COARSE_DENSE;
		}
	}
	amg_count_launches(M);                                // the tail reads coarse_kind and d_factor at every launch: it follows a flip
	return 0;
}

// out = cycle(start, in) for one column of rows[start] values: the levels above the first folded one through their handles, the rest
// as one launch. start = 0 is amg_apply; with no fold this enqueues what it has always enqueued.
static int
amg_cycle(spmv_mi355x_amg * M, int start, const void * in_dev, void * out_dev, hipStream_t st)
{
	const bool f32 = M->f32;
	const int nl = M->levels, nu = M->opts.sweeps, cs = M->opts.coarse_sweeps, f = amg_fold_first(M);
	const bool dense = M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE;
	if (in_dev == out_dev)
	{
		// the level reads b after it has written x: an apply in place works on a copy of `in`
		HIP_TRY(hipMemcpyAsync(M->lev[(size_t) start].b, in_dev, (size_t) M->lev[(size_t) start].n * (f32 ? 4 : 8), hipMemcpyDeviceToDevice, st));
		in_dev = M->lev[(size_t) start].b;
	}
	auto rhs = [&](int l) { return l == start ? in_dev : (const void *) M->lev[(size_t) l].b; };
	auto sol = [&](int l) { return l == start ? out_dev : M->lev[(size_t) l].x; };
	auto tail = [&](int l) {
		return launch_amg_fold_tail(f32, 1, M->fold->d_single, l, nl - 1, rhs(l), 1, sol(l), 1, 1, nu, cs, dense ? M->d_factor : nullptr, st);
	};
	if (start >= f)
		return tail(start);
	auto sweep = [&](int l) {
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(spmv_mi355x_spmv_device_async(L.A, sol(l), L.t, 0, st));
		return launch_amg_sweep(f32, L.w, rhs(l), L.t, sol(l), L.n, st);
	};
	const int bottom = std::min(f, nl - 1);                   // the level the handles stop above
	for (int l = start; l < bottom; l++)
	{
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(launch_amg_first(f32, L.w, rhs(l), sol(l), L.n, st));
		for (int s = 1; s < nu; s++)
			ABI_TRY(sweep(l));
		ABI_TRY(spmv_mi355x_spmv_device_async(L.A, sol(l), L.t, 0, st));
		ABI_TRY(launch_amg_residual(f32, rhs(l), L.t, L.n, st));
		ABI_TRY(spmv_mi355x_spmv_device_async(L.R, L.t, M->lev[(size_t) l + 1].b, 0, st));
	}
	if (f < nl)
		ABI_TRY(tail(f));
	else
	{
		const int l = nl - 1;
		AmgLevel & L = M->lev[(size_t) l];
		if (dense)
			ABI_TRY(launch_amg_dense_solve(f32, M->d_factor, rhs(l), sol(l), (int) L.n, st));
		else
		{
			ABI_TRY(launch_amg_first(f32, L.w, rhs(l), sol(l), L.n, st));
			for (int s = 1; s < cs; s++)
				ABI_TRY(sweep(l));
		}
	}
	for (int l = bottom - 1; l >= start; l--)
	{
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(spmv_mi355x_spmv_device_async(L.P, M->lev[(size_t) l + 1].x, sol(l), 1, st));
		for (int s = 0; s < nu; s++)
			ABI_TRY(sweep(l));
	}
	return 0;
}

// the k-column descriptors of the tail: the single ones with the blocks mb, mx, mt for vectors (after amg_multi_reserve, which has
// synchronised the device when it replaced them)
static int
amg_fold_multi_descriptors(spmv_mi355x_amg * M)
{
	AmgFold * F = M->fold;
	if (!F || M->multi_k == 0)
		return 0;
	std::vector<AmgFoldLevel> d = F->host;
	for (int l = F->first; l < M->levels; l++)
	{
		d[(size_t) l].b = M->mb[(size_t) l];
		d[(size_t) l].x = M->mx[(size_t) l];
		d[(size_t) l].t = M->mt[(size_t) l];
	}
	HIP_TRY(hipMemcpy(F->d_multi, d.data(), d.size() * sizeof(AmgFoldLevel), hipMemcpyHostToDevice));
	return 0;
}

template <typename T>
static int
amg_fold_keep(AmgFold * F, T ** out, size_t count, const T * host)
{
	void * p = nullptr;
	const size_t bytes = std::max<size_t>(count, 1) * sizeof(T);
	ABI_TRY(dev_alloc_bytes(&p, bytes));
	F->owned.push_back(p);
	F->bytes += (double) bytes;
	*out = (T *) p;
	if (host && count)
		HIP_TRY(hipMemcpy(p, host, count * sizeof(T), hipMemcpyHostToDevice));
	return 0;
}

// `count` fp64 values narrowed to the handle's precision, as create narrows them, on the device
static int
amg_fold_keep_values(AmgFold * F, bool f32, void ** out, const double * host, size_t count)
{
	if (!f32)
		return amg_fold_keep(F, (double **) out, count, host);
	std::vector<float> v(count);
	for (size_t e = 0; e < count; e++)
		v[e] = (float) host[e];
	return amg_fold_keep(F, (float **) out, count, v.data());
}

// The fold's data for the levels first .. levels - 1: the CSR copies of A_l and P_l from the host copies the hierarchy keeps, R_l as
// the stable transposition of P_l (rows ascending within a column: the device transposition's order), the descriptors.
static int
amg_fold_build(spmv_mi355x_amg * M, int first)
{
	AmgFold * F = new AmgFold();
	M->fold = F;
	F->first = first;
	const size_t nl = (size_t) M->levels;
	F->host.assign(nl, AmgFoldLevel{});
	F->va.assign(nl, nullptr);
	F->p_va.assign(nl, nullptr);
	F->r_va.assign(nl, nullptr);
	for (size_t l = (size_t) first; l < nl; l++)
	{
		const AmgLevel & L = M->lev[l];
		AmgFoldLevel & D = F->host[l];
		int * rp, * ci;
		ABI_TRY(amg_fold_keep(F, &rp, (size_t) L.n + 1, (const int *) L.rp.data()));
		ABI_TRY(amg_fold_keep(F, &ci, (size_t) L.nnz, (const int *) L.ci.data()));
		ABI_TRY(amg_fold_keep_values(F, M->f32, &F->va[l], L.va.data(), (size_t) L.nnz));
		D.a_rp = rp;
		D.a_ci = ci;
		D.a_va = F->va[l];
		D.w = L.w;
		D.b = L.b;
		D.x = L.x;
		D.t = L.t;
		D.n = (int) L.n;
		const int g = amg_fold_lanes(L.n, L.nnz);
		for (D.lg = 0; (1 << D.lg) < g; D.lg++)
			;
		if (!L.P)
			continue;
		const long nc = L.aggregates, nnz_p = L.nnz_p;
		ABI_TRY(amg_fold_keep(F, &rp, (size_t) L.n + 1, (const int *) L.p_rp.data()));
		ABI_TRY(amg_fold_keep(F, &ci, (size_t) nnz_p, (const int *) L.p_ci.data()));
		ABI_TRY(amg_fold_keep_values(F, M->f32, &F->p_va[l], L.p_va.data(), (size_t) nnz_p));
		D.p_rp = rp;
		D.p_ci = ci;
		D.p_va = F->p_va[l];
		std::vector<int> r_rp((size_t) nc + 1, 0), r_ci((size_t) std::max<long>(nnz_p, 1)), at((size_t) std::max<long>(nc, 1));
		std::vector<double> r_va((size_t) std::max<long>(nnz_p, 1));
		for (long e = 0; e < nnz_p; e++)
			r_rp[(size_t) L.p_ci[(size_t) e] + 1]++;
		for (long j = 0; j < nc; j++)
		{
			r_rp[(size_t) j + 1] += r_rp[(size_t) j];
			at[(size_t) j] = r_rp[(size_t) j];
		}
		for (long i = 0; i < L.n; i++)
			for (long e = L.p_rp[(size_t) i]; e < L.p_rp[(size_t) i + 1]; e++)
			{
				const int to = at[(size_t) L.p_ci[(size_t) e]]++;
				r_ci[(size_t) to] = (int) i;
				r_va[(size_t) to] = L.p_va[(size_t) e];
			}
		ABI_TRY(amg_fold_keep(F, &rp, (size_t) nc + 1, (const int *) r_rp.data()));
		ABI_TRY(amg_fold_keep(F, &ci, (size_t) nnz_p, (const int *) r_ci.data()));
		ABI_TRY(amg_fold_keep_values(F, M->f32, &F->r_va[l], r_va.data(), (size_t) nnz_p));
		D.r_rp = rp;
		D.r_ci = ci;
		D.r_va = F->r_va[l];
	}
	ABI_TRY(amg_fold_keep(F, &F->d_single, nl, F->host.data()));
	ABI_TRY(amg_fold_keep(F, &F->d_multi, nl, F->host.data()));
	return amg_fold_multi_descriptors(M);
}

}  // namespace spmv

using namespace spmv;

extern "C" {

static const AmgLevel * amg_level_of(const char * what, const spmv_mi355x_amg * M, int level);

// amg_create (popts_in == NULL, what = "amg_create") and amg_create_with
static int
amg_create_impl(const char * what, spmv_mi355x_amg ** out, int format, int precision, long n, const int32_t * row_ptr, const int32_t * col_idx,
		const double * values, const spmv_mi355x_amg_opts * amg_opts, const spmv_mi355x_amg_prolongator_opts * popts_in,
		const spmv_mi355x_opts * opts_in)
{
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
	spmv_mi355x_amg_opts a = {(int) sizeof(spmv_mi355x_amg_opts), 0.08, 10, 128, 1, 4};
	if (amg_opts)
	{
		const size_t sz = std::min<size_t>(sizeof(a), (size_t) std::max(amg_opts->struct_size, 0));
		if (sz < 8)
		{
			set_error("%s: amg_opts->struct_size not set", what);
			return 1;
		}
		memcpy(&a, amg_opts, sz);
		a.struct_size = (int) sizeof(a);
	}
	if (!amg_scalars_ok(what, format, precision, n, o, a))
		return 1;
	spmv_mi355x_amg_prolongator_opts po = {(int) sizeof(spmv_mi355x_amg_prolongator_opts), 0, nullptr};
	if (popts_in)
	{
		const size_t sz = std::min<size_t>(sizeof(po), (size_t) std::max(popts_in->struct_size, 0));
		if (sz < 8)
		{
			set_error("%s: prolongator_opts->struct_size not set", what);
			return 1;
		}
		memcpy(&po, popts_in, sz);
		if (po.filtered < 0 || po.filtered > 1)
		{
			set_error("%s: prolongator_opts->filtered = %d out of range 0..1", what, po.filtered);
			return 1;
		}
	}
	// 2. NULL pointers
	const bool entries = row_ptr && row_ptr[n] > 0;
	if (!out || !row_ptr || (entries && (!col_idx || !values)))
	{
		set_error("%s: NULL argument (%s%s%s%s )", what, !out ? " out" : "", !row_ptr ? " row_ptr" : "", entries && !col_idx ? " col_idx" : "",
				entries && !values ? " values" : "");
		return 1;
	}
	// 3. to 5. the pattern, no column twice, the diagonal
	if (amg_check_matrix(what, n, row_ptr, col_idx, values))
		return 1;
	// the near-null vector: finite and not 0
	for (long i = 0; po.near_null && i < n; i++)
		if (!std::isfinite(po.near_null[i]) || po.near_null[i] == 0)
		{
			set_error("%s: near_null[%ld] = %g: every entry must be finite and not 0", what, i, po.near_null[i]);
			return 1;
		}
	// 6. the device
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

	spmv_mi355x_amg * M = new spmv_mi355x_amg();
	M->precision = precision;
	M->f32 = precision == SPMV_MI355X_F32;
	M->device = device;
	M->format = format;
	M->n = n;
	M->opts = a;
	M->filtered = po.filtered != 0;
	M->has_nn = po.near_null != nullptr;
	if (n > 0)
	{
		M->lev.reserve(SPMV_MI355X_AMG_MAX_LEVELS + 1);
		M->lev.emplace_back();
		AmgLevel & L = M->lev[0];
		L.n = n;
		L.nnz = row_ptr[n];
		L.rp.assign(row_ptr, row_ptr + n + 1);
		L.ci.assign(col_idx, col_idx + L.nnz);
		L.va.assign(values, values + L.nnz);
		if (po.near_null)
			L.nn.assign(po.near_null, po.near_null + n);
		if (amg_build(M, o))
		{
			std::string msg = spmv_mi355x_last_error();
			amg_free(M);
			for (const char * own : {"amg_create: ", "amg_create_with: "})
				if (msg.rfind(own, 0) == 0)
					msg = msg.substr(strlen(own));
			set_error("%s: %s", what, msg.c_str());
			return 1;
		}
	}
	M->setup_seconds = amg_since(t_start);
	*out = M;
	return 0;
}

int
spmv_mi355x_amg_create(spmv_mi355x_amg ** out, int format, int precision, long n, const int32_t * row_ptr, const int32_t * col_idx,
		const double * values, const spmv_mi355x_amg_opts * amg_opts, const spmv_mi355x_opts * opts_in)
{
	return amg_create_impl("amg_create", out, format, precision, n, row_ptr, col_idx, values, amg_opts, nullptr, opts_in);
}

int
spmv_mi355x_amg_create_with(spmv_mi355x_amg ** out, int format, int precision, long n, const int32_t * row_ptr, const int32_t * col_idx,
		const double * values, const spmv_mi355x_amg_opts * amg_opts, const spmv_mi355x_amg_prolongator_opts * prolongator_opts,
		const spmv_mi355x_opts * opts_in)
{
	return amg_create_impl("amg_create_with", out, format, precision, n, row_ptr, col_idx, values, amg_opts, prolongator_opts, opts_in);
}

int
spmv_mi355x_amg_prolongator_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_prolongator_stats * info)
{
	if (!M || !info)
	{
		set_error("amg_prolongator_info: NULL %s", !M ? "handle" : "info");
		return 1;
	}
	if (!info_size_ok("amg_prolongator_info", info))
		return 1;
	spmv_mi355x_amg_prolongator_stats s;
	memset(&s, 0, sizeof(s));
	s.filtered = M->filtered;
	s.has_near_null = M->has_nn;
	for (int l = 0; l < M->levels; l++)
	{
		const AmgLevel & L = M->lev[(size_t) l];
		if (!L.P)
			continue;
		s.nnz_filtered[l] = L.nnz_f;
		s.unfiltered_rows[l] = L.unfiltered_rows;
		s.omega_p[l] = L.omega_p;
		s.rho_p[l] = L.rho_p;
	}
	put_info(info, info->struct_size, s);
	return 0;
}

int
spmv_mi355x_amg_near_null(const spmv_mi355x_amg * M, int level, double * out)
{
	const AmgLevel * L = amg_level_of("amg_near_null", M, level);
	if (!L)
		return 1;
	if (!L->nn.empty() && !out)
	{
		set_error("amg_near_null: NULL out");
		return 1;
	}
	if (!L->nn.empty())
		memcpy(out, L->nn.data(), L->nn.size() * sizeof(double));
	return 0;
}

int
spmv_mi355x_amg_destroy(spmv_mi355x_amg * M)
{
	if (!M)
		return 0;
	(void) hipSetDevice(M->device);
	amg_free(M);
	return 0;
}

int
spmv_mi355x_amg_apply_device_async(spmv_mi355x_amg * M, const void * in_dev, void * out_dev, void * hip_stream)
{
	if (!M || (M->n > 0 && (!in_dev || !out_dev)))
	{
		set_error("amg_apply: NULL argument (%s%s%s )", !M ? " M" : "", M && !in_dev ? " in" : "", M && !out_dev ? " out" : "");
		return 1;
	}
	if (M->n == 0)
		return 0;
	if (M->update_failed)
	{
		set_error("amg_apply: the last amg_update_values of this hierarchy failed below level 0 and left it half rewritten: update it "
				"with values it accepts first");
		return 1;
	}
	return amg_cycle(M, 0, in_dev, out_dev, (hipStream_t) hip_stream);
}

int
spmv_mi355x_amg_apply_level_device_async(spmv_mi355x_amg * M, int level, const void * in_dev, void * out_dev, void * hip_stream)
{
	const char * what = "amg_apply_level";
	if (!M)
	{
		set_error("%s: NULL handle", what);
		return 1;
	}
	if (M->update_failed)
	{
		set_error("%s: the last amg_update_values of this hierarchy failed below level 0 and left it half rewritten: update it with "
				"values it accepts first", what);
		return 1;
	}
	if (level < 0 || level >= M->levels)
	{
		set_error("%s: level %d out of range: the hierarchy has %d", what, level, M->levels);
		return 1;
	}
	if (!in_dev || !out_dev)
	{
		set_error("%s: NULL argument (%s%s )", what, !in_dev ? " in" : "", !out_dev ? " out" : "");
		return 1;
	}
	return amg_cycle(M, level, in_dev, out_dev, (hipStream_t) hip_stream);
}

int
spmv_mi355x_amg_apply(spmv_mi355x_amg * M, const void * in_host, void * out_host)
{
	if (!M || (M->n > 0 && (!in_host || !out_host)))
	{
		set_error("amg_apply: NULL argument (%s%s%s )", !M ? " M" : "", M && !in_host ? " in" : "", M && !out_host ? " out" : "");
		return 1;
	}
	if (M->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(M->device));
	const size_t bytes = (size_t) M->n * (M->f32 ? 4 : 8);
	if (!M->d_in && (dev_alloc_bytes(&M->d_in, bytes) || dev_alloc_bytes(&M->d_out, bytes)))
		return 1;
	HIP_TRY(hipMemcpyAsync(M->d_in, in_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_amg_apply_device_async(M, M->d_in, M->d_out, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(out_host, M->d_out, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

// the checks every k-column entry shares, in the single apply's wording; *empty: n == 0, nothing to do
static bool
amg_multi_arguments_ok(const char * what, spmv_mi355x_amg * M, int k, const void * in, long ldin, void * out, long ldout, bool * empty)
{
	*empty = false;
	if (!M || (M->n > 0 && (!in || !out)))
	{
		set_error("%s: NULL argument (%s%s%s )", what, !M ? " M" : "", M && !in ? " in" : "", M && !out ? " out" : "");
		return false;
	}
	if (k < 1)
	{
		set_error("%s: k = %d: at least one column is needed", what, k);
		return false;
	}
	if (ldin < k || ldout < k)
	{
		set_error("%s: ldin = %ld, ldout = %ld: both must be >= k = %d", what, ldin, ldout, k);
		return false;
	}
	if (M->n == 0)
	{
		*empty = true;
		return true;
	}
	if (M->update_failed)
	{
		set_error("%s: the last amg_update_values of this hierarchy failed below level 0 and left it half rewritten: update it with "
				"values it accepts first", what);
		return false;
	}
	return true;
}

// the per-level blocks for k columns; a larger k frees the smaller blocks after the device has finished with them
static int
amg_multi_reserve(spmv_mi355x_amg * M, int k)
{
	if (k <= M->multi_k)
		return 0;
	HIP_TRY(hipDeviceSynchronize());
	for (std::vector<void *> * v : {&M->mb, &M->mx, &M->mt})
	{
		for (void * p : *v)
			if (p)
				(void) hipFree(p);
		v->assign((size_t) M->levels, nullptr);
	}
	M->vector_bytes -= M->multi_bytes;
	M->multi_bytes = 0;
	M->multi_k = 0;
	for (int l = 0; l < M->levels; l++)
	{
		const size_t bytes = (size_t) M->lev[(size_t) l].n * (size_t) k * (M->f32 ? 4 : 8);
		for (std::vector<void *> * v : {&M->mb, &M->mx, &M->mt})
		{
			if (l == 0 && v == &M->mx)
				continue;
			ABI_TRY(dev_alloc_bytes(&(*v)[(size_t) l], bytes));
			M->multi_bytes += (double) bytes;
		}
	}
	M->vector_bytes += M->multi_bytes;
	M->multi_k = k;
	return amg_fold_multi_descriptors(M);
}

int
spmv_mi355x_amg_apply_multi_device_async(spmv_mi355x_amg * M, int k, const void * in_dev, long ldin, void * out_dev, long ldout,
		void * hip_stream)
{
	bool empty;
	if (!amg_multi_arguments_ok("amg_apply_multi", M, k, in_dev, ldin, out_dev, ldout, &empty))
		return 1;
	if (in_dev == out_dev && ldin != ldout)
	{
		set_error("amg_apply_multi: in == out needs ldin == ldout (got %ld and %ld)", ldin, ldout);
		return 1;
	}
	if (empty)
		return 0;
	ABI_TRY(amg_multi_reserve(M, k));
	hipStream_t st = (hipStream_t) hip_stream;
	const bool f32 = M->f32;
	const size_t vs = f32 ? 4 : 8;
	const int nl = M->levels, nu = M->opts.sweeps;
	const long ld = k;                                                // of the hierarchy's blocks, whatever k they were allocated for
	if (in_dev == out_dev)
	{
		// level 0 reads b after it has written x: an apply in place works on a copy of the k columns of `in`
		HIP_TRY(hipMemcpy2DAsync(M->mb[0], (size_t) ld * vs, in_dev, (size_t) ldin * vs, (size_t) k * vs, (size_t) M->n,
				hipMemcpyDeviceToDevice, st));
		in_dev = M->mb[0];
		ldin = ld;
	}
	auto rhs = [&](int l) { return l == 0 ? in_dev : (const void *) M->mb[(size_t) l]; };
	auto sol = [&](int l) { return l == 0 ? out_dev : M->mx[(size_t) l]; };
	auto ldb = [&](int l) { return l == 0 ? ldin : ld; };
	auto ldx = [&](int l) { return l == 0 ? ldout : ld; };
	auto sweep = [&](int l) {
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(spmv_mi355x_spmm_device_async(L.A, k, sol(l), ldx(l), M->mt[(size_t) l], ld, 0, st));
		return launch_amg_sweep_multi(f32, k, L.w, rhs(l), ldb(l), M->mt[(size_t) l], ld, sol(l), ldx(l), L.n, st);
	};
	const int f = amg_fold_first(M), bottom = std::min(f, nl - 1);
	for (int l = 0; l < bottom; l++)
	{
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(launch_amg_first_multi(f32, k, L.w, rhs(l), ldb(l), sol(l), ldx(l), L.n, st));
		for (int s = 1; s < nu; s++)
			ABI_TRY(sweep(l));
		ABI_TRY(spmv_mi355x_spmm_device_async(L.A, k, sol(l), ldx(l), M->mt[(size_t) l], ld, 0, st));
		ABI_TRY(launch_amg_residual_multi(f32, k, rhs(l), ldb(l), M->mt[(size_t) l], ld, L.n, st));
		ABI_TRY(spmv_mi355x_spmm_device_async(L.R, k, M->mt[(size_t) l], ld, M->mb[(size_t) l + 1], ld, 0, st));
	}
	if (f < nl)
		// the rest of the cycle: one launch per chunk of columns
		ABI_TRY(launch_amg_fold_tail(f32, k, M->fold->d_multi, f, nl - 1, rhs(f), ldb(f), sol(f), ldx(f), ld, nu, M->opts.coarse_sweeps,
				M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE ? M->d_factor : nullptr, st));
	else
	{
		const int l = nl - 1;
		AmgLevel & L = M->lev[(size_t) l];
		if (M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE)
			ABI_TRY(launch_amg_dense_solve_multi(f32, k, M->d_factor, rhs(l), ldb(l), sol(l), ldx(l), (int) L.n, st));
		else
		{
			ABI_TRY(launch_amg_first_multi(f32, k, L.w, rhs(l), ldb(l), sol(l), ldx(l), L.n, st));
			for (int s = 1; s < M->opts.coarse_sweeps; s++)
				ABI_TRY(sweep(l));
		}
	}
	for (int l = bottom - 1; l >= 0; l--)
	{
		AmgLevel & L = M->lev[(size_t) l];
		ABI_TRY(spmv_mi355x_spmm_device_async(L.P, k, M->mx[(size_t) l + 1], ld, sol(l), ldx(l), 1, st));
		for (int s = 0; s < nu; s++)
			ABI_TRY(sweep(l));
	}
	return 0;
}

int
spmv_mi355x_amg_apply_multi(spmv_mi355x_amg * M, int k, const void * in_host, void * out_host)
{
	bool empty;
	if (!amg_multi_arguments_ok("amg_apply_multi", M, k, in_host, k, out_host, k, &empty))
		return 1;
	if (empty)
		return 0;
	HIP_TRY(hipSetDevice(M->device));
	const size_t bytes = (size_t) M->n * (size_t) k * (M->f32 ? 4 : 8);
	if (k > M->multi_host_k)
	{
		HIP_TRY(hipDeviceSynchronize());
		for (void ** p : {&M->d_in_multi, &M->d_out_multi})
		{
			if (*p)
				(void) hipFree(*p);
			*p = nullptr;
		}
		M->multi_host_k = 0;
		if (dev_alloc_bytes(&M->d_in_multi, bytes) || dev_alloc_bytes(&M->d_out_multi, bytes))
			return 1;
		M->multi_host_k = k;
	}
	HIP_TRY(hipMemcpyAsync(M->d_in_multi, in_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_amg_apply_multi_device_async(M, k, M->d_in_multi, k, M->d_out_multi, k, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(out_host, M->d_out_multi, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

// Host only. The cycle's products are, per coarsened level, 2 nu with A_l, one with R_l and one with P_l, and coarse_sweeps - 1 with the
// A of a last level that is not factorised; its vector launches are those of the single cycle, once per chunk of k.
int
spmv_mi355x_amg_apply_multi_plan(const spmv_mi355x_amg * M, int k, long * matrix_passes_out, long * launches_out)
{
	if (!M || !matrix_passes_out || !launches_out)
	{
		set_error("amg_apply_multi_plan: NULL argument (%s%s%s )", !M ? " M" : "", !matrix_passes_out ? " matrix_passes_out" : "",
				!launches_out ? " launches_out" : "");
		return 1;
	}
	if (k < 1)
	{
		set_error("amg_apply_multi_plan: k = %d: at least one column is needed", k);
		return 1;
	}
	long passes = 0;
	const int nu = M->opts.sweeps, cs = M->opts.coarse_sweeps;
	const bool dense = M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE;
	// a folded tail has no product of a handle: its one launch per chunk is among the vector launches below
	for (int l = 0; l < std::min(M->levels, amg_fold_first(M)); l++)
	{
		const AmgLevel & L = M->lev[(size_t) l];
		const bool last = l == M->levels - 1;
		const struct { spmv_mi355x_matrix * h; long times; } products[] = {{L.A, last ? (dense ? 0 : cs - 1) : 2 * nu}, {L.R, last ? 0 : 1},
				{L.P, last ? 0 : 1}};
		for (const auto & pr : products)
		{
			if (!pr.times)
				continue;
			int p = 0, cols = 0;
			ABI_TRY(spmv_mi355x_spmm_plan(pr.h, k, &p, &cols));
			passes += pr.times * p;
		}
	}
	const long chunks = (long) column_chunks(k).size();
	*matrix_passes_out = passes;
	*launches_out = M->levels > 0 ? passes + chunks * (M->launches - M->spmvs) : 0;
	return 0;
}

int
spmv_mi355x_amg_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_stats * info)
{
	if (!M || !info)
	{
		set_error("amg_info: NULL %s", !M ? "handle" : "info");
		return 1;
	}
	if (!info_size_ok("amg_info", info))
		return 1;
	spmv_mi355x_amg_stats s;
	memset(&s, 0, sizeof(s));
	s.levels = M->levels;
	s.coarse_kind = M->coarse_kind;
	s.stalled = M->stalled;
	double nnz_sum = 0, rows_sum = 0;
	for (int l = 0; l < M->levels; l++)
	{
		const AmgLevel & L = M->lev[(size_t) l];
		s.rows[l] = L.n;
		s.nnz[l] = L.nnz;
		s.nnz_p[l] = L.nnz_p;
		s.aggregates[l] = L.aggregates;
		s.mis_rounds[l] = L.mis_rounds;
		s.omega[l] = L.omega;
		s.rho[l] = L.rho;
		nnz_sum += (double) L.nnz;
		rows_sum += (double) L.n;
	}
	if (M->levels > 0)
	{
		s.operator_complexity = nnz_sum / (double) M->lev[0].nnz;
		s.grid_complexity = rows_sum / (double) M->lev[0].n;
	}
	s.spmvs_per_apply = M->spmvs;
	s.launches_per_apply = M->launches;
	s.setup_seconds = M->setup_seconds;
	s.coarsen_seconds = M->coarsen_seconds;
	s.spgemm_seconds = M->spgemm_seconds;
	s.transpose_seconds = M->transpose_seconds;
	s.create_seconds = M->create_seconds;
	s.download_seconds = M->download_seconds;
	put_info(info, info->struct_size, s);
	return 0;
}

int
spmv_mi355x_amg_set_fold(spmv_mi355x_amg * M, int fold_rows)
{
	const char * what = "amg_set_fold";
	if (!M)
	{
		set_error("%s: NULL handle", what);
		return 1;
	}
	if (fold_rows < 0 || fold_rows > AMG_FOLD_MAX_ROWS)
	{
		set_error("%s: fold_rows = %d out of range 0..%d", what, fold_rows, AMG_FOLD_MAX_ROWS);
		return 1;
	}
	if (M->update_failed)
	{
		set_error("%s: the last amg_update_values of this hierarchy failed below level 0 and left it half rewritten: update it with "
				"values it accepts first", what);
		return 1;
	}
	if (M->levels == 0)
	{
		M->fold_rows = fold_rows;
		return 0;
	}
	HIP_TRY(hipSetDevice(M->device));
	HIP_TRY(hipDeviceSynchronize());
	amg_fold_free(M);
	M->fold_rows = fold_rows;
	int first = M->levels;
	for (int l = M->levels - 1; l >= 0; l--)
		if (M->lev[(size_t) l].n <= fold_rows)
			first = l;
	int rc = 0;
	if (first < M->levels)
	{
		// the host copies of the values are what an update left on the device
		rc = amg_refresh_host(M) || amg_fold_build(M, first);
		if (rc)
		{
			const std::string msg = spmv_mi355x_last_error();
			amg_fold_free(M);
			M->fold_rows = 0;
			set_error("%s: %s", what, msg.c_str());
		}
	}
	amg_count_launches(M);
	return rc;
}

int
spmv_mi355x_amg_fold_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_fold_stats * info)
{
	if (!M || !info)
	{
		set_error("amg_fold_info: NULL %s", !M ? "handle" : "info");
		return 1;
	}
	if (!info_size_ok("amg_fold_info", info))
		return 1;
	spmv_mi355x_amg_fold_stats s;
	memset(&s, 0, sizeof(s));
	const int nu = M->opts.sweeps, cs = M->opts.coarse_sweeps;
	s.fold_rows = M->fold_rows;
	s.first_level = amg_fold_first(M);
	s.folded_levels = M->levels - s.first_level;
	s.launches_per_apply = M->launches;
	s.spmvs_per_apply = M->spmvs;
	for (int l = s.first_level; l < M->levels; l++)
	{
		const AmgLevel & L = M->lev[(size_t) l];
		const long with_a = L.P ? 2 * nu : M->coarse_kind == SPMV_MI355X_AMG_COARSE_DENSE ? 0 : cs - 1;
		s.tail_products += with_a + (L.P ? 2 : 0);
		s.tail_entries += with_a * L.nnz + (L.P ? 2 * L.nnz_p : 0);
		s.lanes_per_row[l] = 1 << M->fold->host[(size_t) l].lg;
	}
	s.bytes = M->fold ? M->fold->bytes : 0;
	put_info(info, info->struct_size, s);
	return 0;
}

static const AmgLevel *
amg_level_of(const char * what, const spmv_mi355x_amg * M, int level)
{
	if (!M)
	{
		set_error("%s: NULL handle", what);
		return nullptr;
	}
	if (level < 0 || level >= M->levels)
	{
		set_error("%s: level %d out of range: the hierarchy has %d", what, level, M->levels);
		return nullptr;
	}
	return &M->lev[(size_t) level];
}

int
spmv_mi355x_amg_level_matrices(const spmv_mi355x_amg * M, int level, spmv_mi355x_matrix ** A_out, spmv_mi355x_matrix ** P_out,
		spmv_mi355x_matrix ** R_out)
{
	const AmgLevel * L = amg_level_of("amg_level_matrices", M, level);
	if (!L)
		return 1;
	if (A_out)
		*A_out = L->A;
	if (P_out)
		*P_out = L->P;
	if (R_out)
		*R_out = L->R;
	return 0;
}

int
spmv_mi355x_amg_aggregates(const spmv_mi355x_amg * M, int level, int32_t * out)
{
	const AmgLevel * L = amg_level_of("amg_aggregates", M, level);
	if (!L)
		return 1;
	if (!L->agg.empty() && !out)
	{
		set_error("amg_aggregates: NULL out");
		return 1;
	}
	if (!L->agg.empty())
		memcpy(out, L->agg.data(), L->agg.size() * sizeof(int32_t));
	return 0;
}

int
spmv_mi355x_amg_level_csr(const spmv_mi355x_amg * M, int level, int which, int32_t * row_ptr_out, int32_t * col_idx_out, double * values_out)
{
	const AmgLevel * L = amg_level_of("amg_level_csr", M, level);
	if (!L)
		return 1;
	if (which != SPMV_MI355X_AMG_A && which != SPMV_MI355X_AMG_P && which != SPMV_MI355X_AMG_AF)
	{
		set_error("amg_level_csr: which = %d: SPMV_MI355X_AMG_A, SPMV_MI355X_AMG_P or SPMV_MI355X_AMG_AF", which);
		return 1;
	}
	if (which == SPMV_MI355X_AMG_AF)
	{
		if (!M->filtered)
		{
			set_error("amg_level_csr: SPMV_MI355X_AMG_AF: the hierarchy was built with filtered = 0");
			return 1;
		}
		if (!L->P)
		{
			set_error("amg_level_csr: level %d is the last: it has no filtered operator", level);
			return 1;
		}
		if (values_out && L->nnz_f > 0 && amg_refresh_host(const_cast<spmv_mi355x_amg *>(M)))
			return 1;
		if (row_ptr_out)
			memcpy(row_ptr_out, L->f_rp.data(), (size_t) (L->n + 1) * sizeof(int32_t));
		if (col_idx_out && L->nnz_f > 0)
			memcpy(col_idx_out, L->f_ci.data(), (size_t) L->nnz_f * sizeof(int32_t));
		if (values_out && L->nnz_f > 0)
			memcpy(values_out, L->f_va.data(), (size_t) L->nnz_f * sizeof(double));
		return 0;
	}
	const bool p = which == SPMV_MI355X_AMG_P;
	if (p && !L->P)
	{
		set_error("amg_level_csr: level %d is the last: it has no prolongator", level);
		return 1;
	}
	const long nnz = p ? L->nnz_p : L->nnz;
	// after an update the values live on the device: they come to the host when somebody asks
	if (values_out && nnz > 0 && amg_refresh_host(const_cast<spmv_mi355x_amg *>(M)))
		return 1;
	if (row_ptr_out)
		memcpy(row_ptr_out, (p ? L->p_rp : L->rp).data(), (size_t) (L->n + 1) * sizeof(int32_t));
	if (col_idx_out && nnz > 0)
		memcpy(col_idx_out, (p ? L->p_ci : L->ci).data(), (size_t) nnz * sizeof(int32_t));
	if (values_out && nnz > 0)
		memcpy(values_out, (p ? L->p_va : L->va).data(), (size_t) nnz * sizeof(double));
	return 0;
}

int
spmv_mi355x_amg_update_values_state(const spmv_mi355x_amg * M)
{
	if (!M)
	{
		set_error("amg_update_values_state: NULL handle");
		return 0;
	}
	if (!amg_handles_updatable("amg_update_values", M))
		return 0;
	return M->update_failed ? 3 : M->upd ? 2 : 1;
}

int
spmv_mi355x_amg_update_values_prepare(spmv_mi355x_amg * M)
{
	const char * what = "amg_update_values_prepare";
	if (!M)
	{
		set_error("%s: NULL handle", what);
		return 1;
	}
	if (!amg_handles_updatable(what, M))
		return 1;
	if (M->upd)
		return 0;
	const auto t0 = std::chrono::steady_clock::now();
	HIP_TRY(hipSetDevice(M->device));
	AmgUpdate * u = new AmgUpdate();
	u->lev.resize((size_t) M->levels);
	int rc = amg_keep(u, &u->d_part, (size_t) AMG_MAX_GRID) || amg_keep(u, &u->d_count, (size_t) 2 * (SPMV_MI355X_AMG_MAX_LEVELS + 1))
			|| amg_keep(u, &u->d_factor, (size_t) AMG_DENSE_MAX * (AMG_DENSE_MAX + 1) / 2);
	for (int l = 0; l < M->levels && !rc; l++)
		rc = amg_prepare_level(M, u, l);
	if (rc)
	{
		const std::string msg = spmv_mi355x_last_error();
		amg_update_free(u);
		if (msg.rfind("amg_update_values_prepare:", 0) != 0)
			set_error("%s: %s", what, msg.c_str());
		return 1;
	}
	u->prepare_seconds = amg_since(t0);
	M->upd = u;
	return 0;
}

int
spmv_mi355x_amg_update_values_device(spmv_mi355x_amg * M, const double * values_dev, void * hip_stream)
{
	const char * what = "amg_update_values";
	if (!M || (M->n > 0 && M->lev[0].nnz > 0 && !values_dev))
	{
		set_error("%s: NULL %s", what, !M ? "handle" : "values");
		return 1;
	}
	if (!amg_handles_updatable(what, M))
		return 1;
	AmgUpdate * u = M->upd;
	if (!u)
	{
		set_error("%s: spmv_mi355x_amg_update_values_prepare has not been called on this hierarchy", what);
		return 1;
	}
	if (reinterpret_cast<uintptr_t>(values_dev) & 7)
	{
		set_error("%s: the values must be 8-byte aligned", what);
		return 1;
	}
	if (M->n == 0)
		return 0;
	hipStream_t st = (hipStream_t) hip_stream;
	const auto t0 = std::chrono::steady_clock::now();
	HIP_TRY(hipSetDevice(M->device));
	// level 0 is checked on the caller's array before anything of the hierarchy is written
	HIP_TRY(hipMemsetAsync(u->d_count, 0, (size_t) (SPMV_MI355X_AMG_MAX_LEVELS + 1) * 4, st));
	int bad = 0;
	double rho = 0;
	ABI_TRY(amg_update_diag(M, 0, values_dev, st, &bad, &rho));
	if (bad > 0)
	{
		long row = -1;
		double d = 0;
		ABI_TRY(amg_first_bad_row(M, 0, &row, &d));
		set_error("%s: the diagonal of row %ld of level 0 is %g: it must be finite and > 0 (the hierarchy is unchanged)", what, row, d);
		return 1;
	}
	if (!std::isfinite(rho) || !(rho > 0))
	{
		set_error("%s: level 0: max_i sum_j |a_ij| / a_ii = %g is not a positive finite number (the hierarchy is unchanged)", what, rho);
		return 1;
	}
	if (M->filtered && M->lev[0].P)
	{
		double rho_p = 0;
		ABI_TRY(amg_update_filter(M, 0, values_dev, nullptr, st, &bad, &rho_p));
		if (bad > 0)
		{
			long row = -1;
			double d = 0;
			ABI_TRY(amg_first_bad_lump(M, 0, &row, &d));
			set_error("%s: the lumped diagonal of row %ld of level 0 is %g: the row was filtered at create and cannot fall back now (the "
					"hierarchy is unchanged)", what, row, d);
			return 1;
		}
	}
	HIP_TRY(hipMemcpyAsync(u->lev[0].d_va, values_dev, (size_t) M->lev[0].nnz * 8, hipMemcpyDeviceToDevice, st));
	u->spgemm_seconds = u->handle_seconds = 0;
	u->host_stale = true;
	M->update_failed = true;                              // until every level is through
	if (amg_update_levels(M, rho, st))
	{
		const std::string msg = spmv_mi355x_last_error();
		if (msg.rfind("amg_update_values:", 0) != 0)
			set_error("%s: %s", what, msg.c_str());
		(void) hipStreamSynchronize(st);
		return 1;
	}
	M->update_failed = false;
	u->updates++;
	u->update_seconds = amg_since(t0);
	return 0;
}

int
spmv_mi355x_amg_update_values(spmv_mi355x_amg * M, const double * values_host)
{
	const char * what = "amg_update_values";
	if (!M || (M->n > 0 && M->lev[0].nnz > 0 && !values_host))
	{
		set_error("%s: NULL %s", what, !M ? "handle" : "values");
		return 1;
	}
	if (!amg_handles_updatable(what, M))
		return 1;
	if (!M->upd)
	{
		set_error("%s: spmv_mi355x_amg_update_values_prepare has not been called on this hierarchy", what);
		return 1;
	}
	if (M->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(M->device));
	DeviceBuffers tmp;
	double * d_va = nullptr;
	const size_t count = (size_t) M->lev[0].nnz;
	ABI_TRY(tmp.alloc(&d_va, count * 8));
	HIP_TRY(hipMemcpy(d_va, values_host, count * 8, hipMemcpyHostToDevice));
	return spmv_mi355x_amg_update_values_device(M, d_va, nullptr);
}

int
spmv_mi355x_amg_update_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_update_stats * info)
{
	if (!M || !info)
	{
		set_error("amg_update_info: NULL %s", !M ? "handle" : "info");
		return 1;
	}
	if (!info_size_ok("amg_update_info", info))
		return 1;
	spmv_mi355x_amg_update_stats s;
	memset(&s, 0, sizeof(s));
	s.prepared = M->upd != nullptr;
	s.failed = M->update_failed;
	if (const AmgUpdate * u = M->upd)
	{
		s.updates = u->updates;
		s.prepare_bytes = u->bytes;
		s.prepare_seconds = u->prepare_seconds;
		s.update_seconds = u->update_seconds;
		s.spgemm_seconds = u->spgemm_seconds;
		s.handle_seconds = u->handle_seconds;
	}
	put_info(info, info->struct_size, s);
	return 0;
}

double
spmv_mi355x_amg_mem_footprint(const spmv_mi355x_amg * M)
{
	if (!M)
		return 0;
	double bytes = M->vector_bytes + (M->fold ? M->fold->bytes : 0);
	for (const AmgLevel & L : M->lev)
		for (const spmv_mi355x_matrix * h : {L.A, L.P, L.R})
			if (h)
				bytes += spmv_mi355x_mem_footprint(h);
	return bytes;
}

}  // extern "C"

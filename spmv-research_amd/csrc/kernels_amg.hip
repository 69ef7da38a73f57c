// The kernels of the smoothed-aggregation AMG (include/spmv_mi355x.h "AMG", amg.hpp for the mapping): steps 1 to 5 of the setup, one
// lane per row; the three vector kernels of the cycle; the dense coarsest solve; and what an update of the values adds (the checked
// step 1, the weights, the dense factor); and steps 5a to 5c of amg_create_with (the filter, the aggregate norms of a near-null
// vector, the prolongator from both). The arithmetic is the header's, as written: this file is compiled with contraction off,
// and every fma in it is spelled out.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "amg.hpp"
#include "solvers_common.hpp"

#pragma clang fp contract(off)

namespace spmv {

#define AMG_ROWS(i, n) for (long i = (long) blockIdx.x * AMG_TB + threadIdx.x; i < (n); i += (long) gridDim.x * AMG_TB)

// j in S(i), j != i: a_ij^2 >= theta^2 (d_i d_j). No sqrt, no contraction.
__device__ __forceinline__ bool
amg_strong(double a, double di, double dj, double theta2)
{
	return a * a >= theta2 * (di * dj);
}

__device__ __forceinline__ unsigned long long
amg_key(int state, long i)
{
	const unsigned h = (unsigned) i * AMG_HASH_MUL;
	return ((unsigned long long) state << 62) | ((unsigned long long) (h >> 1) << 31) | (unsigned long long) i;
}

__global__ __launch_bounds__(AMG_TB) void
amg_diag_kernel(AmgCsr a, double * __restrict__ d, double * __restrict__ part)
{
	__shared__ double sh[AMG_TB];
	double worst = 0;
	AMG_ROWS(i, a.n)
	{
		double di = 0, sum = 0;
		bool found = false;
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			const double v = a.va[e];
			if (!found && a.ci[e] == i)
			{
				di = v;
				found = true;
			}
			sum = sum + fabs(v);
		}
		d[i] = di;
		worst = fmax(worst, sum / di);
	}
	sh[threadIdx.x] = worst;
	__syncthreads();
	for (int s = AMG_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
			sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
		__syncthreads();
	}
	if (threadIdx.x == 0)
		part[blockIdx.x] = sh[0];
}

// step 1 for an update: amg_diag_kernel's d and partials, operation for operation, and *bad += the rows whose diagonal is absent, not
// finite or <= 0 (zeroed by the caller)
__global__ __launch_bounds__(AMG_TB) void
amg_diag_check_kernel(AmgCsr a, double * __restrict__ d, double * __restrict__ part, int * __restrict__ bad)
{
	__shared__ double sh[AMG_TB];
	__shared__ int shb[AMG_TB];
	double worst = 0;
	int wrong = 0;
	AMG_ROWS(i, a.n)
	{
		double di = 0, sum = 0;
		bool found = false;
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			const double v = a.va[e];
			if (!found && a.ci[e] == i)
			{
				di = v;
				found = true;
			}
			sum = sum + fabs(v);
		}
		d[i] = di;
		worst = fmax(worst, sum / di);
		wrong += !(isfinite(di) && di > 0);
	}
	sh[threadIdx.x] = worst;
	shb[threadIdx.x] = wrong;
	__syncthreads();
	for (int s = AMG_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
		{
			sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
			shb[threadIdx.x] += shb[threadIdx.x + s];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		part[blockIdx.x] = sh[0];
		if (shb[0] > 0)
			atomicAdd(bad, shb[0]);                           // an integer count: its sum does not depend on the order
	}
}

// w_i = omega / d_i, an IEEE division in fp64, narrowed to the handle's precision: the host loop of amg_build_level
template <typename T>
__global__ __launch_bounds__(AMG_TB) void
amg_weights_kernel(long n, const double * __restrict__ d, double omega, T * __restrict__ w)
{
	AMG_ROWS(i, n)
		w[i] = (T) (omega / d[i]);
}

__global__ __launch_bounds__(AMG_TB) void
amg_mis_init_kernel(long n, int * __restrict__ state, unsigned long long * __restrict__ key0)
{
	AMG_ROWS(i, n)
	{
		state[i] = 1;
		key0[i] = amg_key(1, i);
	}
}

__global__ __launch_bounds__(AMG_TB) void
amg_mis_sweep_kernel(AmgCsr a, const double * __restrict__ d, double theta2, const unsigned long long * __restrict__ in,
		unsigned long long * __restrict__ out)
{
	AMG_ROWS(i, a.n)
	{
		const double di = d[i];
		unsigned long long best = in[i];
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			const int j = a.ci[e];
			if (j != i && amg_strong(a.va[e], di, d[j], theta2))
				best = max(best, in[j]);
		}
		out[i] = best;
	}
}

__global__ __launch_bounds__(AMG_TB) void
amg_mis_decide_kernel(long n, int * __restrict__ state, unsigned long long * __restrict__ key0, const unsigned long long * __restrict__ key2,
		int * __restrict__ undecided)
{
	__shared__ int sh[AMG_TB];
	int left = 0;
	AMG_ROWS(i, n)
	{
		if (state[i] != 1)
			continue;
		const unsigned long long k = key2[i];
		int s = 1;
		if (k == key0[i])
			s = 2;
		else if ((k >> 62) == 2)
			s = 0;
		if (s != 1)
		{
			state[i] = s;
			key0[i] = amg_key(s, i);
		}
		else
			left++;
	}
	sh[threadIdx.x] = left;
	__syncthreads();
	for (int s = AMG_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
			sh[threadIdx.x] += sh[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0 && sh[0] > 0)
		atomicAdd(undecided, sh[0]);                      // an integer count: its sum does not depend on the order
}

__global__ __launch_bounds__(AMG_TB) void
amg_root_flag_kernel(long n, const int * __restrict__ state, int * __restrict__ flag)
{
	AMG_ROWS(i, n)
		flag[i] = state[i] == 2;
}

// a root takes its own number; a node with a root in S(i) that root's (roots lie more than 2 apart: there is at most one); else -1
__global__ __launch_bounds__(AMG_TB) void
amg_agg_pass1_kernel(AmgCsr a, const double * __restrict__ d, double theta2, const int * __restrict__ state, const int * __restrict__ id,
		int * __restrict__ agg1)
{
	AMG_ROWS(i, a.n)
	{
		int g = -1;
		if (state[i] == 2)
			g = id[i];
		else
		{
			const double di = d[i];
			for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
			{
				const int j = a.ci[e];
				if (j != i && state[j] == 2 && amg_strong(a.va[e], di, d[j], theta2))
					g = id[j];
			}
		}
		agg1[i] = g;
	}
}

// a node still free takes the aggregate of its assigned strong neighbour with the largest |a_ij|, ties to the smallest j
__global__ __launch_bounds__(AMG_TB) void
amg_agg_pass2_kernel(AmgCsr a, const double * __restrict__ d, double theta2, const int * __restrict__ agg1, int * __restrict__ agg2)
{
	AMG_ROWS(i, a.n)
	{
		int g = agg1[i];
		if (g < 0)
		{
			const double di = d[i];
			double best = -1.0;
			int best_j = 0x7fffffff;
			for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
			{
				const int j = a.ci[e];
				const double v = a.va[e];
				if (j == i || agg1[j] < 0 || !amg_strong(v, di, d[j], theta2))
					continue;
				const double m = fabs(v);
				if (m > best || (m == best && j < best_j))
				{
					best = m;
					best_j = j;
					g = agg1[j];
				}
			}
		}
		agg2[i] = g;
	}
}

// P_ij = (agg(i) == j ? 1 : 0) - (omega / d_i) * (A T)_ij over the entries of row i of A T
__global__ __launch_bounds__(AMG_TB) void
amg_prolong_kernel(long n, const int * __restrict__ at_rp, const int * __restrict__ at_ci, const double * __restrict__ at_va,
		const int * __restrict__ agg, const double * __restrict__ d, double omega, double * __restrict__ p_va)
{
	AMG_ROWS(i, n)
	{
		const double scale = omega / d[i];
		const int g = agg[i];
		for (int e = at_rp[i]; e < at_rp[i + 1]; e++)
			p_va[e] = (at_ci[e] == g ? 1.0 : 0.0) - scale * at_va[e];
	}
}

// ---- steps 5a to 5c: the filtered operator, the tentative prolongator of a near-null vector, the prolongator from both ---------------

// 5a, the count pass: kept[i] = the entries row i keeps (the first stored a_ii and S(i)), dF_i = d_i + lump with lump the sum of the
// others in stored order from +0.0; a dF_i that is not finite or not > 0 sends the row back to all its entries and d_i (fb[i] = 1)
__global__ __launch_bounds__(AMG_TB) void
amg_filter_count_kernel(AmgCsr a, const double * __restrict__ d, double theta2, int * __restrict__ kept, int * __restrict__ fb,
		double * __restrict__ df)
{
	AMG_ROWS(i, a.n)
	{
		const double di = d[i];
		double lump = 0.0;
		int keep = 0;
		bool found = false;
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			const int j = a.ci[e];
			const double v = a.va[e];
			bool k;
			if (j == i)
			{
				k = !found;
				found = true;
			}
			else
				k = amg_strong(v, di, d[j], theta2);
			if (k)
				keep++;
			else
				lump = lump + v;
		}
		const double dl = di + lump;
		const bool back = !(isfinite(dl) && dl > 0);
		kept[i] = back ? a.rp[i + 1] - a.rp[i] : keep;
		fb[i] = back;
		df[i] = back ? di : dl;
	}
}

// 5a, the fill pass: A_F's columns and values in A's stored order with dF_i at the diagonal's position, the map of A_F's entries
// into A's, and part[workgroup] = the workgroup's max of (sum_j |aF_ij|) / dF_i as amg_diag_kernel writes its own
__global__ __launch_bounds__(AMG_TB) void
amg_filter_fill_kernel(AmgCsr a, const double * __restrict__ d, double theta2, const int * __restrict__ f_rp, const int * __restrict__ fb,
		const double * __restrict__ df, int * __restrict__ f_ci, double * __restrict__ f_va, int * __restrict__ map, double * __restrict__ part)
{
	__shared__ double sh[AMG_TB];
	double worst = 0;
	AMG_ROWS(i, a.n)
	{
		const double di = d[i], dfi = df[i];
		const bool all = fb[i] != 0;
		const int q1 = f_rp[i + 1];
		double sum = 0;
		int q = f_rp[i];
		bool found = false;
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			const int j = a.ci[e];
			double v = a.va[e];
			bool k;
			if (j == i)
			{
				k = !found;
				if (k)
					v = dfi;
				found = true;
			}
			else
				k = amg_strong(v, di, d[j], theta2);
			if ((k || all) && q < q1)
			{
				f_ci[q] = j;
				f_va[q] = v;
				map[q] = e;
				q++;
				sum = sum + fabs(v);
			}
		}
		worst = fmax(worst, sum / dfi);
	}
	sh[threadIdx.x] = worst;
	__syncthreads();
	for (int s = AMG_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
			sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
		__syncthreads();
	}
	if (threadIdx.x == 0)
		part[blockIdx.x] = sh[0];
}

// 5a for an update, the kept pattern frozen: the entries of row i that the map does not name are lumped in stored order, dF_i and
// A_F's values follow as above (f_va NULL: only dF and the count, the check of level 0), *bad += the rows filtered at create
// (fb[i] == 0) whose dF_i is not finite or not > 0 (zeroed by the caller)
__global__ __launch_bounds__(AMG_TB) void
amg_filter_values_kernel(AmgCsr a, const double * __restrict__ d, const int * __restrict__ f_rp, const int * __restrict__ map,
		const int * __restrict__ fb, double * __restrict__ df, double * __restrict__ f_va, double * __restrict__ part, int * __restrict__ bad)
{
	__shared__ double sh[AMG_TB];
	__shared__ int shb[AMG_TB];
	double worst = 0;
	int wrong = 0;
	AMG_ROWS(i, a.n)
	{
		const double di = d[i];
		const int q1 = f_rp[i + 1];
		double lump = 0.0;
		int q = f_rp[i];
		for (int e = a.rp[i]; e < a.rp[i + 1]; e++)
		{
			if (q < q1 && map[q] == e)
				q++;
			else
				lump = lump + a.va[e];
		}
		const double dfi = fb[i] ? di : di + lump;
		df[i] = dfi;
		wrong += !(isfinite(dfi) && dfi > 0);
		if (f_va)
		{
			double sum = 0;
			bool found = false;
			for (q = f_rp[i]; q < q1; q++)
			{
				const int e = map[q];
				double v = a.va[e];
				if (!found && a.ci[e] == i)
				{
					v = dfi;
					found = true;
				}
				f_va[q] = v;
				sum = sum + fabs(v);
			}
			worst = fmax(worst, sum / dfi);
		}
	}
	sh[threadIdx.x] = worst;
	shb[threadIdx.x] = wrong;
	__syncthreads();
	for (int s = AMG_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
		{
			sh[threadIdx.x] = fmax(sh[threadIdx.x], sh[threadIdx.x + s]);
			shb[threadIdx.x] += shb[threadIdx.x + s];
		}
		__syncthreads();
	}
	if (threadIdx.x == 0)
	{
		part[blockIdx.x] = sh[0];
		if (shb[0] > 0)
			atomicAdd(bad, shb[0]);                           // an integer count: its sum does not depend on the order
	}
}

// 5b: one lane per aggregate over its members' b in ascending row order (the transposition of T's pattern carries them):
// s = +0.0, s = s + b_i * b_i, nrm = sqrt(s)
__global__ __launch_bounds__(AMG_TB) void
amg_agg_norm_kernel(long nc, const int * __restrict__ m_rp, const double * __restrict__ m_b, double * __restrict__ nrm)
{
	AMG_ROWS(g, nc)
	{
		double s = 0.0;
		for (int e = m_rp[g]; e < m_rp[g + 1]; e++)
		{
			const double b = m_b[e];
			s = s + b * b;
		}
		nrm[g] = sqrt(s);
	}
}

// 5b: t_i = b_i / nrm_agg(i), an IEEE division
__global__ __launch_bounds__(AMG_TB) void
amg_tentative_kernel(long n, const double * __restrict__ b, const int * __restrict__ agg, const double * __restrict__ nrm,
		double * __restrict__ t)
{
	AMG_ROWS(i, n)
		t[i] = b[i] / nrm[agg[i]];
}

// 5c: P_ij = (agg(i) == j ? t_i : 0) - (omega_p / dF_i) * (A_F T)_ij over the entries of row i of A_F T
__global__ __launch_bounds__(AMG_TB) void
amg_prolong_t_kernel(long n, const int * __restrict__ at_rp, const int * __restrict__ at_ci, const double * __restrict__ at_va,
		const int * __restrict__ agg, const double * __restrict__ t, const double * __restrict__ df, double omega_p, double * __restrict__ p_va)
{
	AMG_ROWS(i, n)
	{
		const double scale = omega_p / df[i], ti = t[i];
		const int g = agg[i];
		for (int e = at_rp[i]; e < at_rp[i + 1]; e++)
			p_va[e] = (at_ci[e] == g ? ti : 0.0) - scale * at_va[e];
	}
}

// ---- the cycle -----------------------------------------------------------------------------------------------------------------------

template <typename T>
__global__ __launch_bounds__(VB) void
amg_first_kernel(const T * __restrict__ w, const T * __restrict__ b, T * __restrict__ x, long n)
{
	GRID_STRIDE(i, n)
		x[i] = w[i] * b[i];
}

template <typename T>
__global__ __launch_bounds__(VB) void
amg_sweep_kernel(const T * __restrict__ w, const T * __restrict__ b, const T * __restrict__ t, T * __restrict__ x, long n)
{
	GRID_STRIDE(i, n)
		x[i] = x[i] + w[i] * (b[i] - t[i]);
}

template <typename T>
__global__ __launch_bounds__(VB) void
amg_residual_kernel(const T * __restrict__ b, T * __restrict__ t, long n)
{
	GRID_STRIDE(i, n)
		t[i] = b[i] - t[i];
}

// L y = b column by column, then L^t x = y: lane a keeps y_a in a register, the lane of the column posts y_k / L_kk, one barrier,
// and the lanes below (above, on the way back) take their fma. Every lane runs all n trips of both loops.
template <typename T>
__global__ __launch_bounds__(AMG_DENSE_MAX) void
amg_dense_solve_kernel(const double * __restrict__ Lg, const T * __restrict__ b, T * __restrict__ x, int n)
{
	__shared__ double L[AMG_DENSE_MAX * (AMG_DENSE_MAX + 1) / 2];
	__shared__ double piv[AMG_DENSE_MAX];
	const int a = threadIdx.x;
	const int row = a * (a + 1) / 2;
	for (int e = a; e < n * (n + 1) / 2; e += AMG_DENSE_MAX)
		L[e] = Lg[e];
	double y = a < n ? (double) b[a] : 0.0;
	__syncthreads();
	for (int k = 0; k < n; k++)
	{
		if (a == k)
			piv[k] = y / L[row + k];
		__syncthreads();
		if (a > k && a < n)
			y = fma(-L[row + k], piv[k], y);
	}
	y = a < n ? piv[a] : 0.0;
	__syncthreads();
	for (int k = n - 1; k >= 0; k--)
	{
		if (a == k)
			piv[k] = y / L[row + k];
		__syncthreads();
		if (a < k)
			y = fma(-L[k * (k + 1) / 2 + a], piv[k], y);
	}
	if (a < n)
		x[a] = (T) piv[a];
}

// The packed factor of the header's loop, in place in LDS: the lower triangle of the CSR is scattered into the triangle (an absent
// entry is 0), then for column k lane a >= k runs its fma chain over the finished columns p < k, lane k posts its pivot, one barrier,
// lane k keeps sqrt(pivot) and the lanes below divide by it, one barrier. A pivot that is <= 0 or not finite raises *failed (a plain
// store; zeroed by the caller) and the loop goes on: every lane runs all n trips and meets every barrier, the factor is then not used.
__global__ __launch_bounds__(AMG_DENSE_MAX) void
amg_dense_factor_kernel(AmgCsr A, double * __restrict__ Fg, int * __restrict__ failed)
{
	__shared__ double S[AMG_DENSE_MAX * (AMG_DENSE_MAX + 1) / 2];
	__shared__ double piv;
	const int n = (int) A.n;
	const int a = threadIdx.x;
	const int row = a * (a + 1) / 2;
	const int len = n * (n + 1) / 2;
	for (int e = a; e < len; e += AMG_DENSE_MAX)
		S[e] = 0.0;
	__syncthreads();
	if (a < n)
		for (int e = A.rp[a]; e < A.rp[a + 1]; e++)
		{
			const int j = A.ci[e];
			if (j >= 0 && j <= a)
				S[row + j] = A.va[e];
		}
	__syncthreads();
	for (int k = 0; k < n; k++)
	{
		const int rk = k * (k + 1) / 2;
		double s = 0.0;
		if (a >= k && a < n)
		{
			s = S[row + k];
			for (int p = 0; p < k; p++)
				s = fma(-S[row + p], S[rk + p], s);
		}
		if (a == k)
		{
			piv = s;
			if (!(isfinite(s) && s > 0))
				*failed = 1;
		}
		__syncthreads();
		const double root = sqrt(piv);
		if (a == k)
			S[rk + k] = root;
		else if (a > k && a < n)
			S[row + k] = s / root;
		__syncthreads();
	}
	for (int e = a; e < len; e += AMG_DENSE_MAX)
		Fg[e] = S[e];
}

// ---- launchers -----------------------------------------------------------------------------------------------------------------------

#define AMG_LAUNCH(kernel, n, st, ...)                                                          \
	do {                                                                                        \
		if ((n) > 0)                                                                            \
			hipLaunchKernelGGL(kernel, dim3(amg_grid(n)), dim3(AMG_TB), 0, st, __VA_ARGS__);    \
		HIP_TRY(hipGetLastError());                                                             \
		return 0;                                                                               \
	} while (0)

int
launch_amg_diag(const AmgCsr & a, double * d, double * part, hipStream_t st)
{
	AMG_LAUNCH(amg_diag_kernel, a.n, st, a, d, part);
}

int
launch_amg_diag_check(const AmgCsr & a, double * d, double * part, int * bad, hipStream_t st)
{
	AMG_LAUNCH(amg_diag_check_kernel, a.n, st, a, d, part, bad);
}

int
launch_amg_weights(bool f32, long n, const double * d, double omega, void * w, hipStream_t st)
{
	if (f32)
		AMG_LAUNCH(amg_weights_kernel<float>, n, st, n, d, omega, (float *) w);
	AMG_LAUNCH(amg_weights_kernel<double>, n, st, n, d, omega, (double *) w);
}

int
launch_amg_dense_factor(const AmgCsr & a, double * F, int * failed, hipStream_t st)
{
	if (a.n > 0 && a.n <= AMG_DENSE_MAX)
		hipLaunchKernelGGL(amg_dense_factor_kernel, dim3(1), dim3(AMG_DENSE_MAX), 0, st, a, F, failed);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_amg_mis_init(long n, int * state, unsigned long long * key0, hipStream_t st)
{
	AMG_LAUNCH(amg_mis_init_kernel, n, st, n, state, key0);
}

int
launch_amg_mis_sweep(const AmgCsr & a, const double * d, double theta2, const unsigned long long * in, unsigned long long * out, hipStream_t st)
{
	AMG_LAUNCH(amg_mis_sweep_kernel, a.n, st, a, d, theta2, in, out);
}

int
launch_amg_mis_decide(long n, int * state, unsigned long long * key0, const unsigned long long * key2, int * undecided, hipStream_t st)
{
	AMG_LAUNCH(amg_mis_decide_kernel, n, st, n, state, key0, key2, undecided);
}

size_t
amg_scan_bytes(long n)
{
	size_t bytes = 0;
	(void) hipcub::DeviceScan::ExclusiveSum(nullptr, bytes, (const int *) nullptr, (int *) nullptr, (int) n);
	return bytes;
}

int
launch_amg_number_roots(long n, const int * state, int * flag, int * id, void * scan_tmp, size_t scan_bytes, hipStream_t st)
{
	if (n <= 0)
		return 0;
	hipLaunchKernelGGL(amg_root_flag_kernel, dim3(amg_grid(n)), dim3(AMG_TB), 0, st, n, state, flag);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, (const int *) flag, id, (int) n, st));
	return 0;
}

int
launch_amg_agg_pass1(const AmgCsr & a, const double * d, double theta2, const int * state, const int * id, int * agg1, hipStream_t st)
{
	AMG_LAUNCH(amg_agg_pass1_kernel, a.n, st, a, d, theta2, state, id, agg1);
}

int
launch_amg_agg_pass2(const AmgCsr & a, const double * d, double theta2, const int * agg1, int * agg2, hipStream_t st)
{
	AMG_LAUNCH(amg_agg_pass2_kernel, a.n, st, a, d, theta2, agg1, agg2);
}

int
launch_amg_prolong(long n, const int * at_rp, const int * at_ci, const double * at_va, const int * agg, const double * d, double omega,
		double * p_va, hipStream_t st)
{
	AMG_LAUNCH(amg_prolong_kernel, n, st, n, at_rp, at_ci, at_va, agg, d, omega, p_va);
}

int
launch_amg_filter_count(const AmgCsr & a, const double * d, double theta2, int * kept, int * fb, double * df, hipStream_t st)
{
	AMG_LAUNCH(amg_filter_count_kernel, a.n, st, a, d, theta2, kept, fb, df);
}

int
launch_amg_offsets(long count, const int * in, int * out, void * scan_tmp, size_t scan_bytes, hipStream_t st)
{
	if (count <= 0)
		return 0;
	HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, in, out, (int) count, st));
	return 0;
}

int
launch_amg_filter_fill(const AmgCsr & a, const double * d, double theta2, const int * f_rp, const int * fb, const double * df, int * f_ci,
		double * f_va, int * map, double * part, hipStream_t st)
{
	AMG_LAUNCH(amg_filter_fill_kernel, a.n, st, a, d, theta2, f_rp, fb, df, f_ci, f_va, map, part);
}

int
launch_amg_filter_values(const AmgCsr & a, const double * d, const int * f_rp, const int * map, const int * fb, double * df, double * f_va,
		double * part, int * bad, hipStream_t st)
{
	AMG_LAUNCH(amg_filter_values_kernel, a.n, st, a, d, f_rp, map, fb, df, f_va, part, bad);
}

int
launch_amg_agg_norm(long nc, const int * m_rp, const double * m_b, double * nrm, hipStream_t st)
{
	AMG_LAUNCH(amg_agg_norm_kernel, nc, st, nc, m_rp, m_b, nrm);
}

int
launch_amg_tentative(long n, const double * b, const int * agg, const double * nrm, double * t, hipStream_t st)
{
	AMG_LAUNCH(amg_tentative_kernel, n, st, n, b, agg, nrm, t);
}

int
launch_amg_prolong_t(long n, const int * at_rp, const int * at_ci, const double * at_va, const int * agg, const double * t, const double * df,
		double omega_p, double * p_va, hipStream_t st)
{
	AMG_LAUNCH(amg_prolong_t_kernel, n, st, n, at_rp, at_ci, at_va, agg, t, df, omega_p, p_va);
}

int
launch_amg_first(bool f32, const void * w, const void * b, void * x, long n, hipStream_t st)
{
	if (n > 0)
	{
		if (f32)
			hipLaunchKernelGGL((amg_first_kernel<float>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const float *) w, (const float *) b,
					(float *) x, n);
		else
			hipLaunchKernelGGL((amg_first_kernel<double>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const double *) w, (const double *) b,
					(double *) x, n);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_amg_sweep(bool f32, const void * w, const void * b, const void * t, void * x, long n, hipStream_t st)
{
	if (n > 0)
	{
		if (f32)
			hipLaunchKernelGGL((amg_sweep_kernel<float>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const float *) w, (const float *) b,
					(const float *) t, (float *) x, n);
		else
			hipLaunchKernelGGL((amg_sweep_kernel<double>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const double *) w, (const double *) b,
					(const double *) t, (double *) x, n);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_amg_residual(bool f32, const void * b, void * t, long n, hipStream_t st)
{
	if (n > 0)
	{
		if (f32)
			hipLaunchKernelGGL((amg_residual_kernel<float>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const float *) b, (float *) t, n);
		else
			hipLaunchKernelGGL((amg_residual_kernel<double>), dim3(solver_blocks(n)), dim3(VB), 0, st, (const double *) b, (double *) t, n);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_amg_dense_solve(bool f32, const double * L, const void * b, void * x, int n, hipStream_t st)
{
	if (n > 0)
	{
		if (f32)
			hipLaunchKernelGGL((amg_dense_solve_kernel<float>), dim3(1), dim3(AMG_DENSE_MAX), 0, st, L, (const float *) b, (float *) x, n);
		else
			hipLaunchKernelGGL((amg_dense_solve_kernel<double>), dim3(1), dim3(AMG_DENSE_MAX), 0, st, L, (const double *) b, (double *) x, n);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

// ---- the cycle for k columns ---------------------------------------------------------------------------------------------------------
// The three vector kernels and the dense solve for a chunk of KC in {8, 4, 2, 1} columns c0.. of row-major blocks (row i at ptr + i * ld).
// A thread owns row i of its chunk: it reads w[i] once and KC contiguous values per block, as one vector load where the block's base,
// its ld and c0 are multiples of KC. Per element the expressions are those of the single kernels above, so column j holds their bits.

template <typename T, int KC>
__device__ __forceinline__ bool
amg_row_vec(const T * p, long ld, int c0)
{
	return ld % KC == 0 && c0 % KC == 0 && (size_t) p % (KC * sizeof(T)) == 0;
}

template <typename T, int KC>
__global__ __launch_bounds__(VB) void
amg_first_multi_kernel(const T * __restrict__ w, const T * __restrict__ b, long ldb, T * __restrict__ x, long ldx, int c0, long n)
{
	const bool vb = amg_row_vec<T, KC>(b, ldb, c0), vx = amg_row_vec<T, KC>(x, ldx, c0);
	GRID_STRIDE(i, n)
	{
		const T wi = w[i];
		T bv[KC], xv[KC];
		load_row<T, KC>(bv, b + i * ldb + c0, vb);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			xv[c] = wi * bv[c];
		store_row<T, KC>(x + i * ldx + c0, xv, vx);
	}
}

// b and x may be the caller's blocks with their own ld; t is the hierarchy's
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
amg_sweep_multi_kernel(const T * __restrict__ w, const T * __restrict__ b, long ldb, const T * __restrict__ t, long ldt, T * __restrict__ x,
		long ldx, int c0, long n)
{
	const bool vb = amg_row_vec<T, KC>(b, ldb, c0), vt = amg_row_vec<T, KC>(t, ldt, c0), vx = amg_row_vec<T, KC>(x, ldx, c0);
	GRID_STRIDE(i, n)
	{
		const T wi = w[i];
		T bv[KC], tv[KC], xv[KC];
		load_row<T, KC>(bv, b + i * ldb + c0, vb);
		load_row<T, KC>(tv, t + i * ldt + c0, vt);
		load_row<T, KC>(xv, x + i * ldx + c0, vx);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			xv[c] = xv[c] + wi * (bv[c] - tv[c]);
		store_row<T, KC>(x + i * ldx + c0, xv, vx);
	}
}

template <typename T, int KC>
__global__ __launch_bounds__(VB) void
amg_residual_multi_kernel(const T * __restrict__ b, long ldb, T * __restrict__ t, long ldt, int c0, long n)
{
	const bool vb = amg_row_vec<T, KC>(b, ldb, c0), vt = amg_row_vec<T, KC>(t, ldt, c0);
	GRID_STRIDE(i, n)
	{
		T bv[KC], tv[KC];
		load_row<T, KC>(bv, b + i * ldb + c0, vb);
		load_row<T, KC>(tv, t + i * ldt + c0, vt);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			tv[c] = bv[c] - tv[c];
		store_row<T, KC>(t + i * ldt + c0, tv, vt);
	}
}

// amg_dense_solve_kernel for the KC columns c0..: the packed factor goes into LDS once, lane a keeps y_a of every column in registers,
// the lane of column k of L posts KC quotients, and there is still one barrier per column of L in each direction. Per column of the
// block the division and the fma chain are the single kernel's.
template <typename T, int KC>
__global__ __launch_bounds__(AMG_DENSE_MAX) void
amg_dense_solve_multi_kernel(const double * __restrict__ Lg, const T * __restrict__ b, long ldb, T * __restrict__ x, long ldx, int c0, int n)
{
	__shared__ double L[AMG_DENSE_MAX * (AMG_DENSE_MAX + 1) / 2];
	__shared__ double piv[AMG_DENSE_MAX][KC];
	const int a = threadIdx.x;
	const int row = a * (a + 1) / 2;
	for (int e = a; e < n * (n + 1) / 2; e += AMG_DENSE_MAX)
		L[e] = Lg[e];
	double y[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
		y[c] = a < n ? (double) b[(long) a * ldb + c0 + c] : 0.0;
	__syncthreads();
	for (int k = 0; k < n; k++)
	{
		if (a == k)
		{
			const double d = L[row + k];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				piv[k][c] = y[c] / d;
		}
		__syncthreads();
		if (a > k && a < n)
		{
			const double l = L[row + k];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				y[c] = fma(-l, piv[k][c], y[c]);
		}
	}
	#pragma unroll
	for (int c = 0; c < KC; c++)
		y[c] = a < n ? piv[a][c] : 0.0;
	__syncthreads();
	for (int k = n - 1; k >= 0; k--)
	{
		if (a == k)
		{
			const double d = L[row + k];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				piv[k][c] = y[c] / d;
		}
		__syncthreads();
		if (a < k)
		{
			const double l = L[k * (k + 1) / 2 + a];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				y[c] = fma(-l, piv[k][c], y[c]);
		}
	}
	if (a < n)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
			x[(long) a * ldx + c0 + c] = (T) piv[a][c];
	}
}

// one launch per chunk of k, in column order
#define AMG_MULTI(kernel, grid, block, ...)                                                                                              \
	if (n > 0)                                                                                                                           \
		for_chunks(column_chunks(k), [&](int c0, auto kc) {                                                                              \
			constexpr int KC = decltype(kc)::value;                                                                                      \
			if (f32)                                                                                                                     \
			{                                                                                                                            \
				typedef float T;                                                                                                         \
				hipLaunchKernelGGL((kernel<T, KC>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);                                         \
			}                                                                                                                            \
			else                                                                                                                         \
			{                                                                                                                            \
				typedef double T;                                                                                                        \
				hipLaunchKernelGGL((kernel<T, KC>), dim3(grid), dim3(block), 0, st, __VA_ARGS__);                                         \
			}                                                                                                                            \
			return 0;                                                                                                                    \
		});                                                                                                                              \
	HIP_TRY(hipGetLastError());                                                                                                          \
	return 0

int
launch_amg_first_multi(bool f32, int k, const void * w, const void * b, long ldb, void * x, long ldx, long n, hipStream_t st)
{
	AMG_MULTI(amg_first_multi_kernel, solver_blocks(n), VB, (const T *) w, (const T *) b, ldb, (T *) x, ldx, c0, n);
}

int
launch_amg_sweep_multi(bool f32, int k, const void * w, const void * b, long ldb, const void * t, long ldt, void * x, long ldx, long n,
		hipStream_t st)
{
	AMG_MULTI(amg_sweep_multi_kernel, solver_blocks(n), VB, (const T *) w, (const T *) b, ldb, (const T *) t, ldt, (T *) x, ldx, c0, n);
}

int
launch_amg_residual_multi(bool f32, int k, const void * b, long ldb, void * t, long ldt, long n, hipStream_t st)
{
	AMG_MULTI(amg_residual_multi_kernel, solver_blocks(n), VB, (const T *) b, ldb, (T *) t, ldt, c0, n);
}

int
launch_amg_dense_solve_multi(bool f32, int k, const double * L, const void * b, long ldb, void * x, long ldx, int n, hipStream_t st)
{
	AMG_MULTI(amg_dense_solve_multi_kernel, 1, AMG_DENSE_MAX, L, (const T *) b, ldb, (T *) x, ldx, c0, n);
}

}  // namespace spmv

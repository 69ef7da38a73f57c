// What the single- and multi-RHS Krylov solvers (solvers.hip, solvers_multi.hip) share: the launch shape of the vector
// kernels, the device state, the deterministic two-stage dot products, the host progress word, the explicit-residual
// decision, the device buffer owner and the Jacobi diagonal.
#pragma once

#include <vector>

#include "common.hpp"

namespace spmv {

constexpr int VB = 256;           // threads per block of the vector kernels
constexpr int MAX_PART = 1024;    // partial sums per quantity
constexpr int RESTART_K = 100;    // bench_cg.cpp:178
constexpr int POLL = 32;          // the host looks at the progress word every POLL iterations

struct SolverState {
	double err, err_explicit, err_best, eps, eps_counter;
	double zr;                    // CG: (z, r)          BiCGSTAB: s_pk_p = (r0_, rk)
	long k;                       // completed loop bodies = num_loops_out
	long restarts;
	int done;                     // the `err < eps` break was reached
	int pad;
};

enum { P_A = 0, P_B, P_C, P_D, P_E, P_F, NUM_SLOTS };

__device__ __forceinline__ double
block_sum(double v)
{
	__shared__ double sh[VB / WAVE];
	__shared__ double total;
	for (int o = WAVE / 2; o > 0; o >>= 1)
		v += __shfl_down(v, o, WAVE);
	__syncthreads();                       // protects sh/total against the previous call
	if (threadIdx.x % WAVE == 0)
		sh[threadIdx.x / WAVE] = v;
	__syncthreads();
	if (threadIdx.x == 0)
	{
		double s = 0;
		for (int w = 0; w < VB / WAVE; w++)
			s += sh[w];
		total = s;
	}
	__syncthreads();
	return total;
}

// Every block reduces the nb partials of one slot in the same order: all blocks get the same bits.
__device__ __forceinline__ double
sum_partials(const double * __restrict__ part, int slot, int nb)
{
	const double * p = part + (long) slot * MAX_PART;
	double v = 0;
	for (int i = threadIdx.x; i < nb; i += VB)
		v += p[i];
	return block_sum(v);
}

__device__ __forceinline__ void
store_partial(double * __restrict__ part, int slot, double v)
{
	v = block_sum(v);
	if (threadIdx.x == 0)
		part[(long) slot * MAX_PART + blockIdx.x] = v;
}

// (iterations the device has finished, loop count at the break or -1) for the host, in host-mapped pinned memory
__device__ __forceinline__ void
post_progress(volatile long * host_progress, long finished, long broke_at)
{
	host_progress[1] = broke_at;
	__threadfence_system();
	host_progress[0] = finished;
	__threadfence_system();
}

#define GRID_STRIDE(i, m) for (long i = (long) blockIdx.x * VB + threadIdx.x; i < (m); i += (long) gridDim.x * VB)

// Explicit-residual bookkeeping (bench_cg.cpp:186-236, bench_bicg.cpp:277-302): partial A holds |b - A x|^2.
// promote: x_best = x when err_explicit < err_best. restart (CG, allow_restart): r = r_explicit, p = z = r/K and
// partial C = z.r. Decisions are recomputed identically by explicit_fin_kernel, which then updates the state in place.
__device__ __forceinline__ void
explicit_decide(const SolverState & st, double err_explicit, int allow_restart, bool & promote, bool & restart)
{
	promote = err_explicit < st.err_best;
	const double err_best = promote ? err_explicit : st.err_best;
	restart = allow_restart && (err_best > st.eps_counter) && (err_explicit / st.err > 1e3);
}

struct DeviceBuffers {
	std::vector<void *> ptrs;
	void * pinned = nullptr;
	~DeviceBuffers()
	{
		for (void * p : ptrs)
			(void) hipFree(p);
		if (pinned)
			(void) hipHostFree(pinned);
	}
	template <typename P>
	int alloc(P ** out, size_t bytes)
	{
		void * p = nullptr;
		HIP_TRY(hipMalloc(&p, bytes ? bytes : 8));
		ptrs.push_back(p);
		*out = (P *) p;
		return 0;
	}
};

// Jacobi preconditioner: the first stored entry of row i whose column is i (bench_cg.cpp:114-134).
template <typename T>
static long
jacobi_diagonal(const int32_t * row_ptr, const int32_t * col, const double * val, long m, long row_offset, T * K)
{
	long bad = -1;
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(static)
	for (long i = 0; i < m; i++)
	{
		T k = 0;
		for (long j = row_ptr[i]; j < row_ptr[i + 1]; j++)
			if (col[j] == i + row_offset)
			{
				k = (T) val[j];
				break;
			}
		K[i] = k;
		if (k == 0)
		{
			#pragma omp critical
			if (bad < 0 || i < bad)
				bad = i;
		}
	}
	return bad;
}

#define ABI_TRY(expr)       \
	do {                    \
		if ((expr))         \
			return 1;       \
	} while (0)

}  // namespace spmv

// What the Krylov solvers (solvers.hip, solver_cgls.hip, solver_minres.hip, solver_gmres.hip) share. Device side: the launch
// shape of the vector kernels, the device state, the deterministic two-stage dot products, the post to the host progress word, the
// explicit-residual decision. Host side: the device buffer owner, the Jacobi diagonal, and the run-ahead driver of every solve loop
// (solver_blocks, ProgressGate, info_size_ok / put_info, host_sum).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstring>
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

// (iterations the device has finished, loop count at the break or -1) for the host (ProgressGate below), in host-mapped pinned memory
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
	~DeviceBuffers()
	{
		for (void * p : ptrs)
			(void) hipFree(p);
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

// ------------------------------------------------------------------------------------------------ the host's half of a solve

// Blocks of every vector kernel of a solve over len elements = partials per slot.
inline int
solver_blocks(long len)
{
	return (int) std::min<long>(MAX_PART, std::max<long>(1, (len + 4 * VB - 1) / (4 * VB)));
}

// The progress word that post_progress() writes, and the gate that keeps the enqueueing host at most 2*POLL iterations ahead of
// the device and stops it after a break. Each solve loop starts with
//   bool stop; ABI_TRY(gate.wait(it, "<solver>", stream, &stop)); if (stop) break;
struct ProgressGate {
	volatile long * host = nullptr;   // [0] iterations finished, [1] loop count at the break or -1
	long * dev = nullptr;             // the same two words as the kernels see them
	double spin_seconds = 0;          // spent waiting for the device, for SPMV_MI355X_SOLVER_DEBUG

	ProgressGate() = default;
	ProgressGate(const ProgressGate &) = delete;
	ProgressGate & operator=(const ProgressGate &) = delete;
	~ProgressGate()
	{
		if (host)
			(void) hipHostFree((void *) host);
	}

	int init()
	{
		void * p = nullptr;
		HIP_TRY(hipHostMalloc(&p, 2 * sizeof(long), hipHostMallocMapped | hipHostMallocCoherent));
		host = (volatile long *) p;
		host[0] = 0;
		host[1] = -1;
		HIP_TRY(hipHostGetDevicePointer((void **) &dev, p, 0));
		return 0;
	}

	// Acts every POLL iterations from 2*POLL on. The wait is plain reads of the mapped word with no HIP call in the loop:
	// hipEventSynchronize there was measured to stall the queue for up to 100 ms at a time. rc 1 on a HIP error or when the
	// device posts nothing for 120 s.
	int wait(long it, const char * what, hipStream_t stream, bool * stop)
	{
		*stop = false;
		if (it % POLL != 0 || it < 2 * POLL)
			return 0;
		const auto t_wait = std::chrono::steady_clock::now();
		long spins = 0;
		while (host[0] < it - POLL)
		{
			if ((++spins & 0xfff) == 0)
			{
				HIP_TRY(hipGetLastError());
				if (std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count() > 120.0)
				{
					set_error("%s: the device made no progress for 120 s at iteration %ld", what, it);
					(void) hipStreamSynchronize(stream);
					return 1;
				}
			}
			__builtin_ia32_pause();
		}
		spin_seconds += std::chrono::duration<double>(std::chrono::steady_clock::now() - t_wait).count();
		// The stop rule that every rank of a distributed solve evaluates identically, so that all stop enqueueing at the same
		// iteration: only what the device had posted by iteration it - POLL counts (the wait above guarantees it is visible),
		// never "whatever is visible now".
		const long broke_at = host[1];
		*stop = broke_at >= 0 && broke_at <= it - POLL;
		return 0;
	}
};

// The first check of a caller's info struct: its struct_size must at least cover the field itself.
template <typename Info>
inline bool
info_size_ok(const char * what, const Info * info)
{
	if (info && info->struct_size < 8)
	{
		set_error("%s: info->struct_size not set", what);
		return false;
	}
	return true;
}

// Writes the first min(want, sizeof(out)) bytes of out to dst, struct_size set to that count (want = the caller's struct_size).
template <typename Info>
inline void
put_info(void * dst, unsigned want, Info & out)
{
	out.struct_size = (unsigned) std::min<size_t>(want, sizeof(out));
	memcpy(dst, &out, out.struct_size);
}

// The sum of nb downloaded partials from part_host[slot_offset] on, left to right.
inline double
host_sum(const double * part_host, size_t slot_offset, int nb)
{
	double v = 0;
	for (int i = 0; i < nb; i++)
		v += part_host[slot_offset + i];
	return v;
}

}  // namespace spmv

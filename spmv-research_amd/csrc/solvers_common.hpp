// What the Krylov solvers (solvers.hip, solver_cgls.hip, solver_minres.hip, solver_gmres.hip) share. Device side: the launch
// shape of the vector kernels, the device state, the deterministic two-stage dot products, the post to the host progress word, the
// explicit-residual decision, the k-column forms of the reductions and the row loads. Host side: the device buffer owner, the Jacobi
// diagonal, the split of k columns into chunks, and the run-ahead driver of every solve loop (solver_blocks, ProgressGate,
// info_size_ok / put_info, host_sum).
#pragma once

#include <algorithm>
#include <chrono>
#include <cstring>
#include <type_traits>
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

// ---- k columns at once (solvers.hip, solver_pcg_tri.hip, the k-column cycle of kernels_amg.hip): a vector kernel serves a chunk
// of KC in {8, 4, 2, 1} columns of a row-major block, and every per-column dot product goes through the additions of block_sum /
// sum_partials / store_partial in their order, so a column returns the bits of the single-vector kernels whatever chunk it sits in.

constexpr int MAX_KC = 8;          // columns per chunk

// block_sum() for N values at once: each value goes through the same shuffle tree and the same in-order sum of the
// VB / WAVE wave partials, behind one set of barriers.
template <int N>
__device__ __forceinline__ void
block_sum_n(double * v)
{
	__shared__ double sh[N][VB / WAVE];
	__shared__ double total[N];
	#pragma unroll
	for (int c = 0; c < N; c++)
		for (int o = WAVE / 2; o > 0; o >>= 1)
			v[c] += __shfl_down(v[c], o, WAVE);
	__syncthreads();                       // protects sh/total against the previous call
	if (threadIdx.x % WAVE == 0)
	{
		#pragma unroll
		for (int c = 0; c < N; c++)
			sh[c][threadIdx.x / WAVE] = v[c];
	}
	__syncthreads();
	if (threadIdx.x < N)
	{
		double s = 0;
		for (int w = 0; w < VB / WAVE; w++)
			s += sh[threadIdx.x][w];
		total[threadIdx.x] = s;
	}
	__syncthreads();
	#pragma unroll
	for (int c = 0; c < N; c++)
		v[c] = total[c];
}

__host__ __device__ __forceinline__ long
part_at(int col, int slot)
{
	return ((long) col * NUM_SLOTS + slot) * MAX_PART;
}

// sum_partials() of S slots for the KC columns c0.. : out[s * KC + c]
template <int KC, int S>
__device__ __forceinline__ void
sum_partials_n(const double * __restrict__ part, int c0, const int (&slot)[S], int nb, double * out)
{
	#pragma unroll
	for (int s = 0; s < S; s++)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const double * p = part + part_at(c0 + c, slot[s]);
			double v = 0;
			for (int i = threadIdx.x; i < nb; i += VB)
				v += p[i];
			out[s * KC + c] = v;
		}
	}
	block_sum_n<S * KC>(out);
}

// store_partial() of S slots for the KC columns c0.. from v[s * KC + c]; only the columns in `keep` are written
template <int KC, int S>
__device__ __forceinline__ void
store_partials_n(double * __restrict__ part, int c0, const int (&slot)[S], double * v, unsigned keep)
{
	block_sum_n<S * KC>(v);
	if (threadIdx.x == 0)
	{
		#pragma unroll
		for (int s = 0; s < S; s++)
		{
			#pragma unroll
			for (int c = 0; c < KC; c++)
				if (keep >> c & 1)
					part[part_at(c0 + c, slot[s]) + blockIdx.x] = v[s * KC + c];
		}
	}
}

// KC contiguous values of one row; `vec` (uniform) when the row start is KC-aligned
template <typename T, int KC>
__device__ __forceinline__ void
load_row(T (&o)[KC], const T * p, bool vec)
{
	if constexpr (KC > 1)
	{
		if (vec)
		{
			typedef T V __attribute__((ext_vector_type(KC)));
			const V t = *(const V *) p;
			#pragma unroll
			for (int c = 0; c < KC; c++)
				o[c] = t[c];
			return;
		}
	}
	#pragma unroll
	for (int c = 0; c < KC; c++)
		o[c] = p[c];
}

template <typename T, int KC>
__device__ __forceinline__ void
store_row(T * p, const T (&o)[KC], bool vec)
{
	if constexpr (KC > 1)
	{
		if (vec)
		{
			typedef T V __attribute__((ext_vector_type(KC)));
			V t;
			#pragma unroll
			for (int c = 0; c < KC; c++)
				t[c] = o[c];
			*(V *) p = t;
			return;
		}
	}
	#pragma unroll
	for (int c = 0; c < KC; c++)
		p[c] = o[c];
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

struct Chunk {
	int c0, kc;
};

// k = 8s, then the binary remainder (the SpMM's column passes)
inline std::vector<Chunk>
column_chunks(int k)
{
	std::vector<Chunk> out;
	int c0 = 0;
	for (; k - c0 >= MAX_KC; c0 += MAX_KC)
		out.push_back({c0, MAX_KC});
	for (int w = MAX_KC / 2; w >= 1; w /= 2)
		if (k - c0 >= w)
		{
			out.push_back({c0, w});
			c0 += w;
		}
	return out;
}

// f(c0, std::integral_constant<int, KC>) for every chunk, in column order; stops at the first f that returns nonzero
template <typename F>
inline int
for_chunks(const std::vector<Chunk> & chunks, F && f)
{
	for (const Chunk & ch : chunks)
	{
		int rc;
		switch (ch.kc)
		{
		case 8: rc = f(ch.c0, std::integral_constant<int, 8>()); break;
		case 4: rc = f(ch.c0, std::integral_constant<int, 4>()); break;
		case 2: rc = f(ch.c0, std::integral_constant<int, 2>()); break;
		default: rc = f(ch.c0, std::integral_constant<int, 1>()); break;
		}
		if (rc)
			return rc;
	}
	return 0;
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

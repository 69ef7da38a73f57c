// Device-resident Krylov callers of the SpMV path: Jacobi-preconditioned CG and BiCGSTAB.
//
// What they replace in the reference (benchmark_code/BENCH/src):
//   spmv_mi355x_pcg        preconditioned_cg()        bench_cg.cpp:93-322
//   spmv_mi355x_pbicgstab  preconditioned_bicgstab()  bench_bicg.cpp:149-459
// The reference keeps every vector on the host and calls MF->spmv(host x, host y) once or twice per iteration, so a GPU
// backend pays an upload of x and a download of y around every launch. Here all vectors live in HBM and
// the loop never waits for the host:
//   * the scalars (alpha, beta, omega, the error norms, the loop counter) live in a small device struct; the kernels of
//     iteration k read state[k&1] and block 0 of the last kernel writes state[(k+1)&1] (no read/write race, no sync);
//   * dots are two-stage: every block writes one partial per quantity, and every block of the CONSUMING kernel re-reduces
//     the <= 1024 partials in a fixed order — deterministic, and no separate "finish the reduction" launch;
//   * the `err < eps` break (bench_cg.cpp:238) becomes a device flag that predicates every later vector kernel off, so
//     x, x_best, the counter and the history are frozen exactly where the reference breaks; the last kernel of every
//     iteration also posts (iterations finished, loop count at the break) into the host-mapped progress word, which lets
//     the host stop enqueueing after a break and stay at most 2*POLL iterations ahead (ProgressGate, solvers_common.hpp);
//   * the vector updates around the SpMV are fused: CG = SpMV + 3 passes (p.Ap | x,r update + z.r, r.r | p update),
//     BiCGSTAB = 2 SpMV + 5 passes. z = r/K and h = x + s_a*y are never materialised.
// Same iteration semantics as the reference: Jacobi K = first stored diagonal entry (error on a zero), x0 = 0,
// eps = 1e-15*|b|, explicit residual every 100 iterations with x_best tracking and (CG only) the restart rule.
// Dot products accumulate in double for both precisions (the reference accumulates in ValueType with an OpenMP
// thread-count-dependent order, so its last bits are not reproducible either).
//
// One set of kernels and one host solve<T> serve all six entry points: k independent systems A x_j = b_j are solved
// together, and the single-RHS and row-partitioned (_dist) entries are its k = 1 case. Column j of spmv_mi355x_pcg_multi /
// spmv_mi355x_pbicgstab_multi returns exactly what spmv_mi355x_pcg / _pbicgstab return for b_j on the same handle. The
// k recurrences stay independent (this is not block CG with a shared subspace); what they share is the matrix pass, the
// launches and the Jacobi diagonal:
//   * every solver vector is a row-major m x k block (ld = k), K is one vector of m; the _multi entries' matrix product is
//     one spmv_mi355x_spmm_device_async over the k columns, bit-identical per column to the SpMV of the single entries;
//   * each vector kernel serves a chunk of KC in {8, 4, 2, 1} columns (k = 8s, then the binary remainder, as the SpMM
//     does); a thread owns row i of its chunk, so it reads KC contiguous values per vector (vector loads when ld and the
//     chunk start are multiples of KC);
//   * bit-identity: every per-column dot product goes through the same additions in the same order whatever chunk the
//     column sits in (same nb and grid-stride rows per (block, thread), same wave shuffle tree, same in-order sum of the
//     4 wave partials, same order over the partials), and every element update is the same T expression, so FMA
//     contraction matches; the KC columns only share the LDS barriers of one block reduction;
//   * state is SolverState[2][k], partials are [k][NUM_SLOTS][MAX_PART]; each column has its own `done` flag, which
//     freezes that column only (its values are stored back unchanged; the SpMM keeps computing it);
//   * block 0 of the last chunk of an iteration's last kernel posts (iterations finished, loop count at which the last
//     still-running column broke, or -1) to the progress word, so the one stop rule fires once every column has broken.

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <type_traits>
#include <vector>

#include "common.hpp"
#include "solvers_common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

// the columns of the chunk that have not reached the `err < eps` break
template <int KC>
__device__ __forceinline__ unsigned
live_mask(const SolverState * __restrict__ st_p, int c0)
{
	unsigned live = 0;
	#pragma unroll
	for (int c = 0; c < KC; c++)
		if (!st_p[c0 + c].done)
			live |= 1u << c;
	return live;
}

// ------------------------------------------------------------------------------------------------ shared kernels
// Every vector kernel below serves the KC columns c0.. of the m x k blocks (row stride ld), each column on its own.

// r = b - Ax ; partials: A = r.r, B = b.b     (bench_cg.cpp:146-150,163-166)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
residual_kernel(const T * __restrict__ b, const T * __restrict__ Ax, T * __restrict__ r, long m, long ld, int c0,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double acc[2 * KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T bv[KC], av[KC], rv[KC];
		load_row(bv, b + o, vec);
		load_row(av, Ax + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T bi = bv[c];
			const T ri = bi + (T) -1 * av[c];
			rv[c] = ri;
			acc[c] += (double) ri * (double) ri;
			acc[KC + c] += (double) bi * (double) bi;
		}
		store_row(r + o, rv, vec);
	}
	store_partials_n<KC, 2>(part, c0, {P_A, P_B}, acc, ~0u);
}

// the explicit-residual step of the chunk's columns (explicit_decide, solvers_common.hpp): x_best = x on a promotion;
// r = r_explicit, p = z = r/K and partial C = z.r on a restart
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
explicit_kernel(const SolverState * __restrict__ st_p, const T * __restrict__ x, T * __restrict__ x_best,
		const T * __restrict__ r_explicit, T * __restrict__ r, T * __restrict__ p, const T * __restrict__ K, long m, long ld,
		int c0, int nb, int allow_restart, int ignore_done, double * __restrict__ part)
{
	const unsigned act = ignore_done ? (1u << KC) - 1 : live_mask<KC>(st_p, c0);
	if (!act)
		return;
	double ee[KC];
	sum_partials_n<KC, 1>(part, c0, {P_A}, nb, ee);
	unsigned promote = 0, restart = 0;
	#pragma unroll
	for (int c = 0; c < KC; c++)
	{
		bool pr, rs;
		explicit_decide(st_p[c0 + c], sqrt(ee[c]), allow_restart, pr, rs);
		if (act >> c & 1)
		{
			promote |= (unsigned) pr << c;
			restart |= (unsigned) rs << c;
		}
	}
	double zr[KC] = {};
	if (promote | restart)
	{
		GRID_STRIDE(i, m)
		{
			const long o = i * ld + c0;
			#pragma unroll
			for (int c = 0; c < KC; c++)
			{
				if (promote >> c & 1)
					x_best[o + c] = x[o + c];
				if (restart >> c & 1)
				{
					const T ri = r_explicit[o + c];
					const T zi = ri / K[i];
					r[o + c] = ri;
					p[o + c] = zi;
					zr[c] += (double) zi * (double) ri;
				}
			}
		}
	}
	if (restart)
		store_partials_n<KC, 1>(part, c0, {P_C}, zr, restart);
}

// the same decisions again, then the state of column blockIdx.x updated in place; one block per column
__global__ __launch_bounds__(VB) void
explicit_fin_kernel(SolverState * __restrict__ st_base, int nb, int allow_restart, int ignore_done, const double * __restrict__ part_base)
{
	SolverState * st_p = st_base + blockIdx.x;
	const double * part = part_base + part_at(blockIdx.x, 0);
	SolverState st = *st_p;
	if (st.done && !ignore_done)
		return;
	const double err_explicit = sqrt(sum_partials(part, P_A, nb));
	bool promote, restart;
	explicit_decide(st, err_explicit, allow_restart, promote, restart);
	double zr = 0;
	if (restart)
		zr = sum_partials(part, P_C, nb);
	if (threadIdx.x == 0)
	{
		st.err_explicit = err_explicit;
		if (promote)
			st.err_best = err_explicit;
		if (restart)
		{
			st.zr = zr;
			st.restarts++;
		}
		*st_p = st;
	}
}

// eps / eps_counter / first error (bench_cg.cpp:159-182); one block per column. mode 0 = CG (zr = z.r from partial C),
// mode 1 = BiCGSTAB (zr = s_pk_p = (r0_, rk) = r.r since r0_ = rk, bench_bicg.cpp:232-241).
__global__ __launch_bounds__(VB) void
init_state_kernel(SolverState * __restrict__ st_base, int k, int nb, int mode, const double * __restrict__ part_base)
{
	const double * part = part_base + part_at(blockIdx.x, 0);
	const double rr = sum_partials(part, P_A, nb);
	const double bb = sum_partials(part, P_B, nb);
	const double zr = mode == 0 ? sum_partials(part, P_C, nb) : rr;
	if (threadIdx.x == 0)
	{
		SolverState st;
		const double b_norm = sqrt(bb);
		st.err = sqrt(rr);
		st.eps = 1.0e-15 * b_norm;
		st.eps_counter = 1.0e-7 * b_norm;
		st.err_explicit = st.err;
		st.err_best = st.err;
		st.zr = zr;
		st.k = 0;
		st.restarts = 0;
		st.done = mode == 0 && st.err < st.eps;      // the first `if (err < eps) break` (k = 0); BiCGSTAB never breaks
		st.pad = 0;
		st_base[blockIdx.x] = st;
		st_base[k + blockIdx.x] = st;
	}
}

// history rows of the chunk's columns at iteration it (block 0, thread 0)
template <int KC>
__device__ __forceinline__ void
record_history(const SolverState * __restrict__ st_p, int c0, unsigned cols, double * __restrict__ history, long hist_ld, long it)
{
	if (history && blockIdx.x == 0 && threadIdx.x == 0)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
			if (cols >> c & 1)
			{
				const SolverState & st = st_p[c0 + c];
				double * h = history + (c0 + c) * hist_ld + 3 * it;
				h[0] = st.err;
				h[1] = st.err_explicit;
				h[2] = st.err_best;
			}
	}
}

// (iterations finished, loop count at which the last still-running column broke, or -1) from the next states of all
// k columns: the earlier chunks wrote theirs in earlier launches, this thread wrote its own chunk's
__device__ __forceinline__ void
post_columns_progress(const SolverState * st_next, int k, long it, volatile long * host_progress)
{
	long broke_at = 0;
	for (int c = 0; c < k; c++)
	{
		if (!st_next[c].done)
		{
			broke_at = -1;
			break;
		}
		broke_at = st_next[c].k > broke_at ? st_next[c].k : broke_at;
	}
	post_progress(host_progress, it + 1, broke_at);
}

// ------------------------------------------------------------------------------------------------ CG

// z0 = r0/K, p0 = z0 (bench_cg.cpp:153-157); partial C = z.r
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
cg_init_kernel(const T * __restrict__ r, const T * __restrict__ K, T * __restrict__ p, long m, long ld, int c0,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double zr[KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T rv[KC], pv[KC];
		load_row(rv, r + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T ri = rv[c];
			const T zi = ri / ki;
			pv[c] = zi;
			zr[c] += (double) zi * (double) ri;
		}
		store_row(p + o, pv, vec);
	}
	store_partials_n<KC, 1>(part, c0, {P_C}, zr, ~0u);
}

// partial A = p.Ap ; block 0 records the per-iteration report line (bench_cg.cpp:249)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
cg_dot_kernel(const SolverState * __restrict__ st_p, const T * __restrict__ p, const T * __restrict__ Ap, long m, long ld,
		int c0, double * __restrict__ history, long hist_ld, long it, double * __restrict__ part)
{
	const unsigned live = live_mask<KC>(st_p, c0);
	if (!live)
		return;
	record_history<KC>(st_p, c0, live, history, hist_ld, it);
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double s[KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T pv[KC], av[KC];
		load_row(pv, p + o, vec);
		load_row(av, Ap + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			s[c] += (double) pv[c] * (double) av[c];
	}
	store_partials_n<KC, 1>(part, c0, {P_A}, s, live);
}

// ak = (z.r)/(p.Ap); x += ak p; r -= ak Ap; z = r/K (not stored); partials D = z.r, E = r.r   (bench_cg.cpp:259-274)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
cg_update_kernel(const SolverState * __restrict__ st_p, T * __restrict__ x, T * __restrict__ r, const T * __restrict__ p,
		const T * __restrict__ Ap, const T * __restrict__ K, long m, long ld, int c0, int nb, double * __restrict__ part)
{
	const unsigned live = live_mask<KC>(st_p, c0);
	if (!live)
		return;
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double pap[KC];
	sum_partials_n<KC, 1>(part, c0, {P_A}, nb, pap);
	T ak[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
		ak[c] = (T) (st_p[c0 + c].zr / pap[c]);
	double acc[2 * KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T xv[KC], rv[KC], pv[KC], av[KC];
		load_row(xv, x + o, vec);
		load_row(rv, r + o, vec);
		load_row(pv, p + o, vec);
		load_row(av, Ap + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T xi = xv[c] + ak[c] * pv[c];
			const T ri = rv[c] + (-ak[c]) * av[c];
			const T zi = ri / ki;
			acc[c] += (double) zi * (double) ri;
			acc[KC + c] += (double) ri * (double) ri;
			if (live >> c & 1)
			{
				xv[c] = xi;
				rv[c] = ri;
			}
		}
		store_row(x + o, xv, vec);
		store_row(r + o, rv, vec);
	}
	store_partials_n<KC, 2>(part, c0, {P_D, P_E}, acc, live);
}

// bk = (z.r)_new / (z.r)_old ; p = z + bk p (bench_cg.cpp:278-283); block 0 writes the next states: k+1, err = |r| and the
// `err < eps` break of the next loop top (bench_cg.cpp:209-214,238-239); the last chunk posts progress
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
cg_direction_kernel(const SolverState * __restrict__ st_p, SolverState * __restrict__ st_next, const T * __restrict__ r,
		T * __restrict__ p, const T * __restrict__ K, long m, long ld, int c0, int k, int nb, const double * __restrict__ part,
		long it, volatile long * host_progress)
{
	const unsigned live = live_mask<KC>(st_p, c0);
	double zr_new[KC] = {}, rr[KC] = {};
	if (live)
	{
		const bool vec = ld % KC == 0 && c0 % KC == 0;
		sum_partials_n<KC, 1>(part, c0, {P_D}, nb, zr_new);
		T bk[KC];
		#pragma unroll
		for (int c = 0; c < KC; c++)
			bk[c] = (T) (zr_new[c] / st_p[c0 + c].zr);
		GRID_STRIDE(i, m)
		{
			const long o = i * ld + c0;
			T rv[KC], pv[KC];
			load_row(rv, r + o, vec);
			load_row(pv, p + o, vec);
			const T ki = K[i];
			#pragma unroll
			for (int c = 0; c < KC; c++)
			{
				const T pi = rv[c] / ki + bk[c] * pv[c];
				if (live >> c & 1)
					pv[c] = pi;
			}
			store_row(p + o, pv, vec);
		}
	}
	if (blockIdx.x == 0)
	{
		if (live)
			sum_partials_n<KC, 1>(part, c0, {P_E}, nb, rr);
		if (threadIdx.x == 0)
		{
			#pragma unroll
			for (int c = 0; c < KC; c++)
			{
				SolverState nx = st_p[c0 + c];
				if (live >> c & 1)
				{
					nx.zr = zr_new[c];
					nx.err = sqrt(rr[c]);
					nx.k = nx.k + 1;
					nx.done = nx.err < nx.eps;
				}
				st_next[c0 + c] = nx;
			}
			if (c0 + KC == k)
				post_columns_progress(st_next, k, it, host_progress);
		}
	}
}

// ------------------------------------------------------------------------------------------------ BiCGSTAB

// r0_ = r, p = r, y = p/K (bench_bicg.cpp:232-246,328-332)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_init_kernel(const T * __restrict__ r, const T * __restrict__ K, T * __restrict__ r0, T * __restrict__ p, T * __restrict__ y,
		long m, long ld, int c0)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T rv[KC], yv[KC];
		load_row(rv, r + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
			yv[c] = rv[c] / ki;
		store_row(r0 + o, rv, vec);
		store_row(p + o, rv, vec);
		store_row(y + o, yv, vec);
	}
}

// partial A = r0_.v ; block 0 records the report line (bench_bicg.cpp:323)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_dot_kernel(const SolverState * __restrict__ st_p, const T * __restrict__ r0, const T * __restrict__ v, long m, long ld,
		int c0, double * __restrict__ history, long hist_ld, long it, double * __restrict__ part)
{
	record_history<KC>(st_p, c0, ~0u, history, hist_ld, it);
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double s[KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T r0v[KC], vv[KC];
		load_row(r0v, r0 + o, vec);
		load_row(vv, v + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			s[c] += (double) r0v[c] * (double) vv[c];
	}
	store_partials_n<KC, 1>(part, c0, {P_A}, s, ~0u);
}

// s_a = s_pk_p / (r0_.v); s = r - s_a v; z = s/K (bench_bicg.cpp:343-360)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_s_kernel(const SolverState * __restrict__ st_p, const T * __restrict__ r, const T * __restrict__ v, const T * __restrict__ K,
		T * __restrict__ s, T * __restrict__ z, long m, long ld, int c0, int nb, const double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double pa[KC];
	sum_partials_n<KC, 1>(part, c0, {P_A}, nb, pa);
	T s_a[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
		s_a[c] = (T) ((T) st_p[c0 + c].zr / (T) pa[c]);
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T rv[KC], vv[KC], sv[KC], zv[KC];
		load_row(rv, r + o, vec);
		load_row(vv, v + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T si = rv[c] + (-s_a[c]) * vv[c];
			sv[c] = si;
			zv[c] = si / ki;
		}
		store_row(s + o, sv, vec);
		store_row(z + o, zv, vec);
	}
}

// partials B = sum (t/K)(s/K), C = sum (t/K)^2 (bench_bicg.cpp:374-391)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_omega_kernel(const T * __restrict__ t, const T * __restrict__ s, const T * __restrict__ K, long m, long ld, int c0,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double acc[2 * KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T tv[KC], sv[KC];
		load_row(tv, t + o, vec);
		load_row(sv, s + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T v1 = tv[c] / ki;
			const T v2 = sv[c] / ki;
			acc[c] += (double) v1 * (double) v2;
			acc[KC + c] += (double) v1 * (double) v1;
		}
	}
	store_partials_n<KC, 2>(part, c0, {P_B, P_C}, acc, ~0u);
}

// s_w; r = s - s_w t; x = (x + s_a y) + s_w z; partials D = r0_.r, E = r.r (bench_bicg.cpp:350,394-402)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_update_kernel(const SolverState * __restrict__ st_p, const T * __restrict__ s, const T * __restrict__ t, const T * __restrict__ y,
		const T * __restrict__ z, const T * __restrict__ r0, T * __restrict__ r, T * __restrict__ x, long m, long ld, int c0, int nb,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double q[3 * KC];
	sum_partials_n<KC, 3>(part, c0, {P_A, P_B, P_C}, nb, q);
	T s_a[KC], s_w[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
	{
		s_a[c] = (T) ((T) st_p[c0 + c].zr / (T) q[c]);
		s_w[c] = (T) ((T) q[KC + c] / (T) q[2 * KC + c]);
	}
	double acc[2 * KC] = {};
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T sv[KC], tv[KC], yv[KC], zv[KC], r0v[KC], rv[KC], xv[KC];
		load_row(sv, s + o, vec);
		load_row(tv, t + o, vec);
		load_row(yv, y + o, vec);
		load_row(zv, z + o, vec);
		load_row(r0v, r0 + o, vec);
		load_row(xv, x + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T ri = sv[c] + (-s_w[c]) * tv[c];
			rv[c] = ri;
			const T hi = xv[c] + s_a[c] * yv[c];
			xv[c] = hi + s_w[c] * zv[c];
			acc[c] += (double) r0v[c] * (double) ri;
			acc[KC + c] += (double) ri * (double) ri;
		}
		store_row(r + o, rv, vec);
		store_row(x + o, xv, vec);
	}
	store_partials_n<KC, 2>(part, c0, {P_D, P_E}, acc, ~0u);
}

// s_b = (s_pk/s_pk_p)(s_a/s_w); p = r + s_b (p - s_w v); y = p/K for the next iteration; block 0 writes the next states;
// the last chunk posts progress (bench_bicg.cpp:402-419, 304-311, 328-332)
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
bicg_direction_kernel(const SolverState * __restrict__ st_p, SolverState * __restrict__ st_next, const T * __restrict__ r,
		const T * __restrict__ v, const T * __restrict__ K, T * __restrict__ p, T * __restrict__ y, long m, long ld, int c0, int k,
		int nb, const double * __restrict__ part, long it, volatile long * host_progress)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double q[4 * KC];
	sum_partials_n<KC, 4>(part, c0, {P_A, P_B, P_C, P_D}, nb, q);
	T s_w[KC], s_b[KC], s_pk[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
	{
		const T s_pk_p = (T) st_p[c0 + c].zr;
		const T s_a = (T) (s_pk_p / (T) q[c]);
		s_w[c] = (T) ((T) q[KC + c] / (T) q[2 * KC + c]);
		const double s_pk_d = q[3 * KC + c];
		s_pk[c] = (T) s_pk_d;
		s_b[c] = (s_pk[c] / s_pk_p) * (s_a / s_w[c]);
	}
	GRID_STRIDE(i, m)
	{
		const long o = i * ld + c0;
		T rv[KC], vv[KC], pv[KC], yv[KC];
		load_row(rv, r + o, vec);
		load_row(vv, v + o, vec);
		load_row(pv, p + o, vec);
		const T ki = K[i];
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T pi = rv[c] + s_b[c] * (pv[c] - s_w[c] * vv[c]);
			pv[c] = pi;
			yv[c] = pi / ki;
		}
		store_row(p + o, pv, vec);
		store_row(y + o, yv, vec);
	}
	if (blockIdx.x == 0)
	{
		double rr[KC];
		sum_partials_n<KC, 1>(part, c0, {P_E}, nb, rr);
		if (threadIdx.x == 0)
		{
			#pragma unroll
			for (int c = 0; c < KC; c++)
			{
				SolverState nx = st_p[c0 + c];
				nx.zr = (double) s_pk[c];
				nx.err = sqrt(rr[c]);
				nx.k = nx.k + 1;
				st_next[c0 + c] = nx;
			}
			if (c0 + KC == k)
				post_progress(host_progress, it + 1, -1);
		}
	}
}

// Distributed solves (k = 1): the per-block partials of up to 3 slots are summed into red[], all-reduced over the ranks by the
// caller's collective, and written back as the single partial of their slot (consumers then run with nb = 1).
struct SlotList {
	int n;
	int s[3];
};

__global__ __launch_bounds__(VB) void
reduce_slots_kernel(const double * __restrict__ part, int nb, SlotList sl, double * __restrict__ red)
{
	const double v = sum_partials(part, sl.s[blockIdx.x], nb);
	if (threadIdx.x == 0)
		red[blockIdx.x] = v;
}

__global__ void
scatter_slots_kernel(double * __restrict__ part, SlotList sl, const double * __restrict__ red)
{
	if ((int) threadIdx.x < sl.n)
		part[(long) sl.s[threadIdx.x] * MAX_PART] = red[threadIdx.x];
}

// ------------------------------------------------------------------------------------------------ host side

// The one solve behind all six entry points. `multi`: the _multi entries, whose matrix product is the SpMM for every k
// (1 included) and whose messages carry `what`; the single entries (k = 1) use the SpMV and, with `dist` (row-partitioned,
// k = 1 only), the caller's callbacks.
template <typename T>
static int
solve(const char * what, bool multi, int method, spmv_mi355x_matrix * A, const spmv_mi355x_dist_ops * dist, int k, long m_arg,
		const int32_t * row_ptr, const int32_t * col, const double * val, const void * b_host, void * x_host, long max_iterations,
		double * history_host, spmv_mi355x_solver_info * info)
{
	const auto t_start = std::chrono::steady_clock::now();
	const long m = dist ? m_arg : spmv_mi355x_rows(A);
	const long ld = k;
	hipStream_t stream = nullptr;
	ProgressGate gate;                // outlives buf, whose hipFree waits for the kernels that post to it
	DeviceBuffers buf;
	const size_t vb = (size_t) m * k * sizeof(T);

	std::vector<T> K_host((size_t) std::max<long>(m, 1));
	const long bad = jacobi_diagonal<T>(row_ptr, col, val, m, dist ? dist->row_offset : 0, K_host.data());
	if (bad >= 0)
	{
		if (multi)
			set_error("%s: bad K, zero in diagonal (row %ld)", what, bad);
		else
			set_error("bad K, zero in diagonal (row %ld)", bad);
		return 1;
	}

	T * b, * K, * x, * x_best, * r, * r_explicit, * p, * Ap;
	T * r0 = nullptr, * y = nullptr, * z = nullptr, * s = nullptr, * v = nullptr;
	// Plain allocations, the SpMV outputs (Ap, v) included: the engine's placement search (placement.hip) costs ~1 s and leaves the
	// driver clearing 160 GiB for seconds afterwards — more than a solve of a few hundred iterations takes (measured: 0.27 instead of
	// 0.24 ms per CG iteration on the 160^3 stencil right after it). A caller who solves many systems with one handle can hand in
	// vectors from spmv_mi355x_output_alloc through the device-pointer entry points instead.
	for (T ** q : {&b, &x, &x_best, &r, &r_explicit, &p, &Ap})
		ABI_TRY(buf.alloc(q, vb));
	ABI_TRY(buf.alloc(&K, (size_t) m * sizeof(T)));
	if (method == 1)
		for (T ** q : {&r0, &y, &z, &s, &v})
			ABI_TRY(buf.alloc(q, vb));
	double * part, * history = nullptr;
	SolverState * st;
	const size_t part_bytes = sizeof(double) * (size_t) k * NUM_SLOTS * MAX_PART;
	ABI_TRY(buf.alloc(&part, part_bytes));
	ABI_TRY(buf.alloc(&st, 2 * (size_t) k * sizeof(SolverState)));
	const long hist_ld = 3 * max_iterations;
	if (history_host && max_iterations > 0)
	{
		ABI_TRY(buf.alloc(&history, sizeof(double) * (size_t) k * hist_ld));
		HIP_TRY(hipMemsetAsync(history, 0, sizeof(double) * (size_t) k * hist_ld, stream));
	}
	ABI_TRY(gate.init());

	HIP_TRY(hipMemcpyAsync(b, b_host, vb, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemcpyAsync(K, K_host.data(), (size_t) m * sizeof(T), hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemsetAsync(x, 0, vb, stream));                    // x0 = 0 (bench_cg.cpp:139-145)
	HIP_TRY(hipMemsetAsync(x_best, 0, vb, stream));
	HIP_TRY(hipMemsetAsync(part, 0, part_bytes, stream));

	// one launch shape for every k: the same rows per (block, thread), hence the same additions per column
	const int nb = solver_blocks(m);
	const dim3 grid(nb), block(VB), per_col(k);
	const std::vector<Chunk> chunks = column_chunks(k);
	long spmv_calls = 0;
	auto product = [&](const T * in, T * out) {
		spmv_calls++;
		if (dist)
		{
			if (dist->spmv(dist->ctx, in, out))
			{
				set_error("solver: the caller's distributed spmv callback failed");
				return 1;
			}
			return 0;
		}
		if (multi)
			return spmv_mi355x_spmm_device_async(A, k, in, ld, out, ld, 0, stream);
		return spmv_mi355x_spmv_device_async(A, in, out, 0, stream);
	};
	// single GPU: consumers re-reduce the nb per-block partials themselves. Distributed (k = 1, so column 0's slot s starts at
	// s * MAX_PART): the listed slots are reduced, summed over the ranks by the caller's collective and put back as ONE partial;
	// consumers then read nbc = 1 partial.
	const int nbc = dist ? 1 : nb;
	auto global_reduce = [&](SlotList sl) {
		if (!dist)
			return 0;
		hipLaunchKernelGGL(reduce_slots_kernel, dim3(sl.n), block, 0, stream, part, nb, sl, dist->reduce_buf_dev);
		if (dist->allreduce_sum(dist->ctx, dist->reduce_buf_dev, sl.n))
		{
			set_error("solver: the caller's all-reduce callback failed");
			return 1;
		}
		hipLaunchKernelGGL(scatter_slots_kernel, dim3(1), dim3(WAVE), 0, stream, part, sl, dist->reduce_buf_dev);
		return 0;
	};
	// |b - A x|^2 into partial A of every column, r_explicit = b - A x
	auto explicit_residual = [&](const T * xx) {
		if (product(xx, Ap))
			return 1;
		for_chunks(chunks, [&](int c0, auto kc) {
			hipLaunchKernelGGL((residual_kernel<T, decltype(kc)::value>), grid, block, 0, stream, b, Ap, r_explicit, m, ld, c0, part);
			return 0;
		});
		return global_reduce({1, {P_A, 0, 0}});
	};
	auto explicit_step = [&](SolverState * cur, int allow_restart, int ignore_done) {
		for_chunks(chunks, [&](int c0, auto kc) {
			hipLaunchKernelGGL((explicit_kernel<T, decltype(kc)::value>), grid, block, 0, stream, cur, x, x_best, r_explicit, r, p, K, m, ld,
					c0, nbc, allow_restart, ignore_done, part);
			return 0;
		});
		if (allow_restart && global_reduce({1, {P_C, 0, 0}}))         // z.r of a restart (stale and unread otherwise)
			return 1;
		hipLaunchKernelGGL(explicit_fin_kernel, per_col, block, 0, stream, cur, nbc, allow_restart, ignore_done, part);
		return 0;
	};

	// r0 = b - A x0
	ABI_TRY(product(x, Ap));
	for_chunks(chunks, [&](int c0, auto kc) {
		constexpr int KC = decltype(kc)::value;
		hipLaunchKernelGGL((residual_kernel<T, KC>), grid, block, 0, stream, b, Ap, r, m, ld, c0, part);
		if (method == 0)
			hipLaunchKernelGGL((cg_init_kernel<T, KC>), grid, block, 0, stream, r, K, p, m, ld, c0, part);
		else
			hipLaunchKernelGGL((bicg_init_kernel<T, KC>), grid, block, 0, stream, r, K, r0, p, y, m, ld, c0);
		return 0;
	});
	ABI_TRY(global_reduce({3, {P_A, P_B, P_C}}));
	hipLaunchKernelGGL(init_state_kernel, per_col, block, 0, stream, st, k, nbc, method, part);
	HIP_TRY(hipGetLastError());

	const bool debug = getenv("SPMV_MI355X_SOLVER_DEBUG") != nullptr;
	const auto t_loop = std::chrono::steady_clock::now();
	long it = 0;
	for (; it < max_iterations; it++)
	{
		bool stop;
		ABI_TRY(gate.wait(it, what, stream, &stop));
		if (stop)
			break;
		SolverState * cur = st + (it & 1) * k, * nxt = st + ((it + 1) & 1) * k;
		if (it > 0 && it % RESTART_K == 0)
		{
			ABI_TRY(explicit_residual(x));
			ABI_TRY(explicit_step(cur, method == 0, 0));
		}
		if (method == 0)
		{
			ABI_TRY(product(p, Ap));
			for_chunks(chunks, [&](int c0, auto kc) {
				hipLaunchKernelGGL((cg_dot_kernel<T, decltype(kc)::value>), grid, block, 0, stream, cur, p, Ap, m, ld, c0, history, hist_ld,
						it, part);
				return 0;
			});
			ABI_TRY(global_reduce({1, {P_A, 0, 0}}));
			for_chunks(chunks, [&](int c0, auto kc) {
				hipLaunchKernelGGL((cg_update_kernel<T, decltype(kc)::value>), grid, block, 0, stream, cur, x, r, p, Ap, K, m, ld, c0, nbc,
						part);
				return 0;
			});
			ABI_TRY(global_reduce({2, {P_D, P_E, 0}}));
			for_chunks(chunks, [&](int c0, auto kc) {
				hipLaunchKernelGGL((cg_direction_kernel<T, decltype(kc)::value>), grid, block, 0, stream, cur, nxt, r, p, K, m, ld, c0, k,
						nbc, part, it, gate.dev);
				return 0;
			});
		}
		else
		{
			// dot and s, omega and update stay paired per chunk; a distributed solve has one chunk (k = 1), so the global_reduce
			// between them still follows the whole kernel
			ABI_TRY(product(y, v));
			ABI_TRY(for_chunks(chunks, [&](int c0, auto kc) {
				constexpr int KC = decltype(kc)::value;
				hipLaunchKernelGGL((bicg_dot_kernel<T, KC>), grid, block, 0, stream, cur, r0, v, m, ld, c0, history, hist_ld, it, part);
				if (global_reduce({1, {P_A, 0, 0}}))
					return 1;
				hipLaunchKernelGGL((bicg_s_kernel<T, KC>), grid, block, 0, stream, cur, r, v, K, s, z, m, ld, c0, nbc, part);
				return 0;
			}));
			ABI_TRY(product(z, Ap));                             // t = A z
			ABI_TRY(for_chunks(chunks, [&](int c0, auto kc) {
				constexpr int KC = decltype(kc)::value;
				hipLaunchKernelGGL((bicg_omega_kernel<T, KC>), grid, block, 0, stream, Ap, s, K, m, ld, c0, part);
				if (global_reduce({2, {P_B, P_C, 0}}))
					return 1;
				hipLaunchKernelGGL((bicg_update_kernel<T, KC>), grid, block, 0, stream, cur, s, Ap, y, z, r0, r, x, m, ld, c0, nbc, part);
				return 0;
			}));
			ABI_TRY(global_reduce({2, {P_D, P_E, 0}}));
			for_chunks(chunks, [&](int c0, auto kc) {
				hipLaunchKernelGGL((bicg_direction_kernel<T, decltype(kc)::value>), grid, block, 0, stream, cur, nxt, r, v, K, p, y, m, ld,
						c0, k, nbc, part, it, gate.dev);
				return 0;
			});
		}
	}
	HIP_TRY(hipGetLastError());
	const auto t_loop_end = std::chrono::steady_clock::now();
	if (debug)
	{
		HIP_TRY(hipStreamSynchronize(stream));
		const auto t_sync = std::chrono::steady_clock::now();
		fprintf(stderr, "[%s k %d] setup %.3f ms, enqueue loop %.3f ms (spin %.3f ms), drain %.3f ms, %ld iterations launched\n", what, k,
				std::chrono::duration<double>(t_loop - t_start).count() * 1e3,
				std::chrono::duration<double>(t_loop_end - t_loop).count() * 1e3, gate.spin_seconds * 1e3,
				std::chrono::duration<double>(t_sync - t_loop_end).count() * 1e3, it);
	}

	// final explicit residual of x, promotion of x_best (bench_cg.cpp:288-306); runs after a break too
	SolverState * fin = st + (it & 1) * k;
	ABI_TRY(explicit_residual(x));
	ABI_TRY(explicit_step(fin, 0, 1));
	// the harness's own check of the returned vector: error = |b - A x_best| (bench_cg.cpp:412-418)
	ABI_TRY(explicit_residual(x_best));
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(x_host, x_best, vb, hipMemcpyDeviceToHost, stream));
	std::vector<SolverState> st_host((size_t) k);
	std::vector<double> part_host((size_t) k * NUM_SLOTS * MAX_PART);
	HIP_TRY(hipMemcpyAsync(st_host.data(), fin, sizeof(SolverState) * k, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(part_host.data(), part, part_bytes, hipMemcpyDeviceToHost, stream));
	if (history)
		HIP_TRY(hipMemcpyAsync(history_host, history, sizeof(double) * (size_t) k * hist_ld, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	if (info)
	{
		// info[0].struct_size is the caller's stride; every element is written with that size
		const unsigned want = info->struct_size;
		const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
		if (debug)
			fprintf(stderr, "[%s k %d] tail (final residuals, downloads) %.3f ms, total %.3f ms\n", what, k,
					std::chrono::duration<double>(std::chrono::steady_clock::now() - t_loop_end).count() * 1e3, seconds * 1e3);
		for (int c = 0; c < k; c++)
		{
			spmv_mi355x_solver_info out;
			memset(&out, 0, sizeof(out));
			const SolverState & sc = st_host[c];
			out.iterations = sc.k;
			out.error = std::sqrt(host_sum(part_host.data(), part_at(c, P_A), nbc));
			out.error_best = sc.err_best;
			out.eps = sc.eps;
			out.eps_counter = sc.eps_counter;
			out.restarts = sc.restarts;
			out.spmv_calls = spmv_calls - 1;                      // the last one is the harness's check, not the solver's
			out.seconds = seconds;
			put_info((char *) info + (size_t) c * want, want, out);
		}
	}
	return 0;
}

static int
solve_entry(int method, spmv_mi355x_matrix * A, const int32_t * row_ptr, const int32_t * col, const double * val, const void * b_host,
		void * x_host, long max_iterations, double * history_host, spmv_mi355x_solver_info * info)
{
	if (!A || !row_ptr || !b_host || !x_host)
	{
		set_error("solver: NULL argument");
		return 1;
	}
	if (!info_size_ok("solver", info))
		return 1;
	if (spmv_mi355x_rows(A) != spmv_mi355x_cols(A))
	{
		set_error("the matrix must be square");                  // bench_cg.cpp:487-488
		return 1;
	}
	if (max_iterations < 0)
	{
		set_error("solver: max_iterations < 0");
		return 1;
	}
	if (spmv_mi355x_nnz(A) > 0 && (!col || !val))
	{
		set_error("solver: NULL CSR arrays");
		return 1;
	}
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	if (spmv_mi355x_precision(A) == SPMV_MI355X_F32)
		return solve<float>("solver", false, method, A, nullptr, 1, 0, row_ptr, col, val, b_host, x_host, max_iterations, history_host, info);
	return solve<double>("solver", false, method, A, nullptr, 1, 0, row_ptr, col, val, b_host, x_host, max_iterations, history_host, info);
}

static int
solve_dist_entry(int method, const spmv_mi355x_dist_ops * ops, int precision, long m_local, const int32_t * row_ptr, const int32_t * col,
		const double * val, const void * b_host, void * x_host, long max_iterations, double * history_host,
		spmv_mi355x_solver_info * info)
{
	if (!ops || ops->struct_size < sizeof(spmv_mi355x_dist_ops) || !ops->spmv || !ops->allreduce_sum || !ops->reduce_buf_dev)
	{
		set_error("distributed solver: ops incomplete (struct_size, spmv, allreduce_sum and reduce_buf_dev are required)");
		return 1;
	}
	if (!row_ptr || !b_host || !x_host || m_local < 0 || max_iterations < 0 || (row_ptr[m_local] > 0 && (!col || !val)))
	{
		set_error("distributed solver: bad argument");
		return 1;
	}
	if (!info_size_ok("solver", info))
		return 1;
	if (precision == SPMV_MI355X_F32)
		return solve<float>("solver", false, method, nullptr, ops, 1, m_local, row_ptr, col, val, b_host, x_host, max_iterations,
				history_host, info);
	if (precision == SPMV_MI355X_F64)
		return solve<double>("solver", false, method, nullptr, ops, 1, m_local, row_ptr, col, val, b_host, x_host, max_iterations,
				history_host, info);
	set_error("unknown precision %d", precision);
	return 1;
}

static int
solve_multi_entry(const char * what, int method, spmv_mi355x_matrix * A, int k, const int32_t * row_ptr, const int32_t * col,
		const double * val, const void * b_host, void * x_host, long max_iterations, double * history_host,
		spmv_mi355x_solver_info * info)
{
	// every argument check comes before the device is touched
	if (k < 1)
	{
		set_error("%s: k must be >= 1 (got %d)", what, k);
		return 1;
	}
	if (!info_size_ok(what, info))
		return 1;
	if (!A || !row_ptr || !b_host || !x_host)
	{
		set_error("%s: NULL argument", what);
		return 1;
	}
	if (spmv_mi355x_rows(A) != spmv_mi355x_cols(A))
	{
		set_error("%s: the matrix must be square", what);
		return 1;
	}
	if (max_iterations < 0)
	{
		set_error("%s: max_iterations < 0", what);
		return 1;
	}
	if (spmv_mi355x_nnz(A) > 0 && (!col || !val))
	{
		set_error("%s: NULL CSR arrays", what);
		return 1;
	}
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	if (spmv_mi355x_precision(A) == SPMV_MI355X_F32)
		return solve<float>(what, true, method, A, nullptr, k, 0, row_ptr, col, val, b_host, x_host, max_iterations, history_host, info);
	return solve<double>(what, true, method, A, nullptr, k, 0, row_ptr, col, val, b_host, x_host, max_iterations, history_host, info);
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_pcg_dist(const spmv_mi355x_dist_ops * ops, int precision, long m_local, const int32_t * row_ptr_local,
		const int32_t * col_idx_global, const double * values_fp64, const void * b_local_host, void * x_local_host,
		long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_dist_entry(0, ops, precision, m_local, row_ptr_local, col_idx_global, values_fp64, b_local_host, x_local_host,
			max_iterations, history_out, info);
}

int
spmv_mi355x_pbicgstab_dist(const spmv_mi355x_dist_ops * ops, int precision, long m_local, const int32_t * row_ptr_local,
		const int32_t * col_idx_global, const double * values_fp64, const void * b_local_host, void * x_local_host,
		long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_dist_entry(1, ops, precision, m_local, row_ptr_local, col_idx_global, values_fp64, b_local_host, x_local_host,
			max_iterations, history_out, info);
}

int
spmv_mi355x_pcg(spmv_mi355x_matrix * A, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * b_host, void * x_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_entry(0, A, row_ptr, col_idx, values_fp64, b_host, x_host, max_iterations, history_out, info);
}

int
spmv_mi355x_pbicgstab(spmv_mi355x_matrix * A, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * b_host, void * x_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_entry(1, A, row_ptr, col_idx, values_fp64, b_host, x_host, max_iterations, history_out, info);
}

int
spmv_mi355x_pcg_multi(spmv_mi355x_matrix * A, int k, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * B_host, void * X_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_multi_entry("pcg_multi", 0, A, k, row_ptr, col_idx, values_fp64, B_host, X_res_out_host, max_iterations,
			history_out, info);
}

int
spmv_mi355x_pbicgstab_multi(spmv_mi355x_matrix * A, int k, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * B_host, void * X_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info)
{
	return spmv::solve_multi_entry("pbicgstab_multi", 1, A, k, row_ptr, col_idx, values_fp64, B_host, X_res_out_host, max_iterations,
			history_out, info);
}

}

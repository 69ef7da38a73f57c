// Device-resident preconditioned CG of the tol-based family (MINRES, GMRES, CGLS): A x = b from x0 = 0 for a square SYMMETRIC
// POSITIVE DEFINITE matrix over one handle of A, preconditioned by M^-1 v = second^-1 (scale o (first^-1 v)), a
// spmv_mi355x_tri_precond with each part optional (the SGS of A, the caller's IC(0), a Jacobi scale, nothing).
//
// The recurrences, every scalar and every dot fp64, vectors in the handle's precision:
//   x = 0; r = b; rnorm0 = |b|                     (0: stop 3, x = 0, every norm 0; not finite: stop 4)
//   z = M^-1 r; p = z; rz = r.z                    (not finite or <= 0: stop 4, 0 iterations, x = 0)
//   loop k = 1, 2, ... while k <= max_iterations:
//       q = A p; pq = p.q                          (not finite or <= 0: stop 4; x, iterations, history as before this body)
//       alpha = rz / pq; x += alpha p; r -= alpha q; rr = r.r; history[k-1] = sqrt(rr); iterations = k
//       if tol > 0 and sqrt(rr) <= tol rnorm0: stop 1;  else if rr == 0: stop 5
//       z = M^-1 r; rz' = r.z                      (not finite or <= 0: stop 4; this body's x is kept)
//       beta = rz' / rz; rz = rz'; p = z + beta p
// Built like solver_minres.hip: the state ping-pongs between two slots, dots are two-stage and deterministic (every block of the
// consumer re-sums the partials in the same order), a device `done` flag predicates every later vector kernel off, and the host
// loop is ProgressGate of solvers_common.hpp.
//
// ONE BODY, SEVEN ENTRIES. spmv_mi355x_pcg_tri / _pcg_fsai / _pcg_amg, their _multi forms and _pcg_trsm_multi all run pcg_tri_solve over k columns: k
// independent solves A x_j = b_j, each with the recurrences, stop rules and freeze of this comment, sharing every launch. This is not
// block CG. The single entries are k = 1. Every vector is a row-major n x k block (ld = k); a vector kernel serves a chunk of KC in
// {8, 4, 2, 1} columns c0.. and a thread owns row i of its chunk (solvers_common.hpp). The state is PcgTriState[2][k], the partials
// are [k][PCG_TRI_SLOTS][MAX_PART], the history row of column j starts at j * max_iterations. An entry passes in the two things that
// differ:
//   the matrix product q = A p   SpmvProduct (the single entries) or SpmmProduct (the _multi entries, also for k = 1)
//   enqueue z = M^-1 r           TriApply (pcg_tri: the three parts of tri_precond.hpp on an n x 1 block, so triangular parts are served
//                                by the single-vector kernels), ScaleApplyMulti (pcg_tri_multi: a Jacobi scale; a triangular part is
//                                refused there), TriApplyMulti (pcg_trsm_multi: the three parts on the n x k block, the triangular ones
//                                by the k-column solve of trsv.hip, a chunk of columns per pass), FsaiApply / FsaiApplyMulti (the two
//                                SpMVs or SpMMs G^t (G r) of an fsai handle, fsai.hip), AmgApply / AmgApplyMulti (one V cycle of an amg
//                                handle, amg.hip)
// so a single solve uses neither the SpMM nor a k-column apply, which are other kernels and allocate k-column blocks of their own.
// BIT FOR BIT. Per column the grid, the rows per (block, thread), the shuffle tree and the order over the partials do not depend on the
// chunk a column sits in, and every element update is the same T expression, so on a handle with a deterministic SpMV column j of a
// _multi call returns what the single call on b_j returns.
//
// Per iteration: 1 SpMV (SpMM) + M's own launches + 4 vector launches per chunk, 3 without a preconditioner
//   q = A p | pcg_tri_dot (partials of p.q) | pcg_tri_update (alpha; x += alpha p; r -= alpha q; partials of r.r) |
//   [ z = M^-1 r | pcg_tri_dot (partials of r.z) ] |
//   pcg_tri_direction (the verdicts, beta, the next state, the history row, the progress word; p = z + beta p).
// pcg_fsai: 3 SpMVs (A, G, G^t) and the 4 vector launches.
// Without a preconditioner z is r: no z is stored, nothing is launched for it and rz' is the rr of pcg_tri_update, so
// precond = (NULL, ones, NULL) returns the bits of precond = NULL.
// A cut with fewer launches would have to form a dot product and consume it in the same launch, which needs a grid-wide barrier:
// p.q must be complete before alpha, r.r (and r.z) before beta. Three reductions with their consumers are four launches.
// Stored blocks, n x k values each: b, x, r, p, q, and z when M has a part; the scale (n values) when given.
//
// BREAKDOWN of p.q. pcg_tri_update reaches the verdict in every block from the same partials and leaves the column's vectors as they
// are; pcg_tri_direction, the only kernel that writes the state, re-sums the same partials, reaches the same verdict and records
// done / stop 4 with k unchanged.
//
// THE FREEZE, PER COLUMN. The matrix product and the preconditioner (triangular solves, scale kernel, the SpMVs of an fsai apply, the
// SpMVs and vector kernels of an amg cycle) know nothing of `done` and run however far the host is ahead; what they write is q, z and
// the preconditioner handle's own scratch, which only the predicated kernels read. Each column has its own `done`: a done column's
// x, r and p are stored back as loaded, its state is copied, its partials and its history are not written. So after a stop nothing
// the caller sees of that column moves. The last chunk of pcg_tri_direction posts progress: the loop count at which the last column
// stopped once every column is done.

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "solvers_common.hpp"
#include "amg.hpp"
#include "fsai.hpp"
#include "tri_precond.hpp"
#include "trsv.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

struct PcgTriState {
	double rnorm0;                // |b|
	double rz;                    // r.z of the running direction
	double rr;                    // r.r of the recurrence after body k
	long k;                       // completed loop bodies
	int done;                     // a stop rule fired: every later vector kernel is predicated off
	int stop;                     // 0 while running, else 1 / 3 / 4 / 5 of spmv_mi355x_pcg_tri_info.stop (2 is the host's: never done)
};

// one producer kernel per slot
enum { T_BB = 0, T_PQ, T_RR, T_RZ, T_ER, T_XX, PCG_TRI_SLOTS };

// a positive finite number: what p.q and r.z must be
__device__ __forceinline__ bool
pcg_tri_positive(double v)
{
	return v > 0 && v < INFINITY;
}

static_assert((int) PCG_TRI_SLOTS == (int) NUM_SLOTS, "part_at() lays the partials out by NUM_SLOTS");

template <int KC>
__device__ __forceinline__ unsigned
pcg_tri_live(const PcgTriState * __restrict__ st_p, int c0)
{
	unsigned live = 0;
	#pragma unroll
	for (int c = 0; c < KC; c++)
		if (!st_p[c0 + c].done)
			live |= 1u << c;
	return live;
}

// r = b; x = 0; without a preconditioner also p = b; partial BB = b.b
template <typename T, int KC, bool PRE>
__global__ __launch_bounds__(VB) void
pcg_tri_start_kernel(const T * __restrict__ b, T * __restrict__ r, T * __restrict__ p, T * __restrict__ x, long n, long ld, int c0,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double bb[KC] = {};
	GRID_STRIDE(i, n)
	{
		const long o = i * ld + c0;
		T bv[KC], zero[KC];
		load_row(bv, b + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			zero[c] = 0;
			bb[c] = fma((double) bv[c], (double) bv[c], bb[c]);
		}
		store_row(r + o, bv, vec);
		store_row(x + o, zero, vec);
		if (!PRE)
			store_row(p + o, bv, vec);
	}
	store_partials_n<KC, 1>(part, c0, {T_BB}, bb, ~0u);
}

// 1 block. b.b == 0: x = 0 is the solution (stop 3); not finite: stop 4. Without a preconditioner rz = b.b.
template <int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_init_state_kernel(PcgTriState * __restrict__ st_p, int k, int c0, int nb, const double * __restrict__ part)
{
	double bbv[KC];
	sum_partials_n<KC, 1>(part, c0, {T_BB}, nb, bbv);
	if (threadIdx.x == 0)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const double bb = bbv[c];
			PcgTriState st;
			const bool bad = !(bb >= 0) || !(bb < INFINITY);
			st.rnorm0 = bad ? 0 : sqrt(bb);
			st.rz = bb;
			st.rr = bb;
			st.k = 0;
			st.done = bad || bb == 0;
			st.stop = bad ? 4 : bb == 0 ? 3 : 0;
			st_p[c0 + c] = st;
			st_p[k + c0 + c] = st;
		}
	}
}

// partials of u.v into `slot` for the chunk's live columns: p.q, and r.z under a preconditioner
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_dot_kernel(const PcgTriState * __restrict__ st_p, const T * __restrict__ u, const T * __restrict__ v, long n, long ld, int c0,
		double * __restrict__ part, int slot)
{
	const unsigned live = pcg_tri_live<KC>(st_p, c0);
	if (!live)
		return;
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double s[KC] = {};
	GRID_STRIDE(i, n)
	{
		const long o = i * ld + c0;
		T uv[KC], vv[KC];
		load_row(uv, u + o, vec);
		load_row(vv, v + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			s[c] = fma((double) uv[c], (double) vv[c], s[c]);
	}
	store_partials_n<KC, 1>(part, c0, {slot}, s, live);
}

// With a preconditioner, the start: rz = r.z from the partials, p = z where rz is positive. Block 0 writes the next states (stop 4:
// rz not positive).
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_begin_kernel(const PcgTriState * __restrict__ st_p, PcgTriState * __restrict__ st_next, T * __restrict__ p,
		const T * __restrict__ z, long n, long ld, int c0, int nb, const double * __restrict__ part)
{
	const unsigned live = pcg_tri_live<KC>(st_p, c0);
	const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
	double rz[KC] = {};
	unsigned ok = 0;
	if (live)
	{
		sum_partials_n<KC, 1>(part, c0, {T_RZ}, nb, rz);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			if ((live >> c & 1) && pcg_tri_positive(rz[c]))
				ok |= 1u << c;
	}
	if (ok)
	{
		const bool vec = ld % KC == 0 && c0 % KC == 0;
		GRID_STRIDE(i, n)
		{
			const long o = i * ld + c0;
			T pv[KC], zv[KC];
			load_row(pv, p + o, vec);
			load_row(zv, z + o, vec);
			#pragma unroll
			for (int c = 0; c < KC; c++)
				if (ok >> c & 1)
					pv[c] = zv[c];
			store_row(p + o, pv, vec);
		}
	}
	if (lead)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			PcgTriState nx = st_p[c0 + c];
			if (live >> c & 1)
			{
				nx.rz = rz[c];
				nx.stop = (ok >> c & 1) ? 0 : 4;
				nx.done = !(ok >> c & 1);
			}
			st_next[c0 + c] = nx;
		}
	}
}

// alpha = rz / (p.q) identically in every block; x += alpha p; r -= alpha q; partial RR = r.r. A column whose p.q is not positive is
// left as it is, like a done one.
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_update_kernel(const PcgTriState * __restrict__ st_p, T * __restrict__ x, T * __restrict__ r, const T * __restrict__ p,
		const T * __restrict__ q, long n, long ld, int c0, int nb, double * __restrict__ part)
{
	const unsigned live = pcg_tri_live<KC>(st_p, c0);
	if (!live)
		return;
	double pq[KC];
	sum_partials_n<KC, 1>(part, c0, {T_PQ}, nb, pq);
	unsigned act = 0;
	T alpha[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
	{
		if ((live >> c & 1) && pcg_tri_positive(pq[c]))
			act |= 1u << c;
		alpha[c] = (T) (st_p[c0 + c].rz / pq[c]);
	}
	if (!act)
		return;
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double rr[KC] = {};
	GRID_STRIDE(i, n)
	{
		const long o = i * ld + c0;
		T xv[KC], rv[KC], pv[KC], qv[KC];
		load_row(xv, x + o, vec);
		load_row(rv, r + o, vec);
		load_row(pv, p + o, vec);
		load_row(qv, q + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T xi = xv[c] + alpha[c] * pv[c];
			const T ri = rv[c] - alpha[c] * qv[c];
			rr[c] = fma((double) ri, (double) ri, rr[c]);
			if (act >> c & 1)
			{
				xv[c] = xi;
				rv[c] = ri;
			}
		}
		store_row(x + o, xv, vec);
		store_row(r + o, rv, vec);
	}
	store_partials_n<KC, 1>(part, c0, {T_RR}, rr, act);
}

// (iterations finished, the loop count at which the last column stopped, or -1 while one runs) from the next states of all k columns:
// the earlier chunks wrote theirs in earlier launches, this thread wrote its own chunk's
__device__ __forceinline__ void
pcg_tri_post_columns(const PcgTriState * st_next, int k, long it, volatile long * host_progress)
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

// The verdicts of the body, identically in every block; p = z + beta p (z = r without a preconditioner) for the columns that go on.
// Block 0 writes the next states and the history rows (column j's at history + j * hist_ld); the last chunk posts progress.
template <typename T, int KC, bool PRE>
__global__ __launch_bounds__(VB) void
pcg_tri_direction_kernel(const PcgTriState * __restrict__ st_p, PcgTriState * __restrict__ st_next, T * __restrict__ p,
		const T * __restrict__ z, long n, long ld, int c0, int k, int nb, double tol, const double * __restrict__ part,
		double * __restrict__ history, long hist_ld, long it, volatile long * host_progress)
{
	const unsigned live = pcg_tri_live<KC>(st_p, c0);
	const bool lead = blockIdx.x == 0 && threadIdx.x == 0;
	PcgTriState nx[KC];
	double rnorm[KC] = {};
	unsigned wrote = 0, go = 0;                       // columns that completed a body; columns whose p moves
	T beta[KC];
	#pragma unroll
	for (int c = 0; c < KC; c++)
	{
		nx[c] = st_p[c0 + c];
		beta[c] = 0;
	}
	if (live)
	{
		double sums[3 * KC];
		sum_partials_n<KC, 3>(part, c0, {T_PQ, T_RR, T_RZ}, nb, sums);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			if (!(live >> c & 1))
				continue;
			if (!pcg_tri_positive(sums[c]))
			{
				nx[c].done = 1;                           // x, k and the history of the last good body
				nx[c].stop = 4;
				continue;
			}
			const double rr = sums[KC + c];
			rnorm[c] = sqrt(rr);
			wrote |= 1u << c;
			nx[c].rr = rr;
			nx[c].k = nx[c].k + 1;
			if (tol > 0 && rnorm[c] <= tol * nx[c].rnorm0)
				nx[c].stop = 1;
			else if (rr == 0)
				nx[c].stop = 5;
			else
			{
				const double rz = PRE ? sums[2 * KC + c] : rr;
				if (!pcg_tri_positive(rz))
					nx[c].stop = 4;                           // this body's x is kept
				else
				{
					beta[c] = (T) (rz / nx[c].rz);
					nx[c].rz = rz;
					go |= 1u << c;
				}
			}
			nx[c].done = nx[c].stop != 0;
		}
	}
	if (go)
	{
		const bool vec = ld % KC == 0 && c0 % KC == 0;
		GRID_STRIDE(i, n)
		{
			const long o = i * ld + c0;
			T pv[KC], zv[KC];
			load_row(pv, p + o, vec);
			load_row(zv, z + o, vec);
			#pragma unroll
			for (int c = 0; c < KC; c++)
			{
				const T pi = zv[c] + beta[c] * pv[c];
				if (go >> c & 1)
					pv[c] = pi;
			}
			store_row(p + o, pv, vec);
		}
	}
	if (lead)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			if (history && (wrote >> c & 1))
				history[(long) (c0 + c) * hist_ld + st_p[c0 + c].k] = rnorm[c];
			st_next[c0 + c] = nx[c];
		}
		if (c0 + KC == k)
			pcg_tri_post_columns(st_next, k, it, host_progress);
	}
}

// the tail's explicit residual: q = b - q (q = A x); partials ER = |b - A x|^2 and XX = |x|^2
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_final_kernel(const T * __restrict__ b, T * __restrict__ q, const T * __restrict__ x, long n, long ld, int c0,
		double * __restrict__ part)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	double acc[2 * KC] = {};
	GRID_STRIDE(i, n)
	{
		const long o = i * ld + c0;
		T bv[KC], qv[KC], xv[KC];
		load_row(bv, b + o, vec);
		load_row(qv, q + o, vec);
		load_row(xv, x + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
		{
			const T ri = bv[c] - qv[c];
			qv[c] = ri;
			acc[c] = fma((double) ri, (double) ri, acc[c]);
			acc[KC + c] = fma((double) xv[c], (double) xv[c], acc[KC + c]);
		}
		store_row(q + o, qv, vec);
	}
	store_partials_n<KC, 2>(part, c0, {T_ER, T_XX}, acc, ~0u);
}

// ------------------------------------------------------------------------------------------------ host side

// The solve of k columns behind all six entries. PRE: there is a preconditioner. scale_host: the scale of M or NULL; the solve keeps
// its device copy. product(A, k, in, out, stream) enqueues out = A in on n x k blocks with ld = k. apply(r, z, scale, n, k, chunks, grid,
// stream) enqueues Z = M^-1 R on such blocks; it is never called without PRE. Both return 0 or 1 (error set). `what` names the caller
// in the gate's message. infos: k structs or NULL.
template <typename T, bool PRE, typename Product, typename Apply>
static int
pcg_tri_solve(const char * what, spmv_mi355x_matrix * A, int k, const void * b_host, void * x_host, const void * scale_host,
		Product product, Apply apply, double tol, long max_iterations, double * history_host, spmv_mi355x_pcg_tri_info * infos)
{
	const auto t_start = std::chrono::steady_clock::now();
	const long n = spmv_mi355x_rows(A);
	const long ld = k;
	hipStream_t stream = nullptr;
	ProgressGate gate;                // outlives buf, whose hipFree waits for the kernels that post to it
	DeviceBuffers buf;
	const size_t nbytes = (size_t) n * (size_t) k * sizeof(T);

	// plain allocations, the product's output included: see solve() in solvers.hip
	T * b, * x, * r, * p, * q, * z = nullptr, * scale = nullptr;
	for (T ** v : {&b, &x, &r, &p, &q})
		ABI_TRY(buf.alloc(v, nbytes));
	if (PRE)
		ABI_TRY(buf.alloc(&z, nbytes));
	if (scale_host)
		ABI_TRY(buf.alloc(&scale, (size_t) n * sizeof(T)));
	double * part, * history = nullptr;
	PcgTriState * st;
	const size_t part_bytes = sizeof(double) * (size_t) k * PCG_TRI_SLOTS * MAX_PART;
	ABI_TRY(buf.alloc(&part, part_bytes));
	ABI_TRY(buf.alloc(&st, 2 * (size_t) k * sizeof(PcgTriState)));
	const size_t hist_bytes = sizeof(double) * (size_t) k * (size_t) max_iterations;
	if (history_host && max_iterations > 0)
	{
		ABI_TRY(buf.alloc(&history, hist_bytes));
		HIP_TRY(hipMemsetAsync(history, 0, hist_bytes, stream));
	}
	ABI_TRY(gate.init());

	HIP_TRY(hipMemcpyAsync(b, b_host, nbytes, hipMemcpyHostToDevice, stream));
	if (scale)
		HIP_TRY(hipMemcpyAsync(scale, scale_host, (size_t) n * sizeof(T), hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemsetAsync(part, 0, part_bytes, stream));

	const int nb = solver_blocks(n);
	const dim3 grid(nb), block(VB), one(1);
	const std::vector<Chunk> chunks = column_chunks(k);
	long spmv_calls = 0;
	auto spmv = [&](const T * in, T * out) {
		spmv_calls++;
		return product(A, k, in, out, stream);
	};
	// the states of the moment are st[s & 1][0 .. k); every transition (the start under a preconditioner, a loop body) reads them,
	// writes the other k and adds 1
	long s = 0;
	auto states = [&](long which) { return st + (which & 1) * (long) k; };
	auto dot = [&](const T * u, const T * v, int slot) {
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_dot_kernel<T, KC>), grid, block, 0, stream, states(s), u, v, n, ld, c0, part, slot);
			return 0;
		});
	};
	// Z = M^-1 R and the partials of r.z
	auto precondition = [&]() {
		ABI_TRY(apply((const T *) r, z, (const T *) scale, n, k, chunks, grid, stream));
		dot(r, z, (int) T_RZ);
		return 0;
	};

	for_chunks(chunks, [&](int c0, auto kc) {
		constexpr int KC = decltype(kc)::value;
		hipLaunchKernelGGL((pcg_tri_start_kernel<T, KC, PRE>), grid, block, 0, stream, b, r, p, x, n, ld, c0, part);
		hipLaunchKernelGGL((pcg_tri_init_state_kernel<KC>), one, block, 0, stream, st, k, c0, nb, part);
		return 0;
	});
	if (PRE)
	{
		ABI_TRY(precondition());
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_begin_kernel<T, KC>), grid, block, 0, stream, states(s), states(s + 1), p, z, n, ld, c0, nb, part);
			return 0;
		});
		s++;
	}
	HIP_TRY(hipGetLastError());

	long it = 0;
	for (; it < max_iterations; it++)
	{
		bool stop;
		ABI_TRY(gate.wait(it, what, stream, &stop));
		if (stop)
			break;
		ABI_TRY(spmv(p, q));
		dot(p, q, (int) T_PQ);
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_update_kernel<T, KC>), grid, block, 0, stream, states(s), x, r, p, q, n, ld, c0, nb, part);
			return 0;
		});
		if (PRE)
			ABI_TRY(precondition());
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_direction_kernel<T, KC, PRE>), grid, block, 0, stream, states(s), states(s + 1), p,
					PRE ? (const T *) z : (const T *) r, n, ld, c0, k, nb, tol, part, history, max_iterations, it, gate.dev);
			return 0;
		});
		s++;
	}
	HIP_TRY(hipGetLastError());

	// the explicit norms of the returned columns, |b - A x| and |x|: one product, q is free now; x stays as it froze
	ABI_TRY(spmv(x, q));
	for_chunks(chunks, [&](int c0, auto kc) {
		constexpr int KC = decltype(kc)::value;
		hipLaunchKernelGGL((pcg_tri_final_kernel<T, KC>), grid, block, 0, stream, b, q, x, n, ld, c0, part);
		return 0;
	});
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(x_host, x, nbytes, hipMemcpyDeviceToHost, stream));
	std::vector<PcgTriState> st_host((size_t) k);
	std::vector<double> part_host((size_t) k * PCG_TRI_SLOTS * MAX_PART);
	HIP_TRY(hipMemcpyAsync(st_host.data(), states(s), (size_t) k * sizeof(PcgTriState), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(part_host.data(), part, part_bytes, hipMemcpyDeviceToHost, stream));
	if (history)
		HIP_TRY(hipMemcpyAsync(history_host, history, hist_bytes, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
	for (int j = 0; infos && j < k; j++)
	{
		auto norm_of = [&](int slot) { return std::sqrt(host_sum(part_host.data(), (size_t) part_at(j, slot), nb)); };
		const PcgTriState & sj = st_host[(size_t) j];
		spmv_mi355x_pcg_tri_info out;
		memset(&out, 0, sizeof(out));
		out.iterations = sj.k;
		out.stop = sj.done ? sj.stop : 2;
		out.rnorm = norm_of(T_ER);
		out.rnorm0 = norm_of(T_BB);
		out.prnorm = std::sqrt(sj.rr);
		out.xnorm = norm_of(T_XX);
		out.spmv_calls = spmv_calls;
		out.seconds = seconds;
		put_info(infos + j, infos[j].struct_size, out);
	}
	return 0;
}

// pcg_tri_solve<T, PRE> by the handle's precision and `pre`
template <typename Product, typename Apply>
static int
pcg_tri_dispatch(const char * what, spmv_mi355x_matrix * A, int k, const void * b_host, void * x_host, bool pre, const void * scale_host,
		Product product, Apply apply, double tol, long max_iterations, double * history_host, spmv_mi355x_pcg_tri_info * infos)
{
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	auto run = [&](auto t, auto with) {
		return pcg_tri_solve<decltype(t), decltype(with)::value>(what, A, k, b_host, x_host, scale_host, product, apply, tol, max_iterations,
				history_host, infos);
	};
	if (spmv_mi355x_precision(A) == SPMV_MI355X_F32)
		return pre ? run(float(), std::true_type()) : run(float(), std::false_type());
	return pre ? run(double(), std::true_type()) : run(double(), std::false_type());
}

// The checks of every entry that need no preconditioner, with the caller's name as the prefix: k < 1 and items 1 to 5 of the header.
// `multi` picks the wording of a _multi entry (infos[j], B, X_out). `tri`: M of pcg_tri_multi has a triangular part, which needs no
// handle to see.
static bool
pcg_tri_arguments_ok(const char * what, bool multi, spmv_mi355x_matrix * A, int k, const void * b_host, void * x_out_host, double tol,
		long max_iterations, const spmv_mi355x_pcg_tri_info * infos, bool tri)
{
	// the checks that need no handle come first, so each can be met (and tested) on its own
	if (k < 1)
	{
		set_error("%s: k = %d: at least one right-hand side is needed", what, k);
		return false;
	}
	for (int j = 0; infos && j < k; j++)
		if (infos[j].struct_size < 8)
		{
			if (multi)
				set_error("%s: infos[%d].struct_size not set", what, j);
			else
				set_error("%s: info->struct_size not set", what);
			return false;
		}
	if (!(tol >= 0) || !std::isfinite(tol))
	{
		set_error("%s: tol must be finite and >= 0 (got %g)", what, tol);
		return false;
	}
	if (max_iterations < 0)
	{
		set_error("%s: max_iterations < 0", what);
		return false;
	}
	if (tri)
	{
		set_error("%s: M has a triangular part (first or second): there is no k-column triangular solve, only M = NULL or a scale alone "
				"is served; solve the columns one by one with spmv_mi355x_pcg_tri", what);
		return false;
	}
	if (!A || !b_host || !x_out_host)
	{
		set_error("%s: NULL argument (%s%s%s )", what, !A ? " A" : "", !b_host ? (multi ? " B" : " b") : "",
				!x_out_host ? (multi ? " X_out" : " x_out") : "");
		return false;
	}
	const long m = spmv_mi355x_rows(A), n = spmv_mi355x_cols(A);
	if (m != n)
	{
		set_error("%s: the matrix must be square and symmetric positive definite: the handle is %ld x %ld (a row block of a "
				"larger matrix is not served)", what, m, n);
		return false;
	}
	return true;
}

// F (not NULL) against the matrix it preconditions: n, precision, device
static bool
pcg_tri_fsai_ok(const char * what, const spmv_mi355x_fsai * F, spmv_mi355x_matrix * A)
{
	const long n = spmv_mi355x_cols(A);
	const int precision = spmv_mi355x_precision(A), device = spmv_mi355x_device(A);
	if (F->n != n)
		set_error("%s: F is a preconditioner of %ld rows, the matrix has %ld", what, F->n, n);
	else if (F->precision != precision)
		set_error("%s: F has precision %d, the matrix %d: both must be the same", what, F->precision, precision);
	else if (F->device != device)
		set_error("%s: F lives on device %d, the matrix on device %d", what, F->device, device);
	else
		return true;
	return false;
}

// M (not NULL) against the matrix it preconditions: n, precision, device, then a failed amg_update_values
static bool
pcg_tri_amg_ok(const char * what, const spmv_mi355x_amg * M, spmv_mi355x_matrix * A)
{
	const long n = spmv_mi355x_cols(A);
	const int precision = spmv_mi355x_precision(A), device = spmv_mi355x_device(A);
	if (M->n != n)
		set_error("%s: M is a preconditioner of %ld rows, the matrix has %ld", what, M->n, n);
	else if (M->precision != precision)
		set_error("%s: M has precision %d, the matrix %d: both must be the same", what, M->precision, precision);
	else if (M->device != device)
		set_error("%s: M lives on device %d, the matrix on device %d", what, M->device, device);
	else if (M->update_failed)
		set_error("%s: the last amg_update_values of M failed below level 0 and left it half rewritten: update it with values it "
				"accepts first", what);
	else
		return true;
	return false;
}

// q = A p of the single entries
struct SpmvProduct {
	int operator()(spmv_mi355x_matrix * A, int, const void * in, void * out, hipStream_t stream) const
	{
		return spmv_mi355x_spmv_device_async(A, in, out, 0, stream);
	}
};

// Q = A P of the _multi entries, for every k
struct SpmmProduct {
	int operator()(spmv_mi355x_matrix * A, int k, const void * in, void * out, hipStream_t stream) const
	{
		return spmv_mi355x_spmm_device_async(A, k, in, k, out, k, 0, stream);
	}
};

// z = M^-1 r of pcg_tri: second^-1 (scale o (first^-1 r)), tri_precond.hpp, on one column
struct TriApply {
	spmv_mi355x_trsv * first, * second;
	template <typename T>
	int operator()(const T * r, T * z, const T * scale, long n, int, const std::vector<Chunk> &, dim3 grid, hipStream_t stream) const
	{
		return tri_precond_enqueue<T>(first, scale, second, r, z, n, false, grid, stream);
	}
};

// Z = scale o R: the Jacobi scale of pcg_tri_multi
struct ScaleApplyMulti {
	template <typename T>
	int operator()(const T * r, T * z, const T * scale, long n, int k, const std::vector<Chunk> & chunks, dim3 grid, hipStream_t stream) const
	{
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_scale_multi_kernel<T, KC>), grid, dim3(VB), 0, stream, scale, r, z, n, (long) k, c0);
			return 0;
		});
		return 0;
	}
};

// Z = second^-1 (scale o (first^-1 R)) of pcg_trsm_multi: the three parts of tri_precond.hpp on the n x k block, the triangular ones
// as k-column solves. They know nothing of `done` and write only Z.
struct TriApplyMulti {
	spmv_mi355x_trsv * first, * second;
	template <typename T>
	int operator()(const T * r, T * z, const T * scale, long n, int k, const std::vector<Chunk> & chunks, dim3 grid, hipStream_t stream) const
	{
		return tri_precond_enqueue_multi<T>(first, scale, second, r, z, n, k, chunks, grid, stream);
	}
};

// z = G^t (G r) of pcg_fsai. The two SpMVs write the handle's scratch vector and z, nothing else.
struct FsaiApply {
	spmv_mi355x_fsai * F;
	template <typename T>
	int operator()(const T * r, T * z, const T *, long, int, const std::vector<Chunk> &, dim3, hipStream_t stream) const
	{
		return spmv_mi355x_fsai_apply_device_async(F, r, z, stream);
	}
};

// Z = G^t (G R) of pcg_fsai_multi: the two SpMMs write the fsai handle's scratch block and z
struct FsaiApplyMulti {
	spmv_mi355x_fsai * F;
	template <typename T>
	int operator()(const T * r, T * z, const T *, long, int k, const std::vector<Chunk> &, dim3, hipStream_t stream) const
	{
		return spmv_mi355x_fsai_apply_multi_device_async(F, k, r, k, z, k, stream);
	}
};

// z = M^-1 r of pcg_amg: one V cycle of an amg handle. Its SpMVs and vector kernels write the hierarchy's own vectors and z, nothing else.
struct AmgApply {
	spmv_mi355x_amg * M;
	template <typename T>
	int operator()(const T * r, T * z, const T *, long, int, const std::vector<Chunk> &, dim3, hipStream_t stream) const
	{
		return spmv_mi355x_amg_apply_device_async(M, r, z, stream);
	}
};

// one V cycle for the k columns of pcg_amg_multi: it writes the hierarchy's own blocks and z
struct AmgApplyMulti {
	spmv_mi355x_amg * M;
	template <typename T>
	int operator()(const T * r, T * z, const T *, long, int k, const std::vector<Chunk> &, dim3, hipStream_t stream) const
	{
		return spmv_mi355x_amg_apply_multi_device_async(M, k, r, k, z, k, stream);
	}
};

}  // namespace spmv

extern "C" int
spmv_mi355x_pcg_tri(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, const spmv_mi355x_tri_precond * M, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * info)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_tri", false, A, 1, b_host, x_out_host, tol, max_iterations, info, false))
		return 1;
	if (M && (!tri_precond_size_ok("pcg_tri", M)
			|| !tri_precond_parts_ok("pcg_tri", M, spmv_mi355x_cols(A), spmv_mi355x_precision(A), spmv_mi355x_device(A))))
		return 1;
	const TriApply apply = {M ? M->first : nullptr, M ? M->second : nullptr};
	const void * scale = M ? M->scale_host : nullptr;
	return pcg_tri_dispatch("pcg_tri", A, 1, b_host, x_out_host, apply.first || scale || apply.second, scale, SpmvProduct(), apply, tol,
			max_iterations, history_out, info);
}

extern "C" int
spmv_mi355x_pcg_fsai(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, spmv_mi355x_fsai * F, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * info)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_fsai", false, A, 1, b_host, x_out_host, tol, max_iterations, info, false))
		return 1;
	if (!F)
	{
		set_error("pcg_fsai: F is NULL: spmv_mi355x_pcg_tri with M = NULL is the solve without a preconditioner");
		return 1;
	}
	if (!pcg_tri_fsai_ok("pcg_fsai", F, A))
		return 1;
	return pcg_tri_dispatch("pcg_fsai", A, 1, b_host, x_out_host, true, nullptr, SpmvProduct(), FsaiApply{F}, tol, max_iterations,
			history_out, info);
}

extern "C" int
spmv_mi355x_pcg_amg(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, spmv_mi355x_amg * M, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * info)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_amg", false, A, 1, b_host, x_out_host, tol, max_iterations, info, false))
		return 1;
	if (!M)
	{
		set_error("pcg_amg: M is NULL: spmv_mi355x_pcg_tri with M = NULL is the solve without a preconditioner");
		return 1;
	}
	if (!pcg_tri_amg_ok("pcg_amg", M, A))
		return 1;
	return pcg_tri_dispatch("pcg_amg", A, 1, b_host, x_out_host, true, nullptr, SpmvProduct(), AmgApply{M}, tol, max_iterations,
			history_out, info);
}

extern "C" int
spmv_mi355x_pcg_tri_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, const spmv_mi355x_tri_precond * M,
		double tol, long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos)
{
	using namespace spmv;
	const bool sized = M && M->struct_size >= sizeof(spmv_mi355x_tri_precond);
	if (!pcg_tri_arguments_ok("pcg_tri_multi", true, A, k, B_host, X_out_host, tol, max_iterations, infos,
			sized && (M->first || M->second)))
		return 1;
	if (M && (!tri_precond_size_ok("pcg_tri_multi", M)
			|| !tri_precond_parts_ok("pcg_tri_multi", M, spmv_mi355x_cols(A), spmv_mi355x_precision(A), spmv_mi355x_device(A))))
		return 1;
	const void * scale = M ? M->scale_host : nullptr;
	return pcg_tri_dispatch("pcg_tri_multi", A, k, B_host, X_out_host, scale != nullptr, scale, SpmmProduct(), ScaleApplyMulti(), tol,
			max_iterations, history_out, infos);
}

// pcg_tri_multi without its refusal: any M, the triangular parts through the k-column solve. With M = NULL or a scale alone the
// launches are those of pcg_tri_multi (TriApplyMulti then enqueues the scale kernel of ScaleApplyMulti and nothing else).
extern "C" int
spmv_mi355x_pcg_trsm_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, const spmv_mi355x_tri_precond * M,
		double tol, long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_trsm_multi", true, A, k, B_host, X_out_host, tol, max_iterations, infos, false))
		return 1;
	if (M && (!tri_precond_size_ok("pcg_trsm_multi", M)
			|| !tri_precond_parts_ok("pcg_trsm_multi", M, spmv_mi355x_cols(A), spmv_mi355x_precision(A), spmv_mi355x_device(A))))
		return 1;
	const TriApplyMulti apply = {M ? M->first : nullptr, M ? M->second : nullptr};
	const void * scale = M ? M->scale_host : nullptr;
	return pcg_tri_dispatch("pcg_trsm_multi", A, k, B_host, X_out_host, apply.first || scale || apply.second, scale, SpmmProduct(), apply,
			tol, max_iterations, history_out, infos);
}

extern "C" int
spmv_mi355x_pcg_fsai_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, spmv_mi355x_fsai * F, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_fsai_multi", true, A, k, B_host, X_out_host, tol, max_iterations, infos, false))
		return 1;
	if (!F)
	{
		set_error("pcg_fsai_multi: F is NULL: spmv_mi355x_pcg_tri_multi with M = NULL is the solve without a preconditioner");
		return 1;
	}
	if (!pcg_tri_fsai_ok("pcg_fsai_multi", F, A))
		return 1;
	return pcg_tri_dispatch("pcg_fsai_multi", A, k, B_host, X_out_host, true, nullptr, SpmmProduct(), FsaiApplyMulti{F}, tol,
			max_iterations, history_out, infos);
}

extern "C" int
spmv_mi355x_pcg_amg_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, spmv_mi355x_amg * M, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos)
{
	using namespace spmv;
	if (!pcg_tri_arguments_ok("pcg_amg_multi", true, A, k, B_host, X_out_host, tol, max_iterations, infos, false))
		return 1;
	if (!M)
	{
		set_error("pcg_amg_multi: M is NULL: spmv_mi355x_pcg_tri_multi with M = NULL is the solve without a preconditioner");
		return 1;
	}
	if (!pcg_tri_amg_ok("pcg_amg_multi", M, A))
		return 1;
	return pcg_tri_dispatch("pcg_amg_multi", A, k, B_host, X_out_host, true, nullptr, SpmmProduct(), AmgApplyMulti{M}, tol,
			max_iterations, history_out, infos);
}

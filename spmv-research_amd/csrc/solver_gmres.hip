// Device-resident restarted GMRES(m): A x = b from x0 = 0 for a square matrix, symmetric or not, over one handle of A, with an
// optional diagonal RIGHT preconditioner given as its inverse: GMRES runs on A diag(minv) and x = diag(minv) u is returned, so
// the residual it minimises is the true |b - A x|.
//
// The recurrences, every scalar and every dot fp64, vectors in the handle's precision (M v = minv v, or v without minv):
//   x = 0; beta0 = |b|                                                            (0: stop 3; not finite: stop 4)
//   r = b; beta = beta0
//   cycle:  v_0 = r / beta; g = (beta, 0, ..., 0); j = 0
//     step, while j < m and it < max_iterations:
//       w = A M v_j;  h = 0
//       twice (CGS2):  c_i = v_i.w for i <= j, all from the same w;  w -= c_0 v_0, ..., w -= c_j v_j in that order;  h_i += c_i
//       hn = h_{j+1} = |w|
//       for i < j:  (h_i, h_{i+1}) = (cs_i h_i + sn_i h_{i+1}, -sn_i h_i + cs_i h_{i+1})
//       rho = hypot(h_j, h_{j+1})                                (not finite or 0: stop 4, the column is dropped: j, it, x as before it)
//       cs_j = h_j / rho; sn_j = h_{j+1} / rho; h_j = rho; R[0..j, j] = h[0..j]
//       g_{j+1} = -sn_j g_j;  g_j = cs_j g_j;  it += 1;  j += 1;  history[it - 1] = |g_j|
//       if tol > 0 and |g_j| <= tol beta0: stop 1;  else if hn == 0: stop 5;  else v_j = w / hn
//     cycle end:  R[0..j, 0..j] y = g[0..j] by back substitution;  u = y_0 v_0 + ... + y_{j-1} v_{j-1} in that order;  x += M u
//     if stopped or it >= max_iterations: leave
//     r = b - A x; beta = |r|; restarts += 1                                        (not finite: stop 4; 0: stop 5)
//
// Built like solver_minres.hip: the state ping-pongs between two slots, one per transition (an inner step or a restart), dots are
// two-stage and deterministic, a device `done` flag predicates every later step kernel off, and the host loop is ProgressGate of
// solvers_common.hpp with `it` counting inner steps. The host knows j = it % m and passes the basis pointers.
// Per inner step: 1 SpMV + 6 launches
//   w = A (z or v_j) | gmres_dots (partials of v_i.w, i <= j) | gmres_reduce (c1_i) | gmres_update (w -= sum c1_i v_i, partials of
//   v_i.w') | gmres_reduce (c2_i) | gmres_update (w -= sum c2_i v_i, partial of |w|^2) | gmres_finish (v_{j+1}, z, rotations, state).
// gmres_reduce runs one block per slot: the consumers read j + 1 finished numbers instead of re-reducing (j + 1) nb partials each.
// Only gmres_finish re-reduces in every block, MINRES's pattern, and that is one slot.
// Stored: the basis, (m + 1) n values with stride n; w, x, b; with minv also minv and z = minv v_j, the SpMV's input. In fp64: R
// (m x m, column major), cs, sn, g, y, c1, c2 and (m + 4) MAX_PART partials.
//
// THE HOT LOOP. The dots take the basis TILE vectors at a time with TILE statically indexed accumulators (a per-thread array indexed
// at run time would live in scratch); the subtraction needs no array at all, it is a chain on one register. A thread meets the same
// elements in both halves of gmres_update, so the dots of the second pass read the w it has just written and no grid-wide
// synchronisation is needed; the basis is read once for the subtraction and once more for those dots.
//
// THE FREEZE. state.pend counts the columns of the running cycle that x does not hold yet. A cycle end (gmres_solve_y, gmres_apply)
// acts on the columns pending in the state and clears the count; it is not predicated on `done`. The host enqueues one after step
// m - 1 of every cycle and one more after the loop: whichever comes first after a stop or at max_iterations applies the partial
// cycle, every later one finds nothing pending. A restart (SpMV, gmres_residual, gmres_restart) is predicated on `done`.
//
// THE TRIANGULAR PRECONDITIONER (spmv_mi355x_gmres_tri, MODE = GMRES_TRI). M v = second^-1 (scale o (first^-1 v)), each part
// optional, the two solves being spmv_mi355x_trsv handles of any kind. The finish and restart kernels write v only, as without a
// preconditioner; behind them the host enqueues on the same stream (tri_precond.hpp, shared with solver_pcg_tri.hip): first
// (v -> z), tri_scale_kernel on z, second in place on z, and then the SpMV of z. At a cycle end gmres_combine_kernel writes u to z, the same steps run on it and gmres_add_kernel does
// x += z; when the scale is the last part (no second) it is multiplied in there, the form the minv path has, which also keeps
// precond = (NULL, s, NULL) bit for bit the solve with minv = s.
// Why the freeze survives: the triangular solves and the scale kernel know nothing of `done` and run however far the host is ahead,
// but everything they write is z, scratch that only the next SpMV or gmres_add_kernel reads. x, the basis and the state are written
// only by kernels that honour `done` or the pending count: gmres_add_kernel adds nothing when napply is 0, so the pending cycle
// is applied exactly once here too.
//
// DEVIATION worth knowing: gmres_finish writes v_{j+1} (and z) in every block whenever hn is finite and > 0, also in a step whose
// verdict, reached by block 0 alone after the serial rotation chain, is stop 1 or 4. Nothing reads that vector after a stop.

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "solvers_common.hpp"
#include "tri_precond.hpp"
#include "trsv.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

constexpr int GMRES_MAX_RESTART = 128;
constexpr int GMRES_TILE = 8;         // basis vectors per pass of the dots: 16 accumulator VGPRs in fp64
enum { GMRES_PLAIN = 0, GMRES_MINV = 1, GMRES_TRI = 2 };     // M of "M v": none, a diagonal, triangular solves

struct GmresState {
	double beta0;                 // |b|
	double gres;                  // |g_{j+1}|: the recursive residual
	long k;                       // completed inner steps
	long restarts;
	int pend;                     // columns of the running cycle not yet applied to x (= j while the solve runs)
	int done;                     // a stop rule fired: every later step and restart kernel is predicated off
	int stop;                     // 0 while running, else 1 / 3 / 4 / 5 of spmv_mi355x_gmres_info.stop (2 is the host's: never done)
	int pad;
};

// slots of the partials: 0 .. m - 1 are v_i.w, then these
enum { G_NRM = 0, G_BB, G_RR, G_XX, GMRES_EXTRA_SLOTS };

// partial BB = b.b; v_0 = b (gmres_restart scales it)
template <typename T>
__global__ __launch_bounds__(VB) void
gmres_start_kernel(const T * __restrict__ b, T * __restrict__ v0, long n, double * __restrict__ part, int slot)
{
	double bb = 0;
	GRID_STRIDE(i, n)
	{
		const T bi = b[i];
		v0[i] = bi;
		bb += (double) bi * (double) bi;
	}
	store_partial(part, slot, bb);
}

// Partials of v_{t0 + k}.w for k < cnt <= TILE into slots t0 + k. The accumulators are indexed by the unrolled k only.
template <typename T>
__device__ __forceinline__ void
gmres_tile_dots(const T * __restrict__ V, const T * w, long n, int t0, int cnt, double * __restrict__ part)
{
	double acc[GMRES_TILE];
	#pragma unroll
	for (int k = 0; k < GMRES_TILE; k++)
		acc[k] = 0;
	const T * v = V + (long) t0 * n;
	if (cnt == GMRES_TILE)
	{
		GRID_STRIDE(e, n)
		{
			const double we = (double) w[e];
			#pragma unroll
			for (int k = 0; k < GMRES_TILE; k++)
				acc[k] += (double) v[(long) k * n + e] * we;
		}
	}
	else
	{
		GRID_STRIDE(e, n)
		{
			const double we = (double) w[e];
			#pragma unroll
			for (int k = 0; k < GMRES_TILE; k++)
				if (k < cnt)
					acc[k] += (double) v[(long) k * n + e] * we;
		}
	}
	#pragma unroll
	for (int k = 0; k < GMRES_TILE; k++)
		if (k < cnt)
			store_partial(part, t0 + k, acc[k]);
}

// partials of v_i.w for i < cnt in one launch
template <typename T>
__global__ __launch_bounds__(VB) void
gmres_dots_kernel(const GmresState * __restrict__ st_p, const T * __restrict__ V, const T * __restrict__ w, long n, int cnt,
		double * __restrict__ part)
{
	if (st_p->done)
		return;
	for (int t0 = 0; t0 < cnt; t0 += GMRES_TILE)
		gmres_tile_dots(V, w, n, t0, min(GMRES_TILE, cnt - t0), part);
}

// grid = the slots: block i sums the nb partials of slot i in the order every reduction here uses
__global__ __launch_bounds__(VB) void
gmres_reduce_kernel(const GmresState * __restrict__ st_p, const double * __restrict__ part, int nb, double * __restrict__ c)
{
	if (st_p->done)
		return;
	const double v = sum_partials(part, blockIdx.x, nb);
	if (threadIdx.x == 0)
		c[blockIdx.x] = v;
}

// w -= c_0 v_0, ..., w -= c_{cnt-1} v_{cnt-1}; then the partials of v_i.w for the second pass, or (LAST) the partial of |w|^2
template <typename T, bool LAST>
__global__ __launch_bounds__(VB) void
gmres_update_kernel(const GmresState * __restrict__ st_p, const T * __restrict__ V, T * w, long n, int cnt,
		const double * __restrict__ c, double * __restrict__ part, int slot_nrm)
{
	if (st_p->done)
		return;
	double nrm = 0;
	GRID_STRIDE(e, n)
	{
		T we = w[e];
		const T * v = V + e;
		#pragma unroll 4
		for (int i = 0; i < cnt; i++)
			we -= (T) c[i] * v[(long) i * n];
		w[e] = we;
		if (LAST)
			nrm += (double) we * (double) we;
	}
	if (LAST)
		store_partial(part, slot_nrm, nrm);
	else
		for (int t0 = 0; t0 < cnt; t0 += GMRES_TILE)
			gmres_tile_dots(V, w, n, t0, min(GMRES_TILE, cnt - t0), part);
}

// hn = |w| identically in every block; v_{j+1} = w / hn and z = minv v_{j+1} when hn is finite and > 0. Block 0: h = c1 + c2, the j
// stored rotations, the new one, g, the history row, the verdict, the next state and the progress word.
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
gmres_finish_kernel(const GmresState * __restrict__ st_p, GmresState * __restrict__ st_next, T * __restrict__ v_next,
		T * __restrict__ z, const T * __restrict__ w, const T * __restrict__ minv, long n, int nb, int j, int m,
		const double * __restrict__ c1, const double * __restrict__ c2, double * __restrict__ R, double * __restrict__ cs,
		double * __restrict__ sn, double * __restrict__ g, double tol, const double * __restrict__ part, int slot_nrm,
		double * __restrict__ history, long it, volatile long * host_progress)
{
	const GmresState st = *st_p;
	if (st.done)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			*st_next = st;
			post_progress(host_progress, it + 1, st.k);
		}
		return;
	}
	const double hn = sqrt(sum_partials(part, slot_nrm, nb));
	if (hn > 0 && hn < INFINITY)
	{
		const T inv = (T) (1.0 / hn);
		GRID_STRIDE(e, n)
		{
			const T ve = inv * w[e];
			v_next[e] = ve;
			if (PRE)
				z[e] = minv[e] * ve;
		}
	}
	if (blockIdx.x != 0 || threadIdx.x != 0)
		return;
	GmresState nx = st;
	double * col = R + (long) j * m;
	double hj = c1[0] + c2[0];
	for (int i = 0; i < j; i++)
	{
		const double hi1 = c1[i + 1] + c2[i + 1];
		col[i] = cs[i] * hj + sn[i] * hi1;
		hj = -sn[i] * hj + cs[i] * hi1;
	}
	const double rho = hypot(hj, hn);
	if (!(rho > 0) || !(rho < INFINITY))
	{
		nx.done = 1;                              // k, pend and x of the last good step
		nx.stop = 4;
		*st_next = nx;
		post_progress(host_progress, it + 1, nx.k);
		return;
	}
	const double c = hj / rho, s = hn / rho, gj = g[j];
	cs[j] = c;
	sn[j] = s;
	col[j] = rho;
	g[j + 1] = -s * gj;
	g[j] = c * gj;
	nx.gres = fabs(s * gj);
	nx.k = st.k + 1;
	nx.pend = j + 1;
	if (history)
		history[st.k] = nx.gres;
	if (tol > 0 && nx.gres <= tol * st.beta0)
		nx.stop = 1;
	else if (hn == 0)
		nx.stop = 5;
	nx.done = nx.stop != 0;
	*st_next = nx;
	post_progress(host_progress, it + 1, nx.done ? nx.k : -1);
}

// 1 block, the state in place. p = the pending columns: R[0..p, 0..p] y = g[0..p], column by column from the last, g in LDS.
// napply = p for gmres_apply and pend = 0: the next cycle end finds nothing.
__global__ __launch_bounds__(VB) void
gmres_solve_y_kernel(GmresState * __restrict__ st_p, const double * __restrict__ R, const double * __restrict__ g, int m,
		double * __restrict__ y, int * __restrict__ napply)
{
	__shared__ double rhs[GMRES_MAX_RESTART];
	__shared__ double yi_sh;
	const int p = st_p->pend;
	const int t = threadIdx.x;
	if (t < p)
		rhs[t] = g[t];
	__syncthreads();
	for (int i = p - 1; i >= 0; i--)
	{
		const double * col = R + (long) i * m;
		if (t == 0)
		{
			yi_sh = rhs[i] / col[i];
			y[i] = yi_sh;
		}
		__syncthreads();
		if (t < i)
			rhs[t] -= col[t] * yi_sh;
		__syncthreads();
	}
	if (t == 0)
	{
		*napply = p;
		st_p->pend = 0;
	}
}

// x += minv (y_0 v_0 + ... + y_{p-1} v_{p-1}), p = napply
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
gmres_apply_kernel(const int * __restrict__ napply, const T * __restrict__ V, const double * __restrict__ y,
		const T * __restrict__ minv, T * __restrict__ x, long n)
{
	const int p = *napply;
	if (p == 0)
		return;
	GRID_STRIDE(e, n)
	{
		T u = 0;
		const T * v = V + e;
		#pragma unroll 4
		for (int i = 0; i < p; i++)
			u += (T) y[i] * v[(long) i * n];
		x[e] = x[e] + (PRE ? minv[e] * u : u);
	}
}

// GMRES_TRI: u = y_0 v_0 + ... + y_{p-1} v_{p-1}, p = napply, into the scratch vector
template <typename T>
__global__ __launch_bounds__(VB) void
gmres_combine_kernel(const int * __restrict__ napply, const T * __restrict__ V, const double * __restrict__ y, T * __restrict__ u_out,
		long n)
{
	const int p = *napply;
	if (p == 0)
		return;
	GRID_STRIDE(e, n)
	{
		T u = 0;
		const T * v = V + e;
		#pragma unroll 4
		for (int i = 0; i < p; i++)
			u += (T) y[i] * v[(long) i * n];
		u_out[e] = u;
	}
}

// GMRES_TRI: x += z, or x += scale o z when the scale is the last part of M; nothing when no column was pending
template <typename T, bool SCALE>
__global__ __launch_bounds__(VB) void
gmres_add_kernel(const int * __restrict__ napply, const T * __restrict__ z, const T * __restrict__ scale, T * __restrict__ x, long n)
{
	if (*napply == 0)
		return;
	GRID_STRIDE(e, n)
	{
		const T u = z[e];
		x[e] = x[e] + (SCALE ? scale[e] * u : u);
	}
}

// r = b - q (q = A x) into v_0; partial of |r|^2
template <typename T>
__global__ __launch_bounds__(VB) void
gmres_residual_kernel(const GmresState * __restrict__ st_p, const T * __restrict__ b, const T * __restrict__ q,
		T * __restrict__ v0, long n, double * __restrict__ part, int slot)
{
	if (st_p->done)
		return;
	double rr = 0;
	GRID_STRIDE(i, n)
	{
		const T ri = b[i] - q[i];
		v0[i] = ri;
		rr += (double) ri * (double) ri;
	}
	store_partial(part, slot, rr);
}

// beta = sqrt(slot) identically in every block; v_0 /= beta and z = minv v_0 when beta is finite and > 0. Block 0: g_0 = beta and the
// next state. first: the start of the solve (beta0, stop 3 for b == 0); else a restart (restarts + 1, stop 5 for r == 0).
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
gmres_restart_kernel(const GmresState * __restrict__ st_p, GmresState * __restrict__ st_next, T * __restrict__ v0,
		T * __restrict__ z, const T * __restrict__ minv, long n, int nb, const double * __restrict__ part, int slot, int first,
		double * __restrict__ g)
{
	const GmresState st = *st_p;
	if (st.done)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
			*st_next = st;
		return;
	}
	const double beta = sqrt(sum_partials(part, slot, nb));
	const bool ok = beta > 0 && beta < INFINITY;
	if (ok)
	{
		const T inv = (T) (1.0 / beta);
		GRID_STRIDE(e, n)
		{
			const T ve = inv * v0[e];
			v0[e] = ve;
			if (PRE)
				z[e] = minv[e] * ve;
		}
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		GmresState nx = st;
		if (first)
			nx.beta0 = beta;
		else
			nx.restarts = st.restarts + 1;
		nx.gres = beta;
		nx.pend = 0;
		nx.stop = ok ? 0 : beta == 0 ? (first ? 3 : 5) : 4;
		nx.done = nx.stop != 0;
		g[0] = beta;
		*st_next = nx;
	}
}

// the tail's explicit residual: q = b - q (q = A x); partials RR = |b - A x|^2 and XX = |x|^2
template <typename T>
__global__ __launch_bounds__(VB) void
gmres_final_kernel(const T * __restrict__ b, T * __restrict__ q, const T * __restrict__ x, long n, double * __restrict__ part,
		int slot_rr, int slot_xx)
{
	double rr = 0, xx = 0;
	GRID_STRIDE(i, n)
	{
		const T xi = x[i];
		const T ri = b[i] - q[i];
		q[i] = ri;
		rr += (double) ri * (double) ri;
		xx += (double) xi * (double) xi;
	}
	store_partial(part, slot_rr, rr);
	store_partial(part, slot_xx, xx);
}

// ------------------------------------------------------------------------------------------------ host side

// minv_host: the inverse diagonal under GMRES_MINV, the scale of M (or NULL) under GMRES_TRI
template <typename T, int MODE>
static int
gmres_solve(spmv_mi355x_matrix * A, const void * b_host, void * x_host, int m, const void * minv_host, double tol,
		long max_iterations, double * history_host, spmv_mi355x_gmres_info * info, spmv_mi355x_trsv * first = nullptr,
		spmv_mi355x_trsv * second = nullptr)
{
	constexpr bool PRE = MODE == GMRES_MINV;      // what the fused kernels see: under GMRES_TRI they write v only
	constexpr bool TRI = MODE == GMRES_TRI;
	const auto t_start = std::chrono::steady_clock::now();
	const long n = spmv_mi355x_rows(A);
	hipStream_t stream = nullptr;
	ProgressGate gate;                // outlives buf, whose hipFree waits for the kernels that post to it
	DeviceBuffers buf;
	const size_t nbytes = (size_t) n * sizeof(T);

	// plain allocations, the SpMV output included: see solve() in solvers.hip
	T * b, * x, * w, * V, * z = nullptr, * minv = nullptr;
	for (T ** p : {&b, &x, &w})
		ABI_TRY(buf.alloc(p, nbytes));
	ABI_TRY(buf.alloc(&V, nbytes * (size_t) (m + 1)));
	if (PRE || TRI)
		ABI_TRY(buf.alloc(&z, nbytes));
	if (PRE || (TRI && minv_host))
		ABI_TRY(buf.alloc(&minv, nbytes));
	// one fp64 block: R (m * m), cs, sn (m each), g (m + 1), y, c1, c2 (m each)
	const size_t small_count = (size_t) m * m + 6 * (size_t) m + 1;
	double * small, * part, * history = nullptr;
	GmresState * st;
	int * napply;
	ABI_TRY(buf.alloc(&small, sizeof(double) * small_count));
	double * R = small, * cs = R + (size_t) m * m, * sn = cs + m, * g = sn + m, * y = g + m + 1, * c1 = y + m, * c2 = c1 + m;
	const int slots = m + GMRES_EXTRA_SLOTS, s_nrm = m + G_NRM, s_bb = m + G_BB, s_rr = m + G_RR, s_xx = m + G_XX;
	const size_t part_bytes = sizeof(double) * (size_t) slots * MAX_PART;
	ABI_TRY(buf.alloc(&part, part_bytes));
	ABI_TRY(buf.alloc(&st, 2 * sizeof(GmresState)));
	ABI_TRY(buf.alloc(&napply, sizeof(int)));
	const size_t hist_bytes = sizeof(double) * (size_t) max_iterations;
	if (history_host && max_iterations > 0)
	{
		ABI_TRY(buf.alloc(&history, hist_bytes));
		HIP_TRY(hipMemsetAsync(history, 0, hist_bytes, stream));
	}
	ABI_TRY(gate.init());

	HIP_TRY(hipMemcpyAsync(b, b_host, nbytes, hipMemcpyHostToDevice, stream));
	if (minv)
		HIP_TRY(hipMemcpyAsync(minv, minv_host, nbytes, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemsetAsync(part, 0, part_bytes, stream));
	HIP_TRY(hipMemsetAsync(small, 0, sizeof(double) * small_count, stream));
	HIP_TRY(hipMemsetAsync(st, 0, 2 * sizeof(GmresState), stream));
	HIP_TRY(hipMemsetAsync(napply, 0, sizeof(int), stream));
	HIP_TRY(hipMemsetAsync(x, 0, nbytes ? nbytes : 8, stream));

	const int nb = solver_blocks(n);
	const dim3 grid(nb), block(VB), one(1);
	long spmv_calls = 0;
	auto spmv = [&](const T * in, T * out) {
		spmv_calls++;
		return spmv_mi355x_spmv_device_async(A, in, out, 0, stream);
	};
	// the state of the moment is st[s & 1]; every transition (an inner step, a restart) reads it, writes the other slot and adds 1
	long s = 0;
	// GMRES_TRI: z = M in, part by part; `in` may be z. With defer_scale a scale that is M's last part is left to the caller.
	auto precond = [&](const T * in, bool defer_scale) {
		return tri_precond_enqueue<T>(first, minv, second, in, z, n, defer_scale, grid, stream);
	};
	auto cycle_end = [&]() {
		hipLaunchKernelGGL(gmres_solve_y_kernel, one, block, 0, stream, st + (s & 1), R, g, m, y, napply);
		if (!TRI)
		{
			hipLaunchKernelGGL((gmres_apply_kernel<T, PRE>), grid, block, 0, stream, napply, V, y, minv, x, n);
			return 0;
		}
		hipLaunchKernelGGL((gmres_combine_kernel<T>), grid, block, 0, stream, napply, V, y, z, n);
		ABI_TRY(precond(z, true));
		if (minv && !second)
			hipLaunchKernelGGL((gmres_add_kernel<T, true>), grid, block, 0, stream, napply, z, minv, x, n);
		else
			hipLaunchKernelGGL((gmres_add_kernel<T, false>), grid, block, 0, stream, napply, z, minv, x, n);
		return 0;
	};

	hipLaunchKernelGGL((gmres_start_kernel<T>), grid, block, 0, stream, b, V, n, part, s_bb);
	hipLaunchKernelGGL((gmres_restart_kernel<T, PRE>), grid, block, 0, stream, st + (s & 1), st + ((s + 1) & 1), V, z, minv, n, nb,
			part, s_bb, 1, g);
	s++;
	if (TRI)
		ABI_TRY(precond(V, false));
	HIP_TRY(hipGetLastError());

	long it = 0;
	for (; it < max_iterations; it++)
	{
		bool stop;
		ABI_TRY(gate.wait(it, "gmres", stream, &stop));
		if (stop)
			break;
		const int j = (int) (it % m);
		GmresState * cur = st + (s & 1), * nxt = st + ((s + 1) & 1);
		ABI_TRY(spmv(PRE || TRI ? z : V + (size_t) j * n, w));
		hipLaunchKernelGGL((gmres_dots_kernel<T>), grid, block, 0, stream, cur, V, w, n, j + 1, part);
		hipLaunchKernelGGL(gmres_reduce_kernel, dim3(j + 1), block, 0, stream, cur, part, nb, c1);
		hipLaunchKernelGGL((gmres_update_kernel<T, false>), grid, block, 0, stream, cur, V, w, n, j + 1, c1, part, s_nrm);
		hipLaunchKernelGGL(gmres_reduce_kernel, dim3(j + 1), block, 0, stream, cur, part, nb, c2);
		hipLaunchKernelGGL((gmres_update_kernel<T, true>), grid, block, 0, stream, cur, V, w, n, j + 1, c2, part, s_nrm);
		hipLaunchKernelGGL((gmres_finish_kernel<T, PRE>), grid, block, 0, stream, cur, nxt, V + (size_t) (j + 1) * n, z, w, minv, n,
				nb, j, m, c1, c2, R, cs, sn, g, tol, part, s_nrm, history, it, gate.dev);
		s++;
		if (TRI && j < m - 1)
			ABI_TRY(precond(V + (size_t) (j + 1) * n, false));
		if (j == m - 1)
		{
			ABI_TRY(cycle_end());
			if (it + 1 < max_iterations)
			{
				cur = st + (s & 1), nxt = st + ((s + 1) & 1);
				ABI_TRY(spmv(x, w));
				hipLaunchKernelGGL((gmres_residual_kernel<T>), grid, block, 0, stream, cur, b, w, V, n, part, s_rr);
				hipLaunchKernelGGL((gmres_restart_kernel<T, PRE>), grid, block, 0, stream, cur, nxt, V, z, minv, n, nb, part, s_rr, 0, g);
				s++;
				if (TRI)
					ABI_TRY(precond(V, false));
			}
		}
	}
	ABI_TRY(cycle_end());             // the partial cycle of a stop or of max_iterations, if no cycle end above has met it
	HIP_TRY(hipGetLastError());

	// the explicit norms of the returned x: |b - A x| and |x|. w is free now; x stays as it froze.
	GmresState * fin = st + (s & 1);
	ABI_TRY(spmv(x, w));
	hipLaunchKernelGGL((gmres_final_kernel<T>), grid, block, 0, stream, b, w, x, n, part, s_rr, s_xx);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(x_host, x, nbytes, hipMemcpyDeviceToHost, stream));
	GmresState st_host;
	std::vector<double> part_host((size_t) GMRES_EXTRA_SLOTS * MAX_PART);
	HIP_TRY(hipMemcpyAsync(&st_host, fin, sizeof(GmresState), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(part_host.data(), part + (size_t) m * MAX_PART, sizeof(double) * GMRES_EXTRA_SLOTS * MAX_PART,
			hipMemcpyDeviceToHost, stream));
	if (history)
		HIP_TRY(hipMemcpyAsync(history_host, history, hist_bytes, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	if (info)
	{
		auto norm_of = [&](int slot) { return std::sqrt(host_sum(part_host.data(), (size_t) slot * MAX_PART, nb)); };
		spmv_mi355x_gmres_info out;
		memset(&out, 0, sizeof(out));
		out.iterations = st_host.k;
		out.stop = st_host.done ? st_host.stop : 2;
		out.restarts = st_host.restarts;
		out.rnorm = norm_of(G_RR);
		out.rnorm0 = norm_of(G_BB);
		out.prnorm = st_host.gres;
		out.xnorm = norm_of(G_XX);
		out.spmv_calls = spmv_calls;
		out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
		put_info(info, info->struct_size, out);
	}
	return 0;
}

// the first entry of minv that is not finite or not > 0, or -1
template <typename T>
static long
gmres_bad_minv(const void * minv_host, long n)
{
	const T * d = (const T *) minv_host;
	for (long i = 0; i < n; i++)
		if (!(d[i] > 0) || !std::isfinite(d[i]))
			return i;
	return -1;
}

// what both entries check first, in the order of the header: the scalars, the NULL pointers, the shape
static int
gmres_check_common(const char * what, spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, int restart, double tol,
		long max_iterations, spmv_mi355x_gmres_info * info)
{
	// the checks that need no handle come first, so each can be met (and tested) on its own
	if (!info_size_ok(what, info))
		return 1;
	if (restart < 1 || restart > GMRES_MAX_RESTART)
	{
		set_error("%s: restart must be 1 .. %d (got %d)", what, GMRES_MAX_RESTART, restart);
		return 1;
	}
	if (!(tol >= 0) || !std::isfinite(tol))
	{
		set_error("%s: tol must be finite and >= 0 (got %g)", what, tol);
		return 1;
	}
	if (max_iterations < 0)
	{
		set_error("%s: max_iterations < 0", what);
		return 1;
	}
	if (!A || !b_host || !x_out_host)
	{
		set_error("%s: NULL argument (%s%s%s )", what, !A ? " A" : "", !b_host ? " b" : "", !x_out_host ? " x_out" : "");
		return 1;
	}
	const long m = spmv_mi355x_rows(A), n = spmv_mi355x_cols(A);
	if (m != n)
	{
		set_error("%s: the matrix must be square: the handle is %ld x %ld (a row block of a larger matrix is not served)", what, m, n);
		return 1;
	}
	return 0;
}

}  // namespace spmv

extern "C" int
spmv_mi355x_gmres(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, int restart, const void * minv_host, double tol,
		long max_iterations, double * history_out, spmv_mi355x_gmres_info * info)
{
	using namespace spmv;
	if (gmres_check_common("gmres", A, b_host, x_out_host, restart, tol, max_iterations, info))
		return 1;
	const long n = spmv_mi355x_cols(A);
	const bool f32 = spmv_mi355x_precision(A) == SPMV_MI355X_F32;
	if (minv_host)
	{
		const long bad = f32 ? gmres_bad_minv<float>(minv_host, n) : gmres_bad_minv<double>(minv_host, n);
		if (bad >= 0)
		{
			set_error("gmres: minv[%ld] = %g: every entry of the inverse diagonal preconditioner must be finite and > 0", bad,
					f32 ? (double) ((const float *) minv_host)[bad] : ((const double *) minv_host)[bad]);
			return 1;
		}
	}
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	if (f32)
		return minv_host ? gmres_solve<float, GMRES_MINV>(A, b_host, x_out_host, restart, minv_host, tol, max_iterations, history_out, info)
		                 : gmres_solve<float, GMRES_PLAIN>(A, b_host, x_out_host, restart, nullptr, tol, max_iterations, history_out, info);
	return minv_host ? gmres_solve<double, GMRES_MINV>(A, b_host, x_out_host, restart, minv_host, tol, max_iterations, history_out, info)
	                 : gmres_solve<double, GMRES_PLAIN>(A, b_host, x_out_host, restart, nullptr, tol, max_iterations, history_out, info);
}

extern "C" int
spmv_mi355x_gmres_tri(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, int restart, const spmv_mi355x_tri_precond * M,
		double tol, long max_iterations, double * history_out, spmv_mi355x_gmres_info * info)
{
	using namespace spmv;
	if (gmres_check_common("gmres_tri", A, b_host, x_out_host, restart, tol, max_iterations, info))
		return 1;
	if (!M)
	{
		set_error("gmres_tri: NULL preconditioner M");
		return 1;
	}
	if (!tri_precond_size_ok("gmres_tri", M))
		return 1;
	if (!M->first && !M->scale_host && !M->second)
	{
		set_error("gmres_tri: M has no first, no scale and no second: for a solve without a preconditioner call spmv_mi355x_gmres");
		return 1;
	}
	const int precision = spmv_mi355x_precision(A), device = spmv_mi355x_device(A);
	const bool f32 = precision == SPMV_MI355X_F32;
	if (!tri_precond_parts_ok("gmres_tri", M, spmv_mi355x_cols(A), precision, device))
		return 1;
	HIP_TRY(hipSetDevice(device));
	if (f32)
		return gmres_solve<float, GMRES_TRI>(A, b_host, x_out_host, restart, M->scale_host, tol, max_iterations, history_out, info,
				M->first, M->second);
	return gmres_solve<double, GMRES_TRI>(A, b_host, x_out_host, restart, M->scale_host, tol, max_iterations, history_out, info,
			M->first, M->second);
}

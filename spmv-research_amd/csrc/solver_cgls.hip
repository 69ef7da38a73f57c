// Device-resident CGLS: min |A x - b|^2 + damp |x|^2 for any m x n matrix, over a handle of A and a handle of A^t.
//
// The recurrences (Hestenes-Stiefel CG on the normal equations, A^t A never formed), from x0 = 0:
//   r = b; s = A^t r; p = s; gamma = s.s; gamma0 = gamma
//   loop k: q = A p;  delta = q.q + damp p.p;  alpha = gamma / delta;  x += alpha p;  r -= alpha q;
//           s = A^t r - damp x;  gamma' = s.s;  beta = gamma' / gamma;  p = s + beta p;  gamma = gamma'
//           stop when sqrt(gamma') <= tol sqrt(gamma0)
// Built like solvers.hip (state ping-pong, two-stage deterministic dots re-reduced by every block of the consumer, a device
// `done` flag that predicates every later vector kernel off) and driven by the same host loop: ProgressGate of solvers_common.hpp.
// Per iteration: 2 SpMV + 4 vector launches
//   q = A p | cgls_delta (q.q, p.p) | cgls_update (x, r, r.r) | s = A^t r | cgls_normal (s -= damp x, s.s) | cgls_direction (p, state).
// Stored vectors: b, r, q (m values) and x, p, s (n values), nothing else.
//
// THE TWO LENGTHS. The vectors have m or n values and cgls_delta / cgls_update walk both. Every vector kernel of the solve runs on
// ONE grid of nb = max(nb_m, nb_n) blocks, nb_l = min(1024, max(1, ceil(l / 1024))), and every block strides over whichever lengths
// its kernel touches; a block past the end of the shorter vector contributes a partial of 0. Every producer therefore writes
// exactly nb partials of its slot and every consumer re-reduces exactly nb: there is no second count to mix up, no slot is read
// beyond what its last producer wrote, and the zeroing of the partial array at setup is never relied on.

#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "solvers_common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

struct CglsState {
	double gamma, gamma0;         // |s_k|^2, |A^t b|^2. alpha, beta and delta are recomputed by every block from the partials.
	long k;                       // completed loop bodies
	int done;                     // a stop rule fired: every later vector kernel is predicated off
	int stop;                     // 0 while running, else 1 / 3 / 4 of spmv_mi355x_lsq_info.stop (2 is the host's: never done)
};

// one producer kernel per slot
enum { C_QQ = 0, C_PP, C_RR, C_SS, C_XX, CGLS_SLOTS };

// delta = |q|^2 + damp |p|^2 from the partials of cgls_delta_kernel; the same bits in every block of every kernel that asks
__device__ __forceinline__ double
cgls_delta(const double * __restrict__ part, int nb, double damp)
{
	double delta = sum_partials(part, C_QQ, nb);
	if (damp != 0)
		delta += damp * sum_partials(part, C_PP, nb);
	return delta;
}

// breakdown: alpha = gamma / delta cannot be formed
__device__ __forceinline__ bool
cgls_breakdown(double delta)
{
	return !(delta > 0 && delta < INFINITY);
}

// p = s ; partial SS = s.s = gamma0   (s = A^t b)
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_start_kernel(const T * __restrict__ s, T * __restrict__ p, long n, double * __restrict__ part)
{
	double ss = 0;
	GRID_STRIDE(i, n)
	{
		const T si = s[i];
		p[i] = si;
		ss += (double) si * (double) si;
	}
	store_partial(part, C_SS, ss);
}

// 1 block. A^t b == 0: x = 0 is the solution, nothing to iterate on.
__global__ __launch_bounds__(VB) void
cgls_init_state_kernel(CglsState * __restrict__ st_p, int nb, const double * __restrict__ part)
{
	const double gamma0 = sum_partials(part, C_SS, nb);
	if (threadIdx.x == 0)
	{
		CglsState st;
		st.gamma = gamma0;
		st.gamma0 = gamma0;
		st.k = 0;
		st.done = gamma0 == 0;
		st.stop = st.done ? 3 : 0;
		st_p[0] = st;
		st_p[1] = st;
	}
}

// partials QQ = q.q over m and, when damp != 0, PP = p.p over n   (q = A p)
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_delta_kernel(const CglsState * __restrict__ st_p, const T * __restrict__ q, const T * __restrict__ p, long m, long n,
		double damp, double * __restrict__ part)
{
	if (st_p->done)
		return;
	double qq = 0;
	GRID_STRIDE(i, m)
		qq += (double) q[i] * (double) q[i];
	store_partial(part, C_QQ, qq);
	if (damp != 0)
	{
		double pp = 0;
		GRID_STRIDE(i, n)
			pp += (double) p[i] * (double) p[i];
		store_partial(part, C_PP, pp);
	}
}

// alpha = gamma / delta; x += alpha p over n; r -= alpha q over m; partial RR = r.r. Block 0 posts the breakdown verdict of this
// iteration in *bad (not part of the state slot the other blocks are reading) for cgls_normal_kernel and cgls_direction_kernel,
// and the latter records it in the next state. On a breakdown nothing else is touched.
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_update_kernel(const CglsState * __restrict__ st_p, T * __restrict__ x, T * __restrict__ r, const T * __restrict__ p,
		const T * __restrict__ q, long m, long n, int nb, double damp, double * __restrict__ part, int * __restrict__ bad)
{
	const CglsState st = *st_p;
	if (st.done)
		return;
	const double delta = cgls_delta(part, nb, damp);
	if (blockIdx.x == 0 && threadIdx.x == 0)
		*bad = cgls_breakdown(delta);
	if (cgls_breakdown(delta))
		return;
	const T alpha = (T) (st.gamma / delta);
	GRID_STRIDE(i, n)
		x[i] = x[i] + alpha * p[i];
	double rr = 0;
	GRID_STRIDE(i, m)
	{
		const T ri = r[i] + (-alpha) * q[i];
		r[i] = ri;
		rr += (double) ri * (double) ri;
	}
	store_partial(part, C_RR, rr);
}

// s = A^t r - damp x (s is only read when damp == 0); partial SS = s.s over n
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_normal_kernel(const CglsState * __restrict__ st_p, T * __restrict__ s, const T * __restrict__ x, long n, double damp,
		double * __restrict__ part, const int * __restrict__ bad)
{
	if (st_p->done || *bad)
		return;
	double ss = 0;
	if (damp != 0)
	{
		const T d = (T) damp;
		GRID_STRIDE(i, n)
		{
			const T si = s[i] + (-d) * x[i];
			s[i] = si;
			ss += (double) si * (double) si;
		}
	}
	else
	{
		GRID_STRIDE(i, n)
			ss += (double) s[i] * (double) s[i];
	}
	store_partial(part, C_SS, ss);
}

// gamma' = s.s; beta = gamma' / gamma; p = s + beta p over n. Block 0 writes the next state, the history row (|r|, |s|), the stop
// test and the progress word.
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_direction_kernel(const CglsState * __restrict__ st_p, CglsState * __restrict__ st_next, const T * __restrict__ s,
		T * __restrict__ p, long n, int nb, double tol, const double * __restrict__ part,
		double * __restrict__ history, long it, volatile long * host_progress, const int * __restrict__ bad)
{
	const CglsState st = *st_p;
	if (st.done)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			*st_next = st;
			post_progress(host_progress, it + 1, st.k);
		}
		return;
	}
	if (*bad)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			CglsState nx = st;                    // x, r, p and k of the last good iteration
			nx.done = 1;
			nx.stop = 4;
			*st_next = nx;
			post_progress(host_progress, it + 1, nx.k);
		}
		return;
	}
	const double gamma_new = sum_partials(part, C_SS, nb);
	const T beta = (T) (gamma_new / st.gamma);
	GRID_STRIDE(i, n)
		p[i] = s[i] + beta * p[i];
	if (blockIdx.x == 0)
	{
		const double rr = sum_partials(part, C_RR, nb);
		if (threadIdx.x == 0)
		{
			CglsState nx = st;
			nx.gamma = gamma_new;
			nx.k = st.k + 1;
			if (history)
			{
				history[2 * st.k + 0] = sqrt(rr);
				history[2 * st.k + 1] = sqrt(gamma_new);
			}
			nx.done = tol > 0 && sqrt(gamma_new) <= tol * sqrt(st.gamma0);
			nx.stop = nx.done ? 1 : 0;
			*st_next = nx;
			post_progress(host_progress, it + 1, nx.done ? nx.k : -1);
		}
	}
}

// the tail's explicit residual: q = b - q over m (q = A x); partial RR = |b - A x|^2
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_residual_kernel(const T * __restrict__ b, T * __restrict__ q, long m, double * __restrict__ part)
{
	double rr = 0;
	GRID_STRIDE(i, m)
	{
		const T ri = b[i] + (T) -1 * q[i];
		q[i] = ri;
		rr += (double) ri * (double) ri;
	}
	store_partial(part, C_RR, rr);
}

// the tail's explicit normal residual: partials SS = |s - damp x|^2 (s = A^t (b - A x)) and XX = |x|^2 over n; nothing is written
template <typename T>
__global__ __launch_bounds__(VB) void
cgls_normal_residual_kernel(const T * __restrict__ s, const T * __restrict__ x, long n, double damp, double * __restrict__ part)
{
	const T d = (T) damp;
	double ss = 0, xx = 0;
	GRID_STRIDE(i, n)
	{
		const T xi = x[i];
		const T si = damp != 0 ? s[i] + (-d) * xi : s[i];
		ss += (double) si * (double) si;
		xx += (double) xi * (double) xi;
	}
	store_partial(part, C_SS, ss);
	store_partial(part, C_XX, xx);
}

// ------------------------------------------------------------------------------------------------ host side

template <typename T>
static int
cgls_solve(spmv_mi355x_matrix * A, spmv_mi355x_matrix * At, const void * b_host, void * x_host, double damp, double tol,
		long max_iterations, double * history_host, spmv_mi355x_lsq_info * info)
{
	const auto t_start = std::chrono::steady_clock::now();
	const long m = spmv_mi355x_rows(A), n = spmv_mi355x_cols(A);
	hipStream_t stream = nullptr;
	ProgressGate gate;                // outlives buf, whose hipFree waits for the kernels that post to it
	DeviceBuffers buf;
	const size_t mb = (size_t) m * sizeof(T), nbytes = (size_t) n * sizeof(T);

	// plain allocations, the SpMV outputs (q, s) included: see solve() in solvers.hip
	T * b, * r, * q, * x, * p, * s;
	for (T ** v : {&b, &r, &q})
		ABI_TRY(buf.alloc(v, mb));
	for (T ** v : {&x, &p, &s})
		ABI_TRY(buf.alloc(v, nbytes));
	double * part, * history = nullptr;
	CglsState * st;
	ABI_TRY(buf.alloc(&part, sizeof(double) * CGLS_SLOTS * MAX_PART));
	ABI_TRY(buf.alloc(&st, 2 * sizeof(CglsState)));
	int * bad;                                                        // this iteration's breakdown verdict, cgls_update_kernel's
	ABI_TRY(buf.alloc(&bad, sizeof(int)));
	const size_t hist_bytes = sizeof(double) * 2 * (size_t) max_iterations;
	if (history_host && max_iterations > 0)
	{
		ABI_TRY(buf.alloc(&history, hist_bytes));
		HIP_TRY(hipMemsetAsync(history, 0, hist_bytes, stream));
	}
	ABI_TRY(gate.init());

	HIP_TRY(hipMemcpyAsync(b, b_host, mb, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemsetAsync(x, 0, nbytes, stream));                   // x0 = 0
	HIP_TRY(hipMemcpyAsync(r, b, mb, hipMemcpyDeviceToDevice, stream));
	HIP_TRY(hipMemsetAsync(part, 0, sizeof(double) * CGLS_SLOTS * MAX_PART, stream));
	HIP_TRY(hipMemsetAsync(bad, 0, sizeof(int), stream));

	const int nb = std::max(solver_blocks(m), solver_blocks(n));     // ONE grid for both lengths (head of this file)
	const dim3 grid(nb), block(VB), one(1);
	long spmv_calls = 0;
	auto spmv = [&](spmv_mi355x_matrix * M, const T * in, T * out) {
		spmv_calls++;
		return spmv_mi355x_spmv_device_async(M, in, out, 0, stream);
	};

	// s = A^t b, p = s, gamma0
	ABI_TRY(spmv(At, r, s));
	hipLaunchKernelGGL((cgls_start_kernel<T>), grid, block, 0, stream, s, p, n, part);
	hipLaunchKernelGGL(cgls_init_state_kernel, one, block, 0, stream, st, nb, part);
	HIP_TRY(hipGetLastError());

	long it = 0;
	for (; it < max_iterations; it++)
	{
		bool stop;
		ABI_TRY(gate.wait(it, "cgls", stream, &stop));
		if (stop)
			break;
		CglsState * cur = st + (it & 1), * nxt = st + ((it + 1) & 1);
		ABI_TRY(spmv(A, p, q));
		hipLaunchKernelGGL((cgls_delta_kernel<T>), grid, block, 0, stream, cur, q, p, m, n, damp, part);
		hipLaunchKernelGGL((cgls_update_kernel<T>), grid, block, 0, stream, cur, x, r, p, q, m, n, nb, damp, part, bad);
		ABI_TRY(spmv(At, r, s));
		hipLaunchKernelGGL((cgls_normal_kernel<T>), grid, block, 0, stream, cur, s, x, n, damp, part, bad);
		hipLaunchKernelGGL((cgls_direction_kernel<T>), grid, block, 0, stream, cur, nxt, s, p, n, nb, tol, part, history, it,
				gate.dev, bad);
	}
	HIP_TRY(hipGetLastError());

	// the explicit norms of the returned x: |b - A x|, |A^t (b - A x) - damp x|, |x|. q, s are free now; x, r, p stay as they froze.
	CglsState * fin = st + (it & 1);
	ABI_TRY(spmv(A, x, q));
	hipLaunchKernelGGL((cgls_residual_kernel<T>), grid, block, 0, stream, b, q, m, part);
	ABI_TRY(spmv(At, q, s));
	hipLaunchKernelGGL((cgls_normal_residual_kernel<T>), grid, block, 0, stream, s, x, n, damp, part);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(x_host, x, nbytes, hipMemcpyDeviceToHost, stream));
	CglsState st_host;
	std::vector<double> part_host((size_t) CGLS_SLOTS * MAX_PART);
	HIP_TRY(hipMemcpyAsync(&st_host, fin, sizeof(CglsState), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(part_host.data(), part, sizeof(double) * CGLS_SLOTS * MAX_PART, hipMemcpyDeviceToHost, stream));
	if (history)
		HIP_TRY(hipMemcpyAsync(history_host, history, hist_bytes, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	if (info)
	{
		auto norm_of = [&](int slot) { return std::sqrt(host_sum(part_host.data(), (size_t) slot * MAX_PART, nb)); };
		spmv_mi355x_lsq_info out;
		memset(&out, 0, sizeof(out));
		out.iterations = st_host.k;
		out.stop = st_host.done ? st_host.stop : 2;
		out.rnorm = norm_of(C_RR);
		out.arnorm = norm_of(C_SS);
		out.arnorm0 = std::sqrt(st_host.gamma0);
		out.xnorm = norm_of(C_XX);
		out.spmv_calls = spmv_calls;
		out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
		put_info(info, info->struct_size, out);
	}
	return 0;
}

}  // namespace spmv

extern "C" int
spmv_mi355x_cgls(spmv_mi355x_matrix * A, spmv_mi355x_matrix * At, const void * b_host, void * x_out_host, double damp, double tol,
		long max_iterations, double * history_out, spmv_mi355x_lsq_info * info)
{
	using namespace spmv;
	// the checks that need no handle come first, so each can be met (and tested) on its own
	if (!info_size_ok("cgls", info))
		return 1;
	if (!(damp >= 0) || !std::isfinite(damp))
	{
		set_error("cgls: damp must be finite and >= 0 (got %g)", damp);
		return 1;
	}
	if (!(tol >= 0) || !std::isfinite(tol))
	{
		set_error("cgls: tol must be finite and >= 0 (got %g)", tol);
		return 1;
	}
	if (max_iterations < 0)
	{
		set_error("cgls: max_iterations < 0");
		return 1;
	}
	if (!A || !At || !b_host || !x_out_host)
	{
		set_error("cgls: NULL argument (%s%s%s%s )", !A ? " A" : "", !At ? " At" : "", !b_host ? " b" : "", !x_out_host ? " x_out" : "");
		return 1;
	}
	const long m = spmv_mi355x_rows(A), n = spmv_mi355x_cols(A);
	if (spmv_mi355x_rows(At) != n || spmv_mi355x_cols(At) != m)
	{
		set_error("cgls: At must have the shape of the transpose: A is %ld x %ld, At is %ld x %ld (expected %ld x %ld)", m, n,
				spmv_mi355x_rows(At), spmv_mi355x_cols(At), n, m);
		return 1;
	}
	if (spmv_mi355x_precision(A) != spmv_mi355x_precision(At))
	{
		set_error("cgls: A and At differ in precision (A is %s, At is %s)", spmv_mi355x_precision(A) == SPMV_MI355X_F32 ? "fp32" : "fp64",
				spmv_mi355x_precision(At) == SPMV_MI355X_F32 ? "fp32" : "fp64");
		return 1;
	}
	if (spmv_mi355x_device(A) != spmv_mi355x_device(At))
	{
		set_error("cgls: A and At live on different devices (%d and %d)", spmv_mi355x_device(A), spmv_mi355x_device(At));
		return 1;
	}
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	if (spmv_mi355x_precision(A) == SPMV_MI355X_F32)
		return cgls_solve<float>(A, At, b_host, x_out_host, damp, tol, max_iterations, history_out, info);
	return cgls_solve<double>(A, At, b_host, x_out_host, damp, tol, max_iterations, history_out, info);
}

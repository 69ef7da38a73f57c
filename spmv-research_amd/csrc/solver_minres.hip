// Device-resident MINRES (Paige-Saunders): (A - shift I) x = b for a square SYMMETRIC matrix, indefinite or singular included, over
// one handle of A, with an optional diagonal preconditioner given as its inverse, M^-1 = diag(minv), minv > 0.
//
// The recurrences (scipy's minres without its norm-estimate stopping tests), from x0 = 0, every scalar fp64:
//   r1 = b; y = M^-1 b; beta1 = sqrt(b.y)
//   oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0; r2 = r1
//   loop itn = 1, 2, ...:
//       v = y / beta;  y = A v - shift v;  if itn >= 2: y -= (beta/oldb) r1
//       alfa = v.y;    y -= (alfa/beta) r2;  r1 = r2;  r2 = y;  y = M^-1 r2
//       oldb = beta;   beta = sqrt(r2.y)
//       oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
//       gamma = max(hypot(gbar, beta), DBL_EPSILON); cs = gbar/gamma; sn = beta/gamma; phi = cs phibar; phibar = sn phibar
//       w1 = w2; w2 = w; w = (v - oldeps w1 - delta w2) / gamma;  x += phi w
//       stop when phibar <= tol beta1 (1), else when beta == 0 (5)
// Built like solver_cgls.hip (state ping-pong, two-stage deterministic dots re-reduced by every block of the consumer, a device
// `done` flag that predicates every later vector kernel off) and driven by the same host loop: ProgressGate of solvers_common.hpp.
// Per iteration: 1 SpMV + 3 vector launches
//   y = A v | minres_lanczos (y -= shift v + (beta/oldb) r1, v.y) | minres_orth (y -= (alfa/beta) r2, y.(minv y)) |
//   minres_update (rotation, w, x, next v, state).
// Stored vectors, n values each: b, x, v, three that rotate through the roles r1 / r2 / y, two that rotate through w1 / w2
// (the new w overwrites w1 element by element: it is the only reader of w1), and minv when given. M^-1 r2 is never stored: with
// minv the two kernels that need it multiply on the fly, without minv r2 itself serves and no multiply is issued.
// The roles rotate BY POINTER on the host, which knows the iteration index; once `done` is set nothing is written, so the roles the
// host goes on rotating while it runs ahead do not matter.
//
// BREAKDOWN. Every test of it sits in minres_update, the kernel whose block 0 writes the next state: alfa = v.y not finite,
// r2.(M^-1 r2) negative or not finite, or a rotation scalar not finite. All blocks reach the same verdict from the same partials,
// none touches w, x or v, and block 0 records done / stop 4 with k unchanged: x is that of the last good iteration. No flag
// beside the state is needed (solver_cgls.hip needs one because its verdict falls in a kernel that cannot write the state).

#include <cfloat>
#include <chrono>
#include <cmath>
#include <cstring>
#include <vector>

#include "common.hpp"
#include "solvers_common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

struct MinresState {
	double beta1;                 // sqrt(b . M^-1 b)
	double oldb, beta;            // beta_k, beta_{k+1}
	double dbar, epsln, phibar, cs, sn;
	long k;                       // completed loop bodies
	int done;                     // a stop rule fired: every later vector kernel is predicated off
	int stop;                     // 0 while running, else 1 / 3 / 4 / 5 of spmv_mi355x_minres_info.stop (2 is the host's: never done)
};

// one producer kernel per slot
enum { M_BY = 0, M_BB, M_VY, M_YZ, M_RR, M_XX, MINRES_SLOTS };

// partials BY = b.(minv b) and BB = b.b; r2 = b
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
minres_start_kernel(const T * __restrict__ b, const T * __restrict__ minv, T * __restrict__ r2, long n, double * __restrict__ part)
{
	double by = 0, bb = 0;
	GRID_STRIDE(i, n)
	{
		const T bi = b[i];
		r2[i] = bi;
		bb += (double) bi * (double) bi;
		if (PRE)
			by += (double) bi * (double) (minv[i] * bi);
	}
	store_partial(part, M_BB, bb);
	store_partial(part, M_BY, PRE ? by : bb);
}

// 1 block. b . M^-1 b == 0: x = 0 is the solution (stop 3); negative or not finite: stop 4.
__global__ __launch_bounds__(VB) void
minres_init_state_kernel(MinresState * __restrict__ st_p, int nb, const double * __restrict__ part)
{
	const double by = sum_partials(part, M_BY, nb);
	if (threadIdx.x == 0)
	{
		MinresState st;
		const bool bad = !(by >= 0) || !(by < INFINITY);
		st.beta1 = bad ? 0 : sqrt(by);
		st.oldb = 0;
		st.beta = st.beta1;
		st.dbar = 0;
		st.epsln = 0;
		st.phibar = st.beta1;
		st.cs = -1;
		st.sn = 0;
		st.k = 0;
		st.done = bad || by == 0;
		st.stop = bad ? 4 : by == 0 ? 3 : 0;
		st_p[0] = st;
		st_p[1] = st;
	}
}

// v = (M^-1 b) / beta1; x = w1 = w2 = 0
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
minres_first_v_kernel(const MinresState * __restrict__ st_p, const T * __restrict__ b, const T * __restrict__ minv,
		T * __restrict__ v, T * __restrict__ x, T * __restrict__ wa, T * __restrict__ wb, long n)
{
	const MinresState st = *st_p;
	const T inv = st.done ? (T) 0 : (T) (1.0 / st.beta1);
	GRID_STRIDE(i, n)
	{
		v[i] = inv * (PRE ? minv[i] * b[i] : b[i]);
		x[i] = 0;
		wa[i] = 0;
		wb[i] = 0;
	}
}

// y -= shift v + (beta/oldb) r1 (the r1 term from the second iteration on); partial VY = v.y   (y = A v)
template <typename T>
__global__ __launch_bounds__(VB) void
minres_lanczos_kernel(const MinresState * __restrict__ st_p, T * __restrict__ y, const T * __restrict__ v,
		const T * __restrict__ r1, long n, double shift, double * __restrict__ part)
{
	const MinresState st = *st_p;
	if (st.done)
		return;
	const T s = (T) shift;
	double vy = 0;
	if (st.k >= 1)
	{
		const T c = (T) (st.beta / st.oldb);
		GRID_STRIDE(i, n)
		{
			const T vi = v[i];
			const T yi = y[i] - s * vi - c * r1[i];
			y[i] = yi;
			vy += (double) vi * (double) yi;
		}
	}
	else
	{
		GRID_STRIDE(i, n)
		{
			const T vi = v[i];
			const T yi = y[i] - s * vi;
			y[i] = yi;
			vy += (double) vi * (double) yi;
		}
	}
	store_partial(part, M_VY, vy);
}

// alfa = v.y; y -= (alfa/beta) r2; partial YZ = y.(minv y). y is the next r2.
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
minres_orth_kernel(const MinresState * __restrict__ st_p, T * __restrict__ y, const T * __restrict__ r2,
		const T * __restrict__ minv, long n, int nb, double * __restrict__ part)
{
	const MinresState st = *st_p;
	if (st.done)
		return;
	const T c = (T) (sum_partials(part, M_VY, nb) / st.beta);
	double yz = 0;
	GRID_STRIDE(i, n)
	{
		const T yi = y[i] - c * r2[i];
		y[i] = yi;
		yz += (double) yi * (double) (PRE ? minv[i] * yi : yi);
	}
	store_partial(part, M_YZ, yz);
}

// The rotation from alfa and beta^2 = r2.(M^-1 r2), identically in every block; w = (v - oldeps w1 - delta w2) / gamma written over
// w1; x += phi w; v = (M^-1 r2) / beta for the next iteration. Block 0 writes the next state, the history row, the stop tests and
// the progress word. On a breakdown (head of this file) no vector is touched.
template <typename T, bool PRE>
__global__ __launch_bounds__(VB) void
minres_update_kernel(const MinresState * __restrict__ st_p, MinresState * __restrict__ st_next, T * __restrict__ x,
		T * __restrict__ v, T * __restrict__ w1, const T * __restrict__ w2, const T * __restrict__ r2,
		const T * __restrict__ minv, long n, int nb, double tol, const double * __restrict__ part,
		double * __restrict__ history, long it, volatile long * host_progress)
{
	const MinresState st = *st_p;
	if (st.done)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			*st_next = st;
			post_progress(host_progress, it + 1, st.k);
		}
		return;
	}
	const double alfa = sum_partials(part, M_VY, nb);
	const double beta2 = sum_partials(part, M_YZ, nb);
	MinresState nx = st;
	bool bad = !(beta2 >= 0) || !(beta2 < INFINITY) || !isfinite(alfa);
	double oldeps = 0, delta = 0, gamma = 1, phi = 0;
	if (!bad)
	{
		const double beta = sqrt(beta2);
		oldeps = st.epsln;
		delta = st.cs * st.dbar + st.sn * alfa;
		const double gbar = st.sn * st.dbar - st.cs * alfa;
		nx.oldb = st.beta;
		nx.beta = beta;
		nx.epsln = st.sn * beta;
		nx.dbar = -st.cs * beta;
		gamma = fmax(hypot(gbar, beta), DBL_EPSILON);
		nx.cs = gbar / gamma;
		nx.sn = beta / gamma;
		phi = nx.cs * st.phibar;
		nx.phibar = nx.sn * st.phibar;
		bad = !isfinite(delta) || !isfinite(gamma) || !isfinite(phi) || !isfinite(nx.phibar) || !isfinite(nx.epsln) ||
				!isfinite(nx.dbar);
	}
	if (bad)
	{
		if (blockIdx.x == 0 && threadIdx.x == 0)
		{
			nx = st;                              // x and k of the last good iteration
			nx.done = 1;
			nx.stop = 4;
			*st_next = nx;
			post_progress(host_progress, it + 1, nx.k);
		}
		return;
	}
	const T e = (T) oldeps, d = (T) delta, ig = (T) (1.0 / gamma), ph = (T) phi;
	const bool more = nx.beta > 0;                // beta == 0 is stop 5 below: no next v
	const T ib = more ? (T) (1.0 / nx.beta) : (T) 0;
	GRID_STRIDE(i, n)
	{
		const T wi = (v[i] - e * w1[i] - d * w2[i]) * ig;
		w1[i] = wi;
		x[i] = x[i] + ph * wi;
		if (more)
			v[i] = ib * (PRE ? minv[i] * r2[i] : r2[i]);
	}
	if (blockIdx.x == 0 && threadIdx.x == 0)
	{
		nx.k = st.k + 1;
		if (history)
			history[st.k] = nx.phibar;
		if (tol > 0 && nx.phibar <= tol * st.beta1)
			nx.stop = 1;
		else if (!more)
			nx.stop = 5;
		nx.done = nx.stop != 0;
		*st_next = nx;
		post_progress(host_progress, it + 1, nx.done ? nx.k : -1);
	}
}

// the tail's explicit residual: q = b - (q - shift x) (q = A x); partials RR = |b - (A - shift I) x|^2 and XX = |x|^2
template <typename T>
__global__ __launch_bounds__(VB) void
minres_residual_kernel(const T * __restrict__ b, T * __restrict__ q, const T * __restrict__ x, long n, double shift,
		double * __restrict__ part)
{
	const T s = (T) shift;
	double rr = 0, xx = 0;
	GRID_STRIDE(i, n)
	{
		const T xi = x[i];
		const T ri = b[i] - (q[i] - s * xi);
		q[i] = ri;
		rr += (double) ri * (double) ri;
		xx += (double) xi * (double) xi;
	}
	store_partial(part, M_RR, rr);
	store_partial(part, M_XX, xx);
}

// ------------------------------------------------------------------------------------------------ host side

template <typename T, bool PRE>
static int
minres_solve(spmv_mi355x_matrix * A, const void * b_host, void * x_host, double shift, const void * minv_host, double tol,
		long max_iterations, double * history_host, spmv_mi355x_minres_info * info)
{
	const auto t_start = std::chrono::steady_clock::now();
	const long n = spmv_mi355x_rows(A);
	hipStream_t stream = nullptr;
	ProgressGate gate;                // outlives buf, whose hipFree waits for the kernels that post to it
	DeviceBuffers buf;
	const size_t nbytes = (size_t) n * sizeof(T);

	// plain allocations, the SpMV output included: see solve() in solvers.hip
	T * b, * x, * v, * R[3], * W[2], * minv = nullptr;
	for (T ** p : {&b, &x, &v, &R[0], &R[1], &R[2], &W[0], &W[1]})
		ABI_TRY(buf.alloc(p, nbytes));
	if (PRE)
		ABI_TRY(buf.alloc(&minv, nbytes));
	double * part, * history = nullptr;
	MinresState * st;
	ABI_TRY(buf.alloc(&part, sizeof(double) * MINRES_SLOTS * MAX_PART));
	ABI_TRY(buf.alloc(&st, 2 * sizeof(MinresState)));
	const size_t hist_bytes = sizeof(double) * (size_t) max_iterations;
	if (history_host && max_iterations > 0)
	{
		ABI_TRY(buf.alloc(&history, hist_bytes));
		HIP_TRY(hipMemsetAsync(history, 0, hist_bytes, stream));
	}
	ABI_TRY(gate.init());

	HIP_TRY(hipMemcpyAsync(b, b_host, nbytes, hipMemcpyHostToDevice, stream));
	if (PRE)
		HIP_TRY(hipMemcpyAsync(minv, minv_host, nbytes, hipMemcpyHostToDevice, stream));
	HIP_TRY(hipMemsetAsync(part, 0, sizeof(double) * MINRES_SLOTS * MAX_PART, stream));

	const int nb = solver_blocks(n);
	const dim3 grid(nb), block(VB), one(1);
	long spmv_calls = 0;
	auto spmv = [&](const T * in, T * out) {
		spmv_calls++;
		return spmv_mi355x_spmv_device_async(A, in, out, 0, stream);
	};

	// iteration `it` (from 0) reads r1 = R[it % 3] and r2 = R[(it + 1) % 3] and writes y = R[(it + 2) % 3], the next r2; it reads
	// w2 = W[(it + 1) & 1] and reads, then overwrites, w1 = W[it & 1]. r2 of iteration 0 is b (r1 is not read there).
	hipLaunchKernelGGL((minres_start_kernel<T, PRE>), grid, block, 0, stream, b, minv, R[1], n, part);
	hipLaunchKernelGGL(minres_init_state_kernel, one, block, 0, stream, st, nb, part);
	hipLaunchKernelGGL((minres_first_v_kernel<T, PRE>), grid, block, 0, stream, st, b, minv, v, x, W[0], W[1], n);
	HIP_TRY(hipGetLastError());

	long it = 0;
	for (; it < max_iterations; it++)
	{
		bool stop;
		ABI_TRY(gate.wait(it, "minres", stream, &stop));
		if (stop)
			break;
		MinresState * cur = st + (it & 1), * nxt = st + ((it + 1) & 1);
		T * r1 = R[it % 3], * r2 = R[(it + 1) % 3], * y = R[(it + 2) % 3];
		ABI_TRY(spmv(v, y));
		hipLaunchKernelGGL((minres_lanczos_kernel<T>), grid, block, 0, stream, cur, y, v, r1, n, shift, part);
		hipLaunchKernelGGL((minres_orth_kernel<T, PRE>), grid, block, 0, stream, cur, y, r2, minv, n, nb, part);
		hipLaunchKernelGGL((minres_update_kernel<T, PRE>), grid, block, 0, stream, cur, nxt, x, v, W[it & 1], W[(it + 1) & 1], y,
				minv, n, nb, tol, part, history, it, gate.dev);
	}
	HIP_TRY(hipGetLastError());

	// the explicit norms of the returned x: |b - (A - shift I) x| and |x|. The r's are free now; x stays as it froze.
	MinresState * fin = st + (it & 1);
	T * q = R[0];
	ABI_TRY(spmv(x, q));
	hipLaunchKernelGGL((minres_residual_kernel<T>), grid, block, 0, stream, b, q, x, n, shift, part);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipMemcpyAsync(x_host, x, nbytes, hipMemcpyDeviceToHost, stream));
	MinresState st_host;
	std::vector<double> part_host((size_t) MINRES_SLOTS * MAX_PART);
	HIP_TRY(hipMemcpyAsync(&st_host, fin, sizeof(MinresState), hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipMemcpyAsync(part_host.data(), part, sizeof(double) * MINRES_SLOTS * MAX_PART, hipMemcpyDeviceToHost, stream));
	if (history)
		HIP_TRY(hipMemcpyAsync(history_host, history, hist_bytes, hipMemcpyDeviceToHost, stream));
	HIP_TRY(hipStreamSynchronize(stream));
	if (info)
	{
		auto norm_of = [&](int slot) { return std::sqrt(host_sum(part_host.data(), (size_t) slot * MAX_PART, nb)); };
		spmv_mi355x_minres_info out;
		memset(&out, 0, sizeof(out));
		out.iterations = st_host.k;
		out.stop = st_host.done ? st_host.stop : 2;
		out.rnorm = norm_of(M_RR);
		out.rnorm0 = norm_of(M_BB);
		out.prnorm = st_host.phibar;
		out.prnorm0 = st_host.beta1;
		out.xnorm = norm_of(M_XX);
		out.spmv_calls = spmv_calls;
		out.seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t_start).count();
		put_info(info, info->struct_size, out);
	}
	return 0;
}

// the first entry of minv that is not finite or not > 0, or -1
template <typename T>
static long
minres_bad_minv(const void * minv_host, long n)
{
	const T * d = (const T *) minv_host;
	for (long i = 0; i < n; i++)
		if (!(d[i] > 0) || !std::isfinite(d[i]))
			return i;
	return -1;
}

}  // namespace spmv

extern "C" int
spmv_mi355x_minres(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, double shift, const void * minv_host, double tol,
		long max_iterations, double * history_out, spmv_mi355x_minres_info * info)
{
	using namespace spmv;
	// the checks that need no handle come first, so each can be met (and tested) on its own
	if (!info_size_ok("minres", info))
		return 1;
	if (!std::isfinite(shift))
	{
		set_error("minres: shift must be finite (got %g)", shift);
		return 1;
	}
	if (!(tol >= 0) || !std::isfinite(tol))
	{
		set_error("minres: tol must be finite and >= 0 (got %g)", tol);
		return 1;
	}
	if (max_iterations < 0)
	{
		set_error("minres: max_iterations < 0");
		return 1;
	}
	if (!A || !b_host || !x_out_host)
	{
		set_error("minres: NULL argument (%s%s%s )", !A ? " A" : "", !b_host ? " b" : "", !x_out_host ? " x_out" : "");
		return 1;
	}
	const long m = spmv_mi355x_rows(A), n = spmv_mi355x_cols(A);
	if (m != n)
	{
		set_error("minres: the matrix must be square and symmetric: the handle is %ld x %ld (a row block of a larger matrix is not "
				"served)", m, n);
		return 1;
	}
	const bool f32 = spmv_mi355x_precision(A) == SPMV_MI355X_F32;
	if (minv_host)
	{
		const long bad = f32 ? minres_bad_minv<float>(minv_host, n) : minres_bad_minv<double>(minv_host, n);
		if (bad >= 0)
		{
			set_error("minres: minv[%ld] = %g: every entry of the inverse diagonal preconditioner must be finite and > 0", bad,
					f32 ? (double) ((const float *) minv_host)[bad] : ((const double *) minv_host)[bad]);
			return 1;
		}
	}
	HIP_TRY(hipSetDevice(spmv_mi355x_device(A)));
	if (f32)
		return minv_host ? minres_solve<float, true>(A, b_host, x_out_host, shift, minv_host, tol, max_iterations, history_out, info)
		                 : minres_solve<float, false>(A, b_host, x_out_host, shift, nullptr, tol, max_iterations, history_out, info);
	return minv_host ? minres_solve<double, true>(A, b_host, x_out_host, shift, minv_host, tol, max_iterations, history_out, info)
	                 : minres_solve<double, false>(A, b_host, x_out_host, shift, nullptr, tol, max_iterations, history_out, info);
}

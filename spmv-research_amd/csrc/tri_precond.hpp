// What the solvers that take a spmv_mi355x_tri_precond share (solver_gmres.hip: gmres_tri, solver_pcg_tri.hip: pcg_tri): the
// checks of the struct, with the caller's name as the prefix of every message, and the enqueue of
//     z = second^-1 ( scale o ( first^-1 in ) )
// part by part on one stream. Every part may be absent. The solves are spmv_mi355x_trsv handles of any kind; the scale is one
// elementwise kernel. Nothing here knows a solver's stop flag: everything written is z. tri_precond_enqueue_multi is the same on
// n x k blocks (pcg_trsm_multi), with the k-column solve of trsv.hip for the triangular parts.
#pragma once

#include <cmath>

#include "common.hpp"
#include "solvers_common.hpp"
#include "trsv.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

// out = scale o in, elementwise; `in` may be `out`
template <typename T>
__global__ __launch_bounds__(VB) void
tri_scale_kernel(const T * __restrict__ scale, const T * in, T * out, long n)
{
	GRID_STRIDE(e, n)
		out[e] = scale[e] * in[e];
}

// the first entry of a scale that is not finite or is zero, or -1
template <typename T>
static long
tri_bad_scale(const void * scale_host, long n)
{
	const T * d = (const T *) scale_host;
	for (long i = 0; i < n; i++)
		if (d[i] == 0 || !std::isfinite(d[i]))
			return i;
	return -1;
}

// M (not NULL) is at least as large as the struct this library knows
inline bool
tri_precond_size_ok(const char * what, const spmv_mi355x_tri_precond * M)
{
	if (M->struct_size < sizeof(spmv_mi355x_tri_precond))
	{
		set_error("%s: M->struct_size = %u is smaller than sizeof(spmv_mi355x_tri_precond) = %zu", what, M->struct_size,
				sizeof(spmv_mi355x_tri_precond));
		return false;
	}
	return true;
}

// The parts of M against the matrix they precondition, in the header's order: the handles (first before second: n, precision,
// device), then the scale, a host pass over its n values.
inline bool
tri_precond_parts_ok(const char * what, const spmv_mi355x_tri_precond * M, long n, int precision, int device)
{
	const spmv_mi355x_trsv * parts[2] = {M->first, M->second};
	for (int k = 0; k < 2; k++)
	{
		const spmv_mi355x_trsv * T = parts[k];
		const char * name = k ? "second" : "first";
		if (!T)
			continue;
		if (T->n != n)
			set_error("%s: M->%s is a triangular solve of %ld rows, the matrix has %ld", what, name, T->n, n);
		else if (T->precision != precision)
			set_error("%s: M->%s has precision %d, the matrix %d: both must be the same", what, name, T->precision, precision);
		else if (T->device != device)
			set_error("%s: M->%s lives on device %d, the matrix on device %d", what, name, T->device, device);
		else
			continue;
		return false;
	}
	if (M->scale_host)
	{
		const bool f32 = precision == SPMV_MI355X_F32;
		const long bad = f32 ? tri_bad_scale<float>(M->scale_host, n) : tri_bad_scale<double>(M->scale_host, n);
		if (bad >= 0)
		{
			set_error("%s: scale[%ld] = %g: every entry of the scale must be finite and non-zero", what, bad,
					f32 ? (double) ((const float *) M->scale_host)[bad] : ((const double *) M->scale_host)[bad]);
			return false;
		}
	}
	return true;
}

// z = second^-1 (scale o (first^-1 in)) enqueued on `stream`; `in` may be z. scale is the device copy of M's scale (or NULL). With
// defer_scale a scale that is M's LAST part (no second) is left to the caller. With no part at all nothing is enqueued and z is
// not written.
template <typename T>
static int
tri_precond_enqueue(spmv_mi355x_trsv * first, const T * scale, spmv_mi355x_trsv * second, const T * in, T * z, long n,
		bool defer_scale, dim3 grid, hipStream_t stream)
{
	const T * src = in;
	if (first)
	{
		ABI_TRY(spmv_mi355x_trsv_solve_device_async(first, src, z, stream));
		src = z;
	}
	if (scale && !(defer_scale && !second))
	{
		hipLaunchKernelGGL((tri_scale_kernel<T>), grid, dim3(VB), 0, stream, scale, src, z, n);
		src = z;
	}
	if (second)
		ABI_TRY(spmv_mi355x_trsv_solve_device_async(second, src, z, stream));
	return 0;
}

// out = scale o in for the chunk's columns of row-major n x k blocks: tri_scale_kernel's product per element; `in` may be `out`
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
pcg_tri_scale_multi_kernel(const T * __restrict__ scale, const T * in, T * out, long n, long ld, int c0)
{
	const bool vec = ld % KC == 0 && c0 % KC == 0;
	GRID_STRIDE(i, n)
	{
		const long o = i * ld + c0;
		const T si = scale[i];
		T v[KC];
		load_row(v, in + o, vec);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			v[c] = si * v[c];
		store_row(out + o, v, vec);
	}
}

// Z = second^-1 (scale o (first^-1 IN)) for the k columns of row-major n x k blocks with ld = k, enqueued on `stream`; IN may be Z.
// The triangular parts are k-column solves (spmv_mi355x_trsv_solve_multi_device_async, chunked as the handle needs), the scale is
// one launch per chunk of `chunks`. Per column every operation is that of tri_precond_enqueue. With no part nothing is enqueued.
template <typename T>
static int
tri_precond_enqueue_multi(spmv_mi355x_trsv * first, const T * scale, spmv_mi355x_trsv * second, const T * in, T * z, long n, int k,
		const std::vector<Chunk> & chunks, dim3 grid, hipStream_t stream)
{
	const T * src = in;
	if (first)
	{
		ABI_TRY(spmv_mi355x_trsv_solve_multi_device_async(first, k, src, k, z, k, stream));
		src = z;
	}
	if (scale)
	{
		for_chunks(chunks, [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			hipLaunchKernelGGL((pcg_tri_scale_multi_kernel<T, KC>), grid, dim3(VB), 0, stream, scale, src, z, n, (long) k, c0);
			return 0;
		});
		src = z;
	}
	if (second)
		ABI_TRY(spmv_mi355x_trsv_solve_multi_device_async(second, k, src, k, z, k, stream));
	return 0;
}

}  // namespace spmv

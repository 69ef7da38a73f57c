// update_values for triangular solve handles (include/spmv_mi355x.h "update_values for trsv handles"): the two
// kernels that scatter new values, given in the entry order of the caller's CSR, into the level-sliced layout of trsv.hpp.
//
// slot_src[e] names the entry of the caller's CSR that trsv_build puts in slot e of `val` (-1: padding, never written, so it keeps
// create's zeros); diag_src[p] names the first stored diagonal of row perm[p]. Both maps are derived on the host by the walk that
// trsv_build itself runs (trsv.hip: trsv_layout), so there is one statement of the layout. The narrowing (T) v is the conversion
// trsv_build makes on the host, round to nearest even: an fp32 handle comes out bit for bit.
//
// trsv_update_check_kernel (DIAG_STORED only): a diagonal that is zero or not finite AFTER narrowing reports its row by atomicMin on
// the status word, ILU(0)'s breakdown idiom; the minimum does not depend on the order. trsv_update_write_kernel reads the word
// first: a launch boundary lies between the two kernels, so every thread sees the final word, and when it names a row every thread
// returns and the handle keeps its previous values. No other atomic, no waiting, no LDS; every store is a plain vector store.

#include "trsv.hpp"

namespace spmv {

template <typename T>
__device__ inline bool
trsv_bad_diagonal(T d)
{
	return !(fabs((double) d) <= 1.7976931348623157e308) || d == 0;    // NaN, +-Inf or zero, in the handle's precision
}

template <typename T>
__global__ __launch_bounds__(TRSV_UPDATE_BLOCK) void
trsv_update_check_kernel(const int * __restrict__ diag_src, const int * __restrict__ perm, const double * __restrict__ values,
		unsigned * status, long n)
{
	const long stride = (long) gridDim.x * TRSV_UPDATE_BLOCK;
	for (long p = (long) blockIdx.x * TRSV_UPDATE_BLOCK + threadIdx.x; p < n; p += stride)
	{
		const T d = (T) values[diag_src[p]];
		if (trsv_bad_diagonal(d))
			atomicMin(status, (unsigned) perm[p]);
	}
}

template <typename T>
__global__ __launch_bounds__(TRSV_UPDATE_BLOCK) void
trsv_update_write_kernel(const int * __restrict__ slot_src, const int * __restrict__ diag_src, const double * __restrict__ values,
		T * __restrict__ val, T * __restrict__ diag, const unsigned * status, long slots, long n)
{
	if (*status != TRSV_UPDATE_FINE)          // refused: the handle keeps the values it has
		return;
	const long stride = (long) gridDim.x * TRSV_UPDATE_BLOCK;
	const long t0 = (long) blockIdx.x * TRSV_UPDATE_BLOCK + threadIdx.x;
	// consecutive lanes, consecutive slots: slot_src and val coalesce, values[] is the one gather
	for (long e = t0; e < slots; e += stride)
	{
		const int src = slot_src[e];
		if (src >= 0)
			val[e] = (T) values[src];
	}
	if (diag_src)
		for (long p = t0; p < n; p += stride)
			diag[p] = (T) values[diag_src[p]];
}

static dim3
trsv_update_grid(long work)
{
	return dim3((unsigned) std::min<long>((work + TRSV_UPDATE_BLOCK - 1) / TRSV_UPDATE_BLOCK, TRSV_UPDATE_MAX_GRID));
}

int
launch_trsv_update_check(bool f32, const int * diag_src, const int * perm, const double * values, unsigned * status, long n,
		hipStream_t st)
{
	if (n <= 0)
		return 0;
	const dim3 grid = trsv_update_grid(n), block(TRSV_UPDATE_BLOCK);
	if (f32)
		hipLaunchKernelGGL(trsv_update_check_kernel<float>, grid, block, 0, st, diag_src, perm, values, status, n);
	else
		hipLaunchKernelGGL(trsv_update_check_kernel<double>, grid, block, 0, st, diag_src, perm, values, status, n);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_trsv_update_write(bool f32, const int * slot_src, const int * diag_src, const double * values, void * val, void * diag,
		const unsigned * status, long slots, long n, hipStream_t st)
{
	const long work = std::max(slots, diag_src ? n : 0);
	if (work <= 0)
		return 0;
	const dim3 grid = trsv_update_grid(work), block(TRSV_UPDATE_BLOCK);
	if (f32)
		hipLaunchKernelGGL(trsv_update_write_kernel<float>, grid, block, 0, st, slot_src, diag_src, values, (float *) val, (float *) diag,
				status, slots, n);
	else
		hipLaunchKernelGGL(trsv_update_write_kernel<double>, grid, block, 0, st, slot_src, diag_src, values, (double *) val,
				(double *) diag, status, slots, n);
	HIP_TRY(hipGetLastError());
	return 0;
}

}  // namespace spmv

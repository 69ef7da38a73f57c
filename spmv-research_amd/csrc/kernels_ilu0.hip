// The two kernels of the device ILU(0) (include/spmv_mi355x.h "ILU(0)") over the arrays of ilu0.hpp.
//
// ilu0_level_kernel: one level. A group of LANES lanes (4 .. 64, always inside one wave) owns row i and walks its k steps in
// ascending k:
//     m = f[p] / f[dia[k]]                                   every lane of the group computes the same m
//     the lanes stride over the entries q of row k beyond its diagonal, find column col[q] in row i by binary search over the sorted
//     columns behind p, and where it is stored at r do       f[r] = fma(-m, f[q], f[r])
//     lane 0 stores f[p] = m
// Row k belongs to an earlier level: it was finished by an earlier launch on the same stream, and no row of this launch writes it.
// Inside one step no two lanes touch the same r (row k stores a column once) and r > p, so a step has no conflict of its own.
// BETWEEN steps there is one: step k' > k reads, through other lanes, what step k wrote (its multiplier f[p'] and the f[r] it
// updates). It is closed by a workgroup barrier after every step, the SpGEMM kernels' idiom: the barrier orders the workgroup's global
// stores before its later global loads, and the lanes of a group sit in one workgroup. A workgroup holds ILU0_BLOCK / LANES rows, so
// every group walks as many steps as the workgroup's longest row (its own steps first, then barriers only): the barrier count is
// uniform. f is neither const nor __restrict__ and is never read through a scalar or read-only path.
// Every f[r] receives its fmas in ascending k whatever LANES is and wherever the row runs: the bits are those of the sequential loop.
//
// ilu0_begin_kernel: f = the caller's values, and the pivots of level 0, whose rows have no k step and get no level launch.
// A pivot that is zero or not finite is reported by atomicMin on one word; the minimum does not depend on the order.

#include "ilu0.hpp"

namespace spmv {

__device__ __forceinline__ bool
ilu0_bad_pivot(double v)
{
	return !(fabs(v) <= 1.7976931348623157e308) || v == 0;    // NaN, +-Inf or zero
}

__global__ __launch_bounds__(ILU0_BLOCK) void
ilu0_begin_kernel(const int * __restrict__ dia, const int * __restrict__ rows, double * f, const double * src, unsigned * breakdown,
		long nnz, long count0)
{
	const long stride = (long) gridDim.x * ILU0_BLOCK;
	const long t0 = (long) blockIdx.x * ILU0_BLOCK + threadIdx.x;
	if (src != f)
		for (long e = t0; e < nnz; e += stride)
			f[e] = src[e];
	for (long t = t0; t < count0; t += stride)
	{
		const int i = rows[t];
		if (ilu0_bad_pivot(src[dia[i]]))
			atomicMin(breakdown, (unsigned) i);
	}
}

template <int LANES>
__global__ __launch_bounds__(ILU0_BLOCK) void
ilu0_level_kernel(const int * __restrict__ col, const int * __restrict__ beg, const int * __restrict__ dia,
		const int * __restrict__ end, const int * __restrict__ rows, double * f, unsigned * breakdown, long count)
{
	constexpr int ROWS = ILU0_BLOCK / LANES;
	__shared__ int steps[ROWS];
	const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
	for (long base = (long) blockIdx.x * ROWS; base < count; base += (long) gridDim.x * ROWS)     // uniform in the workgroup
	{
		const bool have = base + grp < count;
		int i = 0, p0 = 0, d = 0, e = 0;
		if (have)
		{
			i = rows[base + grp];
			p0 = beg[i];
			d = dia[i];
			e = end[i];
		}
		if (lane == 0)
			steps[grp] = d - p0;
		__syncthreads();
		int most = 0;
		for (int g = 0; g < ROWS; g++)
			most = max(most, steps[g]);
		for (int s = 0; s < most; s++)
		{
			const int p = p0 + s;
			if (p < d)
			{
				const int k = col[p];
				const int dk = dia[k], ek = end[k];
				const double m = f[p] / f[dk];
				for (int q = dk + 1 + lane; q < ek; q += LANES)
				{
					const int j = col[q];
					int lo = p + 1, hi = e;
					while (lo < hi)
					{
						const int mid = (lo + hi) >> 1;
						if (col[mid] < j)
							lo = mid + 1;
						else
							hi = mid;
					}
					if (lo < e && col[lo] == j)
						f[lo] = fma(-m, f[q], f[lo]);
				}
				if (lane == 0)
					f[p] = m;
			}
			__syncthreads();          // step s of every row of the workgroup is in memory before step s + 1 reads it
		}
		if (have && lane == 0 && ilu0_bad_pivot(f[d]))
			atomicMin(breakdown, (unsigned) i);
		__syncthreads();                  // the next trip rewrites steps[]
	}
}

int
launch_ilu0_begin(const Ilu0Arrays & a, long nnz, const double * src, long count0, hipStream_t st)
{
	const long work = std::max(nnz, count0);
	if (work <= 0)
		return 0;
	const dim3 grid((unsigned) std::min<long>((work + ILU0_BLOCK - 1) / ILU0_BLOCK, ILU0_MAX_GRID)), block(ILU0_BLOCK);
	hipLaunchKernelGGL(ilu0_begin_kernel, grid, block, 0, st, a.dia, a.rows, a.f, src, a.breakdown, nnz, count0);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <int LANES>
static int
level_launch(const Ilu0Arrays & a, long pos0, long count, hipStream_t st)
{
	constexpr int ROWS = ILU0_BLOCK / LANES;
	const dim3 grid((unsigned) std::min<long>((count + ROWS - 1) / ROWS, ILU0_MAX_GRID)), block(ILU0_BLOCK);
	hipLaunchKernelGGL(ilu0_level_kernel<LANES>, grid, block, 0, st, a.col, a.beg, a.dia, a.end, a.rows + pos0, a.f, a.breakdown, count);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_ilu0_level(const Ilu0Arrays & a, long pos0, long count, int lanes, hipStream_t st)
{
	if (count <= 0)
		return 0;
	switch (lanes)
	{
	case 4: return level_launch<4>(a, pos0, count, st);
	case 8: return level_launch<8>(a, pos0, count, st);
	case 16: return level_launch<16>(a, pos0, count, st);
	case 32: return level_launch<32>(a, pos0, count, st);
	default: return level_launch<64>(a, pos0, count, st);
	}
}

}  // namespace spmv

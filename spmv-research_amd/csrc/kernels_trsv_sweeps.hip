// Jacobi sweeps for T x = b over the level-sliced layout of trsv.hpp (DESIGN.md "Triangular solves by Jacobi sweeps"). With
// T = D + N:  x(1) = D^-1 b,  x(m + 1) = D^-1 (b - N x(m)).  One launch is one sweep over ALL n positions, one lane per row, one wave
// per slice: lane r of slice s owns position slice_pos[s] + r and reads entry k of its row at slice_ptr[s] + k * lanes + r, so the
// loads of one k are contiguous across the wave as in the level kernel. The row arithmetic is that of the exact kernels (trsv_rows.hpp:
// entries in stored order, fma_t, one IEEE division), so a row whose inputs are final returns the exact solve's bits: a row of level
// l from sweep l + 1 on, every row from `levels` sweeps on (tests/trsv_sweeps_reference.c is the sequential restatement).
//
// No lane writes what a lane of the same launch gathers: a sweep reads src and writes dst, two different buffers (trsv.hip picks
// them). src is therefore const __restrict__ here, which the exact kernels cannot afford. b and dst are NOT restrict: in the first
// sweep of an in-place solve they are the same vector, read and then written by the one lane that owns the row.
//
// A blocked handle runs the same kernel: its stored columns are block-local, so the gathers index src from the first row of the
// row's block, (perm[p] / block_rows) * block_rows. There is no LDS window and no barrier anywhere in this file.
//
// The first sweep is a kernel of its own (FIRST): x = b / d, or x = b under UNIT. It reads neither val nor col nor src, so an Inf
// or NaN entry cannot reach a one-sweep result, and it can save b for an in-place solve (keep) in the same pass.
//
// KC in {8, 4, 2, 1} columns of row-major blocks: a lane loads its (value, column) pairs once and keeps KC sums, per column the
// chain of the single solve. The single-vector solve IS the KC = 1 instantiation with leading dimensions 1.
//
// Grid: at most TRSV_SWEEP_MAX_GRID workgroups of four waves, each wave striding over the slices; a slice of one row (a level of one
// row) costs a whole wave for one lane, which is the layout's price and is not hidden here.

#include "solvers_common.hpp"
#include "trsv.hpp"
#include "trsv_rows.hpp"

namespace spmv {

constexpr long TRSV_SWEEP_MAX_GRID = 2048;        // 8 workgroups of 256 threads on each of 256 CUs, TRSV_UPDATE_MAX_GRID's rule
constexpr int TRSV_SWEEP_WAVES = TRSV_SWEEP_BLOCK / TRSV_SLICE;

template <typename T>
struct TrsvSweepBlock {
	const T * b;
	const T * src;
	T * dst;
	T * keep;
	long ldb, lds, ldd;
	bool vb, vs, vd;                  // every row of that block is KC-aligned: vector access (keep always is: ld = KC)
};

// slice_pos[s] = level_ptr[l] + (s - level_slice[l]) * TRSV_SLICE for the level l that owns slice s (level_slice is strictly
// increasing: every level has a row), slice_pos[slices] = n. One thread per entry.
__global__ __launch_bounds__(TRSV_SWEEP_BLOCK) void
trsv_sweep_map_kernel(const int * __restrict__ level_ptr, const int * __restrict__ level_slice, int levels, long slices, int n,
		int * __restrict__ slice_pos)
{
	for (long s = (long) blockIdx.x * TRSV_SWEEP_BLOCK + threadIdx.x; s <= slices; s += (long) gridDim.x * TRSV_SWEEP_BLOCK)
	{
		if (s == slices)
		{
			slice_pos[s] = n;
			continue;
		}
		int lo = 0, hi = levels;          // level_slice[lo] <= s < level_slice[hi]
		while (hi - lo > 1)
		{
			const int mid = lo + (hi - lo) / 2;
			if (level_slice[mid] <= s)
				lo = mid;
			else
				hi = mid;
		}
		slice_pos[s] = level_ptr[lo] + (int) (s - level_slice[lo]) * TRSV_SLICE;
	}
}

template <typename T, bool UNIT, int KC, bool FIRST>
__global__ __launch_bounds__(TRSV_SWEEP_BLOCK) void
trsv_sweep_multi_kernel(TrsvTyped<T> a, const int * __restrict__ slice_pos, long slices, int block_rows, TrsvSweepBlock<T> blk)
{
	constexpr int U = trsv_unroll_multi<T, KC>();
	const T * __restrict__ src = blk.src;
	const int r = threadIdx.x % TRSV_SLICE;
	for (long s = (long) blockIdx.x * TRSV_SWEEP_WAVES + threadIdx.x / TRSV_SLICE; s < slices; s += (long) gridDim.x * TRSV_SWEEP_WAVES)
	{
		const int p0 = slice_pos[s];
		const int lanes = slice_pos[s + 1] - p0;          // only a level's last slice is short
		if (r >= lanes)
			continue;
		const int p = p0 + r;
		const int i = a.perm[p];
		T v[KC];
		load_row(v, blk.b + (long) i * blk.ldb, blk.vb);
		if constexpr (FIRST)
		{
			if (blk.keep)
				store_row(blk.keep + (long) i * KC, v, true);
		}
		else
		{
			const int cnt = a.len[p];
			const int64_t base = a.slice_ptr[s] + r;
			const T * xg = src + (block_rows ? (long) (i / block_rows) * block_rows * blk.lds : 0);
			for (int k = 0; k < cnt; k += U)
			{
				T av[U];
				int cv[U];
				trsv_entries_n<T, U>(a, base, lanes, cnt, k, av, cv);
				trsv_apply_multi<T, KC, U>(xg, blk.lds, blk.vs, cnt, k, av, cv, v);
			}
		}
		if constexpr (!UNIT)
		{
			const T d = a.diag[p];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				v[c] = v[c] / d;
		}
		store_row(blk.dst + (long) i * blk.ldd, v, blk.vd);
	}
}

int
launch_trsv_sweep_map(const TrsvArrays & a, long levels, long slices, long n, int * slice_pos, hipStream_t st)
{
	const long grid = std::min<long>(TRSV_SWEEP_MAX_GRID, (slices + 1 + TRSV_SWEEP_BLOCK - 1) / TRSV_SWEEP_BLOCK);
	hipLaunchKernelGGL(trsv_sweep_map_kernel, dim3((unsigned) grid), dim3(TRSV_SWEEP_BLOCK), 0, st, a.level_ptr, a.level_slice,
			(int) levels, slices, (int) n, slice_pos);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_trsv_sweep(bool f32, bool unit, const TrsvArrays & a, const int * slice_pos, long slices, long block_rows, const TrsvSweep & s,
		hipStream_t st)
{
	return trsv_multi_dispatch(f32, unit, s.kc, [&](auto t, auto u, auto kc) {
		using T = decltype(t);
		constexpr bool UNIT = decltype(u)::value;
		constexpr int KC = decltype(kc)::value;
		auto vec = [&](const void * base, long ld) {
			return KC > 1 && base && ld % KC == 0 && (uintptr_t) base % (KC * sizeof(T)) == 0;
		};
		const TrsvSweepBlock<T> blk = {(const T *) s.b, (const T *) s.src, (T *) s.dst, (T *) s.keep, s.ldb, s.lds, s.ldd,
			vec(s.b, s.ldb), vec(s.src, s.lds), vec(s.dst, s.ldd)};
		const long grid = std::min<long>(TRSV_SWEEP_MAX_GRID, (slices + TRSV_SWEEP_WAVES - 1) / TRSV_SWEEP_WAVES);
		if (s.first)
			hipLaunchKernelGGL((trsv_sweep_multi_kernel<T, UNIT, KC, true>), dim3((unsigned) grid), dim3(TRSV_SWEEP_BLOCK), 0, st,
					typed<T>(a), slice_pos, slices, (int) block_rows, blk);
		else
			hipLaunchKernelGGL((trsv_sweep_multi_kernel<T, UNIT, KC, false>), dim3((unsigned) grid), dim3(TRSV_SWEEP_BLOCK), 0, st,
					typed<T>(a), slice_pos, slices, (int) block_rows, blk);
		HIP_TRY(hipGetLastError());
		return 0;
	});
}

}  // namespace spmv

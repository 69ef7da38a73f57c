// The three kernels of the sparse triangular solve T x = b over the level-sliced layout of trsv.hpp. One lane owns one row:
//   s = b[i];  for each kept off-diagonal entry (i, j, a) in stored order: s = fma(-a, x[j], s);  x[i] = s / d_i  (or s under UNIT)
// in the handle's precision, with an IEEE division. A row's result depends on its own entry order only, never on which lane,
// workgroup or launch computes it, so every plan gives the bits of the sequential loop (tests/trsv_reference.c).
//
// trsv_level_kernel: one level, one lane per row, any number of workgroups. Every x[j] it reads belongs to an earlier level and was
// written by an earlier launch on the same stream: the launch boundary is the only ordering between workgroups anywhere in this file.
// trsv_chain_kernel: a run of consecutive thin levels in ONE workgroup, which walks them with a barrier in between.
// trsv_blocked_kernel: the whole solve of a blocked handle, one workgroup per block of rows, each walking its own block's levels with
// its block's part of x in LDS. No workgroup reads what another one writes.
// Each has a k-column form (trsv_*_multi_kernel, at the end of this file) that solves T X = B for a chunk of 8, 4, 2 or 1 columns
// of a row-major block in one pass over the same arrays. The single-vector kernels are not routed through those: they stay as they
// are, and the k-column forms return their bits column by column.
//
// x is read and written inside one launch by the first two kernels (in the chain kernel the reads DEPEND on the writes), and b may be
// x in all three: neither pointer is const, __restrict__ or loaded through a non-temporal / read-only path.

#include <type_traits>

#include "solvers_common.hpp"
#include "trsv.hpp"
#include "trsv_rows.hpp"          // TrsvTyped, typed(), TRSV_UNROLL and the k-column row helpers, shared with the sweep kernels

namespace spmv {

// What a row needs that does not depend on x: where it is, b[i], the diagonal and its first TRSV_UNROLL entries. The chain kernel
// loads it for the NEXT level before the barrier that ends the current one, so that behind the barrier only the gathers of x remain.
template <typename T>
struct TrsvHead {
	int cnt, i, lanes;
	int64_t base;
	T s, d;
	T a[TRSV_UNROLL];
	int c[TRSV_UNROLL];
};

// TRSV_UNROLL entries of a row from entry k on, k < cnt. Slots at or beyond cnt repeat entry k (a valid address: padding is never
// read) and are never used.
template <typename T>
__device__ __forceinline__ void
trsv_entries(const TrsvTyped<T> & a, int64_t base, int lanes, int cnt, int k, T (&av)[TRSV_UNROLL], int (&cv)[TRSV_UNROLL])
{
	#pragma unroll
	for (int j = 0; j < TRSV_UNROLL; j++)
	{
		const int64_t e = base + (int64_t) (k + j < cnt ? k + j : k) * lanes;
		av[j] = a.val[e];
		cv[j] = a.col[e];
	}
}

// the gathers and the fmas of those entries, in stored order
template <typename T>
__device__ __forceinline__ T
trsv_apply(const T * x, int cnt, int k, const T (&av)[TRSV_UNROLL], const int (&cv)[TRSV_UNROLL], T s)
{
	T xv[TRSV_UNROLL];
	#pragma unroll
	for (int j = 0; j < TRSV_UNROLL; j++)
		xv[j] = x[cv[j]];
	#pragma unroll
	for (int j = 0; j < TRSV_UNROLL; j++)
		if (k + j < cnt)
			s = fma_t<T>(-av[j], xv[j], s);
	return s;
}

// row number q of a level that starts at position pos0 with `rows` rows and slice slice0
template <typename T, bool UNIT>
__device__ __forceinline__ void
trsv_head(const TrsvTyped<T> & a, int pos0, int rows, int slice0, int q, const T * b, TrsvHead<T> & h)
{
	const int p = pos0 + q;
	const int first = q & ~(TRSV_SLICE - 1);                                  // first row of this lane's slice within the level
	h.lanes = rows - first < TRSV_SLICE ? rows - first : TRSV_SLICE;          // only a level's last slice is short
	h.base = a.slice_ptr[slice0 + q / TRSV_SLICE] + (q - first);
	h.cnt = a.len[p];
	h.i = a.perm[p];
	h.s = b[h.i];
	h.d = UNIT ? (T) 1 : a.diag[p];
	if (h.cnt > 0)
		trsv_entries<T>(a, h.base, h.lanes, h.cnt, 0, h.a, h.c);
	else
	{
		#pragma unroll
		for (int j = 0; j < TRSV_UNROLL; j++)
		{
			h.a[j] = 0;
			h.c[j] = h.i;
		}
	}
}

// x[i] of the row whose head is h; xg is what the stored columns index: x itself, or the block's part of x in LDS
template <typename T, bool UNIT>
__device__ __forceinline__ T
trsv_value(const TrsvTyped<T> & a, const TrsvHead<T> & h, const T * xg)
{
	T s = h.s;
	if (h.cnt > 0)
		s = trsv_apply<T>(xg, h.cnt, 0, h.a, h.c, s);
	for (int k = TRSV_UNROLL; k < h.cnt; k += TRSV_UNROLL)
	{
		T av[TRSV_UNROLL];
		int cv[TRSV_UNROLL];
		trsv_entries<T>(a, h.base, h.lanes, h.cnt, k, av, cv);
		s = trsv_apply<T>(xg, h.cnt, k, av, cv, s);
	}
	return UNIT ? s : s / h.d;
}

template <typename T, bool UNIT>
__device__ __forceinline__ void
trsv_finish(const TrsvTyped<T> & a, const TrsvHead<T> & h, T * x)
{
	x[h.i] = trsv_value<T, UNIT>(a, h, x);
}

template <typename T, bool UNIT>
__device__ __forceinline__ void
trsv_row(const TrsvTyped<T> & a, int pos0, int rows, int slice0, int q, const T * b, T * x)
{
	TrsvHead<T> h;
	trsv_head<T, UNIT>(a, pos0, rows, slice0, q, b, h);
	trsv_finish<T, UNIT>(a, h, x);
}

template <typename T, bool UNIT>
__global__ __launch_bounds__(TRSV_LEVEL_BLOCK) void
trsv_level_kernel(TrsvTyped<T> a, int pos0, int rows, int slice0, const T * b, T * x)
{
	const int q = blockIdx.x * TRSV_LEVEL_BLOCK + threadIdx.x;
	if (q < rows)
		trsv_row<T, UNIT>(a, pos0, rows, slice0, q, b, x);
}

// ONE workgroup. The loop over the levels and the barrier in it are uniform: every thread executes every barrier, whether or not
// a level has a row for it.
// What orders level l's stores of x before level l + 1's loads: all waves of a workgroup run on one CU and go through that CU's
// vector L1, which is write-through and sees its own CU's stores, so workgroup scope is all this hand-off needs; no agent-scope
// fence, which exists for readers on OTHER CUs. But s_barrier itself waits for no memory counter: beside the barrier every storing
// wave must have drained its stores (s_waitcnt vmcnt(0)) BEFORE it arrives, and the compiler must not move a load of x across the
// barrier. The explicit wait gives the first on every path, __syncthreads() (a workgroup-scope release / acquire pair around
// s_barrier) the second.
// A thread's first row of the next level is begun (trsv_head: nothing of it reads x; b[i], which may be x[i], is written by this
// thread alone) before that wait, so its loads fly while the stores drain and only the gathers of x follow the barrier.
template <typename T, bool UNIT>
__global__ __launch_bounds__(TRSV_CHAIN_BLOCK_MAX) void
trsv_chain_kernel(TrsvTyped<T> a, int l0, int l1, const T * b, T * x)
{
	const int t = threadIdx.x;
	int pos0 = a.level_ptr[l0], end = a.level_ptr[l0 + 1], slice0 = a.level_slice[l0];
	TrsvHead<T> h;
	bool have = t < end - pos0;
	if (have)
		trsv_head<T, UNIT>(a, pos0, end - pos0, slice0, t, b, h);
	for (int l = l0; l < l1; l++)
	{
		const int rows = end - pos0;
		if (have)
			trsv_finish<T, UNIT>(a, h, x);
		for (int q = t + blockDim.x; q < rows; q += blockDim.x)
			trsv_row<T, UNIT>(a, pos0, rows, slice0, q, b, x);
		if (l + 1 < l1)
		{
			pos0 = end;
			end = a.level_ptr[l + 2];
			slice0 = a.level_slice[l + 1];
			have = t < end - pos0;
			if (have)
				trsv_head<T, UNIT>(a, pos0, end - pos0, slice0, t, b, h);
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
	}
}

// ONE WORKGROUP PER BLOCK of block_rows rows; workgroup blk walks the levels block_level[blk] .. block_level[blk + 1] - 1 of its own
// block and keeps the block's part of x in LDS (xs, min(block_rows, n) values of dynamic LDS), which the stored block-local columns
// index directly. Every x[j] a row gathers is a row of the same block and an earlier level: it is read from xs, never from global
// memory. Nothing in this launch reads global x at all; x is only stored to, for the caller.
// The loop over the levels and the barrier in it are uniform per workgroup: every thread executes every barrier of its block, whether
// or not a level has a row for it, and nothing returns before the last one. Different workgroups have different trip counts and share
// nothing: no flag, no atomic, no ordering between them.
// What orders level l's writes before level l + 1's reads: both are LDS accesses of one workgroup, and __syncthreads() is exactly
// that hand-off (every wave waits for its own LDS operations, lgkmcnt(0), before it arrives at s_barrier, and no LDS read is moved
// across it). The chain kernel's s_waitcnt vmcnt(0) is absent ON PURPOSE: it drains the global stores of x because that kernel reads
// them back through the L1; here nobody reads them, so they stay in flight across the levels and only the end of the kernel waits
// for them. xs is never initialised: a row reads only slots that an earlier level of this launch wrote.
// b may be x: a thread reads b[i] (in trsv_head, possibly a level ahead) before the same thread writes x[i], and no other thread of
// any workgroup touches element i.
// As in the chain kernel a thread's first row of the next level is begun before the barrier, so its loads (position, length, b[i],
// diagonal, first entries) fly across it and only LDS reads follow the barrier.
template <typename T, bool UNIT>
__global__ __launch_bounds__(TRSV_BLOCKED_THREADS_MAX) void
trsv_blocked_kernel(TrsvTyped<T> a, int block_rows, const T * b, T * x)
{
	extern __shared__ __align__(16) unsigned char trsv_lds[];
	T * xs = reinterpret_cast<T *>(trsv_lds);
	const int t = threadIdx.x;
	const int row0 = blockIdx.x * block_rows;       // < n < 2^31
	const int l0 = a.block_level[blockIdx.x], l1 = a.block_level[blockIdx.x + 1];
	int pos0 = a.level_ptr[l0], end = a.level_ptr[l0 + 1], slice0 = a.level_slice[l0];
	TrsvHead<T> h;
	bool have = t < end - pos0;
	if (have)
		trsv_head<T, UNIT>(a, pos0, end - pos0, slice0, t, b, h);
	for (int l = l0; l < l1; l++)
	{
		const int rows = end - pos0;
		if (have)
		{
			const T v = trsv_value<T, UNIT>(a, h, xs);
			xs[h.i - row0] = v;
			x[h.i] = v;
		}
		for (int q = t + blockDim.x; q < rows; q += blockDim.x)
		{
			TrsvHead<T> g;
			trsv_head<T, UNIT>(a, pos0, rows, slice0, q, b, g);
			const T v = trsv_value<T, UNIT>(a, g, xs);
			xs[g.i - row0] = v;
			x[g.i] = v;
		}
		if (l + 1 < l1)
		{
			pos0 = end;
			end = a.level_ptr[l + 2];
			slice0 = a.level_slice[l + 1];
			have = t < end - pos0;
			if (have)
				trsv_head<T, UNIT>(a, pos0, end - pos0, slice0, t, b, h);
		}
		__syncthreads();
	}
}

template <typename T, bool UNIT>
static void
level_launch(const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st)
{
	const unsigned grid = (unsigned) ((s.rows + TRSV_LEVEL_BLOCK - 1) / TRSV_LEVEL_BLOCK);
	hipLaunchKernelGGL((trsv_level_kernel<T, UNIT>), dim3(grid), dim3(TRSV_LEVEL_BLOCK), 0, st, typed<T>(a), s.pos0, s.rows, s.slice0,
			(const T *) b, (T *) x);
}

template <typename T, bool UNIT>
static void
chain_launch(const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st)
{
	hipLaunchKernelGGL((trsv_chain_kernel<T, UNIT>), dim3(1), dim3(s.block), 0, st, typed<T>(a), s.l0, s.l1, (const T *) b, (T *) x);
}

int
launch_trsv_level(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st)
{
	if (f32)
		unit ? level_launch<float, true>(a, s, b, x, st) : level_launch<float, false>(a, s, b, x, st);
	else
		unit ? level_launch<double, true>(a, s, b, x, st) : level_launch<double, false>(a, s, b, x, st);
	return 0;
}

int
launch_trsv_chain(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st)
{
	if (f32)
		unit ? chain_launch<float, true>(a, s, b, x, st) : chain_launch<float, false>(a, s, b, x, st);
	else
		unit ? chain_launch<double, true>(a, s, b, x, st) : chain_launch<double, false>(a, s, b, x, st);
	return 0;
}

template <typename T, bool UNIT>
static int
blocked_launch(const TrsvArrays & a, long blocks, int threads, long block_rows, long n, const void * b, void * x, hipStream_t st)
{
	const int lds_bytes = (int) (std::min(block_rows, n) * (long) sizeof(T));
	// more than 64 KiB of dynamic LDS has to be granted per kernel function, once per device
	static int granted[64] = {0};
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	dev = dev < 0 || dev >= 64 ? 0 : dev;
	if (lds_bytes > granted[dev])
	{
		HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&trsv_blocked_kernel<T, UNIT>),
				hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
		granted[dev] = lds_bytes;
	}
	hipLaunchKernelGGL((trsv_blocked_kernel<T, UNIT>), dim3((unsigned) blocks), dim3(threads), lds_bytes, st, typed<T>(a),
			(int) block_rows, (const T *) b, (T *) x);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_trsv_blocked(bool f32, bool unit, const TrsvArrays & a, long blocks, int threads, long block_rows, long n, const void * b,
		void * x, hipStream_t st)
{
	if (f32)
		return unit ? blocked_launch<float, true>(a, blocks, threads, block_rows, n, b, x, st)
		            : blocked_launch<float, false>(a, blocks, threads, block_rows, n, b, x, st);
	return unit ? blocked_launch<double, true>(a, blocks, threads, block_rows, n, b, x, st)
	            : blocked_launch<double, false>(a, blocks, threads, block_rows, n, b, x, st);
}

// ------------------------------------------------------------------------------------------------ k columns
// T X = B for a chunk of KC in {8, 4, 2, 1} columns of row-major blocks (row i at b + i * ldb and x + i * ldx, both pointers already
// at the chunk's first column), over the same layout and the same plan. One lane still owns one row: it loads len, perm, the
// diagonal and every (a, col) pair ONCE and keeps KC partial sums; the KC values of x[col] are one row of the block, gathered by
// load_row (one vector load where the rows are KC-aligned, vb / vx, else KC scalar loads). Per column the fma chain runs in stored
// order and ends in the same IEEE division, so column j returns the bits of the single kernels on column j whatever chunk it sits in.
// The ordering between levels is that of the single kernels, word for word: the launch boundary (level), s_waitcnt vmcnt(0) +
// __syncthreads() (chain), __syncthreads() over LDS (blocked). The head prefetch across the barrier is KEPT for every KC: the head
// holds KC sums in place of one (16 VGPRs at KC = 8 in fp64), and nothing of it reads x.
// In place (b == x, ldb == ldx): a lane reads its own row of b (in the head) before it writes its own row of x, and no other lane
// touches that row's KC columns.
// Registers: the gathers of one trip are U * KC values, so U shrinks as KC * sizeof(T) grows (trsv_unroll_multi); the order of the
// fmas does not depend on U. profiles/r28_trsv_multi.txt has the compiler's resource table: no instantiation uses scratch.

template <typename T>
struct TrsvBlock {
	const T * b;
	T * x;
	long ldb, ldx;
	bool vb, vx;                      // every row of the chunk is KC-aligned: vector access
};

template <typename T, int KC>
struct TrsvHeadMulti {
	static constexpr int U = trsv_unroll_multi<T, KC>();
	int cnt, i, lanes;
	int64_t base;
	T d;
	T s[KC];
	T a[U];
	int c[U];
};

template <typename T, bool UNIT, int KC>
__device__ __forceinline__ void
trsv_head_multi(const TrsvTyped<T> & a, int pos0, int rows, int slice0, int q, const TrsvBlock<T> & blk, TrsvHeadMulti<T, KC> & h)
{
	constexpr int U = TrsvHeadMulti<T, KC>::U;
	const int p = pos0 + q;
	const int first = q & ~(TRSV_SLICE - 1);
	h.lanes = rows - first < TRSV_SLICE ? rows - first : TRSV_SLICE;
	h.base = a.slice_ptr[slice0 + q / TRSV_SLICE] + (q - first);
	h.cnt = a.len[p];
	h.i = a.perm[p];
	load_row(h.s, blk.b + (long) h.i * blk.ldb, blk.vb);
	h.d = UNIT ? (T) 1 : a.diag[p];
	if (h.cnt > 0)
		trsv_entries_n<T, U>(a, h.base, h.lanes, h.cnt, 0, h.a, h.c);
	else
	{
		#pragma unroll
		for (int j = 0; j < U; j++)
		{
			h.a[j] = 0;
			h.c[j] = 0;
		}
	}
}

// the KC values of row h.i
template <typename T, bool UNIT, int KC>
__device__ __forceinline__ void
trsv_value_multi(const TrsvTyped<T> & a, const TrsvHeadMulti<T, KC> & h, const T * xg, long ldg, bool vg, T (&v)[KC])
{
	constexpr int U = TrsvHeadMulti<T, KC>::U;
	#pragma unroll
	for (int c = 0; c < KC; c++)
		v[c] = h.s[c];
	if (h.cnt > 0)
		trsv_apply_multi<T, KC, U>(xg, ldg, vg, h.cnt, 0, h.a, h.c, v);
	for (int k = U; k < h.cnt; k += U)
	{
		T av[U];
		int cv[U];
		trsv_entries_n<T, U>(a, h.base, h.lanes, h.cnt, k, av, cv);
		trsv_apply_multi<T, KC, U>(xg, ldg, vg, h.cnt, k, av, cv, v);
	}
	if (!UNIT)
	{
		#pragma unroll
		for (int c = 0; c < KC; c++)
			v[c] = v[c] / h.d;
	}
}

template <typename T, bool UNIT, int KC>
__device__ __forceinline__ void
trsv_finish_multi(const TrsvTyped<T> & a, const TrsvHeadMulti<T, KC> & h, const TrsvBlock<T> & blk)
{
	T v[KC];
	trsv_value_multi<T, UNIT, KC>(a, h, blk.x, blk.ldx, blk.vx, v);
	store_row(blk.x + (long) h.i * blk.ldx, v, blk.vx);
}

template <typename T, bool UNIT, int KC>
__device__ __forceinline__ void
trsv_row_multi(const TrsvTyped<T> & a, int pos0, int rows, int slice0, int q, const TrsvBlock<T> & blk)
{
	TrsvHeadMulti<T, KC> h;
	trsv_head_multi<T, UNIT, KC>(a, pos0, rows, slice0, q, blk, h);
	trsv_finish_multi<T, UNIT, KC>(a, h, blk);
}

template <typename T, bool UNIT, int KC>
__global__ __launch_bounds__(TRSV_LEVEL_BLOCK) void
trsv_level_multi_kernel(TrsvTyped<T> a, int pos0, int rows, int slice0, TrsvBlock<T> blk)
{
	const int q = blockIdx.x * TRSV_LEVEL_BLOCK + threadIdx.x;
	if (q < rows)
		trsv_row_multi<T, UNIT, KC>(a, pos0, rows, slice0, q, blk);
}

// trsv_chain_kernel for KC columns: ONE workgroup, the same uniform loop, the same drain of the stores of x before the barrier
template <typename T, bool UNIT, int KC>
__global__ __launch_bounds__(TRSV_CHAIN_BLOCK_MAX) void
trsv_chain_multi_kernel(TrsvTyped<T> a, int l0, int l1, TrsvBlock<T> blk)
{
	const int t = threadIdx.x;
	int pos0 = a.level_ptr[l0], end = a.level_ptr[l0 + 1], slice0 = a.level_slice[l0];
	TrsvHeadMulti<T, KC> h;
	bool have = t < end - pos0;
	if (have)
		trsv_head_multi<T, UNIT, KC>(a, pos0, end - pos0, slice0, t, blk, h);
	for (int l = l0; l < l1; l++)
	{
		const int rows = end - pos0;
		if (have)
			trsv_finish_multi<T, UNIT, KC>(a, h, blk);
		for (int q = t + blockDim.x; q < rows; q += blockDim.x)
			trsv_row_multi<T, UNIT, KC>(a, pos0, rows, slice0, q, blk);
		if (l + 1 < l1)
		{
			pos0 = end;
			end = a.level_ptr[l + 2];
			slice0 = a.level_slice[l + 1];
			have = t < end - pos0;
			if (have)
				trsv_head_multi<T, UNIT, KC>(a, pos0, end - pos0, slice0, t, blk, h);
		}
		asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
		__syncthreads();
	}
}

// trsv_blocked_kernel for KC columns: the block's part of X lives in LDS as xs[(i - row0) * KC + c], min(block_rows, n) * KC values,
// and a stored block-local column names a row of KC values there. Nothing reads global x; only __syncthreads() orders the levels.
template <typename T, bool UNIT, int KC>
__global__ __launch_bounds__(TRSV_BLOCKED_THREADS_MAX) void
trsv_blocked_multi_kernel(TrsvTyped<T> a, int block_rows, TrsvBlock<T> blk)
{
	extern __shared__ __align__(64) unsigned char trsv_lds_multi[];
	T * xs = reinterpret_cast<T *>(trsv_lds_multi);
	const int t = threadIdx.x;
	const int row0 = blockIdx.x * block_rows;       // < n < 2^31
	const int l0 = a.block_level[blockIdx.x], l1 = a.block_level[blockIdx.x + 1];
	int pos0 = a.level_ptr[l0], end = a.level_ptr[l0 + 1], slice0 = a.level_slice[l0];
	TrsvHeadMulti<T, KC> h;
	bool have = t < end - pos0;
	if (have)
		trsv_head_multi<T, UNIT, KC>(a, pos0, end - pos0, slice0, t, blk, h);
	for (int l = l0; l < l1; l++)
	{
		const int rows = end - pos0;
		if (have)
		{
			T v[KC];
			trsv_value_multi<T, UNIT, KC>(a, h, xs, KC, true, v);
			store_row(xs + (h.i - row0) * KC, v, true);
			store_row(blk.x + (long) h.i * blk.ldx, v, blk.vx);
		}
		for (int q = t + blockDim.x; q < rows; q += blockDim.x)
		{
			TrsvHeadMulti<T, KC> g;
			T v[KC];
			trsv_head_multi<T, UNIT, KC>(a, pos0, rows, slice0, q, blk, g);
			trsv_value_multi<T, UNIT, KC>(a, g, xs, KC, true, v);
			store_row(xs + (g.i - row0) * KC, v, true);
			store_row(blk.x + (long) g.i * blk.ldx, v, blk.vx);
		}
		if (l + 1 < l1)
		{
			pos0 = end;
			end = a.level_ptr[l + 2];
			slice0 = a.level_slice[l + 1];
			have = t < end - pos0;
			if (have)
				trsv_head_multi<T, UNIT, KC>(a, pos0, end - pos0, slice0, t, blk, h);
		}
		__syncthreads();
	}
}

// the chunk's view of the two blocks: vector access when ld % KC == 0, c0 % KC == 0 and the block's base is aligned to KC values
template <typename T, int KC>
static TrsvBlock<T>
trsv_block(const TrsvCols & c)
{
	auto vec = [&](const void * base, long ld) {
		return KC > 1 && ld % KC == 0 && c.c0 % KC == 0 && (uintptr_t) base % (KC * sizeof(T)) == 0;
	};
	return TrsvBlock<T>{(const T *) c.b + c.c0, (T *) c.x + c.c0, c.ldb, c.ldx, vec(c.b, c.ldb), vec(c.x, c.ldx)};
}

int
launch_trsv_level_multi(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const TrsvCols & c, hipStream_t st)
{
	return trsv_multi_dispatch(f32, unit, c.kc, [&](auto t, auto u, auto kc) {
		using T = decltype(t);
		constexpr bool UNIT = decltype(u)::value;
		constexpr int KC = decltype(kc)::value;
		const unsigned grid = (unsigned) ((s.rows + TRSV_LEVEL_BLOCK - 1) / TRSV_LEVEL_BLOCK);
		hipLaunchKernelGGL((trsv_level_multi_kernel<T, UNIT, KC>), dim3(grid), dim3(TRSV_LEVEL_BLOCK), 0, st, typed<T>(a), s.pos0, s.rows,
				s.slice0, trsv_block<T, KC>(c));
		return 0;
	});
}

int
launch_trsv_chain_multi(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const TrsvCols & c, hipStream_t st)
{
	return trsv_multi_dispatch(f32, unit, c.kc, [&](auto t, auto u, auto kc) {
		using T = decltype(t);
		constexpr bool UNIT = decltype(u)::value;
		constexpr int KC = decltype(kc)::value;
		hipLaunchKernelGGL((trsv_chain_multi_kernel<T, UNIT, KC>), dim3(1), dim3(s.block), 0, st, typed<T>(a), s.l0, s.l1,
				trsv_block<T, KC>(c));
		return 0;
	});
}

template <typename T, bool UNIT, int KC>
static int
blocked_multi_launch(const TrsvArrays & a, long blocks, int threads, long block_rows, long n, const TrsvCols & c, hipStream_t st)
{
	const int lds_bytes = (int) (std::min(block_rows, n) * KC * (long) sizeof(T));
	// as in blocked_launch: the grant is per kernel function, so per instantiation, once per device
	static int granted[64] = {0};
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	dev = dev < 0 || dev >= 64 ? 0 : dev;
	if (lds_bytes > granted[dev])
	{
		HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&trsv_blocked_multi_kernel<T, UNIT, KC>),
				hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
		granted[dev] = lds_bytes;
	}
	hipLaunchKernelGGL((trsv_blocked_multi_kernel<T, UNIT, KC>), dim3((unsigned) blocks), dim3(threads), lds_bytes, st, typed<T>(a),
			(int) block_rows, trsv_block<T, KC>(c));
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_trsv_blocked_multi(bool f32, bool unit, const TrsvArrays & a, long blocks, int threads, long block_rows, long n,
		const TrsvCols & c, hipStream_t st)
{
	return trsv_multi_dispatch(f32, unit, c.kc, [&](auto t, auto u, auto kc) {
		return blocked_multi_launch<decltype(t), decltype(u)::value, decltype(kc)::value>(a, blocks, threads, block_rows, n, c, st);
	});
}

}  // namespace spmv

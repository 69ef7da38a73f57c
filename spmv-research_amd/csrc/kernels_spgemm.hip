// The row kernel of the sparse product C = A B (include/spmv_mi355x.h "SpGEMM", spgemm.hpp for the mapping), in three modes over one
// body:
//   COUNT    the distinct columns of every row of C (and the probes its insertions took beyond their first);
//   FILL     the row's columns, sorted ascending in the table itself (bitonic: a free slot holds SPGEMM_EMPTY, the largest int32, so
//            the w columns end up in front), into c_ci;
//   NUMERIC  the values: acc[j] = fma(a_p, b_q, acc[j]) for the entries p of A's row in stored order, one step per p.
//
// A row's phases, each closed by a workgroup barrier:
//   1. the table cleared (keys SPGEMM_EMPTY, values +0.0);
//   2. the insertions. COUNT and FILL only claim keys, and a claim is a compare-and-swap: the order of the insertions does not
//      matter and the phase holds no barrier. NUMERIC runs one entry of A per step with a barrier after every step: within a step
//      the row's lanes stride over ONE row of B, whose columns are distinct, so every lane owns the slot it finds or claims and
//      updates its value with a plain load and store; the barrier orders that store before the loads of the next step, where the
//      slot may belong to another lane. Every C(i, j) is therefore one fma chain in the order of A's entries;
//   3. COUNT: the occupied slots counted;  FILL: the table sorted, one barrier per stage, then its first w keys stored;
//      NUMERIC: the row's lanes walk the row of c_ci, look every column up in the table and store its value: reads and writes of
//      global memory are contiguous, and the search is a probe in LDS.
// Barriers: every loop that holds one has the same trip count in all threads of the workgroup (the grid-stride loop over the bin's
// list, the widest row of A among the workgroup's rows, and the stages of a sort over a table size that is the bin's constant or,
// in the global bin with one row per workgroup, that row's own).
// Nothing is written outside the row's own table, its own entries of c_ci / c_va, its own words of width / probes, and the error word.

#include "spgemm.hpp"

namespace spmv {

// the slot of `col` in the row's table, claimed if it is new; -1 when T probes found neither (a full table: the sizing rule T >= 2 w
// rules it out, the bound turns a bug into the error word instead of a hang)
__device__ __forceinline__ long
spgemm_slot(int * keys, int log_t, long T, int col, int & extra)
{
	long s = (long) (((unsigned) col * SPGEMM_HASH_MUL) >> (32 - log_t));
	for (long probe = 0; probe < T; probe++)
	{
		int cur = __hip_atomic_load(&keys[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
		if (cur == SPGEMM_EMPTY)
		{
			// on success cur keeps SPGEMM_EMPTY, on failure it becomes the key another lane put there meanwhile
			if (__hip_atomic_compare_exchange_strong(&keys[s], &cur, col, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP))
				return s;
		}
		if (cur == col)
			return s;
		s = (s + 1) & (T - 1);
		extra++;
	}
	return -1;
}

// the slot that holds `col`, -1 if the table does not hold it; the table is complete and no longer changes (after a barrier)
__device__ __forceinline__ long
spgemm_find(const int * keys, int log_t, long T, int col)
{
	long s = (long) (((unsigned) col * SPGEMM_HASH_MUL) >> (32 - log_t));
	for (long probe = 0; probe < T; probe++)
	{
		const int cur = keys[s];
		if (cur == col)
			return s;
		if (cur == SPGEMM_EMPTY)
			return -1;
		s = (s + 1) & (T - 1);
	}
	return -1;
}

template <int LOG_T, int LANES, int ROWS, int MODE>          // LOG_T == 0: the global bin
__global__ __launch_bounds__(LANES * ROWS) void
spgemm_rows_kernel(SpgemmArrays A, const int * __restrict__ bin_rows, long count)
{
	constexpr bool GLOBAL = LOG_T == 0;
	constexpr bool NUMERIC = MODE == SPGEMM_NUMERIC;
	constexpr int T_LDS = GLOBAL ? 1 : (1 << LOG_T);
	__shared__ int K[ROWS][T_LDS];
	__shared__ double V[NUMERIC ? ROWS : 1][NUMERIC ? T_LDS : 1];
	__shared__ int steps[ROWS];

	const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
	int * keys;
	double * vals = nullptr;
	if constexpr (GLOBAL)
	{
		keys = A.slab_keys + (size_t) blockIdx.x * A.slab_t;
		if constexpr (NUMERIC)
			vals = A.slab_vals + (size_t) blockIdx.x * A.slab_t;
	}
	else
	{
		keys = K[grp];
		if constexpr (NUMERIC)
			vals = V[grp];
	}

	// the trip count is the same in every thread of the workgroup: the loop holds barriers
	for (long base = (long) blockIdx.x * ROWS; base < count; base += (long) gridDim.x * ROWS)
	{
		const long slot = base + grp;
		const bool live = slot < count;
		const int i = live ? bin_rows[slot] : 0;
		const int p0 = live ? A.a_rp[i] : 0, p1 = live ? A.a_rp[i + 1] : 0;
		const int c0 = (live && MODE != SPGEMM_COUNT) ? A.c_rp[i] : 0;
		long w = 0;                                           // what the table is sized on
		if (live)
			w = MODE == SPGEMM_COUNT ? min(A.products[i], A.n) : (long) (A.c_rp[i + 1] - c0);
		int log_t = LOG_T;
		bool bad = false;
		if constexpr (GLOBAL)
		{
			log_t = spgemm_log_table(max(w, 1L));
			if (((long) 1 << log_t) > A.slab_t)               // the host sized the slab on the bin's widest row: this never bites
			{
				bad = true;
				log_t = spgemm_log_table(A.slab_t / 2);
			}
		}
		const long T = (long) 1 << log_t;
		// 1.
		for (long t = lane; t < T; t += LANES)
		{
			keys[t] = SPGEMM_EMPTY;
			if constexpr (NUMERIC)
				vals[t] = 0.0;
		}
		if (lane == 0)
			steps[grp] = p1 - p0;
		__syncthreads();
		// 2.
		int extra = 0;
		if constexpr (!NUMERIC)
		{
			for (int p = p0; p < p1; p++)
			{
				const int l = A.a_ci[p];
				const int q1 = A.b_rp[l + 1];
				for (int q = A.b_rp[l] + lane; q < q1; q += LANES)
					bad = spgemm_slot(keys, log_t, T, A.b_ci[q], extra) < 0 || bad;
			}
			__syncthreads();
		}
		else
		{
			int smax = 0;
			for (int r = 0; r < ROWS; r++)
				smax = max(smax, steps[r]);
			for (int st = 0; st < smax; st++)
			{
				const int p = p0 + st;
				if (p < p1)
				{
					const int l = A.a_ci[p];
					const double a = A.a_va[p];
					const int q1 = A.b_rp[l + 1];
					for (int q = A.b_rp[l] + lane; q < q1; q += LANES)
					{
						const long s = spgemm_slot(keys, log_t, T, A.b_ci[q], extra);
						if (s >= 0)
							vals[s] = fma(a, A.b_va[q], vals[s]);
						else
							bad = true;
					}
				}
				__syncthreads();
			}
		}
		if (bad)
			*A.error = i + 1;
		// 3.
		if constexpr (MODE == SPGEMM_COUNT)
		{
			int c = 0;
			for (long t = lane; t < T; t += LANES)
				c += keys[t] != SPGEMM_EMPTY;
			c = group_reduce_sum<int, LANES>(c);
			extra = group_reduce_sum<int, LANES>(extra);
			if (lane == 0 && live)
			{
				A.width[i] = c;
				A.probes[i] = extra;
			}
		}
		else if constexpr (MODE == SPGEMM_FILL)
		{
			for (long k2 = 2; k2 <= T; k2 <<= 1)
				for (long j = k2 >> 1; j > 0; j >>= 1)
				{
					for (long t = lane; t < T / 2; t += LANES)
					{
						const long lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
						const int x = keys[lo], y = keys[hi];
						if ((x > y) == ((lo & k2) == 0))
						{
							keys[lo] = y;
							keys[hi] = x;
						}
					}
					__syncthreads();
				}
			for (long t = lane; t < min(w, T); t += LANES)
				A.c_ci[c0 + t] = keys[t];
		}
		else
		{
			for (long t = lane; t < w; t += LANES)
			{
				const long s = spgemm_find(keys, log_t, T, A.c_ci[c0 + t]);
				if (s >= 0)
					A.c_va[c0 + t] = vals[s];
				else
					*A.error = i + 1;
			}
		}
		__syncthreads();                              // the next trip clears the row's table
	}
}

__global__ __launch_bounds__(256) void
spgemm_products_kernel(long m, const int * __restrict__ a_rp, const int * __restrict__ a_ci, const int * __restrict__ b_rp,
		long * __restrict__ products)
{
	for (long i = (long) blockIdx.x * blockDim.x + threadIdx.x; i < m; i += (long) gridDim.x * blockDim.x)
	{
		long sum = 0;
		for (int p = a_rp[i]; p < a_rp[i + 1]; p++)
			sum += b_rp[a_ci[p] + 1] - b_rp[a_ci[p]];
		products[i] = sum;
	}
}

__global__ __launch_bounds__(256) void
spgemm_narrow_kernel(const long * __restrict__ offsets, int * __restrict__ row_ptr, long count)
{
	for (long i = (long) blockIdx.x * blockDim.x + threadIdx.x; i < count; i += (long) gridDim.x * blockDim.x)
		row_ptr[i] = (int) offsets[i];
}

int
launch_spgemm_products(long m, const int * a_rp, const int * a_ci, const int * b_rp, long * products, hipStream_t st)
{
	if (m <= 0)
		return 0;
	const dim3 grid((unsigned) std::min<long>((m + 255) / 256, 4 * SPGEMM_MAX_GRID)), block(256);
	hipLaunchKernelGGL(spgemm_products_kernel, grid, block, 0, st, m, a_rp, a_ci, b_rp, products);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_spgemm_narrow(const long * offsets, int * row_ptr, long count, hipStream_t st)
{
	if (count <= 0)
		return 0;
	const dim3 grid((unsigned) std::min<long>((count + 255) / 256, 4 * SPGEMM_MAX_GRID)), block(256);
	hipLaunchKernelGGL(spgemm_narrow_kernel, grid, block, 0, st, offsets, row_ptr, count);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <int BIN, int MODE>
static int
launch_bin(const SpgemmArrays & a, const int * bin_rows, long count, int grid_size, hipStream_t st)
{
	constexpr int LOG_T = BIN < SPGEMM_BINS - 1 ? SPGEMM_BIN_LOG_T[BIN < SPGEMM_BINS - 1 ? BIN : 0] : 0;
	constexpr int LANES = SPGEMM_BIN_LANES[BIN], ROWS = SPGEMM_BIN_ROWS[BIN];
	const dim3 grid((unsigned) grid_size), block(LANES * ROWS);
	hipLaunchKernelGGL((spgemm_rows_kernel<LOG_T, LANES, ROWS, MODE>), grid, block, 0, st, a, bin_rows, count);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <int MODE>
static int
launch_mode(int bin, const SpgemmArrays & a, const int * bin_rows, long count, int grid, hipStream_t st)
{
	switch (bin)
	{
		case 0: return launch_bin<0, MODE>(a, bin_rows, count, grid, st);
		case 1: return launch_bin<1, MODE>(a, bin_rows, count, grid, st);
		case 2: return launch_bin<2, MODE>(a, bin_rows, count, grid, st);
		case 3: return launch_bin<3, MODE>(a, bin_rows, count, grid, st);
		case 4: return launch_bin<4, MODE>(a, bin_rows, count, grid, st);
		case 5: return launch_bin<5, MODE>(a, bin_rows, count, grid, st);
		default: return launch_bin<SPGEMM_BINS - 1, MODE>(a, bin_rows, count, grid, st);
	}
}

int
launch_spgemm_rows(int mode, int bin, const SpgemmArrays & a, const int * bin_rows, long count, int grid, hipStream_t st)
{
	if (count <= 0 || grid <= 0)
		return 0;
	switch (mode)
	{
		case SPGEMM_COUNT: return launch_mode<SPGEMM_COUNT>(bin, a, bin_rows, count, grid, st);
		case SPGEMM_FILL: return launch_mode<SPGEMM_FILL>(bin, a, bin_rows, count, grid, st);
		default: return launch_mode<SPGEMM_NUMERIC>(bin, a, bin_rows, count, grid, st);
	}
}

}  // namespace spmv

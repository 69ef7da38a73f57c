// The kernels of the multicolour ordering (include/spmv_mi355x.h "multicolour ordering", color.hpp for the graph, the rule and the
// mapping): the synchronous round, the comparison of two patterns, what derives perm / rank / color_ptr around the two hipcub calls,
// the relabelling and the composition behind the permuted matrix, and the gathers that move values and vectors between the orderings.
// Integers and copies only: nothing here rounds.
#include <hipcub/hipcub.hpp>

#include <algorithm>

#include "color.hpp"
#include "solvers_common.hpp"

namespace spmv {

#define COLOR_ROWS(i, n) for (long i = (long) blockIdx.x * COLOR_TB + threadIdx.x; i < (n); i += (long) gridDim.x * COLOR_TB)

__device__ __forceinline__ unsigned long long
color_key(long i)
{
	const unsigned h = (unsigned) i * COLOR_HASH_MUL;
	return ((unsigned long long) (h >> 1) << 31) | (unsigned long long) i;
}

// the colours base .. base + 63 that the coloured neighbours of row i hold, as a mask
__device__ __forceinline__ unsigned long long
color_window(const ColorGraph & g, const int * __restrict__ cin, long i, int base)
{
	unsigned long long mask = 0;
	for (int t = 0; t < (g.rpt ? 2 : 1); t++)
	{
		const int * rp = t ? g.rpt : g.rp, * ci = t ? g.cit : g.ci;
		for (int e = rp[i]; e < rp[i + 1]; e++)
		{
			const int j = ci[e];
			const int d = (j != i ? cin[j] : -1) - base;      // unsigned compare: an uncoloured neighbour (-1) is outside every window
			if ((unsigned) d < 64u)
				mask |= 1ull << d;
		}
	}
	return mask;
}

__global__ __launch_bounds__(COLOR_TB) void
color_round_kernel(ColorGraph g, const int * __restrict__ cin, int * __restrict__ cout, int * __restrict__ left)
{
	__shared__ int sh[COLOR_TB];
	int mine = 0;
	COLOR_ROWS(i, g.n)
	{
		int c = cin[i];
		if (c < 0)
		{
			const unsigned long long ki = color_key(i);
			unsigned long long mask = 0;                      // window 0, filled on the way
			bool top = true;
			for (int t = 0; top && t < (g.rpt ? 2 : 1); t++)
			{
				const int * rp = t ? g.rpt : g.rp, * ci = t ? g.cit : g.ci;
				for (int e = rp[i]; e < rp[i + 1]; e++)
				{
					const int j = ci[e];
					if (j == i)
						continue;
					const int cj = cin[j];
					if (cj < 0)
					{
						if (color_key(j) > ki)
						{
							top = false;
							break;
						}
					}
					else if (cj < 64)
						mask |= 1ull << cj;
				}
			}
			if (top)
			{
				int base = 0;
				while (mask == ~0ull)                         // all 64 taken: at least 64 neighbours per trip
				{
					base += 64;
					mask = color_window(g, cin, i, base);
				}
				c = base + __builtin_ctzll(~mask);
			}
			else
				mine++;
		}
		cout[i] = c;
	}
	sh[threadIdx.x] = mine;
	__syncthreads();
	for (int s = COLOR_TB / 2; s > 0; s >>= 1)
	{
		if ((int) threadIdx.x < s)
			sh[threadIdx.x] += sh[threadIdx.x + s];
		__syncthreads();
	}
	if (threadIdx.x == 0 && sh[0] > 0)
		atomicAdd(left, sh[0]);                               // an integer count: its sum does not depend on the order
}

// every lane that finds a difference stores the same 1
__global__ __launch_bounds__(COLOR_TB) void
color_differ_kernel(const int * __restrict__ a, const int * __restrict__ b, long count, int * __restrict__ differ)
{
	bool any = false;
	COLOR_ROWS(e, count)
		any |= a[e] != b[e];
	if (any)
		*differ = 1;
}

__global__ __launch_bounds__(COLOR_TB) void
color_iota_kernel(long n, int * __restrict__ iota)
{
	COLOR_ROWS(i, n)
		iota[i] = (int) i;
}

// perm is a permutation of 0 .. n-1 (the sorted iota): every rank[] is written once
__global__ __launch_bounds__(COLOR_TB) void
color_rank_kernel(long n, const int * __restrict__ perm, int * __restrict__ rank)
{
	COLOR_ROWS(p, n)
		rank[perm[p]] = (int) p;
}

__global__ __launch_bounds__(COLOR_TB) void
color_start_kernel(const int * __restrict__ sorted, long n, long num_colors, int * __restrict__ ptr)
{
	COLOR_ROWS(c, num_colors + 1)
	{
		long lo = 0, hi = n;
		while (lo < hi)
		{
			const long mid = (lo + hi) / 2;
			if ((long) sorted[mid] < c)
				lo = mid + 1;
			else
				hi = mid;
		}
		ptr[c] = (int) lo;
	}
}

__global__ __launch_bounds__(COLOR_TB) void
color_relabel_kernel(long count, const int * __restrict__ in, const int * __restrict__ rank, int * __restrict__ out)
{
	COLOR_ROWS(e, count)
		out[e] = rank[in[e]];
}

__global__ __launch_bounds__(COLOR_TB) void
color_compose_kernel(long count, const unsigned * __restrict__ first, const unsigned * __restrict__ second, int * __restrict__ out)
{
	COLOR_ROWS(e, count)
		out[e] = (int) first[second[e]];
}

__global__ __launch_bounds__(COLOR_TB) void
color_gather_values_kernel(long count, const int * __restrict__ map, const double * __restrict__ in, double * __restrict__ out)
{
	COLOR_ROWS(e, count)
		out[e] = in[map[e]];
}

template <typename T, int KC>
__device__ __forceinline__ bool
color_row_vec(const T * p, long ld, int c0)
{
	return ld % KC == 0 && c0 % KC == 0 && (size_t) p % (KC * sizeof(T)) == 0;
}

// a thread owns row p of its chunk: KC contiguous values read from row idx[p], as one vector where the block's base, ld and c0 allow
template <typename T, int KC>
__global__ __launch_bounds__(VB) void
color_gather_rows_kernel(const int * __restrict__ idx, const T * __restrict__ in, long ldin, T * __restrict__ out, long ldout, int c0, long n)
{
	const bool vi = color_row_vec<T, KC>(in, ldin, c0), vo = color_row_vec<T, KC>(out, ldout, c0);
	GRID_STRIDE(p, n)
	{
		T v[KC];
		load_row<T, KC>(v, in + (long) idx[p] * ldin + c0, vi);
		store_row<T, KC>(out + p * ldout + c0, v, vo);
	}
}

#define COLOR_LAUNCH(kernel, n, st, ...)                                                          \
	do {                                                                                          \
		if ((n) > 0)                                                                              \
			hipLaunchKernelGGL(kernel, dim3(color_grid(n)), dim3(COLOR_TB), 0, st, __VA_ARGS__);  \
		HIP_TRY(hipGetLastError());                                                               \
		return 0;                                                                                 \
	} while (0)

int
launch_color_round(const ColorGraph & g, const int * cin, int * cout, int * left, hipStream_t st)
{
	COLOR_LAUNCH(color_round_kernel, g.n, st, g, cin, cout, left);
}

int
launch_color_differ(const int * a, const int * b, long count, int * differ, hipStream_t st)
{
	COLOR_LAUNCH(color_differ_kernel, count, st, a, b, count, differ);
}

static int
color_bits(int max_color)
{
	int bits = 1;
	while ((1L << bits) <= max_color)
		bits++;
	return bits;
}

size_t
color_max_bytes(long n)
{
	size_t bytes = 0;
	const int * in = nullptr;
	int * out = nullptr;
	(void) hipcub::DeviceReduce::Max(nullptr, bytes, in, out, (int) n, (hipStream_t) 0);
	return std::max<size_t>(bytes, 16);
}

size_t
color_sort_bytes(long n, int max_color)
{
	size_t bytes = 0;
	const unsigned * key = nullptr;
	unsigned * key_out = nullptr;
	const int * val = nullptr;
	int * val_out = nullptr;
	(void) hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key, key_out, val, val_out, (int) n, 0, color_bits(max_color), (hipStream_t) 0);
	return std::max<size_t>(bytes, 16);
}

int
launch_color_max(long n, const int * colors, int * max_out, void * tmp, size_t tmp_bytes, hipStream_t st)
{
	if (n > 0)
		HIP_TRY(hipcub::DeviceReduce::Max(tmp, tmp_bytes, colors, max_out, (int) n, st));
	return 0;
}

int
launch_color_sort(long n, const int * colors, int max_color, int * iota, int * sorted, int * perm, int * rank, void * tmp, size_t tmp_bytes,
		hipStream_t st)
{
	if (n <= 0)
		return 0;
	hipLaunchKernelGGL(color_iota_kernel, dim3(color_grid(n)), dim3(COLOR_TB), 0, st, n, iota);
	HIP_TRY(hipGetLastError());
	// colours are >= 0 here: as unsigned keys they sort alike; the sort is stable, so equal colours keep ascending rows
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, reinterpret_cast<const unsigned *>(colors), reinterpret_cast<unsigned *>(sorted), iota,
			perm, (int) n, 0, color_bits(max_color), st));
	hipLaunchKernelGGL(color_rank_kernel, dim3(color_grid(n)), dim3(COLOR_TB), 0, st, n, perm, rank);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_color_start(long n, const int * sorted, long num_colors, int * ptr, hipStream_t st)
{
	COLOR_LAUNCH(color_start_kernel, num_colors + 1, st, sorted, n, num_colors, ptr);
}

int
launch_color_relabel(long count, const int * in, const int * rank, int * out, hipStream_t st)
{
	COLOR_LAUNCH(color_relabel_kernel, count, st, count, in, rank, out);
}

int
launch_color_compose(long count, const unsigned * first, const unsigned * second, int * out, hipStream_t st)
{
	COLOR_LAUNCH(color_compose_kernel, count, st, count, first, second, out);
}

int
launch_color_gather_values(long count, const int * map, const double * in, double * out, hipStream_t st)
{
	COLOR_LAUNCH(color_gather_values_kernel, count, st, count, map, in, out);
}

int
launch_color_gather_rows(bool f32, int k, const int * idx, const void * in, long ldin, void * out, long ldout, long n, hipStream_t st)
{
	if (n > 0)
		for_chunks(column_chunks(k), [&](int c0, auto kc) {
			constexpr int KC = decltype(kc)::value;
			if (f32)
				hipLaunchKernelGGL((color_gather_rows_kernel<float, KC>), dim3(solver_blocks(n)), dim3(VB), 0, st, idx, (const float *) in, ldin,
						(float *) out, ldout, c0, n);
			else
				hipLaunchKernelGGL((color_gather_rows_kernel<double, KC>), dim3(solver_blocks(n)), dim3(VB), 0, st, idx, (const double *) in, ldin,
						(double *) out, ldout, c0, n);
			return 0;
		});
	HIP_TRY(hipGetLastError());
	return 0;
}

}  // namespace spmv

// Multi-vector SpMV on the SELL-64-sigma-delta layout: Y = A X (or Y += A X) for k vectors held row-major, X[c * ldx + j], j < k.
//
// The single-vector kernel (kernels_sell.hip: sell_delta_kernel) streams the whole matrix once per vector, and on the nlpkkt240 twin the
// matrix is three quarters of what one launch moves. Here a lane still owns one row of a 64-row slice, but every index group and value
// group is loaded and decoded ONCE (sell_delta_read.hpp, the same readers as the single-vector kernel) and serves K columns of X: a
// decoded column c is gathered as the K contiguous values X[c * ldx .. c * ldx + K) with the widest loads the alignment of X and ldx
// allows (VW values per load, at most 16 bytes), and K accumulator chains take one FMA per step each, in the step order of the
// single-vector kernel. With S waves per slice the S partial sums of a row meet in LDS and are added in wave order, as in
// sell_delta_split_kernel. So column j of Y is bit-identical to the single-vector product on column j of X.
//
// K is 1, 2, 4 or 8 per launch; a k of any other size runs as passes over the matrix, 8 columns per pass and then the binary remainder
// (launch_sell_delta_spmm). Groups per trip shrink as K grows so that a lane keeps about the single-vector kernel's 16 steps x 8 bytes of
// x in flight (spmm_trip_groups), and every instantiation stays within 128 VGPRs (4 waves per SIMD) without scratch.

#include <algorithm>

#include "sell_delta_read.hpp"

namespace spmv {

constexpr int SPMM_BLOCK = 256;
constexpr int SPMM_WAVES = SPMM_BLOCK / WAVE;

// groups of 4 steps per trip: 4 (16 steps, as the single-vector kernel) while a step's K values of x take at most 8 bytes, then fewer
template <typename T, int K>
constexpr int
spmm_trip_groups()
{
	return 32 / (K * (int) sizeof(T)) >= 4 ? 4 : 32 / (K * (int) sizeof(T)) >= 2 ? 2 : 1;
}

// the K values of row c of X (xp = X + c * ldx), VW at a time: VW > 1 only when X and ldx keep every such run VW-aligned
template <typename T, int K, int VW>
__device__ __forceinline__ void
spmm_gather(const T * __restrict__ xp, T (&xv)[K])
{
	if constexpr (VW == 1)
	{
		#pragma unroll
		for (int j = 0; j < K; j++)
			xv[j] = xp[j];
	}
	else
	{
		typedef T TV __attribute__((ext_vector_type(VW)));
		#pragma unroll
		for (int q = 0; q < K / VW; q++)
		{
			const TV w = *reinterpret_cast<const TV *>(xp + q * VW);
			#pragma unroll
			for (int e = 0; e < VW; e++)
				xv[q * VW + e] = w[e];
		}
	}
}

// the columns of index group g of a slice in mode 0..4 (off: the lane offset of modes 0 / 3)
template <int MODE, bool NT>
struct SpmmCols {
	const unsigned char * ip;                      // the slice's first index group (uniform)
	int lane, off;
	__device__ __forceinline__ void operator()(int g, int (&c)[4]) const
	{
		sell_group_cols<MODE, NT>(ip + (size_t) g * sell_group_bytes(MODE), lane, off, c);
	}
};

// ... of a slice in mode 5 (lane offsets with exceptions); SCALAR: at most four exceptions, corrections through the scalar cache
template <bool NT, bool SCALAR>
struct SpmmCols5 {
	const unsigned char * ip;
	size_t gb;                                     // bytes of one group
	int lane, off;
	Sell5Lane<SCALAR> ln;
	__device__ __forceinline__ void operator()(int g, int (&c)[4]) const
	{
		SellDeltaIdx5 q;
		sell_delta_load_idx5<NT, SCALAR>(q, ip + (size_t) g * gb, ln.rank);
		sell_delta_cols5<SCALAR>(q, ln.ex, lane, off, ln.xl, c);
	}
};

// NG full groups g[0..NG) of a slice: all loads of the trip first (indices, values, then the gathers), then the FMAs step by step
// PAD: the slice holds rows shorter than its width (kernels_sell.hip: sell_delta_group): the steps of a lane from `len`, its row's length, on
// are padding — 0.0 times a column of some other row — and take zeros in place of that row of X
template <typename T, int K, int VW, int NG, bool NT, bool V7, bool PAD, typename Cols, typename SV = T>
__device__ __forceinline__ void
spmm_trip(const Cols & cols, const SellVals<T, NT, V7, SV> & vals, const int (&g)[NG], const T * __restrict__ X, long ldx, T (&acc)[K], int len)
{
	int c[NG][4];
	T v[NG][4];
	T xv[NG][4][K];
	#pragma unroll
	for (int u = 0; u < NG; u++)
		cols(g[u], c[u]);
	#pragma unroll
	for (int u = 0; u < NG; u++)
		vals.group(g[u], v[u]);
	#pragma unroll
	for (int u = 0; u < NG; u++)
		#pragma unroll
		for (int t = 0; t < 4; t++)
			spmm_gather<T, K, VW>(X + (long) c[u][t] * ldx, xv[u][t]);
	if constexpr (PAD)
	{
		#pragma unroll
		for (int u = 0; u < NG; u++)
			#pragma unroll
			for (int t = 0; t < 4; t++)
				#pragma unroll
				for (int j = 0; j < K; j++)
					xv[u][t][j] = 4 * g[u] + t < len ? xv[u][t][j] : T(0);
	}
	#pragma unroll
	for (int u = 0; u < NG; u++)
		#pragma unroll
		for (int t = 0; t < 4; t++)
			#pragma unroll
			for (int j = 0; j < K; j++)
				acc[j] = fma_t<T>(v[u][t], xv[u][t][j], acc[j]);
}

// the last group of a slice whose width is not a multiple of 4: NSTEPS (1..3) real steps
template <typename T, int K, int VW, int NSTEPS, bool NT, bool V7, bool PAD, typename Cols, typename SV = T>
__device__ __forceinline__ void
spmm_tail(const Cols & cols, const SellVals<T, NT, V7, SV> & vals, int g, int lane, const T * __restrict__ X, long ldx, T (&acc)[K], int len)
{
	int c[4];
	cols(g, c);
	T v[3];
	sell_tail_values<T, NT, NSTEPS>(vals.tail(g), lane, v);
	T xv[NSTEPS][K];
	#pragma unroll
	for (int t = 0; t < NSTEPS; t++)
		spmm_gather<T, K, VW>(X + (long) c[t] * ldx, xv[t]);
	if constexpr (PAD)
	{
		#pragma unroll
		for (int t = 0; t < NSTEPS; t++)
			#pragma unroll
			for (int j = 0; j < K; j++)
				xv[t][j] = 4 * g + t < len ? xv[t][j] : T(0);
	}
	#pragma unroll
	for (int t = 0; t < NSTEPS; t++)
		#pragma unroll
		for (int j = 0; j < K; j++)
			acc[j] = fma_t<T>(v[t], xv[t][j], acc[j]);
}

// groups g0, g0 + gs, ... of one slice in order (gs = 1: the whole slice), then its tail group if this wave's sequence reaches it
template <typename T, int K, int VW, bool NT, bool V7, bool PAD = false, typename Cols, typename SV = T>
__device__ __forceinline__ void
spmm_walk(const Cols & cols, const SellVals<T, NT, V7, SV> & vals, int width, int lane, const T * __restrict__ X, long ldx, T (&acc)[K], int g0,
		int gs, int len = 0)
{
	constexpr int NG = PAD ? 1 : spmm_trip_groups<T, K>();     // (a padded slice goes group by group: the few there are get no deep trips of their own)
	const int groups = (width + 3) / 4;            // index groups cover the width rounded up to 4 steps, values only the real steps
	const int rem = width - 4 * (groups - 1);
	const int last = groups - 1;
	const int full = rem == 4 ? groups : last;
	int g = g0;
	for (; g + (NG - 1) * gs < full; g += NG * gs)
	{
		int gg[NG];
		#pragma unroll
		for (int u = 0; u < NG; u++)
			gg[u] = g + u * gs;
		spmm_trip<T, K, VW, NG, NT, V7, PAD>(cols, vals, gg, X, ldx, acc, len);
	}
	if constexpr (NG >= 4)
		if (g + gs < full)
		{
			const int gg[2] = {g, g + gs};
			spmm_trip<T, K, VW, 2, NT, V7, PAD>(cols, vals, gg, X, ldx, acc, len);
			g += 2 * gs;
		}
	if constexpr (NG >= 2)
		if (g < full)
		{
			const int gg[1] = {g};
			spmm_trip<T, K, VW, 1, NT, V7, PAD>(cols, vals, gg, X, ldx, acc, len);
			g += gs;
		}
	if (rem != 4 && g == last)
	{
		if (rem == 1)
			spmm_tail<T, K, VW, 1, NT, V7, PAD>(cols, vals, g, lane, X, ldx, acc, len);
		else if (rem == 2)
			spmm_tail<T, K, VW, 2, NT, V7, PAD>(cols, vals, g, lane, X, ldx, acc, len);
		else
			spmm_tail<T, K, VW, 3, NT, V7, PAD>(cols, vals, g, lane, X, ldx, acc, len);
	}
}

// one slice in its index mode (a wave-uniform branch); ip = the slice's index block
template <typename T, int K, int VW, bool NT, bool V7, typename SV = T>
__device__ __forceinline__ void
spmm_modes(int mode, const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, SV> & vals, int width, int lane, const T * __restrict__ X,
		long ldx, T (&acc)[K], int g0, int gs, bool padded /* uniform */, const int * __restrict__ slice_len /* uniform */)
{
	if (mode == 0)
		spmm_walk<T, K, VW, NT, V7>(SpmmCols<0, NT>{ip, lane, lane}, vals, width, lane, X, ldx, acc, g0, gs);
	else if (padded && (mode == 1 || mode == 2 || mode == 4))
	{
		// rows of different lengths (only the modes with a column per lane and step hold such slices): the padding steps masked
		const int len = slice_len[lane];
		if (mode == 1)
			spmm_walk<T, K, VW, NT, V7, true>(SpmmCols<1, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs, len);
		else if (mode == 2)
			spmm_walk<T, K, VW, NT, V7, true>(SpmmCols<2, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs, len);
		else
			spmm_walk<T, K, VW, NT, V7, true>(SpmmCols<4, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs, len);
	}
	else if (mode == 1)
		spmm_walk<T, K, VW, NT, V7>(SpmmCols<1, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs);
	else if (mode == 2)
		spmm_walk<T, K, VW, NT, V7>(SpmmCols<2, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs);
	else if (mode == 3)
	{
		const int off = ld_stream<NT>(reinterpret_cast<const int *>(ip) + lane);          // the slice's 64 lane offsets, then the groups
		spmm_walk<T, K, VW, NT, V7>(SpmmCols<3, NT>{ip + sell_header_bytes(3), lane, off}, vals, width, lane, X, ldx, acc, g0, gs);
	}
	else if (mode == 5)
	{
		const int off = ld_stream<NT>(reinterpret_cast<const int *>(ip) + lane);
		const unsigned long long mask = *reinterpret_cast<const unsigned long long *>(ip + 4 * WAVE);          // uniform: a scalar load
		const int E = __popcll(mask);
		const size_t gb = sell_group_bytes(5, E);
		ip += sell_header_bytes(5);
		if (E <= 4)
			spmm_walk<T, K, VW, NT, V7>(SpmmCols5<NT, true>{ip, gb, lane, off, Sell5Lane<true>(mask, lane)}, vals, width, lane, X, ldx, acc, g0, gs);
		else
			spmm_walk<T, K, VW, NT, V7>(SpmmCols5<NT, false>{ip, gb, lane, off, Sell5Lane<false>(mask, lane)}, vals, width, lane, X, ldx, acc, g0,
					gs);
	}
	else
		spmm_walk<T, K, VW, NT, V7>(SpmmCols<4, NT>{ip, lane, 0}, vals, width, lane, X, ldx, acc, g0, gs);
}

// S waves per slice (1, 2, 4: the handle's sell_split), wave w of a slice takes its groups w, w + S, ...; V7 = the handle holds slices
// with 7-byte values (each one flagged in desc[2s+1]). Tile order and grid are the single-vector kernel's (the handle's XcdMap).
template <typename T, int K, int VW, int S, bool NT, bool V7>
__global__ __launch_bounds__(SPMM_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void
sell_delta_spmm_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const T * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const T * __restrict__ X, long ldx, T * __restrict__ Y, long ldy, int m, int num_slices,
		int beta, XcdMap map)
{
	constexpr int SPB = SPMM_WAVES / S;            // slices per workgroup
	const unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int wave = threadIdx.x / WAVE;
	const int w = __builtin_amdgcn_readfirstlane(wave % S);
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * SPB + wave / S));
	if (S == 1 && slice >= num_slices)
		return;
	T acc[K];
	#pragma unroll
	for (int j = 0; j < K; j++)
		acc[j] = T(0);
	if (slice < num_slices)
	{
		const int64_t v_off = desc[2 * slice];
		const int64_t i_word = desc[2 * slice + 1];
		const int64_t v_next = desc[2 * slice + 2];
		const int mode = sell_desc_mode(i_word);
		const bool padded = (sell_pad_bits(row_len, num_slices, WAVE)[slice >> 5] >> (slice & 31)) & 1u;     // the slice holds value padding (launch.hpp)
		const int * slice_len = row_len + (long) slice * WAVE;          // the lengths of the slice's 64 rows (uniform)
		const unsigned char * ip = idx + sell_desc_idx(i_word);
		const T * vp = val + v_off + 2 * lane;
		bool done = false;
		if constexpr (V7)
			if (sell_desc_v7(i_word))
			{
				spmm_modes<T, K, VW, NT, true>(mode, ip, SellVals<T, NT, true>{vp, lane, (unsigned) (sell_v7_e0(i_word) - 1) << 20},
						(int) sell_slice_width(v_next - v_off, true), lane, X, ldx, acc, w, S, padded, slice_len);
				done = true;
			}
		if (!done)
			spmm_modes<T, K, VW, NT, false>(mode, ip, SellVals<T, NT, false>{vp, lane, 0u}, (int) sell_slice_width(v_next - v_off, false), lane, X,
					ldx, acc, w, S, padded, slice_len);
	}
	if constexpr (S > 1)
	{
		__shared__ T s_part[SPMM_WAVES][K][WAVE];
		#pragma unroll
		for (int j = 0; j < K; j++)
			s_part[wave][j][lane] = acc[j];
		__syncthreads();
		if (w != 0 || slice >= num_slices)
			return;
		#pragma unroll
		for (int j = 0; j < K; j++)
		{
			T t = s_part[wave][j][lane];
			#pragma unroll
			for (int u = 1; u < S; u++)
				t += s_part[wave + u][j][lane];
			acc[j] = t;
		}
	}
	const long sorted_row = (long) slice * WAVE + lane;
	if (sorted_row < m)
	{
		T * yp = Y + (long) row_of_sorted[sorted_row] * ldy;
		#pragma unroll
		for (int j = 0; j < K; j++)
			yp[j] = beta ? yp[j] + acc[j] : acc[j];
	}
}

// fp32 values under fp64 vectors (opts.value_storage = 1; kernels_sell.hip: sell_delta_mixed_kernel): sell_delta_spmm_kernel<double> on
// values read from the fp32 pair layout and widened, under a name of its own so that every instantiation above keeps its symbol and code
template <int K, int VW, int S, bool NT>
__global__ __launch_bounds__(SPMM_BLOCK) __attribute__((amdgpu_waves_per_eu(4))) void
sell_delta_mixed_spmm_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const float * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const double * __restrict__ X, long ldx, double * __restrict__ Y, long ldy, int m,
		int num_slices, int beta, XcdMap map)
{
	typedef double T;
	constexpr int SPB = SPMM_WAVES / S;            // slices per workgroup
	const unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int wave = threadIdx.x / WAVE;
	const int w = __builtin_amdgcn_readfirstlane(wave % S);
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * SPB + wave / S));
	if (S == 1 && slice >= num_slices)
		return;
	T acc[K];
	#pragma unroll
	for (int j = 0; j < K; j++)
		acc[j] = T(0);
	if (slice < num_slices)
	{
		const int64_t v_off = desc[2 * slice];
		const int64_t i_word = desc[2 * slice + 1];
		const int64_t v_next = desc[2 * slice + 2];
		const int mode = sell_desc_mode(i_word);
		const bool padded = (sell_pad_bits(row_len, num_slices, WAVE)[slice >> 5] >> (slice & 31)) & 1u;     // the slice holds value padding (launch.hpp)
		const int * slice_len = row_len + (long) slice * WAVE;          // the lengths of the slice's 64 rows (uniform)
		const unsigned char * ip = idx + sell_desc_idx(i_word);
		const float * vp = val + v_off + 2 * lane;
		spmm_modes<T, K, VW, NT, false>(mode, ip, SellVals<T, NT, false, float>{vp, lane, 0u}, (int) sell_slice_width(v_next - v_off, false), lane, X,
				ldx, acc, w, S, padded, slice_len);
	}
	if constexpr (S > 1)
	{
		__shared__ T s_part[SPMM_WAVES][K][WAVE];
		#pragma unroll
		for (int j = 0; j < K; j++)
			s_part[wave][j][lane] = acc[j];
		__syncthreads();
		if (w != 0 || slice >= num_slices)
			return;
		#pragma unroll
		for (int j = 0; j < K; j++)
		{
			T t = s_part[wave][j][lane];
			#pragma unroll
			for (int u = 1; u < S; u++)
				t += s_part[wave + u][j][lane];
			acc[j] = t;
		}
	}
	const long sorted_row = (long) slice * WAVE + lane;
	if (sorted_row < m)
	{
		T * yp = Y + (long) row_of_sorted[sorted_row] * ldy;
		#pragma unroll
		for (int j = 0; j < K; j++)
			yp[j] = beta ? yp[j] + acc[j] : acc[j];
	}
}

struct SpmmArgs {
	const int64_t * desc;
	const unsigned char * idx;
	const void * val;
	const int * row_of_sorted;
	const int * row_len;
	int m, num_slices;
};

// MIXED: T = double over values stored as float (sell_delta_mixed_spmm_kernel); V7 is then false
template <typename T, int K, int VW, bool V7, bool MIXED>
static int
spmm_launch(int S, const SpmmArgs & a, const void * X, long ldx, void * Y, long ldy, const LaunchCfg & cfg, unsigned grid, hipStream_t stream)
{
	#define SPMM_LAUNCH(S_, NT_) do { \
			if constexpr (MIXED) \
				hipLaunchKernelGGL((sell_delta_mixed_spmm_kernel<K, VW, S_, NT_>), dim3(grid), dim3(SPMM_BLOCK), 0, stream, a.desc, a.idx, \
						(const float *) a.val, a.row_of_sorted, a.row_len, (const double *) X, ldx, (double *) Y, ldy, a.m, a.num_slices, cfg.beta, cfg.map); \
			else \
				hipLaunchKernelGGL((sell_delta_spmm_kernel<T, K, VW, S_, NT_, V7>), dim3(grid), dim3(SPMM_BLOCK), 0, stream, a.desc, a.idx, \
						(const T *) a.val, a.row_of_sorted, a.row_len, (const T *) X, ldx, (T *) Y, ldy, a.m, a.num_slices, cfg.beta, cfg.map); \
		} while (0)
	if (S == 1)
	{
		if (cfg.nt) SPMM_LAUNCH(1, true);
		else        SPMM_LAUNCH(1, false);
	}
	else if (S == 2)
	{
		if (cfg.nt) SPMM_LAUNCH(2, true);
		else        SPMM_LAUNCH(2, false);
	}
	else if (S == 4)
	{
		if (cfg.nt) SPMM_LAUNCH(4, true);
		else        SPMM_LAUNCH(4, false);
	}
	else
	{
		set_error("sell_delta_spmm: waves per slice must be 1, 2 or 4 (got %d)", S);
		return 1;
	}
	#undef SPMM_LAUNCH
	HIP_TRY(hipGetLastError());
	return 0;
}

// one pass of K columns: vector gathers of VMAX values (16 bytes at most) when X and ldx keep every row's run of K aligned to them
template <typename T, int K, bool V7, bool MIXED>
static int
spmm_pass(int S, const SpmmArgs & a, const void * X, long ldx, void * Y, long ldy, const LaunchCfg & cfg, unsigned grid, hipStream_t stream)
{
	constexpr int VMAX = K < (int) (16 / sizeof(T)) ? K : (int) (16 / sizeof(T));
	if constexpr (VMAX > 1)
		if ((uintptr_t) X % (VMAX * sizeof(T)) == 0 && ldx % VMAX == 0)
			return spmm_launch<T, K, VMAX, V7, MIXED>(S, a, X, ldx, Y, ldy, cfg, grid, stream);
	return spmm_launch<T, K, 1, V7, MIXED>(S, a, X, ldx, Y, ldy, cfg, grid, stream);
}

template <typename T, bool V7, bool MIXED = false>
static int
spmm_passes(int S, const SpmmArgs & a, int k, const void * X, long ldx, void * Y, long ldy, const LaunchCfg & cfg, unsigned grid,
		hipStream_t stream)
{
	for (int j0 = 0; j0 < k;)
	{
		const int K = spmm_pass_cols(SELL_DELTA_SPMM_COLS, k - j0);
		const void * Xp = (const T *) X + j0;
		void * Yp = (T *) Y + j0;
		const int rc = K == 8 ? spmm_pass<T, 8, V7, MIXED>(S, a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		             : K == 4 ? spmm_pass<T, 4, V7, MIXED>(S, a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		             : K == 2 ? spmm_pass<T, 2, V7, MIXED>(S, a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		                      : spmm_pass<T, 1, V7, MIXED>(S, a, Xp, ldx, Yp, ldy, cfg, grid, stream);
		if (rc)
			return rc;
		j0 += K;
	}
	return 0;
}

int
launch_sell_delta_spmm(bool f32, bool val_f32, int waves_per_slice, bool v7, const int64_t * desc, const unsigned char * idx, const void * val,
		const int * row_of_sorted, const int * row_len, int k, const void * X, long ldx, void * Y, long ldy, int m, int num_slices,
		const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	if (k == 1 && ldx == 1 && ldy == 1)            // one contiguous vector: the single-vector kernel itself
		return launch_sell_delta(f32, val_f32, waves_per_slice, v7, desc, idx, val, row_of_sorted, row_len, X, Y, m, num_slices, cfg, stream, grid_out);
	if (val_f32 && v7)
	{
		set_error("sell_delta_spmm: 7-byte values are fp64 only");
		return 1;
	}
	if (f32 && !val_f32)
	{
		set_error("sell_delta_spmm: fp32 vectors over fp64 values are not served");
		return 1;
	}
	const unsigned grid = xcd_grid(cfg.map);
	if (grid_out)
		*grid_out = grid;
	if (grid == 0)
		return 0;
	const SpmmArgs a{desc, idx, val, row_of_sorted, row_len, m, num_slices};
	if (val_f32 && !f32)
		return spmm_passes<double, false, true>(waves_per_slice, a, k, X, ldx, Y, ldy, cfg, grid, stream);
	return f32 ? spmm_passes<float, false>(waves_per_slice, a, k, X, ldx, Y, ldy, cfg, grid, stream)
	     : v7  ? spmm_passes<double, true>(waves_per_slice, a, k, X, ldx, Y, ldy, cfg, grid, stream)
	           : spmm_passes<double, false>(waves_per_slice, a, k, X, ldx, Y, ldy, cfg, grid, stream);
}

// ------------------------------------------------------------------------------------------------ every other layout: per column
// x[i] = X[i * ldx] (column j of a row-major X, X already offset by j) and Y[i * ldy] = y[i] (beta 0) / Y[i * ldy] + y[i] (beta 1)
template <typename T>
__global__ __launch_bounds__(256) void
spmm_column_gather_kernel(const T * __restrict__ X, long ldx, T * __restrict__ x, long n)
{
	for (long i = blockIdx.x * 256L + threadIdx.x; i < n; i += (long) gridDim.x * 256)
		x[i] = X[i * ldx];
}

template <typename T>
__global__ __launch_bounds__(256) void
spmm_column_scatter_kernel(const T * __restrict__ y, T * __restrict__ Y, long ldy, long m, int beta)
{
	for (long i = blockIdx.x * 256L + threadIdx.x; i < m; i += (long) gridDim.x * 256)
		Y[i * ldy] = beta ? Y[i * ldy] + y[i] : y[i];
}

static unsigned
spmm_copy_grid(long count)
{
	return (unsigned) std::max<long>(1, std::min<long>((count + 255) / 256, 8192));
}

int
launch_spmm_column_gather(bool f32, const void * X, long ldx, void * x, long n, hipStream_t stream)
{
	if (n <= 0)
		return 0;
	if (f32)
		hipLaunchKernelGGL(spmm_column_gather_kernel<float>, dim3(spmm_copy_grid(n)), dim3(256), 0, stream, (const float *) X, ldx, (float *) x, n);
	else
		hipLaunchKernelGGL(spmm_column_gather_kernel<double>, dim3(spmm_copy_grid(n)), dim3(256), 0, stream, (const double *) X, ldx, (double *) x, n);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_spmm_column_scatter(bool f32, const void * y, void * Y, long ldy, long m, int beta, hipStream_t stream)
{
	if (m <= 0)
		return 0;
	if (f32)
		hipLaunchKernelGGL(spmm_column_scatter_kernel<float>, dim3(spmm_copy_grid(m)), dim3(256), 0, stream, (const float *) y, (float *) Y, ldy, m, beta);
	else
		hipLaunchKernelGGL(spmm_column_scatter_kernel<double>, dim3(spmm_copy_grid(m)), dim3(256), 0, stream, (const double *) y, (double *) Y, ldy, m,
				beta);
	HIP_TRY(hipGetLastError());
	return 0;
}

}  // namespace spmv

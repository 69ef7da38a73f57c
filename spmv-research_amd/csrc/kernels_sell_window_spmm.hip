// Multi-vector SpMV on the LDS-window SELL layout: Y = A X (or Y += A X) for k vectors held row-major, X[c * ldx + j], j < k.
//
// The single-vector kernel (kernels_sell_window.hip: sell_window_kernel) copies a slice group's window of x into LDS and streams the
// group's indices and values once per vector. Here the same workgroup (same grid, tile order and shape, same stored arrays) copies the
// window's rows of X, K columns each, into LDS once, and every index group and value group is loaded ONCE and serves K accumulator
// chains: a decoded 16-bit column c reads its K values from LDS.
//   * LDS image: row-interleaved, xs[c * K + j] — a lane's K values are contiguous, one ds_read_b64 / ds_read_b128 per 8 / 16 bytes.
//     (The planar image xs[j * (w + 1) + c], K scalar reads per column, is kept behind SELLW_SPMM_PLANAR for the comparison in
//     profiles/r07_spmm_window.txt.)
//   * window copy: element e of the window's w * K values is (row e / K, column e % K), so consecutive lanes read consecutive
//     addresses of a row and, when ldx == K, of the whole window; VW values per load (16 bytes at most) when X and ldx keep every
//     row's run of K aligned to them, one value per load otherwise (odd ldx, X one element off).
//   * order of the additions: wave `part` of a slice takes index groups part, part + S, ... in order and a group's steps 0..3 in
//     order, as the single-vector kernel; with S > 1 the partial sums meet in LDS as [wave][K][lane] and are added in wave order.
//     So column j of Y is bit-identical to the single-vector product on column j of X, for beta 0 and 1 and every S.
//   * K is 1, 2, 4 or 8 per launch. Two groups (8 steps) are in flight per trip, as in the single-vector kernel, while a step's K
//     values take at most 16 bytes, then one group (sellw_spmm_trip_groups), so every instantiation stays within the 128 VGPRs of a
//     1024-thread workgroup without scratch.
//   * LDS of one pass of K columns: align16((wmax + 1) * K * sizeof(T)) + (S > 1 ? threads * K * sizeof(T) : 0), wmax = the handle's
//     widest window. The most columns one pass serves, Kmax, is the largest K in {8, 4, 2, 1} that fits the 160 KiB one workgroup may
//     declare (sell_window_spmm_max_cols); k columns run as passes of the largest power of two <= min(Kmax, columns left).

#include "sell_window_read.hpp"

#ifndef SELLW_SPMM_PLANAR
#define SELLW_SPMM_PLANAR 0
#endif

namespace spmv {

constexpr long SELLW_SPMM_LDS_MAX = 160 * 1024;          // bytes of LDS a single workgroup may declare on gfx950

template <typename T, int K>
constexpr int
sellw_spmm_trip_groups()
{
	return K * (int) sizeof(T) <= 16 ? 2 : 1;
}

// values per load of the window copy, and per LDS read of the interleaved image: 16 bytes at most
template <typename T, int K>
constexpr int
sellw_spmm_vmax()
{
	return K < (int) (16 / sizeof(T)) ? K : (int) (16 / sizeof(T));
}

// where (window row c, column j) lies in the LDS image; plane = w + 1 (planar image only)
template <int K>
__device__ __forceinline__ int
sellw_spmm_slot(int c, int j, int plane)
{
	return SELLW_SPMM_PLANAR ? j * plane + c : c * K + j;
}

// the K values of window row c
template <typename T, int K>
__device__ __forceinline__ void
sellw_spmm_x(const T * __restrict__ xs, unsigned c, int plane, T (&xv)[K])
{
	constexpr int VW = sellw_spmm_vmax<T, K>();
	if constexpr (SELLW_SPMM_PLANAR || VW == 1)
	{
		#pragma unroll
		for (int j = 0; j < K; j++)
			xv[j] = xs[sellw_spmm_slot<K>((int) c, j, plane)];
	}
	else
	{
		typedef T TV __attribute__((ext_vector_type(VW)));
		const TV * p = reinterpret_cast<const TV *>(xs + c * K);
		#pragma unroll
		for (int q = 0; q < K / VW; q++)
		{
			const TV w = p[q];
			#pragma unroll
			for (int e = 0; e < VW; e++)
				xv[q * VW + e] = w[e];
		}
	}
}

// NG index groups g, g + S, ... of one lane: the index loads, then the value loads, all issued before the first LDS read
template <typename T, int NG>
struct SellwSpmmTrip {
	sellw_uint2 d[NG];
	T v[NG][4];
};

template <typename T, int NG, int S, bool NT>
__device__ __forceinline__ void
sellw_spmm_load(SellwSpmmTrip<T, NG> & p, const sellw_uint2 * __restrict__ ip, const T * __restrict__ vp, int g)
{
	#pragma unroll
	for (int u = 0; u < NG; u++)
		p.d[u] = ld_stream<NT>(ip + (size_t) (g + u * S) * WAVE);
	#pragma unroll
	for (int u = 0; u < NG; u++)
		sellw_values<T, NT>(vp + (size_t) (g + u * S) * 4 * WAVE, p.v[u]);
}

// group by group, step by step: one FMA per step on each of the K chains
template <typename T, int K, int NG>
__device__ __forceinline__ void
sellw_spmm_consume(const SellwSpmmTrip<T, NG> & p, const T * __restrict__ xs, int plane, T (&acc)[K])
{
	#pragma unroll
	for (int u = 0; u < NG; u++)
	{
		const unsigned c[4] = {p.d[u].x & 0xffffu, p.d[u].x >> 16, p.d[u].y & 0xffffu, p.d[u].y >> 16};
		T xv[4][K];
		#pragma unroll
		for (int t = 0; t < 4; t++)
			sellw_spmm_x<T, K>(xs, c[t], plane, xv[t]);
		#pragma unroll
		for (int t = 0; t < 4; t++)
			#pragma unroll
			for (int j = 0; j < K; j++)
				acc[j] = fma_t<T>(p.v[u][t], xv[t][j], acc[j]);
	}
}

// grp, sdesc, idx, val, row_of_sorted: the arrays of sell_window_kernel. vw > 1: X and ldx keep every row's K values aligned to
// sellw_spmm_vmax values, the window copy loads that many at a time.
template <typename T, int K, int S, bool NT>
__global__ __launch_bounds__(1024) void
sell_window_spmm_kernel(const int * __restrict__ grp, const int64_t * __restrict__ sdesc, const unsigned short * __restrict__ idx,
		const T * __restrict__ val, const int * __restrict__ row_of_sorted, const T * __restrict__ X, long ldx, T * __restrict__ Y, long ldy,
		int m, int beta, int vw, int part_off /* bytes from the window to the partial sums */, XcdMap map)
{
	extern __shared__ __align__(16) unsigned char sellw_spmm_smem[];
	T * xs = reinterpret_cast<T *>(sellw_spmm_smem);
	constexpr int NG = sellw_spmm_trip_groups<T, K>();
	const unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lo = grp[4 * tile], w = grp[4 * tile + 1], slice0 = grp[4 * tile + 2], ns = grp[4 * tile + 3];
	const int lane = threadIdx.x % WAVE;
	const int wave = __builtin_amdgcn_readfirstlane((int) threadIdx.x / WAVE);
	const int part = wave % S;
	const bool active = wave / S < ns;
	const int slice = slice0 + (active ? wave / S : 0);
	const int64_t v_off = sdesc[2 * slice], i_off = sdesc[2 * slice + 1], v_next = sdesc[2 * slice + 2];
	const int groups = (int) ((v_next - v_off) / (4 * WAVE));
	const T * vp = val + v_off + (16 / (int) sizeof(T)) * lane;
	const sellw_uint2 * ip = reinterpret_cast<const sellw_uint2 *>(idx + i_off) + lane;
	// the wave's first trip is in flight while the window of X is copied into LDS
	int g = part;
	const bool head = active && g + (NG - 1) * S < groups;
	SellwSpmmTrip<T, NG> p;
	if (head)
		sellw_spmm_load<T, NG, S, NT>(p, ip, vp, g);
	const int plane = w + 1;
	const T * Xw = X + (long) lo * ldx;
	constexpr int VW = sellw_spmm_vmax<T, K>();
	bool copied = false;
	if constexpr (VW > 1)
		if (vw > 1)
		{
			typedef T TV __attribute__((ext_vector_type(VW)));
			constexpr int Q = K / VW;
			for (int e = threadIdx.x; e < w * Q; e += blockDim.x)
			{
				const int i = e / Q, q = e % Q;
				const TV t = *reinterpret_cast<const TV *>(Xw + (long) i * ldx + q * VW);
				if constexpr (SELLW_SPMM_PLANAR)
				{
					#pragma unroll
					for (int u = 0; u < VW; u++)
						xs[sellw_spmm_slot<K>(i, q * VW + u, plane)] = t[u];
				}
				else
					*reinterpret_cast<TV *>(xs + i * K + q * VW) = t;
			}
			copied = true;
		}
	if (!copied)
		for (int e = threadIdx.x; e < w * K; e += blockDim.x)
		{
			const int i = e / K, j = e % K;
			xs[sellw_spmm_slot<K>(i, j, plane)] = Xw[(long) i * ldx + j];
		}
	if (threadIdx.x < K)
		xs[sellw_spmm_slot<K>(w, (int) threadIdx.x, plane)] = 0;          // what the padding of EMPTY rows points at, as in sell_window_kernel
	__syncthreads();
	T acc[K];
	#pragma unroll
	for (int j = 0; j < K; j++)
		acc[j] = T(0);
	if (active)
	{
		if (head)
		{
			sellw_spmm_consume<T, K, NG>(p, xs, plane, acc);
			g += NG * S;
		}
		for (; g + (NG - 1) * S < groups; g += NG * S)
		{
			sellw_spmm_load<T, NG, S, NT>(p, ip, vp, g);
			sellw_spmm_consume<T, K, NG>(p, xs, plane, acc);
		}
		if constexpr (NG == 2)
			if (g < groups)
			{
				SellwSpmmTrip<T, 1> q;
				sellw_spmm_load<T, 1, S, NT>(q, ip, vp, g);
				sellw_spmm_consume<T, K, 1>(q, xs, plane, acc);
			}
	}
	if constexpr (S > 1)
	{
		T * sp = reinterpret_cast<T *>(sellw_spmm_smem + part_off);          // [wave][K][lane]
		#pragma unroll
		for (int j = 0; j < K; j++)
			sp[((size_t) wave * K + j) * WAVE + lane] = acc[j];
		__syncthreads();
		if (part != 0 || !active)
			return;
		#pragma unroll
		for (int j = 0; j < K; j++)
		{
			T t = sp[((size_t) wave * K + j) * WAVE + lane];
			#pragma unroll
			for (int u = 1; u < S; u++)
				t += sp[((size_t) (wave + u) * K + j) * WAVE + lane];
			acc[j] = t;
		}
	}
	else if (!active)
		return;
	const long sorted_row = (long) slice * WAVE + lane;
	if (sorted_row < m)
	{
		T * yp = Y + (long) row_of_sorted[sorted_row] * ldy;
		#pragma unroll
		for (int j = 0; j < K; j++)
			yp[j] = beta ? yp[j] + acc[j] : acc[j];
	}
}

static long
sellw_spmm_lds(bool f32, int threads, int S, int wmax, int K)
{
	const long vb = f32 ? 4 : 8;
	return ((long) (wmax + 1) * K * vb + 15) / 16 * 16 + (S > 1 ? (long) threads * K * vb : 0);
}

int
sell_window_spmm_max_cols(bool f32, int waves_per_slice, int slices_per_group, int wmax)
{
	const int threads = waves_per_slice * slices_per_group * WAVE;
	for (int K = 8; K > 1; K /= 2)
		if (sellw_spmm_lds(f32, threads, waves_per_slice, wmax, K) <= SELLW_SPMM_LDS_MAX)
			return K;
	return 1;                                    // what the single-vector kernel declares: the layout was built to fit it
}

struct SellwSpmmArgs {
	const int * grp;
	const int64_t * sdesc;
	const unsigned short * idx;
	const void * val;
	const int * row_of_sorted;
	int m, threads, wmax;
};

// one pass of K columns
template <typename T, int K, int S>
static int
sellw_spmm_launch(const SellwSpmmArgs & a, const void * X, long ldx, void * Y, long ldy, const LaunchCfg & cfg, unsigned grid, hipStream_t stream)
{
	constexpr int VW = sellw_spmm_vmax<T, K>();
	const int vw = VW > 1 && (uintptr_t) X % (VW * sizeof(T)) == 0 && ldx % VW == 0 ? VW : 1;
	const int lds_bytes = (int) sellw_spmm_lds(sizeof(T) == 4, a.threads, S, a.wmax, K);
	const int part_off = lds_bytes - (S > 1 ? a.threads * K * (int) sizeof(T) : 0);
	// more than 64 KiB of dynamic LDS has to be granted per kernel function, once per device
	static int granted[64][2] = {{0}};
	int dev = 0;
	HIP_TRY(hipGetDevice(&dev));
	dev = dev < 0 || dev >= 64 ? 0 : dev;
	int & have = granted[dev][cfg.nt ? 1 : 0];
	if (lds_bytes > have)
	{
		if (cfg.nt)
			HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&sell_window_spmm_kernel<T, K, S, true>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
		else
			HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(&sell_window_spmm_kernel<T, K, S, false>), hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes));
		have = lds_bytes;
	}
	if (cfg.nt)
		hipLaunchKernelGGL((sell_window_spmm_kernel<T, K, S, true>), dim3(grid), dim3(a.threads), lds_bytes, stream, a.grp, a.sdesc, a.idx,
				(const T *) a.val, a.row_of_sorted, (const T *) X, ldx, (T *) Y, ldy, a.m, cfg.beta, vw, part_off, cfg.map);
	else
		hipLaunchKernelGGL((sell_window_spmm_kernel<T, K, S, false>), dim3(grid), dim3(a.threads), lds_bytes, stream, a.grp, a.sdesc, a.idx,
				(const T *) a.val, a.row_of_sorted, (const T *) X, ldx, (T *) Y, ldy, a.m, cfg.beta, vw, part_off, cfg.map);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <typename T, int S>
static int
sellw_spmm_passes(int kmax, const SellwSpmmArgs & a, int k, const void * X, long ldx, void * Y, long ldy, const LaunchCfg & cfg, unsigned grid,
		hipStream_t stream)
{
	for (int j0 = 0; j0 < k;)
	{
		const int K = spmm_pass_cols(kmax, k - j0);
		const void * Xp = (const T *) X + j0;
		void * Yp = (T *) Y + j0;
		const int rc = K == 8 ? sellw_spmm_launch<T, 8, S>(a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		             : K == 4 ? sellw_spmm_launch<T, 4, S>(a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		             : K == 2 ? sellw_spmm_launch<T, 2, S>(a, Xp, ldx, Yp, ldy, cfg, grid, stream)
		                      : sellw_spmm_launch<T, 1, S>(a, Xp, ldx, Yp, ldy, cfg, grid, stream);
		if (rc)
			return rc;
		j0 += K;
	}
	return 0;
}

int
launch_sell_window_spmm(bool f32, int waves_per_slice, int slices_per_group, const int * grp, const int64_t * sdesc, const unsigned short * idx,
		const void * val, const int * row_of_sorted, int k, const void * X, long ldx, void * Y, long ldy, int m, int wmax, const LaunchCfg & cfg,
		hipStream_t stream, long * grid_out)
{
	const int threads = waves_per_slice * slices_per_group * WAVE;
	if (threads < WAVE || threads > 1024)
	{
		set_error("sell window spmm: %d slices x %d waves per workgroup (at most 16 waves)", slices_per_group, waves_per_slice);
		return 1;
	}
	const unsigned grid = xcd_grid(cfg.map);
	if (grid_out)
		*grid_out = grid;
	if (grid == 0)
		return 0;
	const int kmax = sell_window_spmm_max_cols(f32, waves_per_slice, slices_per_group, wmax);
	const SellwSpmmArgs a{grp, sdesc, idx, val, row_of_sorted, m, threads, wmax};
	#define SELLW_SPMM_S(S_) (f32 ? sellw_spmm_passes<float, S_>(kmax, a, k, X, ldx, Y, ldy, cfg, grid, stream) \
	                              : sellw_spmm_passes<double, S_>(kmax, a, k, X, ldx, Y, ldy, cfg, grid, stream))
	switch (waves_per_slice)
	{
		case 1: return SELLW_SPMM_S(1);
		case 2: return SELLW_SPMM_S(2);
		case 4: return SELLW_SPMM_S(4);
		case 8: return SELLW_SPMM_S(8);
	}
	#undef SELLW_SPMM_S
	set_error("sell window spmm: waves per slice must be 1, 2, 4 or 8 (got %d)", waves_per_slice);
	return 1;
}

}  // namespace spmv

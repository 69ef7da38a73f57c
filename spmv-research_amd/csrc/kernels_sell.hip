// SELL-C-sigma SpMV for gfx950.
//
// Replaces the reference's sliced-ELL kernels (benchmark_code/BENCH/src/spmv_kernels/sell_sorted.cpp:338-419 — C = SIMD
// width, hardware gather, y scattered through rev_permutation — and the BSC library driven by sell_c_s.cpp:124-131,
// sell-C-s/RISC-V/sellcs_mv_kernels_epi.c:178-257 — C = 256, sigma = 16384, descending radix sort per window).
//
// Layout (built in build_sell.hip, on the GPU in convert_sell.hip): rows are sorted by length (descending, stable) inside windows of sigma rows; a slice
// is C consecutive sorted rows, stored column-major and padded to the slice's longest row, so that the 64 lanes of ONE
// wavefront read 64 consecutive values / column indices per step:
//       element (row r of the slice, column k)  ->  slice_ptr[s] + k*C + r
// One wavefront owns one slice. With C = 64 a lane owns a row and walks it left to right with one FMA per element
// (padding multiplies 0 by the x entry of the row's own last column; an empty row has none, is padded with column 0 and has its sum
// dropped: row_len, launch.hpp), i.e. y is bit-identical to the sequential CSR row loop, for x that holds Inf or NaN too. With C = 32 / 16 the
// wave covers 2 / 4 consecutive columns per step (lane = (k % TPR)*C + r); the TPR partial sums of a row are combined by
// a fixed xor-butterfly. The slice width is padded to a multiple of TPR. Smaller C = more wavefronts and shorter
// dependent chains for small matrices, at the cost of the butterfly.
//
// y is scattered through row_of_sorted (the reference does the same: sell_sorted.cpp:392-395).

#include <type_traits>

#include "sell_delta_read.hpp"

namespace spmv {

constexpr int SELL_BLOCK = 256;
constexpr int SELL_WAVES = SELL_BLOCK / WAVE;

template <typename T, int C, bool NT>
__global__ __launch_bounds__(SELL_BLOCK) void
sell_kernel(const int64_t * __restrict__ slice_ptr, const int * __restrict__ col, const T * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const T * __restrict__ x, T * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int slice = tile * SELL_WAVES + threadIdx.x / WAVE;
	if (slice >= num_slices)
		return;                       // whole wavefront leaves together: no shuffle after a partial exit
	const int64_t p_s = slice_ptr[slice];
	const int64_t p_e = slice_ptr[slice + 1];
	T s0 = 0, s1 = 0, s2 = 0, s3 = 0;
	int64_t p = p_s + lane;
	// 4 wave-steps per trip: 4 value + 4 index loads in flight per lane before the first dependent x gather.
	// A lane's own partial sums s0..s3 belong to the same row only when C == 64 and are then added in column order
	// below; for the bit-exact C == 64 path a single accumulator chain is used instead.
	if constexpr (C == WAVE)
	{
		for (; p + 3 * WAVE < p_e; p += 4 * WAVE)
		{
			const int c0 = ld_stream<NT>(col + p);
			const int c1 = ld_stream<NT>(col + p + WAVE);
			const int c2 = ld_stream<NT>(col + p + 2 * WAVE);
			const int c3 = ld_stream<NT>(col + p + 3 * WAVE);
			const T v0 = ld_stream<NT>(val + p);
			const T v1 = ld_stream<NT>(val + p + WAVE);
			const T v2 = ld_stream<NT>(val + p + 2 * WAVE);
			const T v3 = ld_stream<NT>(val + p + 3 * WAVE);
			const T x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
			s0 = fma_t<T>(v0, x0, s0);
			s0 = fma_t<T>(v1, x1, s0);
			s0 = fma_t<T>(v2, x2, s0);
			s0 = fma_t<T>(v3, x3, s0);
		}
		if (p < p_e)
		{
			// 1..3 leftover steps as ONE masked batch (a serial tail would expose a full memory round trip per step)
			const bool k1 = p + WAVE < p_e, k2 = p + 2 * WAVE < p_e;
			const int c0 = ld_stream<NT>(col + p);
			const int c1 = k1 ? ld_stream<NT>(col + p + WAVE) : 0;
			const int c2 = k2 ? ld_stream<NT>(col + p + 2 * WAVE) : 0;
			const T v0 = ld_stream<NT>(val + p);
			const T v1 = k1 ? ld_stream<NT>(val + p + WAVE) : T(0);
			const T v2 = k2 ? ld_stream<NT>(val + p + 2 * WAVE) : T(0);
			const T x0 = x[c0];
			const T x1 = k1 ? x[c1] : T(0);
			const T x2 = k2 ? x[c2] : T(0);
			s0 = fma_t<T>(v0, x0, s0);
			if (k1) s0 = fma_t<T>(v1, x1, s0);
			if (k2) s0 = fma_t<T>(v2, x2, s0);
		}
	}
	else
	{
		for (; p + 3 * WAVE < p_e; p += 4 * WAVE)
		{
			const int c0 = ld_stream<NT>(col + p);
			const int c1 = ld_stream<NT>(col + p + WAVE);
			const int c2 = ld_stream<NT>(col + p + 2 * WAVE);
			const int c3 = ld_stream<NT>(col + p + 3 * WAVE);
			const T v0 = ld_stream<NT>(val + p);
			const T v1 = ld_stream<NT>(val + p + WAVE);
			const T v2 = ld_stream<NT>(val + p + 2 * WAVE);
			const T v3 = ld_stream<NT>(val + p + 3 * WAVE);
			s0 = fma_t<T>(v0, x[c0], s0);
			s1 = fma_t<T>(v1, x[c1], s1);
			s2 = fma_t<T>(v2, x[c2], s2);
			s3 = fma_t<T>(v3, x[c3], s3);
		}
		if (p < p_e)
		{
			const bool k1 = p + WAVE < p_e, k2 = p + 2 * WAVE < p_e;
			const int c0 = ld_stream<NT>(col + p);
			const int c1 = k1 ? ld_stream<NT>(col + p + WAVE) : 0;
			const int c2 = k2 ? ld_stream<NT>(col + p + 2 * WAVE) : 0;
			const T v0 = ld_stream<NT>(val + p);
			const T v1 = k1 ? ld_stream<NT>(val + p + WAVE) : T(0);
			const T v2 = k2 ? ld_stream<NT>(val + p + 2 * WAVE) : T(0);
			s0 = fma_t<T>(v0, x[c0], s0);
			if (k1) s1 = fma_t<T>(v1, x[c1], s1);
			if (k2) s2 = fma_t<T>(v2, x[c2], s2);
		}
		s0 = (s0 + s1) + (s2 + s3);
		// combine the TPR = 64/C column phases of each row: lanes r, r+C, r+2C, ...
		#pragma unroll
		for (int off = C; off < WAVE; off <<= 1)
			s0 += shfl_xor_t(s0, off);
	}
	if (lane < C)
	{
		const long sorted_row = (long) slice * C + lane;
		if (sorted_row < m)
		{
			// the padding of a row multiplies 0 by the row's own last column; an empty row has none and is padded with column 0, which is
			// not its own: what it summed (0 * x[0], NaN when x[0] is not finite) is dropped
			if (row_len[sorted_row] == 0)
				s0 = 0;
			T * yp = y + row_of_sorted[sorted_row];
			*yp = beta ? *yp + s0 : s0;
		}
	}
}

// The BSC library's own slice height (sell_c_s.cpp:58-60: C = 256): one workgroup of 256 lanes = one slice, lane r owns sorted
// row r of the slice and walks it left to right with one FMA per element (bit-identical to the sequential CSR loop, as C = 64).
constexpr int SELL_WIDE_C = 256;

template <typename T, bool NT>
__global__ __launch_bounds__(SELL_WIDE_C) void
sell_wide_kernel(const int64_t * __restrict__ slice_ptr, const int * __restrict__ col, const T * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const T * __restrict__ x, T * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	constexpr int C = SELL_WIDE_C;
	const unsigned slice = xcd_tile(blockIdx.x, map);
	if (slice == NO_TILE || (int) slice >= num_slices)
		return;
	const int64_t p_e = slice_ptr[slice + 1];
	int64_t p = slice_ptr[slice] + threadIdx.x;
	T s = 0;
	for (; p + 3 * C < p_e; p += 4 * C)
	{
		const int c0 = ld_stream<NT>(col + p), c1 = ld_stream<NT>(col + p + C), c2 = ld_stream<NT>(col + p + 2 * C), c3 = ld_stream<NT>(col + p + 3 * C);
		const T v0 = ld_stream<NT>(val + p), v1 = ld_stream<NT>(val + p + C), v2 = ld_stream<NT>(val + p + 2 * C), v3 = ld_stream<NT>(val + p + 3 * C);
		const T x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
		s = fma_t<T>(v0, x0, s);
		s = fma_t<T>(v1, x1, s);
		s = fma_t<T>(v2, x2, s);
		s = fma_t<T>(v3, x3, s);
	}
	for (; p < p_e; p += C)
		s = fma_t<T>(ld_stream<NT>(val + p), x[ld_stream<NT>(col + p)], s);
	const long sorted_row = (long) slice * C + threadIdx.x;
	if (sorted_row < m)
	{
		if (row_len[sorted_row] == 0)          // an empty row's padding is not a column of its own (sell_kernel)
			s = 0;
		T * yp = y + row_of_sorted[sorted_row];
		*yp = beta ? *yp + s : s;
	}
}

// ------------------------------------------------------------------------------------------------ SELL-64-sigma-delta
// Column indices are the only compressible stream of SpMV (values are data, x and y are compulsory). In a 64-row slice
// the 64 lanes of step k hold neighbouring rows, and on banded / stencil / FEM matrices their columns sit within a few
// hundred entries of each other. Per slice the indices are therefore stored as one int32 base per step plus one
// unsigned delta per lane: 8 bits (9.06 B per fp64 non-zero), 16 bits (10.06 B), or plain int32 when neither fits (12 B, as
// plain SELL), or as lane offsets with no bytes per lane and step at all (layout: sell_delta_layout.hpp).
// The bases are wave-uniform (scalar loads). Arithmetic and its order are exactly those of sell_kernel<C = 64>: one lane
// per row, one FMA per element, left to right -> bit-identical to the sequential CSR loop; lossless by construction.
// HBM bytes per non-zero drop by up to 24 % (fp64) / 37 % (fp32) below the CSR-normalised "algorithmic" 12 / 8 bytes.
// The value readers and index decoders live in sell_delta_read.hpp, shared with the multi-vector kernel (kernels_sell_spmm.hip).

// PAD: the slice holds rows shorter than its width (modes 1, 2 and 4 only: the others need equally long rows). Their padding steps store
// 0.0 and a column that some OTHER row of the slice uses, so x is kept out of them: a lane's steps from `len` (its row's length) on
// take 0 in place of x[column]. The instantiations without PAD are what they were.
template <typename T, int MODE, bool NT, bool V7, int NSTEPS = 4, typename S = T, bool PAD = false>
__device__ __forceinline__ void
sell_delta_group(const unsigned char * __restrict__ gp /* uniform */, const SellVals<T, NT, V7, S> & vals, int g, int lane, const T * __restrict__ x, T & s,
		int off = 0, int len = 0)
{
	int c[4];
	sell_group_cols<MODE, NT>(gp, lane, off, c);
	const int c0 = c[0], c1 = c[1], c2 = c[2], c3 = c[3];
	if (PAD)
	{
		// (the gathers themselves stay unconditional: every stored column is a valid one)
		T v[4] = {T(0), T(0), T(0), T(0)};
		if (NSTEPS == 4)
			vals.group(g, v);
		else
		{
			T tv[3];
			sell_tail_values<T, NT, NSTEPS>(vals.tail(g), lane, tv);
			v[0] = tv[0];
			v[1] = tv[1];
			v[2] = tv[2];
		}
		const int left = len - 4 * g;                       // real steps of this lane from the group's first on
		const T x0 = left > 0 ? x[c0] : T(0);
		const T x1 = (NSTEPS > 1 && left > 1) ? x[c1] : T(0);
		const T x2 = (NSTEPS > 2 && left > 2) ? x[c2] : T(0);
		const T x3 = (NSTEPS > 3 && left > 3) ? x[c3] : T(0);
		s = fma_t<T>(v[0], x0, s);
		if (NSTEPS > 1) s = fma_t<T>(v[1], x1, s);
		if (NSTEPS > 2) s = fma_t<T>(v[2], x2, s);
		if (NSTEPS > 3) s = fma_t<T>(v[3], x3, s);
	}
	else if (NSTEPS == 4)
	{
		T v[4];
		vals.group(g, v);
		const T x0 = x[c0], x1 = x[c1], x2 = x[c2], x3 = x[c3];
		s = fma_t<T>(v[0], x0, s);
		s = fma_t<T>(v[1], x1, s);
		s = fma_t<T>(v[2], x2, s);
		s = fma_t<T>(v[3], x3, s);
	}
	else
	{
		// last group of a slice whose width is not a multiple of 4: the value array holds only the real steps
		T v[3];
		sell_tail_values<T, NT, NSTEPS>(vals.tail(g), lane, v);
		const T x0 = x[c0];
		const T x1 = NSTEPS > 1 ? x[c1] : T(0);
		const T x2 = NSTEPS > 2 ? x[c2] : T(0);
		s = fma_t<T>(v[0], x0, s);
		if (NSTEPS > 1) s = fma_t<T>(v[1], x1, s);
		if (NSTEPS > 2) s = fma_t<T>(v[2], x2, s);
	}
}

// hipcc sinks a load whose result is only used in the NEXT trip of a loop (through `a = na`) down to that use — the loads are
// invariant, so it may — and the hand-written prefetch becomes a dependent load in front of the gathers again. Passing the prefetched
// registers through an empty asm statement at the END of the trip pins them to the trip they were issued in: the wait for them lands
// behind this trip's gathers and FMAs, where it costs nothing.
__device__ __forceinline__ void
sell_pin(unsigned & v)
{
	asm volatile("" : "+v"(v));
}
__device__ __forceinline__ void
sell_pin(sell_uint2 & v, bool both)
{
	unsigned a = v.x, b = both ? v.y : 0u;
	asm volatile("" : "+v"(a), "+v"(b));
	v.x = a;
	if (both)
		v.y = b;
}


// the full 4-step groups number g0, g0+gs, ... (n of them) of a slice in mode 1 / 2: FOUR groups per trip (16 steps in flight: all loads of a
// trip are issued before its first FMA), their index words fetched one trip ahead; what is left (0..3 groups) as a pair and / or a single
// group on the index words the last trip already fetched. (Two groups per trip: 1 347 us with every index-free mode off; four: see
// profiles/r03_sell_value_pairs.txt.)
template <typename T, int MODE, bool NT, bool V7, int NG, typename S = T>
__device__ __forceinline__ void
sell_delta_consume(const SellDeltaIdx<MODE> * q, const SellVals<T, NT, V7, S> & vals, const int * g, const T * __restrict__ x, T & s)
{
	T v[NG][4];
	int c[NG][4];
	T xv[NG][4];
	#pragma unroll
	for (int u = 0; u < NG; u++)
		vals.group(g[u], v[u]);
	#pragma unroll
	for (int u = 0; u < NG; u++)
		sell_delta_cols<MODE>(q[u], c[u]);
	#pragma unroll
	for (int u = 0; u < NG; u++)
		#pragma unroll
		for (int t = 0; t < 4; t++)
			xv[u][t] = x[c[u][t]];
	#pragma unroll
	for (int u = 0; u < NG; u++)
		#pragma unroll
		for (int t = 0; t < 4; t++)
			s = fma_t<T>(v[u][t], xv[u][t], s);
}

template <typename T, int MODE, bool NT, bool V7, typename S = T>
__device__ __forceinline__ void
sell_delta_piped(const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, S> & vals, int lane, const T * __restrict__ x, T & s, int g0, int gs, int n)
{
	constexpr long GB = sell_group_bytes(MODE);
	if (n <= 0)
		return;
	auto gidx = [&](int k) { return g0 + (k < n ? k : n - 1) * gs; };       // past the end: the last group again (loaded, not used)
	SellDeltaIdx<MODE> q[4], nq[4];
	#pragma unroll
	for (int u = 0; u < 4; u++)
		sell_delta_load_idx<MODE, NT>(q[u], ip + (size_t) gidx(u) * GB, lane);
	int k = 0;
	for (; k + 4 <= n; k += 4)
	{
		#pragma unroll
		for (int u = 0; u < 4; u++)
			sell_delta_load_idx<MODE, NT>(nq[u], ip + (size_t) gidx(k + 4 + u) * GB, lane);
		const int g[4] = {gidx(k), gidx(k + 1), gidx(k + 2), gidx(k + 3)};
		sell_delta_consume<T, MODE, NT, V7, 4>(q, vals, g, x, s);
		#pragma unroll
		for (int u = 0; u < 4; u++)
		{
			sell_pin(nq[u].d, MODE == 2);
			q[u] = nq[u];
		}
	}
	const int r = n - k;                               // 0..3 groups left; q[0..r-1] hold their index words (wave-uniform branches)
	if (r >= 2)
	{
		const int g[2] = {gidx(k), gidx(k + 1)};
		sell_delta_consume<T, MODE, NT, V7, 2>(q, vals, g, x, s);
	}
	if (r == 1)                                        // (constant indices into q: a run-time one would send the array to scratch memory)
	{
		const int g[1] = {gidx(k)};
		sell_delta_consume<T, MODE, NT, V7, 1>(q, vals, g, x, s);
	}
	if (r == 3)
	{
		const int g[1] = {gidx(k + 2)};
		sell_delta_consume<T, MODE, NT, V7, 1>(q + 2, vals, g, x, s);
	}
}

// groups g0, g0+gs, g0+2gs, ... of one slice (gs = 1: the whole slice, in order). PAD (sell_delta_group): the lane's row holds `len`
// entries; such a slice takes the in-place readers below in every mode, without the index words fetched a trip ahead.
template <typename T, int MODE, bool NT, bool PAD, bool V7, typename S>
__device__ __forceinline__ T
sell_delta_slice(const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, S> & vals, int width, int lane, const T * __restrict__ x,
		int g0 = 0, int gs = 1, int len = 0)
{
	constexpr long GB = sell_group_bytes(MODE);
	const int groups = (width + 3) / 4;     // index groups cover the width rounded up to 4 steps, values only the real steps
	const int rem = width - 4 * (groups - 1);
	int off = lane;
	if constexpr (MODE == 3)
	{
		off = ld_stream<NT>(reinterpret_cast<const int *>(ip) + lane);          // the slice's 64 lane offsets, then the groups
		ip += sell_header_bytes(3);
	}
	T s = 0;
	int g = g0;
	const int last = groups - 1;            // the last group holds `rem` (1..4) steps
	if constexpr ((MODE == 1 || MODE == 2) && !PAD)
	{
		const int full = rem == 4 ? groups : last;
		const int n = full > g0 ? (full - g0 + gs - 1) / gs : 0;
		sell_delta_piped<T, MODE, NT, V7>(ip, vals, lane, x, s, g0, gs, n);
		g = g0 + n * gs;
	}
	// 16, then 12, then 8 steps in flight per trip: a slice of 7 full groups (the nlpkkt240 twin's 27-28 entries per row) is 4 + 3. The
	// loads of a trip are independent of its FMAs, so the compiler issues all of them first; deeper trips measured 2-3 % faster than
	// pairs alone on the twin (1 152-1 185 against 1 198-1 207 us, profiles/r03_sell_value_pairs.txt).
	const int full_end = rem == 4 ? groups : last;
	for (; !PAD && g + 3 * gs < full_end; g += 4 * gs)               // (a padded slice goes by pairs: the few there are get no deeper trips of their own)
	{
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + gs) * GB, vals, g + gs, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + 2 * gs) * GB, vals, g + 2 * gs, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + 3 * gs) * GB, vals, g + 3 * gs, lane, x, s, off, len);
	}
	for (; !PAD && g + 2 * gs < full_end; g += 3 * gs)
	{
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + gs) * GB, vals, g + gs, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + 2 * gs) * GB, vals, g + 2 * gs, lane, x, s, off, len);
	}
	for (; g + gs < (rem == 4 ? groups : last); g += 2 * gs)    // 8 steps in flight per trip
	{
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) (g + gs) * GB, vals, g + gs, lane, x, s, off, len);
	}
	for (; g < (rem == 4 ? groups : last); g += gs)
		sell_delta_group<T, MODE, NT, V7, 4, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
	if (rem != 4 && g == last)
	{
		if (rem == 1)
			sell_delta_group<T, MODE, NT, V7, 1, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
		else if (rem == 2)
			sell_delta_group<T, MODE, NT, V7, 2, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
		else
			sell_delta_group<T, MODE, NT, V7, 3, S, PAD>(ip + (size_t) g * GB, vals, g, lane, x, s, off, len);
	}
	return s;
}


// keeps what was fetched a trip ahead in the trip it was fetched in (sell_pin above)
template <bool SCALAR>
__device__ __forceinline__ void
sell_pin5(SellDeltaIdx5 & q)
{
	if constexpr (SCALAR)
	{
		int a = q.corr.x, b = q.corr.y, c = q.corr.z, d = q.corr.w;
		asm volatile("" : "+s"(a), "+s"(b), "+s"(c), "+s"(d));
		q.corr.x = a;
		q.corr.y = b;
		q.corr.z = c;
		q.corr.w = d;
	}
	else
		sell_pin(q.d);
}

template <typename T, bool NT, bool V7, bool SCALAR, typename S = T>
__device__ __forceinline__ T
sell_delta_slice5_body(const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, S> & vals, int width, int lane, const T * __restrict__ x,
		int g0, int gs, unsigned long long mask, int off)
{
	const int E = __popcll(mask);
	const bool ex = (mask >> lane) & 1ull;
	const int rank = ex ? __popcll(mask & ((1ull << lane) - 1ull)) : 0;
	int xl[4] = {0, 0, 0, 0};
	if constexpr (SCALAR)
	{
		unsigned long long mm = mask;
		const int spare = __builtin_ctzll(~mask);                       // a lane that is no exception (at least 48 are not)
		#pragma unroll
		for (int j = 0; j < 4; j++)
		{
			xl[j] = mm ? __builtin_ctzll(mm) : spare;
			mm &= mm - 1ull;
		}
	}
	const size_t GB = sell_group_bytes(5, E);
	const int groups = (width + 3) / 4;
	const int rem = width - 4 * (groups - 1);
	const int last = groups - 1;
	const int full = rem == 4 ? groups : last;
	const int n = full > g0 ? (full - g0 + gs - 1) / gs : 0;     // full groups this wave takes: g0, g0 + gs, ...
	T s = 0;
	if (n > 0)
	{
		// four groups per trip, index words (and corrections) one trip ahead; the 0..3 groups left as a pair and / or a single one
		// (sell_delta_piped above)
		auto gidx = [&](int k) { return g0 + (k < n ? k : n - 1) * gs; };       // past the end: the last group again (loaded, not used)
		auto consume = [&](const SellDeltaIdx5 * q, const int * g, auto ng) {
			constexpr int NG = decltype(ng)::value;
			T v[NG][4];
			int c[NG][4];
			T xv[NG][4];
			#pragma unroll
			for (int u = 0; u < NG; u++)
				vals.group(g[u], v[u]);
			#pragma unroll
			for (int u = 0; u < NG; u++)
				sell_delta_cols5<SCALAR>(q[u], ex, lane, off, xl, c[u]);
			#pragma unroll
			for (int u = 0; u < NG; u++)
				#pragma unroll
				for (int t = 0; t < 4; t++)
					xv[u][t] = x[c[u][t]];
			#pragma unroll
			for (int u = 0; u < NG; u++)
				#pragma unroll
				for (int t = 0; t < 4; t++)
					s = fma_t<T>(v[u][t], xv[u][t], s);
		};
		SellDeltaIdx5 q[4], nq[4];
		#pragma unroll
		for (int u = 0; u < 4; u++)
			sell_delta_load_idx5<NT, SCALAR>(q[u], ip + (size_t) gidx(u) * GB, rank);
		int k = 0;
		for (; k + 4 <= n; k += 4)
		{
			#pragma unroll
			for (int u = 0; u < 4; u++)
				sell_delta_load_idx5<NT, SCALAR>(nq[u], ip + (size_t) gidx(k + 4 + u) * GB, rank);
			const int g[4] = {gidx(k), gidx(k + 1), gidx(k + 2), gidx(k + 3)};
			consume(q, g, std::integral_constant<int, 4>());
			#pragma unroll
			for (int u = 0; u < 4; u++)
			{
				sell_pin5<SCALAR>(nq[u]);
				q[u] = nq[u];
			}
		}
		const int r = n - k;
		if (r >= 2)
		{
			const int g[2] = {gidx(k), gidx(k + 1)};
			consume(q, g, std::integral_constant<int, 2>());
		}
		if (r == 1)
		{
			const int g[1] = {gidx(k)};
			consume(q, g, std::integral_constant<int, 1>());
		}
		if (r == 3)
		{
			const int g[1] = {gidx(k + 2)};
			consume(q + 2, g, std::integral_constant<int, 1>());
		}
	}
	// the last group of a slice whose width is not a multiple of 4 (the value array holds only its `rem` real steps); with several
	// waves per slice it belongs to the wave whose sequence g0, g0 + gs, ... reaches it
	if (rem != 4 && last >= g0 && (last - g0) % gs == 0)
	{
		SellDeltaIdx5 q;
		sell_delta_load_idx5<NT, SCALAR>(q, ip + (size_t) last * GB, rank);
		int c[4];
		sell_delta_cols5<SCALAR>(q, ex, lane, off, xl, c);
		const S * vl = vals.tail(last);
		T tv[3];
		if (rem == 1)
			sell_tail_values<T, NT, 1>(vl, lane, tv);
		else if (rem == 2)
			sell_tail_values<T, NT, 2>(vl, lane, tv);
		else
			sell_tail_values<T, NT, 3>(vl, lane, tv);
		const T v0 = tv[0], v1 = tv[1], v2 = tv[2];
		const T x0 = x[c[0]];
		const T x1 = rem > 1 ? x[c[1]] : T(0);
		const T x2 = rem > 2 ? x[c[2]] : T(0);
		s = fma_t<T>(v0, x0, s);
		if (rem > 1) s = fma_t<T>(v1, x1, s);
		if (rem > 2) s = fma_t<T>(v2, x2, s);
	}
	return s;
}

template <typename T, bool NT, bool V7, typename S = T>
__device__ __forceinline__ T
sell_delta_slice5(const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, S> & vals, int width, int lane, const T * __restrict__ x,
		int g0 = 0, int gs = 1)
{
	const int off = ld_stream<NT>(reinterpret_cast<const int *>(ip) + lane);
	const unsigned long long mask = *reinterpret_cast<const unsigned long long *>(ip + 4 * WAVE);          // uniform: a scalar load
	ip += sell_header_bytes(5);
	if (__popcll(mask) <= 4)
		return sell_delta_slice5_body<T, NT, V7, true>(ip, vals, width, lane, x, g0, gs, mask, off);
	return sell_delta_slice5_body<T, NT, V7, false>(ip, vals, width, lane, x, g0, gs, mask, off);
}

// one slice (groups g0, g0 + gs, ... of it) in its index mode; a wave-uniform branch
template <typename T, bool NT, bool V7, typename S = T>
__device__ __forceinline__ T
sell_delta_modes(int mode, const unsigned char * __restrict__ ip, const SellVals<T, NT, V7, S> & vals, int width, int lane, const T * __restrict__ x,
		int g0, int gs, bool padded /* uniform */, const int * __restrict__ slice_len /* uniform */)
{
	if (mode == 0)
		return sell_delta_slice<T, 0, NT, false>(ip, vals, width, lane, x, g0, gs);
	if (mode == 3)
		return sell_delta_slice<T, 3, NT, false>(ip, vals, width, lane, x, g0, gs);
	if (mode == 5)
		return sell_delta_slice5<T, NT>(ip, vals, width, lane, x, g0, gs);
	// the modes with a column per lane and step are the ones whose slices may hold rows of different lengths: the few that do go to
	// the readers that mask the padding steps (sell_delta_group)
	if (padded)
	{
		const int len = slice_len[lane];
		if (mode == 1)
			return sell_delta_slice<T, 1, NT, true>(ip, vals, width, lane, x, g0, gs, len);
		if (mode == 2)
			return sell_delta_slice<T, 2, NT, true>(ip, vals, width, lane, x, g0, gs, len);
		return sell_delta_slice<T, 4, NT, true>(ip, vals, width, lane, x, g0, gs, len);
	}
	if (mode == 1)
		return sell_delta_slice<T, 1, NT, false>(ip, vals, width, lane, x, g0, gs);
	if (mode == 2)
		return sell_delta_slice<T, 2, NT, false>(ip, vals, width, lane, x, g0, gs);
	return sell_delta_slice<T, 4, NT, false>(ip, vals, width, lane, x, g0, gs);
}

// one slice from its two descriptor words (sell_delta_layout.hpp): V7 = the handle holds slices with 7-byte values, each one flagged in
// desc[2s+1]; without it the code is that of the plain pairs alone. S: the type the values are stored in (sell_delta_read.hpp)
template <typename T, bool NT, bool V7, typename S = T>
__device__ __forceinline__ T
sell_delta_one(const int64_t * __restrict__ desc, int slice, const unsigned char * __restrict__ idx, const S * __restrict__ val, int lane,
		const T * __restrict__ x, int g0, int gs, const int * __restrict__ row_len, int num_slices)
{
	const int64_t v_off = desc[2 * slice];
	const int64_t i_word = desc[2 * slice + 1];
	const int64_t v_next = desc[2 * slice + 2];
	// whether the slice holds value padding (launch.hpp: sell_pad_bits): uniform, a scalar load beside the descriptor's
	const bool padded = (sell_pad_bits(row_len, num_slices, WAVE)[slice >> 5] >> (slice & 31)) & 1u;
	const int * slice_len = row_len + (long) slice * WAVE;          // the lengths of the slice's 64 rows (uniform)
	const int mode = sell_desc_mode(i_word);
	const unsigned char * ip = idx + sell_desc_idx(i_word);
	const S * vp = val + v_off + 2 * lane;
	if (V7 && sell_desc_v7(i_word))
		return sell_delta_modes<T, NT, V7>(mode, ip, SellVals<T, NT, V7, S>{vp, lane, (unsigned) (sell_v7_e0(i_word) - 1) << 20},
				(int) sell_slice_width(v_next - v_off, true), lane, x, g0, gs, padded, slice_len);
	return sell_delta_modes<T, NT, false>(mode, ip, SellVals<T, NT, false, S>{vp, lane, 0u}, (int) sell_slice_width(v_next - v_off, false), lane, x,
			g0, gs, padded, slice_len);
}

// sell_delta_kernel has a workgroup size of its own (launch.hpp: SELL_DELTA_WAVES), apart from the SELL_WAVES that
// sell_delta_split_kernel needs for its LDS sums: ONE slice = one wave per workgroup for fp64 (the nlpkkt240 twin: 1.05 ms against
// 1.09 - 1.10 at four, 1.07 - 1.08 at two; the 8-byte kernel 1.13 against 1.18; profiles/r13_sell_v7_bound.txt). A wave that finishes
// its slice early no longer holds its workgroup's slot until the other three are through. fp32 keeps four (not measured).
static_assert(SELL_WAVES % SELL_DELTA_WAVES == 0, "the handle's tiles are whole numbers of sell_delta_kernel's");
template <typename T> constexpr int sell_delta_waves() { return sizeof(T) == 8 ? SELL_DELTA_WAVES : SELL_WAVES; }

// The handle's tile map counts tiles of SELL_WAVES slices (launch.hpp: sell_slices_per_tile). The same map for tiles of W slices:
// F = SELL_WAVES / W times as many tiles, chunks of F times as many tiles (the same 16 384 rows per chunk), the work-balanced ranges
// cut at the same slices. Every tile, and so every slice, is still dealt exactly once: xcd_tile maps the grid one-to-one onto the tile
// numbers below the grid size for any chunk, and the ranges [start[k], start[k+1]) still partition [0, ntiles).
template <int W>
static XcdMap
sell_delta_tile_map(const XcdMap & mp, int num_slices)
{
	constexpr unsigned F = SELL_WAVES / W;
	XcdMap o = mp;
	o.ntiles = ((unsigned) num_slices + W - 1) / W;
	o.chunk = mp.chunk * F;
	for (int k = 0; k < NUM_XCD; k++)
		o.start[k] = mp.start[k] * F < o.ntiles ? mp.start[k] * F : o.ntiles;
	o.start[NUM_XCD] = o.ntiles;
	return o;
}

// one wave per slice, W of them per workgroup. No occupancy attribute: left alone the compiler gives the V7 kernel 107 VGPRs = 4 waves
// per SIMD, which measured no slower than the 5 waves at 92 VGPRs it was held to before and faster at W = 1 (1.049 - 1.050 against
// 1.051 - 1.090 ms, no scratch either way; profiles/r13_sell_v7_bound.txt).
template <typename T, bool NT, bool V7, int W = sell_delta_waves<T>()>
__global__ __launch_bounds__(W * WAVE) void
sell_delta_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const T * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const T * __restrict__ x, T * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * W + threadIdx.x / WAVE));
	if (slice >= num_slices)
		return;
	const T s = sell_delta_one<T, NT, V7>(desc, slice, idx, val, lane, x, 0, 1, row_len, num_slices);
	const long sorted_row = (long) slice * WAVE + lane;
	if (sorted_row < m)
	{
		T * yp = y + row_of_sorted[sorted_row];
		*yp = beta ? *yp + s : s;
	}
}

// Small matrices (a few thousand slices) cannot fill 256 CUs with one wave per slice: S waves share a slice, wave w takes
// the index groups w, w+S, ..., the S partial sums of a row meet in LDS and are added in wave order (deterministic;
// no longer the sequential order, so parity is to tolerance). One workgroup = 4/S slices.
template <typename T, int S, bool NT, bool V7>
__global__ __launch_bounds__(SELL_BLOCK) void
sell_delta_split_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const T * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const T * __restrict__ x, T * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	constexpr int SPB = SELL_WAVES / S;      // slices per workgroup
	__shared__ T s_part[SELL_WAVES][WAVE];
	unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int wave = threadIdx.x / WAVE;
	const int w = __builtin_amdgcn_readfirstlane(wave % S);          // wave-uniform, and the compiler should know: group addresses stay scalar
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * SPB + wave / S));
	T s = 0;
	if (slice < num_slices)
		s = sell_delta_one<T, NT, V7>(desc, slice, idx, val, lane, x, w, S, row_len, num_slices);
	s_part[wave][lane] = s;
	__syncthreads();
	if (w == 0 && slice < num_slices)
	{
		T t = s_part[wave][lane];
		#pragma unroll
		for (int u = 1; u < S; u++)
			t += s_part[wave + u][lane];
		const long sorted_row = (long) slice * WAVE + lane;
		if (sorted_row < m)
		{
			T * yp = y + row_of_sorted[sorted_row];
			*yp = beta ? *yp + t : t;
		}
	}
}

// fp32 values under fp64 vectors (opts.value_storage = 1): sell_delta_kernel<double> on the fp32 handle's arrays — the values are read
// from the fp32 pair layout and widened (sell_delta_read.hpp), the gathers and FMAs are the fp64 kernel's in its order -> bit-identical
// to the fp64 kernel on the values rounded to fp32. Kernels of their own names, so that every instantiation above keeps its symbol
// and its code. (VGPRs and occupancy beside the fp64 kernels': profiles/r08_value_storage.txt)
template <bool NT>
__global__ __launch_bounds__(SELL_BLOCK) void
sell_delta_mixed_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const float * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const double * __restrict__ x, double * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * SELL_WAVES + threadIdx.x / WAVE));
	if (slice >= num_slices)
		return;
	const double s = sell_delta_one<double, NT, false>(desc, slice, idx, val, lane, x, 0, 1, row_len, num_slices);
	const long sorted_row = (long) slice * WAVE + lane;
	if (sorted_row < m)
	{
		double * yp = y + row_of_sorted[sorted_row];
		*yp = beta ? *yp + s : s;
	}
}

// ... S waves per slice (sell_delta_split_kernel)
template <int S, bool NT>
__global__ __launch_bounds__(SELL_BLOCK) void
sell_delta_mixed_split_kernel(const int64_t * __restrict__ desc, const unsigned char * __restrict__ idx, const float * __restrict__ val,
		const int * __restrict__ row_of_sorted, const int * __restrict__ row_len, const double * __restrict__ x, double * __restrict__ y,
		int m, int num_slices, int beta, XcdMap map)
{
	constexpr int SPB = SELL_WAVES / S;
	__shared__ double s_part[SELL_WAVES][WAVE];
	unsigned tile = xcd_tile(blockIdx.x, map);
	if (tile == NO_TILE)
		return;
	const int lane = threadIdx.x % WAVE;
	const int wave = threadIdx.x / WAVE;
	const int w = __builtin_amdgcn_readfirstlane(wave % S);
	const int slice = __builtin_amdgcn_readfirstlane((int) (tile * SPB + wave / S));
	double s = 0;
	if (slice < num_slices)
		s = sell_delta_one<double, NT, false>(desc, slice, idx, val, lane, x, w, S, row_len, num_slices);
	s_part[wave][lane] = s;
	__syncthreads();
	if (w == 0 && slice < num_slices)
	{
		double t = s_part[wave][lane];
		#pragma unroll
		for (int u = 1; u < S; u++)
			t += s_part[wave + u][lane];
		const long sorted_row = (long) slice * WAVE + lane;
		if (sorted_row < m)
		{
			double * yp = y + row_of_sorted[sorted_row];
			*yp = beta ? *yp + t : t;
		}
	}
}

// MIXED: T = double over values stored as float (sell_delta_mixed_kernel); V7 is then false
template <typename T, bool V7, bool MIXED = false>
static int
sell_delta_launch(int S, const int64_t * desc, const unsigned char * idx, const void * val, const int * row_of_sorted, const int * row_len, const void * x, void * y,
		int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	unsigned grid = xcd_grid(cfg.map);
	if (grid_out)
		*grid_out = grid;
	if (grid == 0)
		return 0;
	typedef std::conditional_t<MIXED, float, T> SV;
	#define SELLD_LAUNCH(K) hipLaunchKernelGGL(K, dim3(grid), dim3(SELL_BLOCK), 0, stream, desc, idx, (const SV *) val, \
			row_of_sorted, row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, cfg.map)
	if (S != 1 && S != 2 && S != 4)
	{
		set_error("sell_delta: waves per slice must be 1, 2 or 4 (got %d)", S);
		return 1;
	}
	if constexpr (MIXED)
	{
		static_assert(std::is_same<T, double>::value && !V7, "fp32 values under fp64 vectors, plain pairs");
		if (S == 1)
		{
			if (cfg.nt) SELLD_LAUNCH((sell_delta_mixed_kernel<true>));
			else        SELLD_LAUNCH((sell_delta_mixed_kernel<false>));
		}
		else if (S == 2)
		{
			if (cfg.nt) SELLD_LAUNCH((sell_delta_mixed_split_kernel<2, true>));
			else        SELLD_LAUNCH((sell_delta_mixed_split_kernel<2, false>));
		}
		else
		{
			if (cfg.nt) SELLD_LAUNCH((sell_delta_mixed_split_kernel<4, true>));
			else        SELLD_LAUNCH((sell_delta_mixed_split_kernel<4, false>));
		}
	}
	else if (S == 1)
	{
		constexpr int W = sell_delta_waves<T>();
		const XcdMap map1 = sell_delta_tile_map<W>(cfg.map, num_slices);
		grid = xcd_grid(map1);
		if (grid_out)
			*grid_out = grid;
		#define SELLD_LAUNCH1(K) hipLaunchKernelGGL(K, dim3(grid), dim3(W * WAVE), 0, stream, desc, idx, (const T *) val, \
				row_of_sorted, row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, map1)
		if (cfg.nt) SELLD_LAUNCH1((sell_delta_kernel<T, true, V7>));
		else        SELLD_LAUNCH1((sell_delta_kernel<T, false, V7>));
		#undef SELLD_LAUNCH1
	}
	else if (S == 2)
	{
		if (cfg.nt) SELLD_LAUNCH((sell_delta_split_kernel<T, 2, true, V7>));
		else        SELLD_LAUNCH((sell_delta_split_kernel<T, 2, false, V7>));
	}
	else
	{
		if (cfg.nt) SELLD_LAUNCH((sell_delta_split_kernel<T, 4, true, V7>));
		else        SELLD_LAUNCH((sell_delta_split_kernel<T, 4, false, V7>));
	}
	#undef SELLD_LAUNCH
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_sell_delta(bool f32, bool val_f32, int waves_per_slice, bool v7, const int64_t * desc, const unsigned char * idx, const void * val, const int * row_of_sorted,
		const int * row_len, const void * x, void * y, int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	if (val_f32 && v7)
	{
		set_error("sell_delta: 7-byte values are fp64 only");
		return 1;
	}
	if (f32 && !val_f32)
	{
		set_error("sell_delta: fp32 vectors over fp64 values are not served");
		return 1;
	}
	if (val_f32 && !f32)
		return sell_delta_launch<double, false, true>(waves_per_slice, desc, idx, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
	return f32 ? sell_delta_launch<float, false>(waves_per_slice, desc, idx, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out)
	     : v7  ? sell_delta_launch<double, true>(waves_per_slice, desc, idx, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out)
	           : sell_delta_launch<double, false>(waves_per_slice, desc, idx, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
}

template <typename T, int C>
static int
sell_launch_c(const int64_t * slice_ptr, const int * col, const void * val, const int * row_of_sorted, const int * row_len, const void * x, void * y,
		int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	unsigned grid = xcd_grid(cfg.map);
	if (grid_out)
		*grid_out = grid;
	if (grid == 0)
		return 0;
	if (cfg.nt)
		hipLaunchKernelGGL((sell_kernel<T, C, true>), dim3(grid), dim3(SELL_BLOCK), 0, stream, slice_ptr, col, (const T *) val,
				row_of_sorted, row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, cfg.map);
	else
		hipLaunchKernelGGL((sell_kernel<T, C, false>), dim3(grid), dim3(SELL_BLOCK), 0, stream, slice_ptr, col, (const T *) val,
				row_of_sorted, row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, cfg.map);
	HIP_TRY(hipGetLastError());
	return 0;
}

template <typename T>
static int
sell_dispatch(int C, const int64_t * slice_ptr, const int * col, const void * val, const int * row_of_sorted, const int * row_len, const void * x, void * y,
		int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	if (C == SELL_WIDE_C)
	{
		const unsigned grid = xcd_grid(cfg.map);
		if (grid_out)
			*grid_out = grid;
		if (grid == 0)
			return 0;
		if (cfg.nt)
			hipLaunchKernelGGL((sell_wide_kernel<T, true>), dim3(grid), dim3(SELL_WIDE_C), 0, stream, slice_ptr, col, (const T *) val, row_of_sorted,
					row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, cfg.map);
		else
			hipLaunchKernelGGL((sell_wide_kernel<T, false>), dim3(grid), dim3(SELL_WIDE_C), 0, stream, slice_ptr, col, (const T *) val, row_of_sorted,
					row_len, (const T *) x, (T *) y, m, num_slices, cfg.beta, cfg.map);
		HIP_TRY(hipGetLastError());
		return 0;
	}
	switch (C)
	{
		case 16: return sell_launch_c<T, 16>(slice_ptr, col, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
		case 32: return sell_launch_c<T, 32>(slice_ptr, col, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
		case 64: return sell_launch_c<T, 64>(slice_ptr, col, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
	}
	set_error("sell: C must be 16, 32, 64 or 256 (got %d)", C);
	return 1;
}

int
launch_sell(bool f32, int C, const int64_t * slice_ptr, const int * col, const void * val, const int * row_of_sorted,
		const int * row_len, const void * x, void * y, int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out)
{
	return f32 ? sell_dispatch<float>(C, slice_ptr, col, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out)
	           : sell_dispatch<double>(C, slice_ptr, col, val, row_of_sorted, row_len, x, y, m, num_slices, cfg, stream, grid_out);
}

}  // namespace spmv

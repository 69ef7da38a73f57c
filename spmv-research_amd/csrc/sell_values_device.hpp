// Device code shared by the GPU builder of the SELL delta layout (convert_sell.hip) and the in-place value update (update_values.hip):
// one wave per 64-row slice, one lane per row. What decides WHICH slices store 7-byte values and HOW a 7-byte group is packed lives
// here once, so that an updated handle holds the bytes a fresh create() would give.
#pragma once

#include "launch.hpp"

namespace spmv {

__device__ __forceinline__ int
wave_min_i(int v)
{
	for (int o = WAVE / 2; o > 0; o >>= 1)
		v = min(v, __shfl_xor(v, o, WAVE));
	return v;
}

__device__ __forceinline__ int
wave_max_i(int v)
{
	for (int o = WAVE / 2; o > 0; o >>= 1)
		v = max(v, __shfl_xor(v, o, WAVE));
	return v;
}

// the CSR row of lane `lane` of slice `sl`: where it starts and how long it is (0, 0 for the lanes behind the last row)
__device__ __forceinline__ void
sell_lane_row(const int * __restrict__ rp, const int * __restrict__ row_of_sorted, long m, long sl, int lane, int & start, int & len)
{
	start = 0;
	len = 0;
	const long i = sl * WAVE + lane;
	if (i < m)
	{
		const int o = row_of_sorted[i];
		start = rp[o];
		len = rp[o + 1] - start;
	}
}

// 7-byte values (sell_delta_layout.hpp): E0 of a slice of `maxlen` steps whose values in its full groups of 4 steps qualify, 0 when they
// do not or the slice has no full group. Every lane gets the same answer. va = the CSR values (fp64), start / len = the lane's row.
__device__ __forceinline__ int
sell_v7_select(const double * __restrict__ va, int start, int len, int maxlen)
{
	const int full = maxlen / 4;
	SellV7Range r;                                      // padding entries are 0.0: exponent 0, always fit
	for (int k = 0; k < min(len, 4 * full); k++)
		r.add(__double_as_longlong(va[start + k]));
	SellV7Range w;
	w.lo = wave_min_i(r.lo);
	w.hi = wave_max_i(r.hi);
	w.bad = __ballot(r.bad) != 0ull;
	return (full > 0 && w.ok()) ? w.e0() : 0;
}

// a lane's four values of a full group as 7-byte records: its four low dwords, then its four 24-bit high parts packed into three
// dwords; b = the first byte of the compressed group
__device__ __forceinline__ void
sell_v7_store_group(unsigned char * __restrict__ b, int lane, const unsigned long long (&vbits)[4], int e0)
{
	unsigned h[4], w[3];
	#pragma unroll
	for (int u = 0; u < 4; u++)
	{
		reinterpret_cast<unsigned *>(b + sell_v7_lo_pos(u, lane))[0] = (unsigned) vbits[u];
		h[u] = sell_v7_encode_hi(vbits[u], e0);
	}
	sell_v7_pack_hi(h, w);
	unsigned * hp = reinterpret_cast<unsigned *>(b + sell_v7_hi_bit(0, lane) / 8);
	hp[0] = w[0];
	hp[1] = w[1];
	hp[2] = w[2];
}

}  // namespace spmv

// Readers of the LDS-window SELL layout's stored arrays (kernels_sell_window.hip: the layout), shared by the single-vector kernels and
// the multi-vector kernel (kernels_sell_window_spmm.hip) so that both decode the same bytes the same way.
#pragma once

#include "launch.hpp"

namespace spmv {

// index group g of a slice: [64 lanes][4 steps] u16, one 8-byte load per lane
typedef unsigned sellw_uint2 __attribute__((ext_vector_type(2)));

// the 4 values of one lane in one group; vp = the group's first element + (16 / sizeof(T)) * lane
template <typename T, bool NT>
__device__ __forceinline__ void
sellw_values(const T * __restrict__ vp, T (&v)[4])
{
	if constexpr (sizeof(T) == 8)
	{
		typedef T T2 __attribute__((ext_vector_type(2)));
		const T2 w0 = ld_stream<NT>(reinterpret_cast<const T2 *>(vp));
		const T2 w1 = ld_stream<NT>(reinterpret_cast<const T2 *>(vp + 2 * WAVE));
		v[0] = w0.x;
		v[1] = w0.y;
		v[2] = w1.x;
		v[3] = w1.y;
	}
	else
	{
		typedef T T4 __attribute__((ext_vector_type(4)));
		const T4 w = ld_stream<NT>(reinterpret_cast<const T4 *>(vp));
		v[0] = w.x;
		v[1] = w.y;
		v[2] = w.z;
		v[3] = w.w;
	}
}

}  // namespace spmv

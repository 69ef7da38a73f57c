// The row helpers that kernels_trsv.hip (the exact solve) and kernels_trsv_sweeps.hip (Jacobi sweeps) share: the typed view of
// TrsvArrays, the loads of a row's (value, column) pairs and the gathers and fmas of those pairs for KC columns. A row's fma chain
// runs in stored order whichever kernel walks it; that is what makes the sweep solve return the exact solve's bits from `levels`
// sweeps on.
#pragma once

#include <type_traits>

#include "solvers_common.hpp"
#include "trsv.hpp"

namespace spmv {

template <typename T>
struct TrsvTyped {
	const T * val;
	const int * col;
	const int64_t * slice_ptr;
	const int * len;
	const int * perm;
	const T * diag;
	const int * level_ptr;
	const int * level_slice;
	const int * block_level;
};

template <typename T>
static TrsvTyped<T>
typed(const TrsvArrays & a)
{
	return TrsvTyped<T>{(const T *) a.val, a.col, a.slice_ptr, a.len, a.perm, (const T *) a.diag, a.level_ptr, a.level_slice, a.block_level};
}

constexpr int TRSV_UNROLL = 4;

template <typename T, int KC>
constexpr int
trsv_unroll_multi()
{
	return KC * sizeof(T) > 32 ? 2 : TRSV_UNROLL;      // at most 64 bytes (16 VGPRs) of gathered x per entry slot
}

template <typename T, int U>
__device__ __forceinline__ void
trsv_entries_n(const TrsvTyped<T> & a, int64_t base, int lanes, int cnt, int k, T (&av)[U], int (&cv)[U])
{
	#pragma unroll
	for (int j = 0; j < U; j++)
	{
		const int64_t e = base + (int64_t) (k + j < cnt ? k + j : k) * lanes;
		av[j] = a.val[e];
		cv[j] = a.col[e];
	}
}

// xg + col * ldg is the row of x that a stored column names: the block itself (ldg = ldx), or the workgroup's part of it in LDS
// (ldg = KC)
template <typename T, int KC, int U>
__device__ __forceinline__ void
trsv_apply_multi(const T * xg, long ldg, bool vg, int cnt, int k, const T (&av)[U], const int (&cv)[U], T (&s)[KC])
{
	T xv[U][KC];
	#pragma unroll
	for (int j = 0; j < U; j++)
		load_row(xv[j], xg + (long) cv[j] * ldg, vg);
	#pragma unroll
	for (int j = 0; j < U; j++)
		if (k + j < cnt)
		{
			#pragma unroll
			for (int c = 0; c < KC; c++)
				s[c] = fma_t<T>(-av[j], xv[j][c], s[c]);
		}
}

// f(T(), bool_constant<UNIT>, integral_constant<int, KC>) for the handle's precision and diagonal and the chunk's width
template <typename F>
static int
trsv_multi_dispatch(bool f32, bool unit, int kc, F && f)
{
	auto by_kc = [&](auto t, auto u) {
		switch (kc)
		{
		case 8: return f(t, u, std::integral_constant<int, 8>());
		case 4: return f(t, u, std::integral_constant<int, 4>());
		case 2: return f(t, u, std::integral_constant<int, 2>());
		default: return f(t, u, std::integral_constant<int, 1>());
		}
	};
	if (f32)
		return unit ? by_kc(float(), std::true_type()) : by_kc(float(), std::false_type());
	return unit ? by_kc(double(), std::true_type()) : by_kc(double(), std::false_type());
}

}  // namespace spmv

// The folded tail of the AMG cycle (include/spmv_mi355x.h "AMG: the small levels as one launch"): everything of the V cycle from the
// first folded level down to the last and back up is ONE launch of ONE workgroup of AMG_FOLD_TB lanes per chunk of columns. The
// operators are the fold's own int32 CSR copies of A_l, P_l and R_l (values in the handle's precision), the vectors are the
// hierarchy's level vectors in global memory, ordered by __syncthreads(). No atomics, no flags, nothing spins; every barrier sits
// outside the row loops, whose trip counts are uniform, so all lanes meet every barrier whatever the level's size.
// THE ARITHMETIC is the header's, as written: this file is compiled with contraction off, the only fused operations are the fma()
// calls. A row's product starts from +0 and takes one fma per entry in stored order; on a level with G lanes per row (amg_fold_lanes)
// lane g of the row's group takes the entries g, g + G, ... of the row and the G partial sums are added by the halving tree
// s_g = s_g + s_{g + h}, h = G/2, ..., 1. tests/amg_fold_reference.c states the same as sequential loops.

#include "amg.hpp"
#include "solvers_common.hpp"

#pragma clang fp contract(off)

namespace spmv {

template <typename T, int KC>
__device__ __forceinline__ bool
fold_row_vec(const T * p, long ld, int c0)
{
	return ld % KC == 0 && c0 % KC == 0 && (size_t) p % (KC * sizeof(T)) == 0;
}

__device__ __forceinline__ float
fold_fma(float a, float b, float c)
{
	return __builtin_fmaf(a, b, c);
}

__device__ __forceinline__ double
fold_fma(double a, double b, double c)
{
	return __builtin_fma(a, b, c);
}

// a block of KC columns c0.. of a row-major vector block: row i at p + i * ld
template <typename T>
struct FoldVec {
	T * p;
	long ld;
};

// s = (row i of the CSR) * x for the KC columns, G = 1 << lg lanes per row; done(i, s) runs in the first lane of the row's group.
// The trip count of the outer loop is the same in every lane.
template <typename T, int KC, typename E>
__device__ __forceinline__ void
fold_product(const int * rp, const int * ci, const T * va, int n, int lg, FoldVec<T> x, int c0, E && done)
{
	const int G = 1 << lg, tid = threadIdx.x, g = tid & (G - 1);
	const int tasks = n << lg;
	const bool vx = fold_row_vec<T, KC>(x.p, x.ld, c0);
	for (int base = 0; base < tasks; base += AMG_FOLD_TB)
	{
		const int task = base + tid;
		const int i = task >> lg;
		T s[KC];
		#pragma unroll
		for (int c = 0; c < KC; c++)
			s[c] = 0;
		if (task < tasks)
		{
			const int end = rp[i + 1];
			for (int e = rp[i] + g; e < end; e += G)
			{
				const T a = va[e];
				T xv[KC];
				load_row<T, KC>(xv, x.p + (long) ci[e] * x.ld + c0, vx);
				#pragma unroll
				for (int c = 0; c < KC; c++)
					s[c] = fold_fma(a, xv[c], s[c]);
			}
		}
		for (int h = G >> 1; h >= 1; h >>= 1)
		{
			#pragma unroll
			for (int c = 0; c < KC; c++)
				s[c] = s[c] + __shfl_down(s[c], h);
		}
		if (task < tasks && g == 0)
			done(i, s);
	}
}

// x = x + w o (b - t) for rows 0 .. n-1
template <typename T, int KC>
__device__ __forceinline__ void
fold_sweep(const T * w, FoldVec<T> b, FoldVec<T> t, FoldVec<T> x, int n, int c0)
{
	const bool vb = fold_row_vec<T, KC>(b.p, b.ld, c0), vt = fold_row_vec<T, KC>(t.p, t.ld, c0), vx = fold_row_vec<T, KC>(x.p, x.ld, c0);
	for (int i = threadIdx.x; i < n; i += AMG_FOLD_TB)
	{
		const T wi = w[i];
		T bv[KC], tv[KC], xv[KC];
		load_row<T, KC>(bv, b.p + (long) i * b.ld + c0, vb);
		load_row<T, KC>(tv, t.p + (long) i * t.ld + c0, vt);
		load_row<T, KC>(xv, x.p + (long) i * x.ld + c0, vx);
		#pragma unroll
		for (int c = 0; c < KC; c++)
			xv[c] = xv[c] + wi * (bv[c] - tv[c]);
		store_row<T, KC>(x.p + (long) i * x.ld + c0, xv, vx);
	}
}

template <typename T, int KC>
__global__ __launch_bounds__(AMG_FOLD_TB) void
amg_fold_tail_kernel(const AmgFoldLevel * __restrict__ lv, int first, int last, const T * in, long ldin, T * out, long ldout, long ld, int c0,
		int nu, int cs, const double * __restrict__ Lg)
{
	__shared__ double Ls[AMG_DENSE_MAX * (AMG_DENSE_MAX + 1) / 2];
	__shared__ double piv[AMG_DENSE_MAX][KC];
	const int tid = threadIdx.x;
	const bool dense = Lg != nullptr;
	if (dense)
	{
		const int nd = lv[last].n;
		for (int e = tid; e < nd * (nd + 1) / 2; e += AMG_FOLD_TB)
			Ls[e] = Lg[e];
	}
	auto rhs = [&](const AmgFoldLevel & L, int l) { return l == first ? FoldVec<T>{const_cast<T *>(in), ldin} : FoldVec<T>{(T *) L.b, ld}; };
	auto sol = [&](const AmgFoldLevel & L, int l) { return l == first ? FoldVec<T>{out, ldout} : FoldVec<T>{(T *) L.x, ld}; };
	// t = A x, a barrier, x = x + w o (b - t), a barrier
	auto sweep = [&](const AmgFoldLevel & L, FoldVec<T> b, FoldVec<T> t, FoldVec<T> x) {
		const bool vt = fold_row_vec<T, KC>(t.p, t.ld, c0);
		fold_product<T, KC>(L.a_rp, L.a_ci, (const T *) L.a_va, L.n, L.lg, x, c0, [&](int i, const T (&s)[KC]) {
			store_row<T, KC>(t.p + (long) i * t.ld + c0, s, vt);
		});
		__syncthreads();
		fold_sweep<T, KC>((const T *) L.w, b, t, x, L.n, c0);
		__syncthreads();
	};
	// x = w o b on the first folded level: below it the restriction's lanes write it
	{
		const AmgFoldLevel L = lv[first];
		if (first < last || !dense)
		{
			const FoldVec<T> b = rhs(L, first), x = sol(L, first);
			const bool vb = fold_row_vec<T, KC>(b.p, b.ld, c0), vx = fold_row_vec<T, KC>(x.p, x.ld, c0);
			const T * w = (const T *) L.w;
			for (int i = tid; i < L.n; i += AMG_FOLD_TB)
			{
				const T wi = w[i];
				T bv[KC], xv[KC];
				load_row<T, KC>(bv, b.p + (long) i * b.ld + c0, vb);
				#pragma unroll
				for (int c = 0; c < KC; c++)
					xv[c] = wi * bv[c];
				store_row<T, KC>(x.p + (long) i * x.ld + c0, xv, vx);
			}
		}
		__syncthreads();
	}
	for (int l = first; l < last; l++)
	{
		const AmgFoldLevel L = lv[l], C = lv[l + 1];
		const FoldVec<T> b = rhs(L, l), x = sol(L, l), t = {(T *) L.t, ld};
		for (int s = 1; s < nu; s++)
			sweep(L, b, t, x);
		// t = b - A x
		{
			const bool vb = fold_row_vec<T, KC>(b.p, b.ld, c0), vt = fold_row_vec<T, KC>(t.p, t.ld, c0);
			fold_product<T, KC>(L.a_rp, L.a_ci, (const T *) L.a_va, L.n, L.lg, x, c0, [&](int i, const T (&s)[KC]) {
				T bv[KC], tv[KC];
				load_row<T, KC>(bv, b.p + (long) i * b.ld + c0, vb);
				#pragma unroll
				for (int c = 0; c < KC; c++)
					tv[c] = bv[c] - s[c];
				store_row<T, KC>(t.p + (long) i * t.ld + c0, tv, vt);
			});
		}
		__syncthreads();
		// b_{l+1} = R t and x_{l+1} = w_{l+1} o b_{l+1}
		{
			T * cb = (T *) C.b, * cx = (T *) C.x;
			const T * cw = (const T *) C.w;
			const bool vcb = fold_row_vec<T, KC>(cb, ld, c0), vcx = fold_row_vec<T, KC>(cx, ld, c0);
			fold_product<T, KC>(L.r_rp, L.r_ci, (const T *) L.r_va, C.n, 0, t, c0, [&](int i, const T (&s)[KC]) {
				const T wi = cw[i];
				T xv[KC];
				#pragma unroll
				for (int c = 0; c < KC; c++)
					xv[c] = wi * s[c];
				store_row<T, KC>(cb + (long) i * ld + c0, s, vcb);
				store_row<T, KC>(cx + (long) i * ld + c0, xv, vcx);
			});
		}
		__syncthreads();
	}
	{
		const AmgFoldLevel L = lv[last];
		const FoldVec<T> b = rhs(L, last), x = sol(L, last), t = {(T *) L.t, ld};
		if (dense)
		{
			// amg_dense_solve_multi_kernel's loops: lane a keeps y_a of every column, one barrier per column of L in each direction
			const int n = L.n, a = tid, row = a * (a + 1) / 2;
			double y[KC];
			#pragma unroll
			for (int c = 0; c < KC; c++)
				y[c] = a < n ? (double) b.p[(long) a * b.ld + c0 + c] : 0.0;
			__syncthreads();
			for (int k = 0; k < n; k++)
			{
				if (a == k)
				{
					const double d = Ls[row + k];
					#pragma unroll
					for (int c = 0; c < KC; c++)
						piv[k][c] = y[c] / d;
				}
				__syncthreads();
				if (a > k && a < n)
				{
					const double m = Ls[row + k];
					#pragma unroll
					for (int c = 0; c < KC; c++)
						y[c] = __builtin_fma(-m, piv[k][c], y[c]);
				}
			}
			#pragma unroll
			for (int c = 0; c < KC; c++)
				y[c] = a < n ? piv[a][c] : 0.0;
			__syncthreads();
			for (int k = n - 1; k >= 0; k--)
			{
				if (a == k)
				{
					const double d = Ls[row + k];
					#pragma unroll
					for (int c = 0; c < KC; c++)
						piv[k][c] = y[c] / d;
				}
				__syncthreads();
				if (a < k)
				{
					const double m = Ls[k * (k + 1) / 2 + a];
					#pragma unroll
					for (int c = 0; c < KC; c++)
						y[c] = __builtin_fma(-m, piv[k][c], y[c]);
				}
			}
			if (a < n)
			{
				#pragma unroll
				for (int c = 0; c < KC; c++)
					x.p[(long) a * x.ld + c0 + c] = (T) piv[a][c];
			}
			__syncthreads();
		}
		else
			for (int s = 1; s < cs; s++)
				sweep(L, b, t, x);
	}
	for (int l = last - 1; l >= first; l--)
	{
		const AmgFoldLevel L = lv[l], C = lv[l + 1];
		const FoldVec<T> b = rhs(L, l), x = sol(L, l), t = {(T *) L.t, ld}, cx = {(T *) C.x, ld};
		// x = x + P x_{l+1}
		{
			const bool vx = fold_row_vec<T, KC>(x.p, x.ld, c0);
			fold_product<T, KC>(L.p_rp, L.p_ci, (const T *) L.p_va, L.n, 0, cx, c0, [&](int i, const T (&s)[KC]) {
				T xv[KC];
				load_row<T, KC>(xv, x.p + (long) i * x.ld + c0, vx);
				#pragma unroll
				for (int c = 0; c < KC; c++)
					xv[c] = xv[c] + s[c];
				store_row<T, KC>(x.p + (long) i * x.ld + c0, xv, vx);
			});
		}
		__syncthreads();
		for (int s = 0; s < nu; s++)
			sweep(L, b, t, x);
	}
}

int
launch_amg_fold_tail(bool f32, int k, const AmgFoldLevel * lv, int first, int last, const void * in, long ldin, void * out, long ldout, long ld,
		int nu, int cs, const double * factor, hipStream_t st)
{
	for_chunks(column_chunks(k), [&](int c0, auto kc) {
		constexpr int KC = decltype(kc)::value;
		if (f32)
			hipLaunchKernelGGL((amg_fold_tail_kernel<float, KC>), dim3(1), dim3(AMG_FOLD_TB), 0, st, lv, first, last, (const float *) in, ldin,
					(float *) out, ldout, ld, c0, nu, cs, factor);
		else
			hipLaunchKernelGGL((amg_fold_tail_kernel<double, KC>), dim3(1), dim3(AMG_FOLD_TB), 0, st, lv, first, last, (const double *) in, ldin,
					(double *) out, ldout, ld, c0, nu, cs, factor);
		return 0;
	});
	HIP_TRY(hipGetLastError());
	return 0;
}

__global__ __launch_bounds__(AMG_TB) void
amg_fold_narrow_kernel(const double * __restrict__ src, float * __restrict__ dst, long n)
{
	for (long i = (long) blockIdx.x * AMG_TB + threadIdx.x; i < n; i += (long) gridDim.x * AMG_TB)
		dst[i] = (float) src[i];
}

int
launch_amg_fold_values(bool f32, const double * src, void * dst, long count, hipStream_t st)
{
	if (count > 0)
	{
		if (f32)
			hipLaunchKernelGGL(amg_fold_narrow_kernel, dim3(amg_grid(count)), dim3(AMG_TB), 0, st, src, (float *) dst, count);
		else
			HIP_TRY(hipMemcpyAsync(dst, src, (size_t) count * 8, hipMemcpyDeviceToDevice, st));
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

}  // namespace spmv

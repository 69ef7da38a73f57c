// The row kernel of the factorized sparse approximate inverse (include/spmv_mi355x.h "FSAI", fsai.hpp for the mapping): row i of G
// from the dense SPD system A(J, J) of the row's pattern columns J, everything fp64, every element's chain of operations the one the
// header pins, so the bits do not depend on which lane takes which element.
//
// A row's phases, each closed by a workgroup barrier:
//   1. J and a zeroed packed triangle S (S[a][b] at a (a + 1) / 2 + b, b <= a) into LDS;
//   2. the gather: lane a walks row J[a] of A and drops every entry with column <= J[a] that J holds (binary search) into S[a][.];
//   3. per column k: (a) lane a >= k runs S[a][k] = fma(-C[a][p], C[k][p], S[a][k]) over p < k; (b) every lane reads the pivot
//      S[k][k], lane a > k divides its S[a][k] by sqrt(pivot) in place, the row's first lane keeps sqrt(pivot) in D[k];
//   4. the back substitution of C^t g = e_s by the row's first lane: its chain is sequential by definition (g_k starts from g_k+1);
//   5. g (or the breakdown rule's row) to global memory, one lane per entry.
// Nothing is written outside the row's own entries of g and its own word of fell_back.

#include "fsai.hpp"

namespace spmv {

template <int SMAX, int LANES, int ROWS>
__global__ __launch_bounds__(LANES * ROWS) void
fsai_rows_kernel(FsaiArrays A, const int * __restrict__ bin_rows, long count)
{
	constexpr int TRI = SMAX * (SMAX + 1) / 2;
	__shared__ double S[ROWS][TRI];
	__shared__ double D[ROWS][SMAX];          // the pivots' square roots, C[k][k]
	__shared__ double Gv[ROWS][SMAX];
	__shared__ int J[ROWS][SMAX];
	__shared__ int width[ROWS];

	const int grp = threadIdx.x / LANES, lane = threadIdx.x % LANES;
	double * Sr = S[grp], * Dr = D[grp], * gr = Gv[grp];
	int * Jr = J[grp];

	// the trip count is the same in every thread of the workgroup: the loop holds barriers
	for (long base = (long) blockIdx.x * ROWS; base < count; base += (long) gridDim.x * ROWS)
	{
		const long slot = base + grp;
		const bool live = slot < count;
		const int i = live ? bin_rows[slot] : 0;
		const long p0 = live ? A.p_rp[i] : 0;
		const int s = live ? min((int) (A.p_rp[i + 1] - p0), SMAX) : 0;     // the host has binned on s: the min never bites
		// 1.
		for (int t = lane; t < s; t += LANES)
			Jr[t] = A.p_ci[p0 + t];
		for (int t = lane; t < s * (s + 1) / 2; t += LANES)
			Sr[t] = 0;
		if (lane == 0)
			width[grp] = s;
		__syncthreads();
		int smax = 0;
		for (int r = 0; r < ROWS; r++)
			smax = max(smax, width[r]);
		// 2.
		for (int a = lane; a < s; a += LANES)
		{
			const int ja = Jr[a];
			const long e1 = A.a_rp[ja + 1];
			for (long e = A.a_rp[ja]; e < e1; e++)
			{
				const int c = A.a_ci[e];
				if (c > ja)
					continue;
				int lo = 0, hi = a;                   // J ascending: c <= J[a], so its place is in [0, a]
				while (lo < hi)
				{
					const int mid = (lo + hi) >> 1;
					if (Jr[mid] < c)
						lo = mid + 1;
					else
						hi = mid;
				}
				if (Jr[lo] == c)
					Sr[a * (a + 1) / 2 + lo] = A.a_va[e];
			}
		}
		__syncthreads();
		const double aii = s > 0 ? Sr[s * (s + 1) / 2 - 1] : 1.0;
		bool bad = false;
		// 3.
		for (int k = 0; k < smax; k++)
		{
			const int kk = k * (k + 1) / 2;
			for (int a = k + lane; a < s; a += LANES)
			{
				const int aa = a * (a + 1) / 2;
				double acc = Sr[aa + k];
				for (int p = 0; p < k; p++)
					acc = fma(-Sr[aa + p], Sr[kk + p], acc);
				Sr[aa + k] = acc;
			}
			__syncthreads();
			if (k < s)
			{
				const double pivot = Sr[kk + k];
				bad = bad || !(pivot > 0 && pivot < INFINITY);
				const double d = sqrt(pivot);
				for (int a = k + 1 + lane; a < s; a += LANES)
					Sr[a * (a + 1) / 2 + k] = Sr[a * (a + 1) / 2 + k] / d;
				if (lane == 0)
					Dr[k] = d;
			}
			__syncthreads();
		}
		// 4.
		if (lane == 0 && s > 0 && !bad)
		{
			gr[s - 1] = 1.0 / Dr[s - 1];
			for (int k = s - 2; k >= 0; k--)
			{
				double t = 0;
				for (int a = k + 1; a < s; a++)
					t = fma(Sr[a * (a + 1) / 2 + k], gr[a], t);
				gr[k] = -t / Dr[k];
			}
		}
		__syncthreads();
		// 5.
		for (int t = lane; t < s; t += LANES)
			A.g[p0 + t] = bad ? (t == s - 1 ? 1.0 / sqrt(aii) : 0.0) : gr[t];
		if (lane == 0 && live)
			A.fell_back[i] = bad;
		__syncthreads();                              // the next trip overwrites the row's LDS
	}
}

template <int BIN>
static int
launch_bin(const FsaiArrays & a, const int * bin_rows, long count, hipStream_t st)
{
	constexpr int SMAX = FSAI_BIN_SMAX[BIN], LANES = FSAI_BIN_LANES[BIN], ROWS = FSAI_BIN_ROWS[BIN];
	const long groups = (count + ROWS - 1) / ROWS;
	const dim3 grid((unsigned) std::min<long>(groups, FSAI_MAX_GRID)), block(LANES * ROWS);
	hipLaunchKernelGGL((fsai_rows_kernel<SMAX, LANES, ROWS>), grid, block, 0, st, a, bin_rows, count);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
launch_fsai_rows(int bin, const FsaiArrays & a, const int * bin_rows, long count, hipStream_t st)
{
	if (count <= 0)
		return 0;
	switch (bin)
	{
		case 0: return launch_bin<0>(a, bin_rows, count, st);
		case 1: return launch_bin<1>(a, bin_rows, count, st);
		case 2: return launch_bin<2>(a, bin_rows, count, st);
		default: return launch_bin<3>(a, bin_rows, count, st);
	}
}

}  // namespace spmv

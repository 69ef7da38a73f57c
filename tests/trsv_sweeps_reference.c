/* The sequential restatement of the Jacobi-sweep triangular solve (include/spmv_mi355x.h "JACOBI SWEEPS"), the reference the GPU
 * sweeps are held to bit for bit. Compiled by tests/trsv_sweeps_cases.py with gcc -O2 -ffp-contract=off: the only fused operations
 * are the explicit fma / fmaf below. With T = D + N:  x(1) = D^-1 b,  x(m + 1) = D^-1 (b - N x(m)),  x = x(sweeps), sweeps >= 1.
 *   uplo 0 = LOWER (entries with column < row are N), 1 = UPPER (column > row)
 *   unit 0 = divide by the first stored entry with column i, 1 = d_i = 1; entries with column i are ignored as in trsv_reference.c
 * The first sweep reads no entry of N (an Inf or NaN there does not reach x(1)); b is read in every sweep and never modified.
 * va, b and x are in the precision of the function; w is scratch of n values; b may not be x or w. */
#include <math.h>
#include <stdint.h>

#define TRSV_SWEEPS_REFERENCE(NAME, T, FMA)                                                                        \
	void NAME(int uplo, int unit, long n, const int32_t * rp, const int32_t * ci, const T * va, long sweeps,   \
			const T * b, T * x, T * w)                                                                 \
	{                                                                                                          \
		/* sweep m writes x when sweeps - m is even: the last one writes x */                              \
		const T * prev = 0;                                                                                \
		for (long m = 1; m <= sweeps; m++)                                                                 \
		{                                                                                                  \
			T * next = (sweeps - m) % 2 == 0 ? x : w;                                                  \
			for (long i = 0; i < n; i++)                                                               \
			{                                                                                          \
				T s = b[i];                                                                        \
				T d = 0;                                                                           \
				int have = 0;                                                                      \
				for (long j = rp[i]; j < rp[i + 1]; j++)                                           \
				{                                                                                  \
					const long c = ci[j];                                                      \
					if (c == i)                                                                \
					{                                                                          \
						if (!have)                                                         \
							d = va[j];                                                 \
						have = 1;                                                          \
					}                                                                          \
					else if (m > 1 && (uplo ? c > i : c < i))                                  \
						s = FMA(-va[j], prev[c], s);                                       \
				}                                                                                  \
				next[i] = unit ? s : s / d;                                                        \
			}                                                                                          \
			prev = next;                                                                               \
		}                                                                                                  \
	}

TRSV_SWEEPS_REFERENCE(trsv_sweeps_reference_f64, double, fma)
TRSV_SWEEPS_REFERENCE(trsv_sweeps_reference_f32, float, fmaf)

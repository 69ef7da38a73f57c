/* The sequential loop of the sparse triangular solve (include/spmv_mi355x.h "sparse triangular solve"), the reference every plan of
 * the GPU solve is held to bit for bit. Compiled by tests/trsv_cases.py with gcc -O2 -ffp-contract=off: the only fused operations
 * are the explicit fma / fmaf below.
 *   uplo 0 = LOWER (entries with column <= row, rows ascending), 1 = UPPER (column >= row, rows descending)
 *   unit 0 = divide by the first stored entry with column i, 1 = d_i = 1 and every entry with column i ignored
 * va, b and x are in the precision of the function; b may be x. */
#include <math.h>
#include <stdint.h>

#define TRSV_REFERENCE(NAME, T, FMA)                                                                               \
	void NAME(int uplo, int unit, long n, const int32_t * rp, const int32_t * ci, const T * va, const T * b, T * x) \
	{                                                                                                          \
		for (long t = 0; t < n; t++)                                                                       \
		{                                                                                                  \
			const long i = uplo ? n - 1 - t : t;                                                       \
			T s = b[i];                                                                                \
			T d = 0;                                                                                   \
			int have = 0;                                                                              \
			for (long j = rp[i]; j < rp[i + 1]; j++)                                                   \
			{                                                                                          \
				const long c = ci[j];                                                              \
				if (c == i)                                                                        \
				{                                                                                  \
					if (!have)                                                                 \
						d = va[j];                                                         \
					have = 1;                                                                  \
				}                                                                                  \
				else if (uplo ? c > i : c < i)                                                     \
					s = FMA(-va[j], x[c], s);                                                  \
			}                                                                                          \
			x[i] = unit ? s : s / d;                                                                   \
		}                                                                                                  \
	}

TRSV_REFERENCE(trsv_reference_f64, double, fma)
TRSV_REFERENCE(trsv_reference_f32, float, fmaf)

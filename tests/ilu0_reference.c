/* The sequential loop of ILU(0) (include/spmv_mi355x.h "ILU(0)"), the reference every plan of the GPU factorization is held to bit
 * for bit. Compiled by tests/ilu0_cases.py with gcc -O2 -ffp-contract=off: the only fused operation is the explicit fma below.
 *   input   a square n x n int32 CSR, columns strictly ascending in every row, a stored diagonal in every row, fp64 values
 *   B       0 = the global factorization; B > 0 = the blocked form: an off-diagonal entry (i, j) takes part only when
 *           j / B == i / B, every other entry keeps A's value in f
 *   f       out: nnz values in A's entry order, unit L strictly below the diagonal, U on and above it
 *   returns the lowest row whose pivot is zero or not finite once the row is finished, -1 when there is none
 * Column j of row i is found through a dense map from columns to positions, not by searching the row. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

long
ilu0_reference(long n, const int32_t * rp, const int32_t * ci, const double * va, long B, double * f)
{
	long * pos = malloc((n > 0 ? n : 1) * sizeof(long));
	long * diag = malloc((n > 0 ? n : 1) * sizeof(long));
	long bad = -1;
	for (long e = 0; e < (n > 0 ? rp[n] : 0); e++)
		f[e] = va[e];
	for (long j = 0; j < n; j++)
		pos[j] = -1;
	for (long i = 0; i < n; i++)
	{
		for (long p = rp[i]; p < rp[i + 1]; p++)
			if (B == 0 || ci[p] / B == i / B)
				pos[ci[p]] = p;
		diag[i] = pos[i];
		for (long p = rp[i]; p < rp[i + 1]; p++)
		{
			const long k = ci[p];
			if (k >= i || pos[k] != p)
				continue;
			f[p] = f[p] / f[diag[k]];
			for (long q = diag[k] + 1; q < rp[k + 1]; q++)
			{
				if (B != 0 && ci[q] / B != k / B)
					continue;
				const long r = pos[ci[q]];
				if (r >= 0)
					f[r] = fma(-f[p], f[q], f[r]);
			}
		}
		if (bad < 0 && (f[diag[i]] == 0 || !isfinite(f[diag[i]])))
			bad = i;
		for (long p = rp[i]; p < rp[i + 1]; p++)
			pos[ci[p]] = -1;
	}
	free(pos);
	free(diag);
	return bad;
}

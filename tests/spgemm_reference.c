/* The sequential reference of C = A B (include/spmv_mi355x.h "SpGEMM"): the header's loop and nothing clever. A dense accumulator
 * per row; acc = +0.0, then for the entries p of row i of A in stored order, for every entry q of B's row col(p),
 * acc[col(q)] = fma(a_p, b_q, acc[col(q)]); the touched columns sorted ascending. Built with gcc -O2 -ffp-contract=off -lm
 * (tests/spgemm_cases.py), so that fma() is the only fused operation.
 *
 * Two calls: with c_col_idx == NULL it writes c_row_ptr (m + 1) and returns nnz(C); with the arrays of that size it writes the
 * columns and the values (a_values / b_values may be NULL with c_values: the pattern alone). Returns -1 when out of memory. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

static int
cmp_int32(const void * a, const void * b)
{
	const int32_t x = *(const int32_t *) a, y = *(const int32_t *) b;
	return (x > y) - (x < y);
}

long
spgemm_reference(long m, long k, long n, const int32_t * a_rp, const int32_t * a_ci, const double * a_va, const int32_t * b_rp,
		const int32_t * b_ci, const double * b_va, int32_t * c_rp, int32_t * c_ci, double * c_va)
{
	double * acc = malloc((size_t) (n > 0 ? n : 1) * sizeof(double));
	int32_t * mark = malloc((size_t) (n > 0 ? n : 1) * sizeof(int32_t));
	int32_t * touched = malloc((size_t) (n > 0 ? n : 1) * sizeof(int32_t));
	long nnz = 0;
	(void) k;
	if (!acc || !mark || !touched)
	{
		free(acc);
		free(mark);
		free(touched);
		return -1;
	}
	for (long j = 0; j < n; j++)
		mark[j] = -1;
	c_rp[0] = 0;
	for (long i = 0; i < m; i++)
	{
		long count = 0;
		for (long p = a_rp[i]; p < a_rp[i + 1]; p++)
		{
			const long l = a_ci[p];
			for (long q = b_rp[l]; q < b_rp[l + 1]; q++)
			{
				const int32_t j = b_ci[q];
				if (mark[j] != i)
				{
					mark[j] = (int32_t) i;
					acc[j] = 0.0;
					touched[count++] = j;
				}
				if (c_va)
					acc[j] = fma(a_va[p], b_va[q], acc[j]);
			}
		}
		if (c_ci)
		{
			qsort(touched, (size_t) count, sizeof(int32_t), cmp_int32);
			for (long t = 0; t < count; t++)
			{
				c_ci[nnz + t] = touched[t];
				if (c_va)
					c_va[nnz + t] = acc[touched[t]];
			}
		}
		nnz += count;
		c_rp[i + 1] = (int32_t) nnz;
	}
	free(acc);
	free(mark);
	free(touched);
	return nnz;
}

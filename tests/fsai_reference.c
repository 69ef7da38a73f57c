/* The sequential restatement of the FSAI row arithmetic of include/spmv_mi355x.h ("FSAI"): one row after the other, one element
 * after the other, explicit fma / sqrt / division in fp64. Compiled by tests/fsai_cases.py with gcc -ffp-contract=off, so nothing is
 * fused or reordered that is not written as fma here. Returns the rows that took the breakdown rule, or -1 for a row wider than
 * MAX_ROW or out of memory. Nothing here is the engine's code. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>

#define MAX_ROW 128

/* A(r, c) for c <= r: the first stored entry of row r with column c, 0 when there is none */
static double
entry(const int32_t * rp, const int32_t * ci, const double * va, long r, long c)
{
	for (long e = rp[r]; e < rp[r + 1]; e++)
		if (ci[e] == c)
			return va[e];
	return 0.0;
}

long
fsai_reference(long n, const int32_t * rp, const int32_t * ci, const double * va, const int32_t * prp, const int32_t * pci, double * g_out)
{
	double * S = malloc(sizeof(double) * MAX_ROW * MAX_ROW);
	double * C = malloc(sizeof(double) * MAX_ROW * MAX_ROW);
	double g[MAX_ROW];
	long fell_back = 0;
	if (!S || !C)
		return -1;
	for (long i = 0; i < n; i++)
	{
		const int32_t * J = pci + prp[i];
		const long s = prp[i + 1] - prp[i];
		int bad = 0;
		if (s > MAX_ROW)
		{
			free(S);
			free(C);
			return -1;
		}
		for (long a = 0; a < s; a++)
			for (long b = 0; b <= a; b++)
				S[a * MAX_ROW + b] = entry(rp, ci, va, J[a], J[b]);
		for (long k = 0; k < s && !bad; k++)
		{
			for (long a = k; a < s; a++)
				for (long p = 0; p < k; p++)
					S[a * MAX_ROW + k] = fma(-C[a * MAX_ROW + p], C[k * MAX_ROW + p], S[a * MAX_ROW + k]);
			const double pivot = S[k * MAX_ROW + k];
			if (!(pivot > 0) || !(pivot < INFINITY))
			{
				bad = 1;
				break;
			}
			C[k * MAX_ROW + k] = sqrt(pivot);
			for (long a = k + 1; a < s; a++)
				C[a * MAX_ROW + k] = S[a * MAX_ROW + k] / C[k * MAX_ROW + k];
		}
		if (bad)
		{
			fell_back++;
			for (long k = 0; k < s; k++)
				g_out[prp[i] + k] = 0.0;
			g_out[prp[i] + s - 1] = 1.0 / sqrt(entry(rp, ci, va, i, i));
			continue;
		}
		g[s - 1] = 1.0 / C[(s - 1) * MAX_ROW + s - 1];
		for (long k = s - 2; k >= 0; k--)
		{
			double t = 0.0;
			for (long a = k + 1; a < s; a++)
				t = fma(C[a * MAX_ROW + k], g[a], t);
			g[k] = -t / C[k * MAX_ROW + k];
		}
		for (long k = 0; k < s; k++)
			g_out[prp[i] + k] = g[k];
	}
	free(S);
	free(C);
	return fell_back;
}

/* The FROZEN hierarchy of include/spmv_mi355x.h "AMG: new values for a hierarchy" as sequential loops: the aggregates of every
 * coarsened level are given, the values of level 0 are new, and steps 1, 5 and 6 run exactly as amg_reference_build runs them (its
 * multiply and transpose, the same expressions for rho, omega and P). Steps 2 to 4 and the stopping rules are not run: the number of
 * levels is the caller's. Compiled like amg_reference.c: gcc -O2 -ffp-contract=off (tests/amg_update_cases.py). The result is a
 * `hierarchy` that amg_reference_level / _csr / _aggregates / _free read. */
#include "amg_reference.c"

/* levels >= 1 (n > 0); agg = the aggregates of levels 0 .. levels - 2 one after the other, aggregates[l] = their number on level l */
void *
amg_update_reference_build(long n, const int * rp, const int * ci, const double * va, int levels, const int * agg, const long * aggregates)
{
	hierarchy * H = calloc(1, sizeof(hierarchy));
	if (n == 0 || levels < 1)
		return H;
	H->lev[0].A = csr_alloc(n, n, rp[n]);
	memcpy(H->lev[0].A.rp, rp, (size_t) (n + 1) * sizeof(int));
	memcpy(H->lev[0].A.ci, ci, (size_t) rp[n] * sizeof(int));
	memcpy(H->lev[0].A.va, va, (size_t) rp[n] * sizeof(double));
	for (int l = 0; l < levels; l++)
	{
		level * L = &H->lev[l];
		const csr * A = &L->A;
		const long nl = A->n;
		double * d = malloc((size_t) (nl ? nl : 1) * sizeof(double));
		H->levels = l + 1;
		L->rho = 0;
		for (long i = 0; i < nl; i++)
		{
			double sum = 0;
			int found = 0;
			d[i] = 0;
			for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			{
				if (!found && A->ci[e] == i)
				{
					d[i] = A->va[e];
					found = 1;
				}
				sum = sum + fabs(A->va[e]);
			}
			L->rho = fmax(L->rho, sum / d[i]);
		}
		L->omega = 4.0 / (3.0 * L->rho);
		if (l + 1 == levels)
		{
			free(d);
			break;
		}
		L->agg = malloc((size_t) nl * sizeof(int));
		memcpy(L->agg, agg, (size_t) nl * sizeof(int));
		agg += nl;
		L->aggregates = aggregates[l];
		L->rounds = 1;                                    /* "coarsened", for the readers; the rounds are create's */
		csr T = csr_alloc(nl, L->aggregates, nl);
		for (long i = 0; i < nl; i++)
		{
			T.rp[i + 1] = (int) (i + 1);
			T.ci[i] = L->agg[i];
			T.va[i] = 1.0;
		}
		L->P = multiply(A, &T);
		for (long i = 0; i < nl; i++)
			for (long e = L->P.rp[i]; e < L->P.rp[i + 1]; e++)
				L->P.va[e] = (L->P.ci[e] == L->agg[i] ? 1.0 : 0.0) - (L->omega / d[i]) * L->P.va[e];
		csr R = transpose(&L->P), AP = multiply(A, &L->P);
		H->lev[l + 1].A = multiply(&R, &AP);
		csr_free(&T);
		csr_free(&R);
		csr_free(&AP);
		free(d);
	}
	return H;
}

/* the smallest diagonal of level l, so that a caller can look for values whose coarse diagonal is not positive */
double
amg_update_reference_min_diagonal(const void * h, int l)
{
	const csr * A = &((const hierarchy *) h)->lev[l].A;
	double least = INFINITY;
	for (long i = 0; i < A->n; i++)
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			if (A->ci[e] == i)
			{
				least = fmin(least, A->va[e]);
				break;
			}
	return least;
}

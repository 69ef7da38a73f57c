/* The hierarchy of include/spmv_mi355x.h "AMG" as sequential loops: steps 1 to 6, the stopping rules, the dense packed Cholesky factor
 * of the last level and its column-by-column solve. Compiled with gcc -O2 -ffp-contract=off (tests/amg_cases.py), so that every
 * product and sum is rounded on its own and the only fused operations are the fma() calls the header writes down. The products
 * restate tests/spgemm_reference.c (acc = +0.0, then one fma per product in the stored order of the left factor's row, columns
 * ascending in the result); the transposition is the stable counting sort by column of csrc/transpose_csr.hip. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAX_LEVELS 17

typedef struct {
	long n, m, nnz;               /* n rows, m columns */
	int * rp, * ci;
	double * va;
} csr;

typedef struct {
	csr A, P;
	int * agg;
	long aggregates, rounds;
	double omega, rho;
} level;

typedef struct {
	int levels, stalled;
	level lev[MAX_LEVELS];
} hierarchy;

static csr
csr_alloc(long n, long m, long nnz)
{
	csr c = {n, m, nnz, calloc((size_t) n + 1, sizeof(int)), calloc((size_t) (nnz ? nnz : 1), sizeof(int)),
	         calloc((size_t) (nnz ? nnz : 1), sizeof(double))};
	return c;
}

static void
csr_free(csr * c)
{
	free(c->rp);
	free(c->ci);
	free(c->va);
	memset(c, 0, sizeof(*c));
}

static int
cmp_int(const void * a, const void * b)
{
	return (*(const int *) a > *(const int *) b) - (*(const int *) a < *(const int *) b);
}

/* C = A B */
static csr
multiply(const csr * A, const csr * B)
{
	const long n = A->n, m = B->m;
	int * mark = malloc((size_t) (m ? m : 1) * sizeof(int)), * cols = malloc((size_t) (m ? m : 1) * sizeof(int));
	double * acc = malloc((size_t) (m ? m : 1) * sizeof(double));
	long nnz = 0;
	for (long j = 0; j < m; j++)
		mark[j] = -1;
	for (long i = 0; i < n; i++)
		for (long p = A->rp[i]; p < A->rp[i + 1]; p++)
			for (long q = B->rp[A->ci[p]]; q < B->rp[A->ci[p] + 1]; q++)
				if (mark[B->ci[q]] != i)
				{
					mark[B->ci[q]] = (int) i;
					nnz++;
				}
	csr C = csr_alloc(n, m, nnz);
	for (long j = 0; j < m; j++)
		mark[j] = -1;
	nnz = 0;
	for (long i = 0; i < n; i++)
	{
		long w = 0;
		for (long p = A->rp[i]; p < A->rp[i + 1]; p++)
			for (long q = B->rp[A->ci[p]]; q < B->rp[A->ci[p] + 1]; q++)
			{
				const int j = B->ci[q];
				if (mark[j] != i)
				{
					mark[j] = (int) i;
					acc[j] = 0.0;
					cols[w++] = j;
				}
				acc[j] = fma(A->va[p], B->va[q], acc[j]);
			}
		qsort(cols, (size_t) w, sizeof(int), cmp_int);
		for (long k = 0; k < w; k++)
		{
			C.ci[nnz] = cols[k];
			C.va[nnz++] = acc[cols[k]];
		}
		C.rp[i + 1] = (int) nnz;
	}
	free(mark);
	free(cols);
	free(acc);
	return C;
}

static csr
transpose(const csr * A)
{
	csr T = csr_alloc(A->m, A->n, A->nnz);
	for (long e = 0; e < A->nnz; e++)
		T.rp[A->ci[e] + 1]++;
	for (long c = 0; c < A->m; c++)
		T.rp[c + 1] += T.rp[c];
	int * pos = malloc((size_t) (A->m ? A->m : 1) * sizeof(int));
	memcpy(pos, T.rp, (size_t) A->m * sizeof(int));
	for (long i = 0; i < A->n; i++)
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
		{
			const int at = pos[A->ci[e]]++;
			T.ci[at] = (int) i;
			T.va[at] = A->va[e];
		}
	free(pos);
	return T;
}

static int
strong(double a, double di, double dj, double theta2)
{
	return a * a >= theta2 * (di * dj);
}

static uint64_t
key_of(int state, long i)
{
	const uint32_t h = (uint32_t) i * 0x9E3779B1u;
	return ((uint64_t) state << 62) | ((uint64_t) (h >> 1) << 31) | (uint64_t) i;
}

static void
sweep(const csr * A, const double * d, double theta2, const uint64_t * in, uint64_t * out)
{
	for (long i = 0; i < A->n; i++)
	{
		uint64_t best = in[i];
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
		{
			const int j = A->ci[e];
			if (j != i && strong(A->va[e], d[i], d[j], theta2) && in[j] > best)
				best = in[j];
		}
		out[i] = best;
	}
}

/* steps 3 and 4: agg (n), returns the number of aggregates */
static long
aggregate(const csr * A, const double * d, double theta2, int * agg, long * rounds_out)
{
	const long n = A->n;
	int * state = malloc((size_t) n * sizeof(int)), * id = malloc((size_t) n * sizeof(int)), * agg1 = malloc((size_t) n * sizeof(int));
	uint64_t * k0 = malloc((size_t) n * 8), * k1 = malloc((size_t) n * 8), * k2 = malloc((size_t) n * 8);
	long undecided = n, rounds = 0, count = 0;
	for (long i = 0; i < n; i++)
		state[i] = 1;
	while (undecided > 0)
	{
		for (long i = 0; i < n; i++)
			k0[i] = key_of(state[i], i);
		sweep(A, d, theta2, k0, k1);
		sweep(A, d, theta2, k1, k2);
		undecided = 0;
		for (long i = 0; i < n; i++)
			if (state[i] == 1)
			{
				if (k2[i] == k0[i])
					state[i] = 2;
				else if ((k2[i] >> 62) == 2)
					state[i] = 0;
				else
					undecided++;
			}
		rounds++;
	}
	for (long i = 0; i < n; i++)
	{
		id[i] = (int) count;
		count += state[i] == 2;
	}
	for (long i = 0; i < n; i++)
	{
		int g = state[i] == 2 ? id[i] : -1;
		if (g < 0)
			for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			{
				const int j = A->ci[e];
				if (j != i && state[j] == 2 && strong(A->va[e], d[i], d[j], theta2))
					g = id[j];
			}
		agg1[i] = g;
	}
	for (long i = 0; i < n; i++)
	{
		int g = agg1[i], best_j = 0x7fffffff;
		double best = -1.0;
		if (g < 0)
			for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			{
				const int j = A->ci[e];
				const double m = fabs(A->va[e]);
				if (j == i || agg1[j] < 0 || !strong(A->va[e], d[i], d[j], theta2))
					continue;
				if (m > best || (m == best && j < best_j))
				{
					best = m;
					best_j = j;
					g = agg1[j];
				}
			}
		agg[i] = g;
	}
	free(state);
	free(id);
	free(agg1);
	free(k0);
	free(k1);
	free(k2);
	*rounds_out = rounds;
	return count;
}

void *
amg_reference_build(long n, const int * rp, const int * ci, const double * va, double theta, int max_levels, int coarse_rows)
{
	hierarchy * H = calloc(1, sizeof(hierarchy));
	const double theta2 = theta * theta;
	if (n == 0)
		return H;
	H->lev[0].A = csr_alloc(n, n, rp[n]);
	memcpy(H->lev[0].A.rp, rp, (size_t) (n + 1) * sizeof(int));
	memcpy(H->lev[0].A.ci, ci, (size_t) rp[n] * sizeof(int));
	memcpy(H->lev[0].A.va, va, (size_t) rp[n] * sizeof(double));
	for (int l = 0;; l++)
	{
		level * L = &H->lev[l];
		const csr * A = &L->A;
		const long nl = A->n;
		double * d = malloc((size_t) nl * sizeof(double));
		H->levels = l + 1;
		L->rho = 0;
		for (long i = 0; i < nl; i++)
		{
			double sum = 0;
			int found = 0;
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
		if (nl <= coarse_rows || l + 1 == max_levels)
		{
			free(d);
			break;
		}
		L->agg = malloc((size_t) nl * sizeof(int));
		L->aggregates = aggregate(A, d, theta2, L->agg, &L->rounds);
		if ((double) L->aggregates > 0.9 * (double) nl)
		{
			H->stalled = 1;
			free(d);
			break;
		}
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

void
amg_reference_free(void * h)
{
	hierarchy * H = h;
	for (int l = 0; l < MAX_LEVELS; l++)
	{
		csr_free(&H->lev[l].A);
		csr_free(&H->lev[l].P);
		free(H->lev[l].agg);
	}
	free(H);
}

int
amg_reference_levels(const void * h)
{
	return ((const hierarchy *) h)->levels;
}

int
amg_reference_stalled(const void * h)
{
	return ((const hierarchy *) h)->stalled;
}

/* out: rows, nnz of A, nnz of P, aggregates, rounds; omega, rho */
void
amg_reference_level(const void * h, int l, long * out, double * out_d)
{
	const level * L = &((const hierarchy *) h)->lev[l];
	out[0] = L->A.n;
	out[1] = L->A.nnz;
	out[2] = L->P.nnz;
	out[3] = L->aggregates;
	out[4] = L->rounds;
	out_d[0] = L->omega;
	out_d[1] = L->rho;
}

/* which: 0 = A_l, 1 = P_l */
void
amg_reference_csr(const void * h, int l, int which, int * rp, int * ci, double * va)
{
	const level * L = &((const hierarchy *) h)->lev[l];
	const csr * c = which ? &L->P : &L->A;
	memcpy(rp, c->rp, (size_t) (c->n + 1) * sizeof(int));
	memcpy(ci, c->ci, (size_t) c->nnz * sizeof(int));
	memcpy(va, c->va, (size_t) c->nnz * sizeof(double));
}

void
amg_reference_aggregates(const void * h, int l, int * out)
{
	const level * L = &((const hierarchy *) h)->lev[l];
	if (L->agg)
		memcpy(out, L->agg, (size_t) L->A.n * sizeof(int));
}

/* the packed factor (row-major lower triangle, n (n + 1) / 2 doubles) of a CSR with unique columns; 1, or 0 at a bad pivot */
int
amg_reference_factor(long n, const int * rp, const int * ci, const double * va, double * F)
{
	double * S = calloc((size_t) (n * (n + 1) / 2 + 1), sizeof(double));
	for (long i = 0; i < n; i++)
		for (long e = rp[i]; e < rp[i + 1]; e++)
			if (ci[e] <= i)
				S[i * (i + 1) / 2 + ci[e]] = va[e];
	for (long k = 0; k < n; k++)
		for (long a = k; a < n; a++)
		{
			double s = S[a * (a + 1) / 2 + k];
			for (long p = 0; p < k; p++)
				s = fma(-F[a * (a + 1) / 2 + p], F[k * (k + 1) / 2 + p], s);
			if (a == k)
			{
				if (!isfinite(s) || !(s > 0))
				{
					free(S);
					return 0;
				}
				F[k * (k + 1) / 2 + k] = sqrt(s);
			}
			else
				F[a * (a + 1) / 2 + k] = s / F[k * (k + 1) / 2 + k];
		}
	free(S);
	return 1;
}

/* L y = b, L^t x = y, column by column */
void
amg_reference_dense_solve(long n, const double * F, const double * b, double * x)
{
	double * y = malloc((size_t) (n ? n : 1) * sizeof(double));
	memcpy(y, b, (size_t) n * sizeof(double));
	for (long k = 0; k < n; k++)
	{
		y[k] = y[k] / F[k * (k + 1) / 2 + k];
		for (long a = k + 1; a < n; a++)
			y[a] = fma(-F[a * (a + 1) / 2 + k], y[k], y[a]);
	}
	for (long k = n - 1; k >= 0; k--)
	{
		x[k] = y[k] / F[k * (k + 1) / 2 + k];
		for (long a = 0; a < k; a++)
			y[a] = fma(-F[k * (k + 1) / 2 + a], x[k], y[a]);
	}
	free(y);
}

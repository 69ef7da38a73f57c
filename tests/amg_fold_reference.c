/* The folded tail of the AMG cycle (include/spmv_mi355x.h "AMG: the small levels as one launch") as sequential loops: the V cycle
 * from a first level down to the last and back, over plain CSR copies of A_l, P_l and R_l in the precision `real`. Compiled with
 * gcc -O2 -ffp-contract=off -DREAL=float and -DREAL=double (tests/amg_fold_cases.py), so that every product and sum is rounded on
 * its own and the only fused operations are the fma() calls written here.
 *   a row's product with G lanes: for g = 0..G-1  s_g = +0, then s_g = fma(a_e, x[col(e)], s_g) for the entries e = begin + g,
 *   begin + g + G, ... of the row in stored order; then for h = G/2, G/4, ..., 1 and g = 0..h-1  s_g = s_g + s_{g+h}; the product
 *   is s_0. G = 1 is the plain chain. The rows of A_l take G_l lanes, those of P_l and R_l one.
 *   LANES PER ROW (amg_fold_reference_lanes): G = the largest power of two <= min(64, nnz / n, 1024 / n) in integer division, 1 where
 *   that minimum is 0.
 *   the cycle below the last level: x = w o b;  nu - 1 times { t = A x; x = x + w o (b - t) };  t = b - A x;  b_{l+1} = R t;
 *   x = x + P cycle(l + 1);  nu times the same sweep. The last level: L y = b, L^t x = y in fp64 column by column when a packed
 *   factor was given, else x = w o b and cs - 1 sweeps. */
#include <math.h>
#include <stdlib.h>
#include <string.h>

#ifndef REAL
#define REAL double
#endif
typedef REAL real;

#define MAX_LEVELS 16
#define MAX_LANES 64

static real
fma_real(real a, real b, real c)
{
	return sizeof(real) == 4 ? (real) fmaf((float) a, (float) b, (float) c) : (real) fma((double) a, (double) b, (double) c);
}

typedef struct {
	long n, nc;
	int G;
	int * a_rp, * a_ci, * p_rp, * p_ci, * r_rp, * r_ci;
	real * a_va, * p_va, * r_va, * w, * b, * x, * t;
} level;

typedef struct {
	int levels, nu, cs, dense;
	double * F;
	level lev[MAX_LEVELS];
} tail;

static void *
copy(const void * src, size_t count, size_t size)
{
	void * p = calloc(count ? count : 1, size);
	if (src && count)
		memcpy(p, src, count * size);
	return p;
}

int
amg_fold_reference_lanes(long n, long nnz)
{
	long cap = MAX_LANES;
	int g = 1;
	if (n <= 0)
		return 1;
	if (nnz / n < cap)
		cap = nnz / n;
	if (1024 / n < cap)
		cap = 1024 / n;
	while (2L * g <= cap)
		g *= 2;
	return g;
}

void *
amg_fold_reference_new(int levels, int nu, int cs)
{
	tail * h = calloc(1, sizeof(tail));
	h->levels = levels;
	h->nu = nu;
	h->cs = cs;
	return h;
}

/* level l: A (n rows, values already in `real`), w, the lanes per row, and unless it is the last level P (n x nc) and R (nc x n) */
void
amg_fold_reference_level(void * hv, int l, long n, const int * a_rp, const int * a_ci, const real * a_va, const real * w, int G, long nc,
		const int * p_rp, const int * p_ci, const real * p_va, const int * r_rp, const int * r_ci, const real * r_va)
{
	level * L = &((tail *) hv)->lev[l];
	L->n = n;
	L->nc = nc;
	L->G = G;
	L->a_rp = copy(a_rp, (size_t) n + 1, sizeof(int));
	L->a_ci = copy(a_ci, (size_t) a_rp[n], sizeof(int));
	L->a_va = copy(a_va, (size_t) a_rp[n], sizeof(real));
	L->w = copy(w, (size_t) n, sizeof(real));
	L->b = copy(NULL, (size_t) n, sizeof(real));
	L->x = copy(NULL, (size_t) n, sizeof(real));
	L->t = copy(NULL, (size_t) n, sizeof(real));
	if (p_rp)
	{
		L->p_rp = copy(p_rp, (size_t) n + 1, sizeof(int));
		L->p_ci = copy(p_ci, (size_t) p_rp[n], sizeof(int));
		L->p_va = copy(p_va, (size_t) p_rp[n], sizeof(real));
		L->r_rp = copy(r_rp, (size_t) nc + 1, sizeof(int));
		L->r_ci = copy(r_ci, (size_t) r_rp[nc], sizeof(int));
		L->r_va = copy(r_va, (size_t) r_rp[nc], sizeof(real));
	}
}

/* the packed factor of the last level (row-major lower triangle, fp64): the level is solved densely */
void
amg_fold_reference_factor(void * hv, const double * F)
{
	tail * h = hv;
	const long n = h->lev[h->levels - 1].n;
	h->F = copy(F, (size_t) (n * (n + 1) / 2), sizeof(double));
	h->dense = 1;
}

void
amg_fold_reference_free(void * hv)
{
	tail * h = hv;
	for (int l = 0; l < MAX_LEVELS; l++)
	{
		level * L = &h->lev[l];
		void * all[] = {L->a_rp, L->a_ci, L->p_rp, L->p_ci, L->r_rp, L->r_ci, L->a_va, L->p_va, L->r_va, L->w, L->b, L->x, L->t};
		for (size_t k = 0; k < sizeof(all) / sizeof(all[0]); k++)
			free(all[k]);
	}
	free(h->F);
	free(h);
}

static real
row_product(const int * rp, const int * ci, const real * va, long i, int G, const real * x)
{
	real s[MAX_LANES];
	for (int g = 0; g < G; g++)
	{
		s[g] = 0;
		for (long e = rp[i] + g; e < rp[i + 1]; e += G)
			s[g] = fma_real(va[e], x[ci[e]], s[g]);
	}
	for (int h = G / 2; h >= 1; h /= 2)
		for (int g = 0; g < h; g++)
			s[g] = s[g] + s[g + h];
	return s[0];
}

static void
sweep(const level * L, const real * b, real * x)
{
	for (long i = 0; i < L->n; i++)
		L->t[i] = row_product(L->a_rp, L->a_ci, L->a_va, i, L->G, x);
	for (long i = 0; i < L->n; i++)
		x[i] = x[i] + L->w[i] * (b[i] - L->t[i]);
}

static void
dense_solve(const double * F, long n, const real * b, real * x)
{
	double * y = malloc((size_t) (n ? n : 1) * sizeof(double));
	for (long a = 0; a < n; a++)
		y[a] = (double) b[a];
	for (long k = 0; k < n; k++)
	{
		y[k] = y[k] / F[k * (k + 1) / 2 + k];
		for (long a = k + 1; a < n; a++)
			y[a] = fma(-F[a * (a + 1) / 2 + k], y[k], y[a]);
	}
	for (long k = n - 1; k >= 0; k--)
	{
		y[k] = y[k] / F[k * (k + 1) / 2 + k];
		for (long a = 0; a < k; a++)
			y[a] = fma(-F[k * (k + 1) / 2 + a], y[k], y[a]);
	}
	for (long a = 0; a < n; a++)
		x[a] = (real) y[a];
	free(y);
}

static void
cycle(tail * h, int l, const real * b, real * x)
{
	level * L = &h->lev[l];
	if (l == h->levels - 1)
	{
		if (h->dense)
		{
			dense_solve(h->F, L->n, b, x);
			return;
		}
		for (long i = 0; i < L->n; i++)
			x[i] = L->w[i] * b[i];
		for (int s = 1; s < h->cs; s++)
			sweep(L, b, x);
		return;
	}
	level * C = &h->lev[l + 1];
	for (long i = 0; i < L->n; i++)
		x[i] = L->w[i] * b[i];
	for (int s = 1; s < h->nu; s++)
		sweep(L, b, x);
	for (long i = 0; i < L->n; i++)
		L->t[i] = b[i] - row_product(L->a_rp, L->a_ci, L->a_va, i, L->G, x);
	for (long j = 0; j < C->n; j++)
		C->b[j] = row_product(L->r_rp, L->r_ci, L->r_va, j, 1, L->t);
	cycle(h, l + 1, C->b, C->x);
	for (long i = 0; i < L->n; i++)
		x[i] = x[i] + row_product(L->p_rp, L->p_ci, L->p_va, i, 1, C->x);
	for (int s = 0; s < h->nu; s++)
		sweep(L, b, x);
}

/* out = cycle(first, in); `in` and `out` hold n_first values and do not overlap */
void
amg_fold_reference_apply(void * hv, int first, const real * in, real * out)
{
	cycle(hv, first, in, out);
}

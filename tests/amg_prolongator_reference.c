/* The hierarchy of include/spmv_mi355x.h "AMG" with steps 5a to 5c of "AMG: a caller's near-null vector and filtered prolongator
 * smoothing" as sequential loops. Compiled with gcc -O2 -ffp-contract=off (tests/amg_prolongator_cases.py). Steps 1 to 4 and 6, the
 * products and the transposition are those of tests/amg_reference.c, which is included as it stands; what is new is the filter, the
 * tentative prolongator of a near-null vector and the prolongator from both, once finding everything itself (amg_prolongator_build)
 * and once with the aggregates, the kept patterns and t given, as an update of the values has them (amg_prolongator_update). */
#include "amg_reference.c"

typedef struct {
	hierarchy H;                  /* first: the accessors of amg_reference.c work on a handle of this type */
	int filtered, has_nn;
	csr F[MAX_LEVELS];            /* A_F of a coarsened level (filtered) */
	int * map[MAX_LEVELS];        /* entry q of A_F is entry map[q] of A_l */
	int * fb[MAX_LEVELS];         /* 1 where the row fell back to all its entries */
	double * b[MAX_LEVELS];       /* the level's near-null vector */
	double * t[MAX_LEVELS];
	long unfiltered[MAX_LEVELS];
	double omega_p[MAX_LEVELS], rho_p[MAX_LEVELS];
	int bad_level;                /* -1, or the level with a bad aggregate norm (build) or a bad lumped diagonal (update) */
	long bad_index;
} phierarchy;

static void
diagonal(const csr * A, double * d, double * rho_out)
{
	double rho = 0;
	for (long i = 0; i < A->n; i++)
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
		rho = fmax(rho, sum / d[i]);
	}
	*rho_out = rho;
}

/* 5a with its own decisions: A_F, map, fb, dF */
static void
filter_level(phierarchy * Q, int l, const double * d, double theta2, double * df)
{
	const csr * A = &Q->H.lev[l].A;
	const long n = A->n;
	int * keep = malloc((size_t) (A->nnz ? A->nnz : 1) * sizeof(int));
	long nnz = 0;
	Q->fb[l] = calloc((size_t) n, sizeof(int));
	for (long i = 0; i < n; i++)
	{
		double lump = 0.0;
		int found = 0;
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
		{
			const int j = A->ci[e];
			int k;
			if (j == i)
			{
				k = !found;
				found = 1;
			}
			else
				k = strong(A->va[e], d[i], d[j], theta2);
			keep[e] = k;
			if (!k)
				lump = lump + A->va[e];
		}
		df[i] = d[i] + lump;
		if (!isfinite(df[i]) || !(df[i] > 0))
		{
			df[i] = d[i];
			Q->fb[l][i] = 1;
			Q->unfiltered[l]++;
			for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
				keep[e] = 1;
		}
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			nnz += keep[e];
	}
	Q->F[l] = csr_alloc(n, n, nnz);
	Q->map[l] = malloc((size_t) (nnz ? nnz : 1) * sizeof(int));
	nnz = 0;
	for (long i = 0; i < n; i++)
	{
		for (long e = A->rp[i]; e < A->rp[i + 1]; e++)
			if (keep[e])
			{
				Q->F[l].ci[nnz] = A->ci[e];
				Q->map[l][nnz++] = (int) e;
			}
		Q->F[l].rp[i + 1] = (int) nnz;
	}
	free(keep);
}

/* A_F's values on its pattern and map from A's values and dF; rho_p */
static void
filter_values(phierarchy * Q, int l, const double * df)
{
	const csr * A = &Q->H.lev[l].A;
	csr * F = &Q->F[l];
	double rho = 0;
	for (long i = 0; i < A->n; i++)
	{
		double sum = 0;
		int found = 0;
		for (long q = F->rp[i]; q < F->rp[i + 1]; q++)
		{
			double v = A->va[Q->map[l][q]];
			if (!found && F->ci[q] == i)
			{
				v = df[i];
				found = 1;
			}
			F->va[q] = v;
			sum = sum + fabs(v);
		}
		rho = fmax(rho, sum / df[i]);
	}
	Q->rho_p[l] = rho;
	Q->omega_p[l] = 4.0 / (3.0 * rho);
}

/* 5c and 6 of level l from A_F (or A_l), t and dF */
static void
prolongate(phierarchy * Q, int l, const double * df)
{
	level * L = &Q->H.lev[l];
	const long nl = L->A.n;
	csr T = csr_alloc(nl, L->aggregates, nl);
	for (long i = 0; i < nl; i++)
	{
		T.rp[i + 1] = (int) (i + 1);
		T.ci[i] = L->agg[i];
		T.va[i] = Q->has_nn ? Q->t[l][i] : 1.0;
	}
	L->P = multiply(Q->filtered ? &Q->F[l] : &L->A, &T);
	for (long i = 0; i < nl; i++)
		for (long e = L->P.rp[i]; e < L->P.rp[i + 1]; e++)
			L->P.va[e] = (L->P.ci[e] == L->agg[i] ? T.va[i] : 0.0) - (Q->omega_p[l] / df[i]) * L->P.va[e];
	csr R = transpose(&L->P), AP = multiply(&L->A, &L->P);
	Q->H.lev[l + 1].A = multiply(&R, &AP);
	csr_free(&T);
	csr_free(&R);
	csr_free(&AP);
}

static phierarchy *
start(long n, const int * rp, const int * ci, const double * va, int filtered, const double * near_null)
{
	phierarchy * Q = calloc(1, sizeof(phierarchy));
	Q->filtered = filtered;
	Q->has_nn = near_null != NULL;
	Q->bad_level = -1;
	if (n == 0)
		return Q;
	Q->H.lev[0].A = csr_alloc(n, n, rp[n]);
	memcpy(Q->H.lev[0].A.rp, rp, (size_t) (n + 1) * sizeof(int));
	memcpy(Q->H.lev[0].A.ci, ci, (size_t) rp[n] * sizeof(int));
	memcpy(Q->H.lev[0].A.va, va, (size_t) rp[n] * sizeof(double));
	if (near_null)
	{
		Q->b[0] = malloc((size_t) n * sizeof(double));
		memcpy(Q->b[0], near_null, (size_t) n * sizeof(double));
	}
	return Q;
}

void *
amg_prolongator_build(long n, const int * rp, const int * ci, const double * va, double theta, int max_levels, int coarse_rows, int filtered,
		const double * near_null)
{
	phierarchy * Q = start(n, rp, ci, va, filtered, near_null);
	hierarchy * H = &Q->H;
	const double theta2 = theta * theta;
	if (n == 0)
		return Q;
	for (int l = 0;; l++)
	{
		level * L = &H->lev[l];
		const long nl = L->A.n;
		double * d = malloc((size_t) nl * sizeof(double)), * df = malloc((size_t) nl * sizeof(double));
		int stop = 0;
		H->levels = l + 1;
		diagonal(&L->A, d, &L->rho);
		L->omega = 4.0 / (3.0 * L->rho);
		if (nl <= coarse_rows || l + 1 == max_levels)
			stop = 1;
		if (!stop)
		{
			L->agg = malloc((size_t) nl * sizeof(int));
			L->aggregates = aggregate(&L->A, d, theta2, L->agg, &L->rounds);
			if ((double) L->aggregates > 0.9 * (double) nl)
				H->stalled = stop = 1;
		}
		if (!stop)
		{
			memcpy(df, d, (size_t) nl * sizeof(double));
			Q->omega_p[l] = L->omega;
			Q->rho_p[l] = L->rho;
			if (filtered)
			{
				filter_level(Q, l, d, theta2, df);
				filter_values(Q, l, df);
			}
			if (Q->has_nn)
			{
				/* the members of an aggregate in ascending i: one pass over i adds to the aggregate's own sum */
				double * s = calloc((size_t) L->aggregates, sizeof(double));
				Q->t[l] = malloc((size_t) nl * sizeof(double));
				for (long i = 0; i < nl; i++)
					s[L->agg[i]] = s[L->agg[i]] + Q->b[l][i] * Q->b[l][i];
				for (long a = 0; a < L->aggregates; a++)
				{
					s[a] = sqrt(s[a]);
					if ((!isfinite(s[a]) || !(s[a] > 0)) && Q->bad_level < 0)
					{
						Q->bad_level = l;
						Q->bad_index = a;
					}
				}
				for (long i = 0; i < nl; i++)
					Q->t[l][i] = Q->b[l][i] / s[L->agg[i]];
				Q->b[l + 1] = s;
				if (Q->bad_level >= 0)
					stop = 1;
			}
		}
		if (!stop)
			prolongate(Q, l, df);
		free(d);
		free(df);
		if (stop)
			break;
	}
	return Q;
}

/* The update: the values va on the structure of `from` (a handle of amg_prolongator_build): its levels, aggregates, kept patterns,
 * maps, fall-back rows, t and b are taken as given; lump, dF, rho_p, omega_p, A_F's values, P and A_{l+1} are recomputed. */
void *
amg_prolongator_update(const void * from, const double * va)
{
	const phierarchy * S = from;
	const long n = S->H.levels ? S->H.lev[0].A.n : 0;
	phierarchy * Q = start(n, n ? S->H.lev[0].A.rp : NULL, n ? S->H.lev[0].A.ci : NULL, va, S->filtered, S->has_nn ? S->b[0] : NULL);
	hierarchy * H = &Q->H;
	H->stalled = S->H.stalled;
	for (int l = 0; l < S->H.levels; l++)
	{
		level * L = &H->lev[l];
		const level * K = &S->H.lev[l];
		const long nl = L->A.n;
		double * d = malloc((size_t) nl * sizeof(double)), * df = malloc((size_t) nl * sizeof(double));
		H->levels = l + 1;
		diagonal(&L->A, d, &L->rho);
		L->omega = 4.0 / (3.0 * L->rho);
		L->rounds = K->rounds;
		L->aggregates = K->aggregates;
		if (K->agg)
		{
			L->agg = malloc((size_t) nl * sizeof(int));
			memcpy(L->agg, K->agg, (size_t) nl * sizeof(int));
		}
		if (K->P.rp)
		{
			memcpy(df, d, (size_t) nl * sizeof(double));
			Q->omega_p[l] = L->omega;
			Q->rho_p[l] = L->rho;
			if (S->filtered)
			{
				const csr * F = &S->F[l];
				Q->F[l] = csr_alloc(nl, nl, F->nnz);
				memcpy(Q->F[l].rp, F->rp, (size_t) (nl + 1) * sizeof(int));
				memcpy(Q->F[l].ci, F->ci, (size_t) F->nnz * sizeof(int));
				Q->map[l] = malloc((size_t) (F->nnz ? F->nnz : 1) * sizeof(int));
				memcpy(Q->map[l], S->map[l], (size_t) F->nnz * sizeof(int));
				Q->fb[l] = malloc((size_t) nl * sizeof(int));
				memcpy(Q->fb[l], S->fb[l], (size_t) nl * sizeof(int));
				Q->unfiltered[l] = S->unfiltered[l];
				for (long i = 0; i < nl; i++)
				{
					double lump = 0.0;
					long q = F->rp[i];
					for (long e = L->A.rp[i]; e < L->A.rp[i + 1]; e++)
					{
						if (q < F->rp[i + 1] && S->map[l][q] == e)
							q++;
						else
							lump = lump + L->A.va[e];
					}
					df[i] = S->fb[l][i] ? d[i] : d[i] + lump;
					if ((!isfinite(df[i]) || !(df[i] > 0)) && Q->bad_level < 0)
					{
						Q->bad_level = l;
						Q->bad_index = i;
					}
				}
				filter_values(Q, l, df);
			}
			if (S->has_nn)
			{
				Q->t[l] = malloc((size_t) nl * sizeof(double));
				memcpy(Q->t[l], S->t[l], (size_t) nl * sizeof(double));
				Q->b[l + 1] = malloc((size_t) K->aggregates * sizeof(double));
				memcpy(Q->b[l + 1], S->b[l + 1], (size_t) K->aggregates * sizeof(double));
			}
			if (Q->bad_level < 0)
				prolongate(Q, l, df);
		}
		free(d);
		free(df);
		if (Q->bad_level >= 0)
			break;
	}
	return Q;
}

void
amg_prolongator_free(void * h)
{
	phierarchy * Q = h;
	for (int l = 0; l < MAX_LEVELS; l++)
	{
		csr_free(&Q->H.lev[l].A);
		csr_free(&Q->H.lev[l].P);
		free(Q->H.lev[l].agg);
		csr_free(&Q->F[l]);
		free(Q->map[l]);
		free(Q->fb[l]);
		free(Q->b[l]);
		free(Q->t[l]);
	}
	free(Q);
}

/* out: filtered, has_nn, bad_level, bad_index */
void
amg_prolongator_flags(const void * h, long * out)
{
	const phierarchy * Q = h;
	out[0] = Q->filtered;
	out[1] = Q->has_nn;
	out[2] = Q->bad_level;
	out[3] = Q->bad_index;
}

/* out: nnz of A_F (nnz of A_l where nothing is filtered; 0 without a prolongator), unfiltered rows; omega_p, rho_p */
void
amg_prolongator_level(const void * h, int l, long * out, double * out_d)
{
	const phierarchy * Q = h;
	const int has_p = Q->H.lev[l].P.rp != NULL;
	out[0] = !has_p ? 0 : Q->filtered ? Q->F[l].nnz : Q->H.lev[l].A.nnz;
	out[1] = Q->unfiltered[l];
	out_d[0] = has_p ? Q->omega_p[l] : 0;
	out_d[1] = has_p ? Q->rho_p[l] : 0;
}

/* A_F of level l and its map */
void
amg_prolongator_filtered_csr(const void * h, int l, int * rp, int * ci, double * va, int * map)
{
	const phierarchy * Q = h;
	const csr * c = &Q->F[l];
	memcpy(rp, c->rp, (size_t) (c->n + 1) * sizeof(int));
	memcpy(ci, c->ci, (size_t) c->nnz * sizeof(int));
	memcpy(va, c->va, (size_t) c->nnz * sizeof(double));
	memcpy(map, Q->map[l], (size_t) c->nnz * sizeof(int));
}

/* b_l (rows of level l) and, where the level was coarsened, t (NULL pointers are skipped) */
void
amg_prolongator_vectors(const void * h, int l, double * b, double * t)
{
	const phierarchy * Q = h;
	const long n = Q->H.lev[l].A.n;
	if (b && Q->b[l])
		memcpy(b, Q->b[l], (size_t) n * sizeof(double));
	if (t && Q->t[l])
		memcpy(t, Q->t[l], (size_t) n * sizeof(double));
}

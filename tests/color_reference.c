/* The reference of the multicolour ordering (include/spmv_mi355x.h "multicolour ordering"): first-fit greedy colouring of the graph of
 * A + A^t (i and j adjacent when a_ij or a_ji is stored, i != j) in DESCENDING KEY ORDER, one vertex after the other, with
 * key(i) = ((uint64) (h >> 1) << 31) | i, h = (uint32) (i * 0x9E3779B1u). The synchronous rounds of the device colour a vertex once
 * every neighbour of higher key is coloured, so they give these colours; the round in which vertex v is coloured is
 * 1 + max(round of its neighbours of higher key), which this loop knows when it reaches v. Returns the number of colours; rounds_out =
 * the last round. Built by tests/color_cases.py with gcc -O2. */
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

static uint64_t
key_of(long i)
{
	const uint32_t h = (uint32_t) i * 0x9E3779B1u;
	return ((uint64_t) (h >> 1) << 31) | (uint64_t) i;
}

static int
by_key_descending(const void * a, const void * b)
{
	const uint64_t x = *(const uint64_t *) a, y = *(const uint64_t *) b;
	return x < y ? 1 : x > y ? -1 : 0;
}

long
color_reference(long n, const int32_t * rp, const int32_t * ci, int32_t * colors, long * rounds_out)
{
	*rounds_out = 0;
	if (n == 0)
		return 0;
	const long nnz = rp[n];
	/* the rows of A^t by counting */
	int32_t * tp = calloc((size_t) n + 1, sizeof(int32_t)), * tc = malloc(((size_t) nnz + 1) * sizeof(int32_t));
	for (long e = 0; e < nnz; e++)
		tp[ci[e] + 1]++;
	for (long i = 0; i < n; i++)
		tp[i + 1] += tp[i];
	int32_t * next = malloc((size_t) n * sizeof(int32_t));
	memcpy(next, tp, (size_t) n * sizeof(int32_t));
	for (long i = 0; i < n; i++)
		for (long e = rp[i]; e < rp[i + 1]; e++)
			tc[next[ci[e]]++] = (int32_t) i;
	uint64_t * order = malloc((size_t) n * sizeof(uint64_t));
	for (long i = 0; i < n; i++)
	{
		order[i] = key_of(i);
		colors[i] = -1;
	}
	qsort(order, (size_t) n, sizeof(uint64_t), by_key_descending);
	int32_t * round = calloc((size_t) n, sizeof(int32_t));
	int32_t * seen = malloc(((size_t) n + 1) * sizeof(int32_t));          /* seen[c] == v + 1: a neighbour of v holds colour c */
	memset(seen, 0, ((size_t) n + 1) * sizeof(int32_t));
	long num_colors = 0, rounds = 0;
	for (long t = 0; t < n; t++)
	{
		const long v = (long) (order[t] & 0x7fffffffu);
		int32_t wait = 0;
		for (int side = 0; side < 2; side++)
		{
			const int32_t * p = side ? tp : rp, * c = side ? tc : ci;
			for (long e = p[v]; e < p[v + 1]; e++)
			{
				const long j = c[e];
				if (j == v || colors[j] < 0)
					continue;                                 /* a neighbour of lower key: still uncoloured */
				seen[colors[j]] = (int32_t) (v + 1);
				if (round[j] > wait)
					wait = round[j];
			}
		}
		int32_t col = 0;
		while (seen[col] == v + 1)
			col++;
		colors[v] = col;
		round[v] = wait + 1;
		if (col + 1 > num_colors)
			num_colors = col + 1;
		if (round[v] > rounds)
			rounds = round[v];
	}
	free(tp);
	free(tc);
	free(next);
	free(order);
	free(round);
	free(seen);
	*rounds_out = rounds;
	return num_colors;
}

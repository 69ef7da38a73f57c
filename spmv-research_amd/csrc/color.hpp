// Multicolour ordering (include/spmv_mi355x.h "multicolour ordering"): what color.hip (the checks, the rounds, the
// permuted matrix, the C ABI) and kernels_color.hip (the kernels and the two hipcub calls) share.
//
// THE GRAPH. The vertices are the rows of a square CSR pattern; i and j (i != j) are adjacent when a_ij OR a_ji is stored. The kernels
// therefore walk row i of A and row i of A^t (the device transposition of the pattern, transpose_csr.hip); when the two patterns are
// equal array for array the second walk is skipped. Stored zeros count, duplicates and a missing diagonal are harmless, rows need not
// be sorted.
// THE RULE. key(i) = ((uint64) (h >> 1) << 31) | i with h = (uint32) (i * COLOR_HASH_MUL): the AMG independent set's keys, all
// different. Rounds are synchronous: a round reads one colour array and writes the other. In a round an uncoloured vertex whose key
// exceeds the key of every UNCOLOURED neighbour takes the smallest colour >= 0 that none of its coloured neighbours holds; everything
// else is copied. A neighbour of lower key is never coloured before the vertex itself, so the result is first-fit greedy colouring in
// descending key order (tests/color_reference.c is that loop), whatever the number of workgroups. The rounds a vertex waits are
// 1 + the longest chain of ever higher keys that starts at it: A CLIQUE OF m VERTICES NEEDS m ROUNDS, a grid or a stencil 6 to 22.
// The host reads one counter per round (the vertices still uncoloured) and stops at 0; COLOR_ROUND_CAP rounds are an error with a
// message. Nothing spins, and nothing is ordered between workgroups except by the launch boundary.
// THE MAPPING. One lane per row, COLOR_TB lanes per workgroup, at most COLOR_MAX_GRID workgroups that walk the rows with a grid stride
// (AMG_TB / AMG_MAX_GRID of amg.hpp: beyond 262 144 rows a workgroup takes a second trip). The smallest free colour is searched in
// windows of 64 colours held as a 64-bit mask: window 0 is filled by the walk that compares the keys, every further window is one more
// walk of the row, and a window is only left when all its 64 colours are taken, so the trips are bounded by degree / 64 + 1. No row
// is refused for its width or its colour count. The one atomic is the integer count of uncoloured vertices, one add per workgroup.
// DERIVED ON THE DEVICE: the largest colour (hipcub reduce), perm = the rows sorted by (colour, row) (one stable hipcub radix sort of
// (colour, row number) over the bits the largest colour takes), rank = its inverse (a scatter), color_ptr = the first sorted position
// of every colour (a lower-bound search, one lane per colour).
// THE PERMUTED MATRIX B = P A P^t is two stable transpositions of the pattern: the columns of A relabelled by rank and transposed give
// the rows = new columns, each in ascending old row; those relabelled by rank and transposed again give the rows = new rows, each in
// ascending new column, equal columns in their stored order. The entry map is the composition of the two sorted id arrays.
// The vector kernels move row-major n x k blocks in chunks of 8 / 4 / 2 / 1 columns (column_chunks), a thread owning one row of its
// chunk: out[p] = in[idx[p]] with idx = perm (forward) or rank (backward), so the stores are the contiguous side in both directions.
//     kernel                          VGPRs   LDS        scratch
//     color_round_kernel                22    1 024 B       0
//     color_differ_kernel               10        0         0
//     color_iota_kernel                 18        0         0
//     color_rank_kernel                 20        0         0
//     color_start_kernel                12        0         0
//     color_relabel_kernel              18        0         0
//     color_compose_kernel              18        0         0
//     color_gather_values_kernel         8        0         0
//     color_gather_rows_kernel <KC = 8 / 4 / 2 / 1>, the largest of fp32 and fp64
//                           24 / 16 / 12 / 24     0         0
// (-Rpass-analysis=kernel-resource-usage, gfx950; no kernel spills.)
#pragma once

#include <vector>

#include "common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

constexpr int COLOR_TB = 256;                             // AMG_TB
constexpr int COLOR_MAX_GRID = 1024;                      // AMG_MAX_GRID: more rows are walked with a grid stride
constexpr int COLOR_ROUND_CAP = 4096;                     // a clique of m vertices needs m rounds: beyond this create refuses
constexpr unsigned COLOR_HASH_MUL = 0x9E3779B1u;          // AMG_HASH_MUL

// the pattern of A and, unless the two are equal, of A^t, on the device (rpt = cit = NULL: one walk)
struct ColorGraph {
	const int * rp, * ci, * rpt, * cit;
	long n;
};

inline int
color_grid(long n)
{
	return (int) std::min<long>(COLOR_MAX_GRID, std::max<long>(1, (n + COLOR_TB - 1) / COLOR_TB));
}

// one round: cout from cin (-1 = uncoloured); *left += the vertices still uncoloured in cout (zeroed by the caller)
int launch_color_round(const ColorGraph & g, const int * cin, int * cout, int * left, hipStream_t st);
// *differ = 1 when a[0 .. count) and b[0 .. count) differ anywhere (zeroed by the caller)
int launch_color_differ(const int * a, const int * b, long count, int * differ, hipStream_t st);
// the bytes of scratch the two hipcub calls below want for n rows (the sort over the bits of max_color)
size_t color_max_bytes(long n);
size_t color_sort_bytes(long n, int max_color);
// *max_out (device) = the largest colour
int launch_color_max(long n, const int * colors, int * max_out, void * tmp, size_t tmp_bytes, hipStream_t st);
// perm = the rows by (colour, row), rank = its inverse, sorted = the colours in that order; iota is n words of scratch
int launch_color_sort(long n, const int * colors, int max_color, int * iota, int * sorted, int * perm, int * rank, void * tmp, size_t tmp_bytes,
		hipStream_t st);
// ptr[c] = the first sorted position whose colour is >= c, c = 0 .. num_colors
int launch_color_start(long n, const int * sorted, long num_colors, int * ptr, hipStream_t st);
// out[e] = rank[in[e]]
int launch_color_relabel(long count, const int * in, const int * rank, int * out, hipStream_t st);
// out[e] = first[second[e]]
int launch_color_compose(long count, const unsigned * first, const unsigned * second, int * out, hipStream_t st);
// out[e] = in[map[e]]
int launch_color_gather_values(long count, const int * map, const double * in, double * out, hipStream_t st);
// out[p * ldout + c] = in[idx[p] * ldin + c] for the k columns of row-major blocks, one launch per chunk of 8, 4, 2 or 1 columns
int launch_color_gather_rows(bool f32, int k, const int * idx, const void * in, long ldin, void * out, long ldout, long n, hipStream_t st);

// color.hip: create with a round cap of the caller's (the ABI passes COLOR_ROUND_CAP; a lower cap is for the tests of the refusal)
int color_create_capped(spmv_mi355x_color ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, int device, int round_cap);

}  // namespace spmv

struct spmv_mi355x_color {
	int device = 0;
	long n = 0, nnz = 0, num_colors = 0, rounds = 0, max_class = 0, min_class = 0;
	int symmetric = 0;
	double transpose_seconds = 0, round_seconds = 0, sort_seconds = 0, permute_seconds = 0;
	std::vector<int32_t> colors, perm, rank, color_ptr;   // the host copies the getters return
	int * d_rp = nullptr, * d_ci = nullptr;               // A's pattern: kept until the permuted matrix is formed
	int * d_perm = nullptr, * d_rank = nullptr;
	int * d_rp_b = nullptr, * d_ci_b = nullptr, * d_map = nullptr;   // B's pattern and the entry map, formed at the first permute call
	bool permuted = false;
	double mem_footprint = 0;
};

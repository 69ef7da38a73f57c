// SpGEMM plans (include/spmv_mi355x.h "SpGEMM"): what spgemm.hip (the checks, the plan, the C ABI) and kernels_spgemm.hip (the row
// kernel) share.
//
// THE MAPPING. C = A B row by row (Gustavson): row i of C is the union of the rows of B that row i of A names, gathered in a hash
// table of the row's own, open addressing with linear probing, hash(col) = (col * 0x9E3779B1) >> (32 - log2 T). The host bins the rows
// on w = the bound of the row's width: min(products_i, n) for the counting pass (COUNT), the true width of C's row, known after it,
// for the pass that writes the columns (FILL) and for the numeric one (NUMERIC). A bin fixes the lanes that own a row, the rows that
// share a workgroup and the table size T, a power of two >= 2 w:
//     bin   w              T        lanes per row   rows per workgroup   threads   LDS COUNT, FILL   LDS NUMERIC
//     0        0 ..   16     32          8                32               256       4 224 B       12 416 B
//     1       17 ..   64    128         16                16               256       8 256 B       24 640 B
//     2       65 ..  128    256         32                 8               256       8 224 B       24 608 B
//     3      129 ..  512   1024         64                 4               256      16 400 B       49 168 B
//     4      513 .. 1024   2048         64                 2               128      16 392 B       49 160 B
//     5     1025 .. 2048   4096         64                 1                64      16 388 B       49 160 B
//     6     2049 ..        >= 2 w       64                 1                64       table in the workgroup's slab of global memory
// Keys (int32 columns, SPGEMM_EMPTY where free) and values (fp64) lie in separate arrays. One launch per non-empty bin over the bin's
// list of rows, at most SPGEMM_MAX_GRID workgroups which walk the list with a grid stride; the slab of the last bin is grid * T_max entries,
// whatever m is. A row's lanes always lie in one wave, but the phases of a row, and the steps of the numeric pass, are separated by
// workgroup barriers and by nothing else: the trip count of every loop that holds a barrier is the same in all threads of the
// workgroup. Keys are claimed with a compare-and-swap on the row's own table; values are read and written plainly. Nothing spins,
// nothing waits on another workgroup: every probe loop ends after T probes at the latest and then raises the error word.
#pragma once

#include <vector>

#include "common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

constexpr int SPGEMM_BINS = 7;                            // the last one keeps its tables in global memory
constexpr int SPGEMM_MAX_GRID = 2048;                     // workgroups per launch; more rows are walked with a grid stride
constexpr int SPGEMM_GLOBAL_GRID = 256;                   // the same for the global bin: its slab is grid * T_max entries ...
constexpr size_t SPGEMM_SLAB_BYTES = (size_t) 1 << 30;    // ... and the grid shrinks (to 1 at the least) until the slab fits this
constexpr int SPGEMM_BIN_WMAX[SPGEMM_BINS - 1] = {16, 64, 128, 512, 1024, 2048};
constexpr int SPGEMM_BIN_LOG_T[SPGEMM_BINS - 1] = {5, 7, 8, 10, 11, 12};
constexpr int SPGEMM_BIN_LANES[SPGEMM_BINS] = {8, 16, 32, 64, 64, 64, 64};
constexpr int SPGEMM_BIN_ROWS[SPGEMM_BINS] = {32, 16, 8, 4, 2, 1, 1};    // rows per workgroup
constexpr int SPGEMM_EMPTY = 0x7fffffff;                  // no column: n < 2^31 - 1, and it sorts behind every column
constexpr unsigned SPGEMM_HASH_MUL = 0x9E3779B1u;

inline int
spgemm_bin_of(long w)
{
	int b = 0;
	while (b < SPGEMM_BINS - 1 && w > SPGEMM_BIN_WMAX[b])
		b++;
	return b;
}

// log2 of the table of a row of the global bin: the smallest power of two >= 2 w (w >= 1)
__host__ __device__ inline int
spgemm_log_table(long w)
{
	int lg = 1;
	while (((long) 1 << lg) < 2 * w)
		lg++;
	return lg;
}

enum { SPGEMM_COUNT = 0, SPGEMM_FILL = 1, SPGEMM_NUMERIC = 2 };

// everything on the device
struct SpgemmArrays {
	const int * a_rp;
	const int * a_ci;
	const int * b_rp;
	const int * b_ci;
	long n;
	const long * products;            // m: what spgemm_count_products wrote
	// COUNT writes width (m, the distinct columns of the row) and probes (m, the probes beyond the first of every insertion)
	long * width;
	int * probes;
	// FILL writes c_ci (the row's columns ascending), NUMERIC reads it; both read c_rp
	const int * c_rp;
	int * c_ci;
	// NUMERIC
	const double * a_va;
	const double * b_va;
	double * c_va;
	// the slab of the global bin: grid * slab_t keys, and as many values in the numeric pass
	int * slab_keys;
	double * slab_vals;
	long slab_t;
	int * error;                      // 0, or 1 + the row whose table was found full
};

int launch_spgemm_products(long m, const int * a_rp, const int * a_ci, const int * b_rp, long * products, hipStream_t st);
// the rows bin_rows[0 .. count) of one bin in one of the three modes, `grid` workgroups, enqueued on st
int launch_spgemm_rows(int mode, int bin, const SpgemmArrays & a, const int * bin_rows, long count, int grid, hipStream_t st);
// row_ptr[i] = (int) offsets[i] for i in [0, count)
int launch_spgemm_narrow(const long * offsets, int * row_ptr, long count, hipStream_t st);

}  // namespace spmv

struct spmv_mi355x_spgemm {
	int device = 0;
	long m = 0, k = 0, n = 0, nnz_a = 0, nnz_b = 0, nnz_c = 0;
	long products = 0, max_row_products = 0, max_row_c = 0, symbolic_probes = 0;
	long symbolic_bin_rows[spmv::SPGEMM_BINS] = {}, numeric_bin_rows[spmv::SPGEMM_BINS] = {};
	double symbolic_seconds = 0, multiply_seconds = 0;
	size_t device_bytes = 0;
	std::vector<int32_t> c_rp;                            // C's row pointer on the host (m + 1); the columns stay on the device
	std::vector<void *> owned;                            // every device allocation of the plan
	int * d_a_rp = nullptr, * d_a_ci = nullptr, * d_b_rp = nullptr, * d_b_ci = nullptr, * d_c_rp = nullptr, * d_c_ci = nullptr;
	long * d_products = nullptr;
	int * d_bin[spmv::SPGEMM_BINS] = {};                  // the row lists of the bins on C's true width (FILL, NUMERIC)
	int grid[spmv::SPGEMM_BINS] = {};
	int * d_slab_keys = nullptr;
	double * d_slab_vals = nullptr;
	long slab_t = 0;
	int * d_error = nullptr;
};

// Factorized sparse approximate inverse (include/spmv_mi355x.h "FSAI"): what fsai.hip (the checks, the handle, the C ABI),
// kernels_fsai.hip (the row kernel) and solver_pcg_tri.hip (pcg_fsai) share.
//
// THE MAPPING. Row i of G is one dense SPD system of s = the row's pattern entries, s <= FSAI_MAX_ROW. The host bins the rows on s;
// a bin fixes the lanes that own a row, the rows that share a workgroup and the LDS a row gets (its packed triangle, the pivots,
// g and the row's columns):
//     bin   s          lanes per row   rows per workgroup   threads   LDS per workgroup   VGPRs   scratch
//     0     1 ..   8         8                32              256         14 464 B          76        0
//     1     9 ..  32        16                16              256         77 888 B          67        0
//     2    33 ..  64        64                 4              256         71 696 B          58        0
//     3    65 .. 128        64                 2              128        137 224 B          56        0
// One launch per non-empty bin over the bin's list of rows, at most FSAI_MAX_GRID workgroups which walk the list with a grid stride.
// A row's lanes always lie in one wave, but the phases of a row are separated by workgroup barriers and by nothing else: the trip
// count of every loop that holds a barrier is that of the workgroup's widest row. No atomics, no flags, nothing spins.
#pragma once

#include <vector>

#include "common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

constexpr int FSAI_BINS = 4;
constexpr int FSAI_MAX_GRID = 2048;                       // workgroups per launch; more rows are walked with a grid stride
constexpr int FSAI_BIN_SMAX[FSAI_BINS] = {8, 32, 64, 128};
constexpr int FSAI_BIN_LANES[FSAI_BINS] = {8, 16, 64, 64};
constexpr int FSAI_BIN_ROWS[FSAI_BINS] = {32, 16, 4, 2};  // rows per workgroup

inline int
fsai_bin_of(int s)
{
	int b = 0;
	while (s > FSAI_BIN_SMAX[b])
		b++;
	return b;
}

// the CSR of A (only entries with column <= row are read), the pattern, and the outputs, all on the device
struct FsaiArrays {
	const int * a_rp;
	const int * a_ci;
	const double * a_va;
	const int * p_rp;
	const int * p_ci;
	double * g;                       // G's values in the pattern's entry order
	int * fell_back;                  // n: 1 where the row took the breakdown rule
};

// the rows bin_rows[0 .. count) of one bin, enqueued on st
int launch_fsai_rows(int bin, const FsaiArrays & a, const int * bin_rows, long count, hipStream_t st);

}  // namespace spmv

struct spmv_mi355x_fsai {
	int precision = 0, device = 0, format = 0;
	bool f32 = false;
	long n = 0, nnz = 0, max_row = 0, fallback_rows = 0;
	double kernel_seconds = 0, download_seconds = 0, create_g_seconds = 0, create_gt_seconds = 0, setup_seconds = 0;
	std::vector<double> values;       // G's fp64 values in the pattern's entry order
	spmv_mi355x_matrix * G = nullptr, * Gt = nullptr;     // both NULL when n == 0
	void * d_scratch = nullptr;       // n values of the handle's precision: G in
	void * d_in = nullptr, * d_out = nullptr;             // the vectors of the host-buffer apply, allocated at its first call
	// apply_multi: n x multi_k values between the two SpMMs, and the blocks of the host-buffer form; they grow with the largest k seen
	void * d_scratch_multi = nullptr, * d_in_multi = nullptr, * d_out_multi = nullptr;
	int multi_k = 0, multi_host_k = 0;
};

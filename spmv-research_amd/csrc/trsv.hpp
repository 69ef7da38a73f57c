// Sparse triangular solve (include/spmv_mi355x.h "sparse triangular solve"): what trsv.hip (analysis, layout, C ABI) and
// kernels_trsv.hip (the two kernels) share.
//
// THE LAYOUT. Rows are permuted by (level, row): position p holds row perm[p], the positions of level l are
// [level_ptr[l], level_ptr[l + 1]). Every level is cut into slices of up to 64 consecutive positions, so a slice never straddles a
// level; the slices of level l are level_slice[l] .. level_slice[l + 1] - 1 and only the last of them can hold fewer than 64 rows.
// A slice of `lanes` rows and width w (the longest of its rows, counted in kept off-diagonal entries) stores w * lanes (value, column)
// pairs from slice_ptr[s] on, entry k of the slice's lane r at slice_ptr[s] + k * lanes + r: lane-per-row loads of one k are
// contiguous, a long row pads its own slice only, and a level of one row stores that row without padding. len[p] is the row's own
// entry count: the kernels stop there, padding is never read. diag[p] is the stored diagonal of row perm[p] in the handle's
// precision (absent under DIAG_UNIT); it is divided by, never inverted.
#pragma once

#include "common.hpp"

namespace spmv {

constexpr int TRSV_SLICE = 64;            // rows per slice = one wave
constexpr int TRSV_LEVEL_BLOCK = 256;     // threads per workgroup of the level kernel
constexpr int TRSV_CHAIN_BLOCK_MAX = 1024;
constexpr int TRSV_CHAIN_ROWS_DEFAULT = 256;      // profiles/r16_trsv.txt: 256 <= 64 < 1024 << 4096 on both large workloads
constexpr int TRSV_CHAIN_ROWS_MAX = 65536;

struct TrsvArrays {
	const void * val;                 // values in the handle's precision, slice by slice
	const int * col;
	const int64_t * slice_ptr;        // slices + 1
	const int * len;                  // n, by position
	const int * perm;                 // n, by position
	const void * diag;                // n, by position; nullptr under DIAG_UNIT
	const int * level_ptr;            // levels + 1
	const int * level_slice;          // levels + 1
};

// one launch of the plan
struct TrsvStep {
	int chain;                        // 1 = the levels [l0, l1) in one workgroup, 0 = level l0 with one lane per row
	int l0, l1;
	int pos0, rows, slice0;           // level steps: first position, rows and first slice of level l0
	int block;                        // chain steps: threads of the one workgroup
};

// b and x may be the same vector (b[i] is read by the one lane that writes x[i])
int launch_trsv_level(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st);
int launch_trsv_chain(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const void * b, void * x, hipStream_t st);

}  // namespace spmv

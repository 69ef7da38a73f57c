// ILU(0) on the device (include/spmv_mi355x.h "ILU(0)"): what ilu0.hip (checks, analysis, C ABI) and kernels_ilu0.hip (the two
// kernels) share.
//
// THE LAYOUT. The factor f lives in A's entry order, so the only arrays beside it are A's columns and, per row i, three entry
// positions: beg[i] <= dia[i] < end[i]. [beg[i], end[i]) are the entries of row i the factorization touches: the whole row for a
// global handle, the entries whose column lies in the row's block for a blocked one (columns ascend, so they are one run). dia[i] is
// the stored diagonal. The k steps of row i are the entries [beg[i], dia[i]); the entries of row k beyond its diagonal are
// (dia[k], end[k]). rows holds the row numbers sorted by (level, row); the positions of level l are [level_ptr[l], level_ptr[l + 1])
// on the host, one launch each from level 1 on.
#pragma once

#include <vector>

#include "common.hpp"

namespace spmv {

constexpr int ILU0_BLOCK = 256;           // threads per workgroup of both kernels
constexpr long ILU0_MAX_GRID = 2048;      // workgroups per launch: 8 resident workgroups of 256 threads on each of 256 CUs

struct Ilu0Arrays {
	const int * col;                  // nnz
	const int * beg, * dia, * end;    // n each: entry positions
	const int * rows;                 // n: the rows by (level, row)
	double * f;                       // nnz
	unsigned * breakdown;             // one word: the lowest row with a bad pivot, 0xffffffff = none
};

// f = src (skipped when src == f) and the pivots of the `count0` rows of level 0, which no level launch visits
int launch_ilu0_begin(const Ilu0Arrays & a, long nnz, const double * src, long count0, hipStream_t st);
// one level: the rows a.rows[pos0 .. pos0 + count), `lanes` lanes per row (4, 8, 16, 32 or 64)
int launch_ilu0_level(const Ilu0Arrays & a, long pos0, long count, int lanes, hipStream_t st);

}  // namespace spmv

struct spmv_mi355x_ilu0 {
	int device = 0;
	long n = 0, nnz = 0, nnz_dropped = 0, levels = 0, max_level_rows = 0;
	long block_rows = 0, blocks = 0;      // 0, 0: a global handle
	long factorizations = 0;
	std::vector<int32_t> level_ptr;       // levels + 1
	std::vector<int> level_lanes;         // levels
	spmv::Ilu0Arrays arr = {};
	void * owned[7] = {};                 // the device arrays behind arr
	double mem_footprint = 0;
};

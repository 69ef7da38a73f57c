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
//
// THE BLOCKED FORM (spmv_mi355x_trsv_create_blocked). The rows are cut into contiguous blocks of block_rows rows, the kept entries
// that couple two blocks are dropped, and every block has its own levels. The layout is the one above with the positions ordered by
// (block, level within the block, row): the levels are numbered through all blocks in that order, block b owns the levels
// block_level[b] .. block_level[b + 1] - 1, and since a slice never straddles a level it never straddles a block either. col holds
// the column WITHIN the block (j - b * block_rows): the one kernel of this form keeps its block's part of x in LDS and indexes it
// with the stored column.
#pragma once

#include <vector>

#include "common.hpp"

namespace spmv {

constexpr int TRSV_SLICE = 64;            // rows per slice = one wave
constexpr int TRSV_LEVEL_BLOCK = 256;     // threads per workgroup of the level kernel
constexpr int TRSV_CHAIN_BLOCK_MAX = 1024;
constexpr int TRSV_CHAIN_ROWS_DEFAULT = 256;      // profiles/r16_trsv.txt: 256 <= 64 < 1024 << 4096 on both large workloads
constexpr int TRSV_CHAIN_ROWS_MAX = 65536;
constexpr int TRSV_BLOCK_ROWS_DEFAULT = 4096;     // NOT from a sweep yet: profiles/r18_trsv_blocked.txt says what was measured
constexpr int TRSV_BLOCK_ROWS_MAX = 16384;        // 16384 fp64 values = 128 KiB of the 160 KiB of LDS a workgroup may declare
constexpr int TRSV_BLOCKED_THREADS_MAX = 1024;
constexpr int TRSV_UPDATE_BLOCK = 256;            // threads per workgroup of the two update_values kernels
constexpr long TRSV_UPDATE_MAX_GRID = 2048;       // their workgroups per launch, ILU0_MAX_GRID's rule: 8 x 256 threads on each of 256 CUs
constexpr unsigned TRSV_UPDATE_FINE = 0xffffffffu;        // the status word when no diagonal was refused; else the lowest bad row

struct TrsvArrays {
	const void * val;                 // values in the handle's precision, slice by slice
	const int * col;
	const int64_t * slice_ptr;        // slices + 1
	const int * len;                  // n, by position
	const int * perm;                 // n, by position
	const void * diag;                // n, by position; nullptr under DIAG_UNIT
	const int * level_ptr;            // levels + 1
	const int * level_slice;          // levels + 1
	const int * block_level;          // blocked handles: blocks + 1; else nullptr
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
// the whole solve of a blocked handle: `blocks` workgroups of `threads` threads, block_rows values of x in LDS each
int launch_trsv_blocked(bool f32, bool unit, const TrsvArrays & a, long blocks, int threads, long block_rows, long n, const void * b,
		void * x, hipStream_t st);

// K COLUMNS. One chunk of a k-column solve: the columns c0 .. c0 + kc - 1, kc in {8, 4, 2, 1}, of the row-major blocks b and x
// (row i at b + i * ldb and x + i * ldx, counted in values; b may be x when ldb == ldx). A chunk is one pass over the plan.
struct TrsvCols {
	const void * b;
	void * x;
	long ldb, ldx;
	int c0, kc;
};

constexpr long TRSV_LDS_BYTES = 160 * 1024;       // what a workgroup may declare: the window rule of the SpMM

int launch_trsv_level_multi(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const TrsvCols & c, hipStream_t st);
int launch_trsv_chain_multi(bool f32, bool unit, const TrsvArrays & a, const TrsvStep & s, const TrsvCols & c, hipStream_t st);
// min(block_rows, n) * kc values of x in LDS per workgroup: the caller keeps kc at or below trsv_blocked_kmax()
int launch_trsv_blocked_multi(bool f32, bool unit, const TrsvArrays & a, long blocks, int threads, long block_rows, long n,
		const TrsvCols & c, hipStream_t st);

// UPDATE_VALUES (kernels_trsv_update.hip). values = the caller's fp64 entries in the order of the CSR given to prepare; slot_src has
// `slots` entries (-1 = padding), diag_src n (nullptr under DIAG_UNIT). check does atomicMin(status, row) for every diagonal that is
// zero or not finite in the handle's precision; write returns at once when status names a row.
int launch_trsv_update_check(bool f32, const int * diag_src, const int * perm, const double * values, unsigned * status, long n,
		hipStream_t st);
int launch_trsv_update_write(bool f32, const int * slot_src, const int * diag_src, const double * values, void * val, void * diag,
		const unsigned * status, long slots, long n, hipStream_t st);

// JACOBI SWEEPS (kernels_trsv_sweeps.hip): T^-1 b approximated by a fixed number of sweeps x <- D^-1 (b - N x), T = D + N, over the
// same arrays. slice_pos (slices + 1 ints, slice_pos[slices] = n) is the first position of every slice; launch_trsv_sweep_map derives
// it on the device from level_ptr / level_slice (`levels` = the number of entries of those two arrays less one).
constexpr int TRSV_SWEEP_BLOCK = 256;             // threads per workgroup of the sweep kernel: four slices
constexpr int TRSV_SWEEPS_MAX = 1 << 20;

// One sweep over kc in {8, 4, 2, 1} columns (one launch). Row i of b is at b + i * ldb, of src at src + i * lds, of dst at
// dst + i * ldd, all three already at the chunk's first column. first: x = b / d (b under UNIT), neither src, val nor col is read,
// and when keep is not NULL row i of b is also copied to keep + i * kc (b may then be dst: the in-place solve saves its b here).
// Later sweeps: no lane writes what any lane of the launch gathers, so src must be neither dst nor b's alias of dst.
struct TrsvSweep {
	const void * b;
	const void * src;
	void * dst;
	void * keep;
	long ldb, lds, ldd;
	int kc;
	bool first;
};

int launch_trsv_sweep_map(const TrsvArrays & a, long levels, long slices, long n, int * slice_pos, hipStream_t st);
// block_rows = 0 for a global handle; else a stored column is block-local and the kernel adds the block's first row
int launch_trsv_sweep(bool f32, bool unit, const TrsvArrays & a, const int * slice_pos, long slices, long block_rows,
		const TrsvSweep & s, hipStream_t st);

// the widest chunk of a blocked handle: the largest KC in {8, 4, 2, 1} whose part of X fits in LDS
inline int
trsv_blocked_kmax(long block_rows, long n, bool f32)
{
	const long rows = block_rows < n ? block_rows : n;
	int kc = 8;
	while (kc > 1 && rows * kc * (f32 ? 4 : 8) > TRSV_LDS_BYTES)
		kc /= 2;
	return kc;
}

}  // namespace spmv

struct spmv_mi355x_trsv {
	int uplo = 0, diag = 0, precision = 0, device = 0;
	bool f32 = false;
	long n = 0, nnz_kept = 0, levels = 0, max_level_rows = 0;
	int chain_rows = 0;
	std::vector<spmv::TrsvStep> plan;     // global handles
	// blocked handles (block_rows > 0): one launch, no plan; levels = the most levels of any block
	long block_rows = 0, blocks = 0, nnz_dropped = 0;
	int threads = 0;
	spmv::TrsvArrays arr = {};
	void * owned[9] = {};                 // the device arrays behind arr
	void * d_b = nullptr, * d_x = nullptr;     // the vectors of the host-buffer solve, allocated at its first call
	void * d_bk = nullptr, * d_xk = nullptr;   // the n x block_k blocks of the host-buffer k-column solve, regrown for a larger k
	int block_k = 0;
	double mem_footprint = 0;
	long slices = 0, slots = 0;           // of the stored layout: slots = slice_ptr[slices] entries of val and col
	long nnz_csr = 0;                     // row_ptr[n] of the CSR given to create, then of the one given to update_values_prepare
	// update_values (trsv.hip): nothing below is allocated before update_values_prepare, none of it counts in mem_footprint
	int upd_state = 1;                    // 1 = prepare is missing, 2 = ready, 3 = the last update was refused
	int * upd_slot_src = nullptr, * upd_diag_src = nullptr;       // device: slots and n entries
	unsigned * upd_status = nullptr;      // device: 16 bytes, the first word is the status word
	std::vector<int32_t> upd_diag_entry;  // host, STORED: the entry of row i's diagonal, for the refusal's message
	double * upd_values = nullptr;        // device staging of the host form, allocated at its first call and kept
	hipEvent_t upd_done = nullptr;        // recorded behind the last async update
	const double * upd_last = nullptr;    // the values of the last async update (device), until its result was taken
	bool upd_pending = false;
	long upd_bad_row = -1;                // what the last result found: the refused row and its diagonal as given (-1: none)
	double upd_bad_value = 0;
	double upd_bytes = 0;
	// Jacobi sweeps (trsv.hip): nothing below is allocated before the first sweep solve, none of it counts in mem_footprint
	long levels_total = 0;                // entries of level_ptr less one: `levels` of a global handle, the sum over the blocks of a blocked one
	int sweeps = 0;                       // trsv_set_sweeps: 0 = the solve entries run the exact plan
	int * swp_slice_pos = nullptr;        // device: slices + 1
	void * swp_keep = nullptr, * swp_buf = nullptr;       // device: n x swp_k values each, regrown for a wider chunk
	int swp_k = 0;
	double swp_bytes = 0;
};

namespace spmv {

// What the host analysis of trsv.hip derives from a pattern; ilu0.hip takes its levels from the same two routines.
struct TrsvAnalysis {
	std::vector<int32_t> level_of_row;     // n
	std::vector<int32_t> level_ptr;        // levels + 1: positions of each level in the (level, row) order
	std::vector<int32_t> level_slice;      // levels + 1: slices of up to TRSV_SLICE rows, none straddling a level
	std::vector<TrsvStep> plan;
	long levels = 0, max_level_rows = 0;
	int chain_rows = 0;
	// the blocked plan: level_of_row, level_ptr and level_slice number the levels through all blocks, `levels` is their count
	std::vector<int32_t> block_level;      // blocks + 1
	long block_rows = 0, blocks = 0, max_block_levels = 0, nnz_dropped = 0;
};

// trsv.hip. 0 = fine, 1 = error set with the prefix `what`.
int trsv_check_pattern(const char * what, long n, const int32_t * rp, const int32_t * ci);
void trsv_analysis(int uplo, long n, const int32_t * rp, const int32_t * ci, int chain_rows, TrsvAnalysis & an);
void trsv_analysis_blocked(int uplo, long n, const int32_t * rp, const int32_t * ci, long block_rows, TrsvAnalysis & an);

}  // namespace spmv

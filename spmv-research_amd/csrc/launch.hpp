// Host-callable launchers of the HIP kernels (one translation unit per kernel family).
// All launchers enqueue on `stream` and return 0 / 1 (error text via spmv::set_error). `f32` selects float.
#pragma once

#include <vector>

#include "common.hpp"

namespace spmv {

struct LaunchCfg {
	XcdMap map;         // tile order over the 8 XCDs (built at conversion time for the kernel's tile geometry)
	int nt;             // nontemporal matrix streams
	int beta;           // 0: y = A x, 1: y += A x
	int unit;           // merge path: every stored value equals unit_value (pattern matrices: 1.0) and the value array is not kept
	double unit_value;
	int kahan;          // csr_scalar: Kahan-compensated row sums (csr.cpp:353-373)
};

// tile geometry of each kernel family (units per workgroup), needed to build the XCD map
inline long csr_scalar_rows_per_tile() { return 256; }
inline long csr_vector_rows_per_tile(int lanes_per_row, int rows_per_group = 1) { return 256L / lanes_per_row * rows_per_group; }
inline long csr_stream_rows_per_tile(int rows_per_wave) { return 4L * rows_per_wave; }
inline long sell_slices_per_tile() { return 4; }
inline long coo_waves_per_tile() { return 4; }

// ---- CSR (kernels_csr.hip)
int launch_csr_scalar(bool f32, const int * row_ptr, const int * col, const void * val, const void * x, void * y,
		int m, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);
int launch_csr_vector(bool f32, int lanes_per_row, int rows_per_group, const int * row_ptr, const int * col, const void * val,
		const void * x, void * y, int m, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// ---- CSR-Stream: one wavefront per block of R consecutive rows (kernels_csr_stream.hip)
int csr_stream_cap();                                                  // non-zeros a row block may hold on the LDS path
int launch_csr_stream(bool f32, int rows_per_wave, const int * row_ptr, const int * col, const void * val, const void * x, void * y,
		int m, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

int csr_stream_t_cap(int rows_per_wave);                               // same, transposed-consumption variant
int launch_csr_stream_t(bool f32, int rows_per_wave, const int * row_ptr, const int * col, const void * val, const void * x, void * y,
		int m, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

int csr_stream_d_cap(int rows_per_wave);
long csr_stream_d_rows_per_tile(int rows_per_wave);                    // rows per workgroup (workgroup size varies with R)                               // same, LDS-DMA variant
int launch_csr_stream_d(bool f32, int rows_per_wave, const int * row_ptr, const int * col, const void * val, const void * x, void * y,
		int m, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);
constexpr int STREAM_SLACK = 512;                                      // entries the LDS-DMA copy may read past a row block

// CSR with the block's x window in LDS (kernels_csr_window.hip)
int csr_window_lds_budget();                                           // bytes of LDS a block's window may take
int launch_csr_window(bool f32, int lanes_per_row, const int * row_ptr, const void * col, int col16, const void * val, const void * x, void * y,
		const int * blk_row, const int * blk_lo, const int * blk_w, int lds_bytes, const LaunchCfg & cfg, hipStream_t stream,
		long * grid_out);

// ---- merge-path CSR (kernels_merge.hip)
int merge_tile_items(bool f32, int items_per_thread);                 // merge items (rows + nnz) per workgroup
int launch_merge_search(const int * row_ptr, int m, int nnz, int tile_items, int num_tiles, int * coords /* [2*(num_tiles+1)] */,
		hipStream_t stream);
int launch_merge(bool f32, int items_per_thread, const int * row_ptr, const int * col, const void * val, const void * x, void * y,
		int m, int nnz, int num_tiles, const int * coords, int * carry_row, void * carry_val,
		const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// ---- SELL-C-sigma (kernels_sell.hip)
int launch_sell(bool f32, int C, const int64_t * slice_ptr, const int * col, const void * val, const int * row_of_sorted,
		const void * x, void * y, int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// SELL-64-sigma with delta-compressed column indices (desc: 2 int64 per slice + terminator, idx: byte stream)
// v7: the handle holds slices with 7-byte values (SELL_V7_FLAG below); launches the kernel variant that looks at the flag
int launch_sell_delta(bool f32, int waves_per_slice, bool v7, const int64_t * desc, const unsigned char * idx, const void * val, const int * row_of_sorted,
		const void * x, void * y, int m, int num_slices, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// SELL-64 with the slice group's x window in LDS and 16-bit window-relative indices (kernels_sell_window.hip)
int sell_window_lds_budget();
int launch_sell_window(bool f32, int waves_per_slice, int slices_per_group, const int * grp, const int64_t * sdesc, const unsigned short * idx,
		const void * val, const int * row_of_sorted, const void * x, void * y, int m, int lds_window_bytes, const LaunchCfg & cfg,
		hipStream_t stream, long * grid_out);

// the same layout holding ONE TRIANGLE of a symmetric matrix: y window in LDS beside the x window, mirrored entries as LDS atomics
int launch_sell_window_sym(bool f32, int waves_per_slice, int slices_per_group, const int * grp, const int64_t * sdesc, const unsigned short * idx,
		const void * val, const int * row_of_sorted, const void * x, void * y, int m, int lds_window_bytes, const LaunchCfg & cfg,
		hipStream_t stream, long * grid_out);

// Sensitivity experiments on the delta layout's index-free modes: SPMV_MI355X_SELL_MODES_OFF, bit 0 = no affine slices (mode 0),
// bit 1 = no per-slice lane offsets (mode 3), bit 2 = no lane offsets with exceptions (mode 5); such slices then store 8- / 16-bit
// deltas per lane. Read at every create().
inline int
sell_modes_off()
{
	const char * e = getenv("SPMV_MI355X_SELL_MODES_OFF");
	return e ? atoi(e) & 7 : 0;
}

// Where value (step k, lane r) of a 64-row slice of the delta layout lies behind the slice's first element: steps in pairs, a lane's steps
// 2p and 2p+1 side by side (kernels_sell.hip: sell_group_values); the last step of an odd width stands alone, one element per lane.
__host__ __device__ inline long
sell_pair_pos(long k, long width, long r)
{
	return (k | 1) < width ? (k / 2) * 128 + r * 2 + (k & 1) : (k / 2) * 128 + r;
}

// 7-byte fp64 values of the delta layout (sell_values). A slice whose stored values in its FULL groups of 4 steps (padding included) are
// all either exponent-0 values (+-0, denormals) or finite normals with biased exponent in [E0, E0 + 6] keeps each of them as a 56-bit
// record: sign (1 bit), exponent code c (3 bits: 0 = exponent field 0, 1..7 = E0 + c - 1), the 52 mantissa bits verbatim. Decoding gives
// back the same bits. A compressed group of 4 steps is 1792 bytes instead of 2048:
//     lo plane [64 lanes][4 dwords]   the low 32 bits of the lane's four values, as they are      (one dwordx4 per lane)
//     hi plane [64 lanes][3 dwords]   the four 24-bit high parts sign|c|mantissa[51:32], packed  (one dwordx3 per lane)
// The 1..3-step tail group stays in today's pairs (sell_pair_pos, relative to the tail's first word). Every slice starts on a multiple of
// 32 words (plain: 64 words per step; compressed: 224 per group, 64 per tail step), so desc[2s] stays an offset in 8-byte words and the
// slice's width follows from the difference of two offsets (sell_v7_width). desc[2s+1] carries the flag (bit 3, free: index blocks are
// 16-byte aligned) and E0 (bits 48..58) beside the index byte offset and the mode.
constexpr int SELL_V7_GROUP_WORDS = 224;                 // 8-byte words of one compressed group (1792 bytes)
constexpr int64_t SELL_V7_FLAG = 8;
constexpr int64_t SELL_IDX_MASK = 0x0000fffffffffff0LL;  // index byte offset of desc[2s+1]

__host__ __device__ inline int
sell_v7_e0(int64_t i_word)
{
	return (int) ((i_word >> 48) & 2047);
}

// width in steps of a compressed slice of `words` 8-byte words: 224 per full group, 64 per tail step (at most 3, 192 < 224)
__host__ __device__ inline long
sell_v7_width(int64_t words)
{
	return 4 * (words / SELL_V7_GROUP_WORDS) + (words % SELL_V7_GROUP_WORDS) / 64;
}

// the exponent range of a set of fp64 values: does it qualify, and with which E0
struct SellV7Range {
	int lo = 2047, hi = 0;                               // lowest / highest biased exponent of the normal values seen
	bool bad = false;                                    // an Inf or NaN
	__host__ __device__ void add(uint64_t bits)
	{
		const int e = (int) ((bits >> 52) & 2047);
		if (e == 2047)
			bad = true;
		else if (e)
		{
			lo = e < lo ? e : lo;
			hi = e > hi ? e : hi;
		}
	}
	__host__ __device__ bool ok() const { return !bad && (lo == 2047 || hi - lo <= 6); }
	__host__ __device__ int e0() const { return lo == 2047 ? 1 : lo; }    // no normal value at all: any E0 does
};

// the 24-bit high part of a value that qualifies for E0
__host__ __device__ inline unsigned
sell_v7_encode_hi(uint64_t bits, int e0)
{
	const unsigned e = (unsigned) (bits >> 52) & 2047u;
	const unsigned c = e ? e - (unsigned) e0 + 1u : 0u;
	return (unsigned) (bits >> 63) << 23 | c << 20 | ((unsigned) (bits >> 32) & 0xfffffu);
}

// ... and back to the value's high dword; bits 24..31 of `h` are ignored, k = (E0 - 1) << 20. Four 32-bit VALU operations.
__host__ __device__ inline unsigned
sell_v7_decode_hi(unsigned h, unsigned k)
{
	const unsigned a = h & 0x7fffffu;                    // c | mantissa[51:32]
	return (a < 0x100000u ? a : a + k) | ((h << 8) & 0x80000000u);
}

// byte position of the low / high part of value (step k < 4 * full groups, lane r) behind a compressed slice's first byte, and the word
// of its hi plane that holds bits [shift, shift + 24) of the packed high parts (shift 24 and 16 run into the next word)
__host__ __device__ inline long
sell_v7_lo_pos(long k, long r)
{
	return (k / 4) * 1792 + r * 16 + (k & 3) * 4;
}
__host__ __device__ inline long
sell_v7_hi_bit(long k, long r)
{
	return ((k / 4) * 1792 + 1024 + r * 12) * 8 + (k & 3) * 24;
}

// 7-byte values: SPMV_MI355X_SELL_VALUES = 0 (auto) | 1 (on) | 2 (off) overrides opts.sell_values; read at every create()
inline int
sell_values_env(int opt)
{
	const char * e = getenv("SPMV_MI355X_SELL_VALUES");
	return e ? atoi(e) : opt;
}

// whether a delta-layout handle looks for slices to store in 7 bytes: fp64, and on (1) or auto (0) with a plain value array of `nnz_ext`
// entries larger than the 256 MiB Infinity Cache (below that the values stay cache-resident from launch to launch: nothing to save)
inline bool
sell_v7_wanted(bool f32, int sell_values, int64_t nnz_ext)
{
	return !f32 && (sell_values == 1 || (sell_values == 0 && (double) nnz_ext * 8 > 256.0 * 1024 * 1024));
}

// ... and of the LDS-window layout, whose slices are padded to whole groups of 4 steps: 16 bytes per lane and load — fp64 as above,
// fp32 a lane's 4 steps of a group side by side (kernels_sell_window.hip: sellw_values)
__host__ __device__ inline long
sellw_val_pos(long k, long r, bool f32)
{
	return f32 ? (k / 4) * 256 + r * 4 + (k & 3) : (k / 2) * 128 + r * 2 + (k & 1);
}

// CSR -> SELL-64-sigma-delta on the GPU (convert_sell.hip); outputs are device arrays owned by the caller
// (sell_values: 0 = auto, 1 = on, 2 = off, sell_v7_wanted; nnz_ext_out = padded entries, val_words_out = stored value elements,
// v7_slices_out = slices with 7-byte values)
int sell_delta_convert_device(bool f32, long m, long n_cols, long nnz, long sigma, int sell_values, const int * rp_host, const int * ci_host,
		const double * va_host, int ** d_row_of_sorted_out, int64_t ** d_desc_out, unsigned char ** d_idx_out, void ** d_val_out,
		std::vector<int64_t> & val_ptr_host, long mode_counts[4], int64_t * nnz_ext_out, int64_t * idx_bytes_out, int64_t * val_words_out,
		long * v7_slices_out);

// the same on a CSR already resident in device memory (rp, ci, va are device pointers; va fp64)
int sell_delta_convert_resident(bool f32, long m, long n_cols, long nnz, long sigma, int sell_values, const int * rp, const int * ci,
		const double * va, int ** d_row_of_sorted_out, int64_t ** d_desc_out, unsigned char ** d_idx_out, void ** d_val_out,
		std::vector<int64_t> & val_ptr_host, long mode_counts[4], int64_t * nnz_ext_out, int64_t * idx_bytes_out, int64_t * val_words_out,
		long * v7_slices_out);
// the entry arrays of the column-blocked layout on the GPU (convert_coo.hip)
int blocked_entries_convert_device(bool f32, bool uniform, long m, long nnz, const int * rp_host, const int * ci_host, const double * va_host, long NR, int WGS, long CH,
		const std::vector<int> & range_row, const std::vector<int> & range_long, const std::vector<int> & long_row, const std::vector<int> & chunk_ptr,
		const std::vector<int> & chunk_row, const std::vector<int> & wg_rows, long SPAN, long BATCH, int slot_bits, int SPARE, long ghost_batches,
		std::vector<int> & batch_ptr, unsigned ** d_ent_out, void ** d_val_out, int ** d_batch_base_out);
// CSR -> the plain column-major SELL-C-sigma layout on the GPU (convert_sell.hip)
int sell_plain_convert_device(bool f32, long m, long nnz, int C, int TPR, long sigma, const int * rp_host, const int * ci_host, const double * va_host,
		int64_t ** d_slice_ptr_out, int ** d_col_out, void ** d_val_out, int ** d_row_of_sorted_out, std::vector<int64_t> & slice_ptr_host);
// CSR -> the LDS-window layout on the GPU (convert_sell.hip); 0 = built, 1 = error, 2 = a group's window is too wide
int sell_window_convert_device(bool f32, long m, long nnz, int NS, bool sym, long lds_budget_bytes, const int * rp_host, const int * ci_host,
		const double * va_host, int ** d_grp_out, int ** d_row_of_sorted_out, int64_t ** d_desc_out, unsigned short ** d_idx_out, void ** d_val_out,
		std::vector<int64_t> & desc_host, int * max_w_out);

// ---- COO (kernels_coo.hip)
int coo_wave_items(int items_per_lane);                                // entries per wavefront
int launch_coo(bool f32, int items_per_lane, const int * rowind, const int * col, const void * val, const void * x, void * y,
		int m, long nnz, int num_waves, int * carry_row, void * carry_val,
		const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// column-blocked COO for graph matrices: y of a workgroup's rows in LDS, entries ordered by column block, one dword per entry
int coo_blocked_rows_cap(bool f32);                                    // rows of y one workgroup can keep in LDS
int coo_blocked_wgs_per_range();                                       // workgroups a row range is dealt to (32 = CUs per XCD)
int coo_blocked_chunk_rows();                                          // rows per chunk of that round-robin deal (16)
int coo_blocked_batch_entries(bool unit);                              // entries of one batch of a workgroup (8 or 4 per lane)
int coo_blocked_spare_slots();                                         // LDS slots behind a workgroup's rows that padding entries add into
int coo_blocked_slot_bits();                                           // low bits of an entry that hold the LDS slot (the rest: column - base)
int coo_blocked_max_long_rows();                                       // rows per range that may be split over its workgroups
int launch_coo_blocked(bool f32, const int * wg_rows, const int * range_row, const int * chunk_ptr, const int * chunk_row, const int * batch_ptr, const int * batch_base,
		const int * range_long,
		const int * long_row, int num_long, const unsigned * ent, const void * val, const void * x, void * y, void * carry, int num_ranges,
		int chunk_rows, int lds_bytes, const LaunchCfg & cfg, hipStream_t stream, long * grid_out);

// ---- small utility kernels (kernels_csr.hip)
int launch_expand_rows(const int * row_ptr, int m, int * rowind, hipStream_t stream);   // CSR -> COO row indices (mkl_coo.cpp:79-90)

}  // namespace spmv

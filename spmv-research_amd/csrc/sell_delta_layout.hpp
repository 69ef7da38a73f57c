// The SELL-64-sigma-delta layout: the one definition of its bytes, for the host builder (build_sell.hip: build_sell_delta), the GPU
// builder (convert_sell.hip), the kernel (kernels_sell.hip: sell_delta_kernel) and the decoder (spmv_mi355x.hip: sell_layout).
//
// Rows are sorted by length inside windows of sigma rows (descending, stable); a slice is 64 consecutive sorted rows, one lane per row.
// Per slice two descriptor words (sell_desc_word), then a terminator (value words, index bytes | 4):
//     desc[2s]   = the slice's first value word; the slice's width follows from the difference of two (sell_slice_width)
//     desc[2s+1] = byte offset of its index block (16-byte aligned) | 7-byte values flag (bit 3) | mode (bits 0..2), E0 in bits 48..58
//
// INDICES: one int32 base per step and, by mode, something per lane, in groups of 4 steps covering the width rounded up to 4 (padding
// steps repeat a column some lane uses), so that a lane's four deltas are ONE dword (8-bit) / ONE dwordx2 (16-bit) load:
//     mode 0  affine, column = base_k + lane         group [4 x int32 base]                                         16 bytes
//     mode 3  lane offsets, column = base_k + off_l  header [64 x int32 off_l] (256 bytes), group [4 x int32 base]  16 bytes
//     mode 1  8-bit deltas                           group [4 x int32 base][64 lanes x 4 x u8]                     272 bytes
//     mode 2  16-bit deltas                          group [4 x int32 base][64 lanes x 4 x u16]                    528 bytes
//     mode 4  plain                                  group [4 steps][64 lanes] int32                              1024 bytes
//     mode 5  lane offsets with exceptions           header [64 x int32 off_l][u64 exception mask][8 bytes 0] (272 bytes),
//                                                    group [4 x int32 base][E x 4 x int8], padded to 16 bytes  32 .. 80 bytes
// Modes 0 / 3 need the 64 rows of a full slice equally long and of one pattern. Mode 5 needs them equally long, with base_k = the
// column of a reference lane (one of 0..3, mode byte md | ref << 3) and off_l = the lane's first column minus the reference's: the rows
// that follow that pattern (SELL5_MIN_REGULAR at the least) store nothing per step, the E <= 16 EXCEPTIONS a signed 8-bit correction
// per step (sell5_corr_pos). Any other slice takes the narrowest of modes 1 / 2 / 4 (sell_mode_byte).
//
// VALUES are stored in PAIRS of steps: a lane's steps 2p and 2p+1 side by side, [pair][lane][2], so that a group of 4 steps is TWO
// 16-byte loads per lane; the last step of an odd width stands alone (sell_pair_pos). Only the real steps are stored.
//
// 7-BYTE fp64 VALUES (sell_values): a slice whose values in its FULL groups of 4 steps (padding included) are all either exponent-0
// (+-0, denormals) or finite normals with biased exponent in [E0, E0 + 6] keeps each of them as a 56-bit record: sign, exponent code c
// (3 bits: 0 = exponent field 0, 1..7 = E0 + c - 1), the 52 mantissa bits verbatim; lossless. A compressed group is 1792 bytes, not 2048:
//     lo plane [64 lanes][4 dwords]   the low 32 bits of the lane's four values                 (one dwordx4 per lane)
//     hi plane [64 lanes][3 dwords]   the four 24-bit high parts sign|c|mantissa[51:32], packed  (one dwordx3 per lane; sell_v7_pack_hi)
// The 1..3-step tail group stays in pairs behind the full groups (sell_pair_slot). Every slice starts on a multiple of 32 words (plain:
// 64 words per step; compressed: 224 per group, 64 per tail step), so desc[2s] stays an offset in 8-byte words.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace spmv {

constexpr int SELL_DELTA_C = 64;                         // rows of a slice, one lane each
constexpr int SELL5_MIN_REGULAR = 48;                    // mode 5: rows of a slice that follow the pattern, at the least
constexpr int SELL_V7_GROUP_WORDS = 224;                 // 8-byte words of one compressed group (1792 bytes)
constexpr int64_t SELL_V7_FLAG = 8;
constexpr int64_t SELL_IDX_MASK = 0x0000fffffffffff0LL;  // index byte offset of desc[2s+1]

// ------------------------------------------------------------------------------------------------ indices
// bytes of one index group of 4 steps in mode `md` (mode 5: with `nex` exception lanes), of the slice header, of a slice of `width` steps
__host__ __device__ constexpr long sell_group_bytes(int md, unsigned nex = 0)
{
	return md == 5 ? 16 + (long) ((nex + 3) / 4 * 16) : (md == 0 || md == 3) ? 16 : md == 1 ? 272 : md == 2 ? 528 : 1024;
}
__host__ __device__ constexpr long sell_header_bytes(int md) { return md == 3 ? 4 * SELL_DELTA_C : md == 5 ? 4 * SELL_DELTA_C + 16 : 0; }
__host__ __device__ constexpr long sell_slice_idx_bytes(int md, unsigned nex, long width)
{
	return sell_header_bytes(md) + (width + 3) / 4 * sell_group_bytes(md, nex);
}

// mode 5 takes a reference lane whose pattern at least SELL5_MIN_REGULAR rows follow, with at least one exception and no row whose
// difference from the pattern needs more than a signed byte (`hard`)
__host__ __device__ constexpr bool sell5_accepts(int nex, bool hard) { return SELL_DELTA_C - nex >= SELL5_MIN_REGULAR && nex > 0 && !hard; }

// the mode byte md | ref << 3 of a slice: `affine` / `rowoff` = its rows follow mode 0's / mode 3's pattern, `ref` = mode 5's reference
// lane (-1: none), `maxdelta` = the widest spread of columns at a step. `modes_off` (sell_modes_off) forbids mode 0 (bit 0), mode 3 (bit 1);
// bit 2 (mode 5) is the caller's: it then finds no reference lane.
__host__ __device__ constexpr int sell_mode_byte(bool affine, bool rowoff, int ref, long maxdelta, int modes_off)
{
	return (affine && !(modes_off & 1)) ? 0 : (rowoff && !(modes_off & 2)) ? 3 : ref >= 0 ? 5 | ref << 3 : maxdelta < 256 ? 1
	       : maxdelta < 65536 ? 2 : 4;
}

// the bucket of spmv_mi355x_matrix::sell_mode_slices a slice of mode byte `mb` counts in: 8-bit, 16-bit, 32-bit indices, lane offsets
// (modes 0, 3, 5: no index bytes per lane and step)
__host__ __device__ constexpr int sell_mode_bucket(int mb)
{
	return ((mb & 7) == 0 || (mb & 7) == 3 || (mb & 7) == 5) ? 3 : (mb & 7) == 1 ? 0 : (mb & 7) == 2 ? 1 : 2;
}

// byte of the group that holds the mode-5 correction of step u of the exception lane of rank `rank`
__host__ __device__ constexpr long sell5_corr_pos(int rank, int u) { return 16 + 4 * rank + u; }

// ------------------------------------------------------------------------------------------------ descriptors
// desc[2s+1] of a slice whose index block starts at byte `idx_off`, in mode `md`, with 7-byte values of exponent base `e0` (0: plain),
// and its fields
__host__ __device__ constexpr int64_t sell_desc_word(int64_t idx_off, int md, int e0)
{
	return idx_off | md | (e0 ? SELL_V7_FLAG | (int64_t) e0 << 48 : 0);
}
__host__ __device__ constexpr int64_t sell_desc_idx(int64_t i_word) { return i_word & SELL_IDX_MASK; }
__host__ __device__ constexpr int sell_desc_mode(int64_t i_word) { return (int) (i_word & 7); }
__host__ __device__ constexpr bool sell_desc_v7(int64_t i_word) { return (i_word & SELL_V7_FLAG) != 0; }
__host__ __device__ constexpr int sell_v7_e0(int64_t i_word) { return (int) ((i_word >> 48) & 2047); }

// ------------------------------------------------------------------------------------------------ values
// width in steps of a compressed slice of `words` 8-byte words: 224 per full group, 64 per tail step (at most 3, 192 < 224)
__host__ __device__ constexpr long sell_v7_width(int64_t words) { return 4 * (words / SELL_V7_GROUP_WORDS) + (words % SELL_V7_GROUP_WORDS) / 64; }
// ... of any slice, `v7` = its desc[2s+1] has the 7-byte flag
__host__ __device__ constexpr long sell_slice_width(int64_t words, bool v7) { return v7 ? sell_v7_width(words) : words / SELL_DELTA_C; }

// value words of a slice of `width` steps whose first `full` groups of 4 steps hold 7-byte values (0: a plain slice)
__host__ __device__ constexpr int64_t sell_slice_val_words(long width, long full)
{
	return (int64_t) full * SELL_V7_GROUP_WORDS + (int64_t) (width - 4 * full) * SELL_DELTA_C;
}

// where value (step k, lane r) of a plain slice lies behind the slice's first element (steps in pairs, the last step of an odd width
// alone), and a step k >= 4 * full behind the `full` compressed groups of a slice with 7-byte values
__host__ __device__ constexpr long sell_pair_pos(long k, long width, long r)
{
	return (k | 1) < width ? (k / 2) * 128 + r * 2 + (k & 1) : (k / 2) * 128 + r;
}
__host__ __device__ constexpr long sell_pair_slot(long k, long width, long r, long full)
{
	return full * SELL_V7_GROUP_WORDS + sell_pair_pos(k, width, r) - full * 4 * SELL_DELTA_C;
}

// byte position of the low part of value (step k < 4 * full groups, lane r) behind a compressed slice's first byte, and the bit of its
// hi plane where the 24-bit high part starts
__host__ __device__ constexpr long sell_v7_lo_pos(long k, long r) { return (k / 4) * 1792 + r * 16 + (k & 3) * 4; }
__host__ __device__ constexpr long sell_v7_hi_bit(long k, long r) { return ((k / 4) * 1792 + 1024 + r * 12) * 8 + (k & 3) * 24; }

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

// a lane's four 24-bit high parts of a group packed into the three dwords of its hi-plane slot, and back (bits 24..31 of the unpacked
// parts are junk: sell_v7_decode_hi ignores them; the kernel unpacks with alignbit)
__host__ __device__ inline void
sell_v7_pack_hi(const unsigned (&h)[4], unsigned (&w)[3])
{
	w[0] = h[0] | h[1] << 24;
	w[1] = h[1] >> 8 | h[2] << 16;
	w[2] = h[2] >> 16 | h[3] << 8;
}
__host__ __device__ inline void
sell_v7_unpack_hi(unsigned w0, unsigned w1, unsigned w2, unsigned (&h)[4])
{
	h[0] = w0;
	h[1] = (unsigned) (((uint64_t) w1 << 32 | w0) >> 24);
	h[2] = (unsigned) (((uint64_t) w2 << 32 | w1) >> 16);
	h[3] = w2 >> 8;
}

// whether a delta-layout handle looks for slices to store in 7 bytes: fp64, and on (1) or auto (0) with a plain value array of `nnz_ext`
// entries larger than the 256 MiB Infinity Cache (below that the values stay cache-resident from launch to launch: nothing to save)
inline bool
sell_v7_wanted(bool f32, int sell_values, int64_t nnz_ext)
{
	return !f32 && (sell_values == 1 || (sell_values == 0 && (double) nnz_ext * 8 > 256.0 * 1024 * 1024));
}

}  // namespace spmv

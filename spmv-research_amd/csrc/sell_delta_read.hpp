// The readers of the SELL-64-sigma-delta layout (sell_delta_layout.hpp) that every kernel walking it shares: the value readers (pairs of
// steps, 7-byte records, the 1..3-step tail) and the index decoders of every mode. The single-vector kernels (kernels_sell.hip:
// sell_delta_kernel, sell_delta_split_kernel) and the multi-vector one (kernels_sell_spmm.hip: sell_delta_spmm_kernel) decode a slice
// with these and nothing else, so that both read the same columns and values in the same order.
#pragma once

#include "launch.hpp"

namespace spmv {

typedef int sell_int4 __attribute__((ext_vector_type(4)));
typedef unsigned sell_uint2 __attribute__((ext_vector_type(2)));

// VALUES of a slice are stored in PAIRS of steps (sell_pair_pos), so that a group of 4 steps is TWO 16-byte loads per lane (fp64;
// global_load_dwordx4) instead of four 8-byte ones. The kernel sits at the issue rate of its vector-memory instructions (4 value loads
// + 4 gathers per group: with the value loads at half the count the nlpkkt240 twin runs 9 % faster on the same bytes,
// profiles/r03_sell_value_pairs.txt). `vp` = the group's first element + 2 * lane.
// S is the type the values are STORED in, T the type the kernel computes in. S = float under T = double (opts.value_storage: fp32
// values under fp64 vectors) reads the fp32 pair layout, two 8-byte loads per group, and widens the four values (v_cvt_f64_f32,
// exact); everything behind the reader is the fp64 kernel's.
template <typename T, bool NT, typename S = T>
__device__ __forceinline__ void
sell_group_values(const S * __restrict__ vp, T (&v)[4])
{
	typedef S S2 __attribute__((ext_vector_type(2)));
	const S2 w0 = ld_stream<NT>(reinterpret_cast<const S2 *>(vp));
	const S2 w1 = ld_stream<NT>(reinterpret_cast<const S2 *>(vp + 2 * WAVE));
	v[0] = w0.x;
	v[1] = w0.y;
	v[2] = w1.x;
	v[3] = w1.y;
}

// the 1..3 real steps of a slice's last group
template <typename T, bool NT, int NSTEPS, typename S = T>
__device__ __forceinline__ void
sell_tail_values(const S * __restrict__ vp, int lane, T (&v)[3])
{
	typedef S S2 __attribute__((ext_vector_type(2)));
	v[1] = v[2] = T(0);
	if (NSTEPS == 1)
		v[0] = ld_stream<NT>(vp - lane);
	else
	{
		const S2 w0 = ld_stream<NT>(reinterpret_cast<const S2 *>(vp));
		v[0] = w0.x;
		v[1] = w0.y;
		if (NSTEPS == 3)
			v[2] = ld_stream<NT>(vp + 2 * WAVE - lane);
	}
}

typedef unsigned sell_uint4 __attribute__((ext_vector_type(4)));
typedef unsigned sell_uint3 __attribute__((ext_vector_type(3), aligned(4)));     // 12 bytes, one global_load_dwordx3

__device__ __forceinline__ double
sell_v7_value(unsigned h, unsigned k, unsigned lo)
{
	return __builtin_bit_cast(double, (unsigned long long) sell_v7_decode_hi(h, k) << 32 | lo);
}

// Where a slice's values come from. V7 = false: the pairs above. V7 = true (fp64, sell_values; layout: sell_delta_layout.hpp): a full group is the
// lane's dwordx4 of low halves and dwordx3 of packed 24-bit high parts — as many load instructions as the pairs, 1792 bytes instead of
// 2048 — decoded with a few 32-bit VALU operations on the high dwords only; the 1..3-step tail group is stored as pairs, behind the
// slice's full groups. `vp` = the slice's first value word + 2 * lane either way, `k` = (E0 - 1) << 20. S: the stored type (above).
template <typename T, bool NT, bool V7, typename S = T>
struct SellVals {
	const S * vp;
	int lane;
	unsigned k;
	__device__ __forceinline__ void group(int g, T (&v)[4]) const
	{
		if constexpr (!V7)
			sell_group_values<T, NT, S>(vp + (size_t) g * 4 * WAVE, v);
		else
		{
			static_assert(sizeof(T) == 8 && sizeof(S) == 8, "7-byte values are fp64 only");
			const unsigned char * b = reinterpret_cast<const unsigned char *>(vp) + (size_t) g * (8 * SELL_V7_GROUP_WORDS);  // lo plane + 16 * lane
			const sell_uint4 lo = ld_stream<NT>(reinterpret_cast<const sell_uint4 *>(b));
			const sell_uint3 * hp = reinterpret_cast<const sell_uint3 *>(b + 1024 - 4 * lane);                   // hi plane + 12 * lane
			sell_uint3 hi;
			if constexpr (NT)
				hi = __builtin_nontemporal_load(hp);
			else
				hi = *hp;
			v[0] = sell_v7_value(hi.x, k, lo.x);                                           // sell_v7_unpack_hi, as alignbit
			v[1] = sell_v7_value(__builtin_amdgcn_alignbit(hi.y, hi.x, 24), k, lo.y);
			v[2] = sell_v7_value(__builtin_amdgcn_alignbit(hi.z, hi.y, 16), k, lo.z);
			v[3] = sell_v7_value(hi.z >> 8, k, lo.w);
		}
	}
	// the group `g` (= the number of full groups) that holds the slice's 1..3 last steps: vp-relative as sell_tail_values wants it
	__device__ __forceinline__ const S * tail(int g) const { return vp + (size_t) g * (V7 ? SELL_V7_GROUP_WORDS : 4 * WAVE); }
};

// Modes 1 and 2 put a dependent load in front of every gather (deltas -> column -> x): their index words are fetched one pair of
// groups AHEAD, so that a trip costs one exposed round trip (the gathers) like the index-free modes, not two.
template <int MODE>
struct SellDeltaIdx {
	sell_int4 base;
	sell_uint2 d;                                  // MODE 1 uses d.x only
};

template <int MODE, bool NT>
__device__ __forceinline__ void
sell_delta_load_idx(SellDeltaIdx<MODE> & q, const unsigned char * __restrict__ gp /* uniform */, int lane)
{
	q.base = *reinterpret_cast<const sell_int4 *>(gp);
	if constexpr (MODE == 1)
		q.d.x = ld_stream<NT>(reinterpret_cast<const unsigned *>(gp + 16) + lane);
	else
		q.d = ld_stream<NT>(reinterpret_cast<const sell_uint2 *>(gp + 16) + lane);
}

template <int MODE>
__device__ __forceinline__ void
sell_delta_cols(const SellDeltaIdx<MODE> & q, int (&c)[4])
{
	if constexpr (MODE == 1)
	{
		c[0] = q.base.x + (int) (q.d.x & 255u);
		c[1] = q.base.y + (int) ((q.d.x >> 8) & 255u);
		c[2] = q.base.z + (int) ((q.d.x >> 16) & 255u);
		c[3] = q.base.w + (int) (q.d.x >> 24);
	}
	else
	{
		c[0] = q.base.x + (int) (q.d.x & 0xffffu);
		c[1] = q.base.y + (int) (q.d.x >> 16);
		c[2] = q.base.z + (int) (q.d.y & 0xffffu);
		c[3] = q.base.w + (int) (q.d.y >> 16);
	}
}

// MODE 5: lane offsets WITH EXCEPTIONS (layout: sell_delta_layout.hpp). Modes 0 and 3 need all 64 rows of a slice to follow one
// pattern; one row out of line (a boundary row of a stencil, a perturbed row) used to send the whole slice back to 8/16-bit deltas per
// lane and step. Here the rows out of line add a signed 8-bit correction per step. An exception lane loads its four corrections as ONE
// dword (sell5_corr_pos); the other lanes load the first exception's (one address for all of them) and drop it. (A first version stored the exception lanes' columns as
// 4 x int32 and loaded them with a dwordx4 per lane: 1 447 us on the 5 %-jittered nlpkkt240 twin against 1 425 us for plain 8/16-bit
// deltas although it moves 7 % fewer bytes — the wide load of all 64 lanes cost more than the bytes saved.) That load sits in front
// of the lane's gathers, so it is fetched one pair of groups ahead like the delta words of modes 1 / 2. Same FMAs in the same order
// as every other mode: bit-identical results.
// Slices with at most FOUR exception rows (the common case: 5 % of the rows out of line puts 3.2 into a slice on average) take the
// corrections through the SCALAR cache instead: the 16 bytes behind the bases hold all of them, one s_load brings bases and corrections,
// and a compare-and-select per exception puts its dword into its lane — no vector-memory instruction at all for the indices, as in modes 0 / 3.
// (The kernel runs at the issue rate of its vector-memory instructions: the per-lane dword load of the general path is a ninth
// instruction per group of 4 steps beside 2 value loads and 4 gathers.)
struct SellDeltaIdx5 {
	sell_int4 base;                                // wave-uniform
	unsigned d;                                    // 4 x int8, exception lanes only            (general path)
	sell_int4 corr;                                // corrections of exceptions 0..3, uniform   (scalar path)
};

// `rank` is 0 for the lanes that are no exception: they load the first exception's corrections (one address for all of them) and drop
// them. No branch around the load: with one the compiler cannot count what is outstanding and waits for everything at every trip.
template <bool NT, bool SCALAR>
__device__ __forceinline__ void
sell_delta_load_idx5(SellDeltaIdx5 & q, const unsigned char * __restrict__ gp /* uniform */, int rank)
{
	q.base = *reinterpret_cast<const sell_int4 *>(gp);
	if constexpr (SCALAR)
		q.corr = *reinterpret_cast<const sell_int4 *>(gp + 16);
	else
		q.d = ld_stream<NT>(reinterpret_cast<const unsigned *>(gp + 16) + rank);
}

template <bool SCALAR>
__device__ __forceinline__ void
sell_delta_cols5(const SellDeltaIdx5 & q, bool ex, int lane, int off, const int (&xl)[4], int (&c)[4])
{
	int d;
	if constexpr (SCALAR)
	{
		// exception j's dword into its lane; slots past the slice's last exception name a lane that is none and hold zeros (a spare lane keeps 0)
		d = lane == xl[0] ? q.corr.x : 0;
		d = lane == xl[1] ? q.corr.y : d;
		d = lane == xl[2] ? q.corr.z : d;
		d = lane == xl[3] ? q.corr.w : d;
	}
	else
		d = ex ? (int) q.d : 0;
	c[0] = q.base.x + off + ((d << 24) >> 24);
	c[1] = q.base.y + off + ((d << 16) >> 24);
	c[2] = q.base.z + off + ((d << 8) >> 24);
	c[3] = q.base.w + off + (d >> 24);
}

// the four columns of lane `lane` in the index group at `gp` (uniform) of a slice in mode 0..4, loaded and decoded in place (`off`: the
// lane offset of modes 0 / 3, = lane in mode 0)
template <int MODE, bool NT>
__device__ __forceinline__ void
sell_group_cols(const unsigned char * __restrict__ gp /* uniform */, int lane, int off, int (&c)[4])
{
	static_assert(MODE >= 0 && MODE <= 4, "mode 5 has its own reader (sell_delta_load_idx5, sell_delta_cols5)");
	if constexpr (MODE == 0 || MODE == 3)
	{
		// step-invariant lane offsets: column of lane l at step k = base_k + off_l. MODE 0 (affine slice: 64 consecutive rows of
		// a stencil diagonal) has off_l = l; MODE 3 stores the 64 offsets once per slice (rows of one kind that are not
		// consecutive). Either way no per-step index bytes per lane, one scalar base per step.
		const sell_int4 base = *reinterpret_cast<const sell_int4 *>(gp);
		c[0] = base.x + off;
		c[1] = base.y + off;
		c[2] = base.z + off;
		c[3] = base.w + off;
	}
	else if constexpr (MODE == 1 || MODE == 2)
	{
		SellDeltaIdx<MODE> q;
		sell_delta_load_idx<MODE, NT>(q, gp, lane);
		sell_delta_cols<MODE>(q, c);
	}
	else
	{
		const int * cp = reinterpret_cast<const int *>(gp) + lane;
		c[0] = ld_stream<NT>(cp);
		c[1] = ld_stream<NT>(cp + WAVE);
		c[2] = ld_stream<NT>(cp + 2 * WAVE);
		c[3] = ld_stream<NT>(cp + 3 * WAVE);
	}
}

// what a lane of a mode-5 slice with exception mask `mask` (uniform) needs to decode its columns: whether it is an exception, its rank
// among them (0 for the others), and with SCALAR the lanes of exceptions 0..3 (slots past the last exception name a spare lane)
template <bool SCALAR>
struct Sell5Lane {
	bool ex;
	int rank;
	int xl[4];
	__device__ __forceinline__ Sell5Lane(unsigned long long mask, int lane)
	{
		ex = (mask >> lane) & 1ull;
		rank = ex ? __popcll(mask & ((1ull << lane) - 1ull)) : 0;
		xl[0] = xl[1] = xl[2] = xl[3] = 0;
		if constexpr (SCALAR)
		{
			unsigned long long mm = mask;
			const int spare = __builtin_ctzll(~mask);                       // a lane that is no exception (at least 48 are not)
			#pragma unroll
			for (int j = 0; j < 4; j++)
			{
				xl[j] = mm ? __builtin_ctzll(mm) : spare;
				mm &= mm - 1ull;
			}
		}
	}
};

}  // namespace spmv

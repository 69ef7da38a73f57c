// decode(encode(v)) of the 7-byte fp64 values of the SELL delta layout (csrc/sell_delta_layout.hpp) and their qualification rule, and
// the layout's size, descriptor and packing helpers, on the host: compiled and run by tests/test_sell_values_codec.py
#include <cstdio>
#include <cstring>
#include <random>

#include "sell_delta_layout.hpp"

using spmv::SellV7Range;

static uint64_t rng_bits(std::mt19937_64 & g, int e)
{
	return (g() & 0x800fffffffffffffULL) | (uint64_t) e << 52;
}

// what the kernel does: the lane's three hi dwords unpacked with alignbit (junk above bit 23), decoded, joined with the lo dword
static uint32_t alignbit(uint32_t hi, uint32_t lo, int s) { return (uint32_t) ((((uint64_t) hi << 32) | lo) >> s); }

static int check_group(const uint64_t (&v)[4], int e0)
{
	uint32_t h[4];
	for (int u = 0; u < 4; u++)
		h[u] = spmv::sell_v7_encode_hi(v[u], e0);
	if ((h[0] | h[1] | h[2] | h[3]) >> 24)
		return 1;
	const uint32_t d0 = h[0] | h[1] << 24, d1 = h[1] >> 8 | h[2] << 16, d2 = h[2] >> 16 | h[3] << 8;
	const uint32_t got[4] = {d0, alignbit(d1, d0, 24), alignbit(d2, d1, 16), d2 >> 8};
	const unsigned k = (unsigned) (e0 - 1) << 20;
	for (int u = 0; u < 4; u++)
		if (((uint64_t) spmv::sell_v7_decode_hi(got[u], k) << 32 | (uint32_t) v[u]) != v[u])
			return 1;
	return 0;
}

// the size, descriptor and packing helpers of the layout against the numbers its description gives
static long check_layout_helpers(std::mt19937_64 & g)
{
	long bad = 0;
	const long want[5] = {16, 272, 528, 16, 1024};
	for (int md = 0; md < 5; md++)
		if (spmv::sell_group_bytes(md) != want[md])
		{
			printf("group bytes of mode %d: %ld\n", md, spmv::sell_group_bytes(md));
			bad++;
		}
	for (unsigned e = 1; e <= 16; e++)
		if (spmv::sell_group_bytes(5, e) != 16 + 16 * (long) ((e + 3) / 4) || spmv::sell_group_bytes(5, e) < 32 || spmv::sell_group_bytes(5, e) > 80)
		{
			printf("group bytes of mode 5 with %u exceptions: %ld\n", e, spmv::sell_group_bytes(5, e));
			bad++;
		}
	bad += spmv::sell_group_bytes(5, 1) != 32 || spmv::sell_group_bytes(5, 16) != 80;
	bad += spmv::sell_header_bytes(0) != 0 || spmv::sell_header_bytes(3) != 256 || spmv::sell_header_bytes(5) != 272;
	// desc[2s+1]: index offset (16-byte aligned, up to 48 bits), mode, 7-byte flag, E0
	const int e0s[] = {0, 1, 2, 1023, 2045, 2046};
	for (int t = 0; t < 100000; t++)
	{
		const int64_t off = t < 2 ? (t ? 0x0000fffffffffff0LL : 0) : (int64_t) (g() & 0x0000fffffffffff0ULL);
		const int md = (int) (g() % 6);
		const int e0 = t < 6 * 6 ? e0s[t % 6] : (g() & 1) ? 0 : 1 + (int) (g() % 2046);
		const int64_t w = spmv::sell_desc_word(off, md, e0);
		if (spmv::sell_desc_idx(w) != off || spmv::sell_desc_mode(w) != md || spmv::sell_desc_v7(w) != (e0 != 0) ||
		    (e0 && spmv::sell_v7_e0(w) != e0))
		{
			if (bad < 20)
				printf("desc word: off %lld mode %d E0 %d\n", (long long) off, md, e0);
			bad++;
		}
	}
	// a slice's width from its value words, plain and 7-byte
	for (long w = 0; w <= 40; w++)
	{
		bad += spmv::sell_slice_width(spmv::sell_slice_val_words(w, 0), false) != w;
		bad += spmv::sell_slice_width(spmv::sell_slice_val_words(w, w / 4), true) != w;
	}
	// the three packed hi dwords of a lane hold each high part at the bits sell_v7_hi_bit names; unpacking gives them back
	for (int t = 0; t < 100000; t++)
	{
		const long r = (long) (g() % 64);
		unsigned h[4], w[3], back[4];
		for (int u = 0; u < 4; u++)
			h[u] = (unsigned) g() & 0xffffffu;
		spmv::sell_v7_pack_hi(h, w);
		unsigned char plane[1792] = {};
		memcpy(plane + spmv::sell_v7_hi_bit(0, r) / 8, w, 12);
		unsigned char bytes[1792] = {};
		for (int u = 0; u < 4; u++)
			for (int b = 0; b < 24; b += 8)
				bytes[(spmv::sell_v7_hi_bit(u, r) + b) / 8] = (unsigned char) (h[u] >> b);
		spmv::sell_v7_unpack_hi(w[0], w[1], w[2], back);
		bool ok = memcmp(plane, bytes, sizeof(plane)) == 0;
		for (int u = 0; u < 4; u++)
			ok = ok && (back[u] & 0xffffffu) == h[u];
		if (!ok)
		{
			if (bad < 20)
				printf("hi plane: lane %ld packs differently\n", r);
			bad++;
		}
	}
	return bad;
}

int main()
{
	std::mt19937_64 g(7);
	long bad = 0, groups = 0, said_no = 0;
	// every E0 with every exponent it covers, +-0 and denormals, random signs and mantissas
	for (int e0 = 1; e0 <= 2046; e0++)
		for (int rep = 0; rep < 64; rep++)
		{
			uint64_t v[4];
			SellV7Range r;
			for (int u = 0; u < 4; u++)
			{
				const int pick = (int) (g() % 10);
				const int e = pick == 0 ? 0 : std::min(2046, e0 + (int) (g() % 7));
				v[u] = pick == 1 ? (g() & 0x8000000000000000ULL) : rng_bits(g, e);      // +-0, denormal (e = 0), normal
				r.add(v[u]);
			}
			if (!r.ok() || (r.lo != 2047 && r.e0() < e0))
			{
				if (bad < 20)
					printf("qualify: values within [%d, %d] refused or E0 %d below them\n", e0, e0 + 6, r.e0());
				bad++;
			}
			bad += check_group(v, e0);                       // any E0 whose range holds the values decodes them
			bad += check_group(v, r.e0());
			groups += 2;
		}
	// random sets over all exponents, Inf and NaN: the rule says yes exactly when every normal lies within 7 binades and nothing is Inf/NaN
	for (int t = 0; t < 2000000; t++)
	{
		const int n = 1 + (int) (g() % 8);
		const int spread = (int) (g() % 10);
		const int base = 1 + (int) (g() % 2046);
		uint64_t v[8];
		int lo = 4096, hi = -1;
		bool special = false;
		for (int i = 0; i < n; i++)
		{
			const int pick = (int) (g() % 40);
			int e = std::min(2046, base + (int) (g() % (spread + 1)));
			if (pick == 0)
				e = 2047;                                      // Inf (mantissa 0) or NaN
			else if (pick == 1)
				e = 0;
			v[i] = rng_bits(g, e);
			if (pick == 0 && (g() & 1))
				v[i] &= 0xfff0000000000000ULL;
			if (e == 2047)
				special = true;
			else if (e)
			{
				lo = std::min(lo, e);
				hi = std::max(hi, e);
			}
		}
		SellV7Range r;
		for (int i = 0; i < n; i++)
			r.add(v[i]);
		const bool want = !special && (hi < 0 || hi - lo <= 6);
		if (r.ok() != want)
		{
			if (bad < 20)
				printf("qualify: set %d says %d, must say %d\n", t, (int) r.ok(), (int) want);
			bad++;
		}
		said_no += !r.ok();
		if (r.ok())
			for (int i = 0; i + 4 <= n; i += 4)
			{
				const uint64_t q[4] = {v[i], v[i + 1], v[i + 2], v[i + 3]};
				bad += check_group(q, r.e0());
				groups++;
			}
	}
	// the width of a compressed slice from its word count
	for (long w = 0; w < 4000; w++)
		if (spmv::sell_v7_width((w / 4) * spmv::SELL_V7_GROUP_WORDS + (w % 4) * 64) != w)
			bad++;
	bad += check_layout_helpers(g);
	printf("groups %ld, sets refused %ld, failures %ld\n", groups, said_no, bad);
	return bad != 0;
}

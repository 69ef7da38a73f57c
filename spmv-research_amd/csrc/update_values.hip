// New values for an existing handle (include/spmv_mi355x.h "new values for an existing handle"): same pattern, new numbers.
//
// Everything create() derives from the PATTERN stays: the sigma-window sort, the index modes and their bytes, the LDS-window groups,
// the tile maps, the uploaded column indices, the placement of the arrays. What is rewritten is the stored value array, at the
// positions the layout headers define (sell_delta_layout.hpp, launch.hpp: sellw_val_pos, slice_ptr + k * C + lane), and, for a delta
// handle that looks for 7-byte slices, what follows from the values: the per-slice selection (sell_values_device.hpp: the builder's
// own code), the value offsets, the flag / E0 fields of the descriptors, and on the host the counts, the tile map, the footprint and
// the name. The contract: the handle ends up byte for byte what create() gives for the new values.
//
// The kernels read nnz * 8 bytes and write the value array once. CSR-ordered layouts: one streaming pass, 16-byte loads and stores.
// SELL layouts: one wave per 64-row slice, one lane per row. A lane that walks its own CSR row reads with a stride of one row length;
// where the rows of a slice are one contiguous stretch of the CSR array that fits the wave's share of LDS, the wave copies the stretch
// with coalesced loads and the lanes walk their rows in LDS instead (SliceValues). SPMV_MI355X_UPDATE_STAGE = 0 / 1 picks the variant.

#include <hipcub/hipcub.hpp>

#include "handle.hpp"
#include "sell_values_device.hpp"

namespace spmv {

constexpr int UPD_BLOCK = 256;
constexpr int UPD_WAVES = UPD_BLOCK / WAVE;
constexpr int UPD_STAGE_CAP = 2048;                     // fp64 values a wave may stage: 4 waves x 16 KiB = the 64 KiB of static LDS

static bool
update_stage_setting()
{
	const char * e = getenv("SPMV_MI355X_UPDATE_STAGE");
	return e ? atoi(e) != 0 : true;
}

// ------------------------------------------------------------------------------------------------ CSR-ordered value arrays
// dst[i] = (T) src[i]; four values per thread. ALIGNED: src is 16-byte aligned (dst, a device allocation, always is).
// differs (merge path; may be nullptr): set when some narrowed value is not the first one (values_uniform on the device)
template <typename T, bool ALIGNED>
__global__ __launch_bounds__(UPD_BLOCK) void
stream_values_kernel(const double * __restrict__ src, T * __restrict__ dst, long n, int * __restrict__ differs)
{
	typedef double D2 __attribute__((ext_vector_type(2)));
	typedef T T2 __attribute__((ext_vector_type(2)));
	typedef T T4 __attribute__((ext_vector_type(4)));
	const long i = ((long) blockIdx.x * UPD_BLOCK + threadIdx.x) * 4;
	if (i >= n)
		return;
	double v[4] = {0, 0, 0, 0};
	const int cnt = n - i >= 4 ? 4 : (int) (n - i);
	if (ALIGNED && cnt == 4)
	{
		const D2 a = __builtin_nontemporal_load(reinterpret_cast<const D2 *>(src + i));
		const D2 b = __builtin_nontemporal_load(reinterpret_cast<const D2 *>(src + i) + 1);
		v[0] = a.x;
		v[1] = a.y;
		v[2] = b.x;
		v[3] = b.y;
	}
	else
		for (int u = 0; u < cnt; u++)
			v[u] = src[i + u];
	if (cnt == 4)
	{
		if constexpr (sizeof(T) == 8)
		{
			T2 a, b;
			a.x = v[0];
			a.y = v[1];
			b.x = v[2];
			b.y = v[3];
			reinterpret_cast<T2 *>(dst + i)[0] = a;
			reinterpret_cast<T2 *>(dst + i)[1] = b;
		}
		else
		{
			T4 a;
			a.x = (T) v[0];
			a.y = (T) v[1];
			a.z = (T) v[2];
			a.w = (T) v[3];
			*reinterpret_cast<T4 *>(dst + i) = a;
		}
	}
	else
		for (int u = 0; u < cnt; u++)
			dst[i + u] = (T) v[u];
	if (differs)
	{
		const T t0 = (T) src[0];
		bool d = false;
		for (int u = 0; u < cnt; u++)
			d = d || (T) v[u] != t0;
		if (d)
			*differs = 1;
	}
}

// ------------------------------------------------------------------------------------------------ the values of a slice's rows
// Where lane `lane` of a wave finds value k of its CSR row (start, len): in global memory, or in the wave's LDS strip after
// slice_values() copied the slice's stretch of the CSR array there.
struct SliceValues {
	const double * va;
	const double * lds;
	int start, rel;
	bool staged;
	__device__ __forceinline__ double operator()(int k) const { return staged ? lds[rel + k] : va[start + k]; }
};

// Every thread of the workgroup calls this (it holds a barrier when STAGE). The rows of the wave's slice are disjoint stretches of
// the CSR array, so they tile [s0, s1) exactly when their lengths add up to s1 - s0.
template <bool STAGE>
__device__ __forceinline__ SliceValues
slice_values(const double * __restrict__ va, double * lds_wave, int start, int len, int lane)
{
	SliceValues sv;
	sv.va = va;
	sv.lds = lds_wave;
	sv.start = start;
	sv.rel = 0;
	sv.staged = false;
	if constexpr (STAGE)
	{
		typedef double D2 __attribute__((ext_vector_type(2)));
		const int s0 = wave_min_i(len > 0 ? start : 0x7fffffff);
		const int s1 = wave_max_i(len > 0 ? start + len : 0);
		int total = len;
		for (int o = WAVE / 2; o > 0; o >>= 1)
			total += __shfl_xor(total, o, WAVE);
		const int S = s1 - s0;
		sv.staged = S > 0 && total == S && S <= UPD_STAGE_CAP;
		if (sv.staged)
		{
			const double * g = va + s0;
			const int head = (int) ((reinterpret_cast<uintptr_t>(g) >> 3) & 1);      // elements in front of the first 16-byte boundary
			const int pairs = (S - head) / 2;
			if (lane == 0 && head)
				lds_wave[0] = g[0];
			for (int p = lane; p < pairs; p += WAVE)
			{
				const D2 w = __builtin_nontemporal_load(reinterpret_cast<const D2 *>(g + head) + p);
				lds_wave[head + 2 * p] = w.x;
				lds_wave[head + 2 * p + 1] = w.y;
			}
			if (lane == 0 && head + 2 * pairs < S)
				lds_wave[S - 1] = g[S - 1];
			sv.rel = start - s0;
		}
		__syncthreads();
	}
	return sv;
}

#define UPD_LDS_STRIP(STAGE, ptr)                                                  \
	double * ptr = nullptr;                                                    \
	if constexpr (STAGE)                                                       \
	{                                                                          \
		__shared__ double upd_lds[UPD_WAVES][UPD_STAGE_CAP];               \
		ptr = upd_lds[threadIdx.x / WAVE];                                 \
	}

// ------------------------------------------------------------------------------------------------ SELL delta layout
// 7-byte selection of every slice (what slice_v7_kernel of the builder computes) and its stored words; entry num_slices = 0
template <bool STAGE>
__global__ __launch_bounds__(UPD_BLOCK) void
update_v7_select_kernel(const int * __restrict__ rp, const double * __restrict__ va, const int * __restrict__ row_of_sorted, long m,
		long num_slices, int * __restrict__ v7_e0, int64_t * __restrict__ val_count)
{
	UPD_LDS_STRIP(STAGE, strip)
	const long sl = ((long) blockIdx.x * UPD_BLOCK + threadIdx.x) / WAVE;
	const int lane = threadIdx.x % WAVE;
	int start = 0, len = 0;
	if (sl < num_slices)
		sell_lane_row(rp, row_of_sorted, m, sl, lane, start, len);
	const SliceValues sv = slice_values<STAGE>(va, strip, start, len, lane);
	if (sl > num_slices)
		return;
	if (sl == num_slices)
	{
		if (lane == 0)
			val_count[sl] = 0;
		return;
	}
	const int maxlen = wave_max_i(len);
	const int e0 = sv.staged ? sell_v7_select(sv.lds, sv.rel, len, maxlen) : sell_v7_select(va, start, len, maxlen);
	if (lane == 0)
	{
		v7_e0[sl] = e0;
		val_count[sl] = sell_slice_val_words(maxlen, e0 ? maxlen / 4 : 0);
	}
}

// the values of every slice at the layout's positions, padding as 0. V7: the handle re-selects its 7-byte slices — val_ptr / v7_e0 are
// the new offsets and E0s, and desc[2s] / the flag and E0 of desc[2s+1] are renewed (index offset and mode kept). Otherwise the
// offsets are the descriptors'.
template <typename T, bool V7, bool STAGE>
__global__ __launch_bounds__(UPD_BLOCK) void
update_delta_kernel(const int * __restrict__ rp, const double * __restrict__ va, const int * __restrict__ row_of_sorted, long m,
		long num_slices, const int64_t * __restrict__ val_ptr, const int * __restrict__ v7_e0, int64_t * __restrict__ desc, T * __restrict__ val)
{
	typedef T T2 __attribute__((ext_vector_type(2)));
	UPD_LDS_STRIP(STAGE, strip)
	const long sl = ((long) blockIdx.x * UPD_BLOCK + threadIdx.x) / WAVE;
	const int lane = threadIdx.x % WAVE;
	int start = 0, len = 0;
	if (sl < num_slices)
		sell_lane_row(rp, row_of_sorted, m, sl, lane, start, len);
	const SliceValues sv = slice_values<STAGE>(va, strip, start, len, lane);
	if (sl > num_slices)
		return;
	if (sl == num_slices)
	{
		if (V7 && lane == 0)
			desc[2 * sl] = val_ptr[sl];                // terminator: the value words; its index word stays
		return;
	}
	const int maxlen = wave_max_i(len);                 // = the stored width (checked by prepare)
	int64_t vb;
	int e0 = 0;
	if constexpr (V7)
	{
		vb = val_ptr[sl];
		e0 = v7_e0[sl];
		if (lane == 0)
		{
			const int64_t old = desc[2 * sl + 1];
			desc[2 * sl] = vb;
			desc[2 * sl + 1] = sell_desc_word(sell_desc_idx(old), sell_desc_mode(old), e0);
		}
	}
	else
		vb = desc[2 * sl];
	const int full = e0 ? maxlen / 4 : 0;
	if constexpr (V7 && sizeof(T) == 8)
		for (int g = 0; g < full; g++)
		{
			unsigned long long vbits[4];
			#pragma unroll
			for (int u = 0; u < 4; u++)
			{
				const int k = g * 4 + u;
				vbits[u] = k < len ? (unsigned long long) __double_as_longlong(sv(k)) : 0ull;
			}
			sell_v7_store_group(reinterpret_cast<unsigned char *>(val + vb) + (size_t) g * (8 * SELL_V7_GROUP_WORDS), lane, vbits, e0);
		}
	// the steps stored in pairs (sell_pair_slot): a lane's steps 2p and 2p+1 side by side, the last step of an odd width alone
	for (int k = 4 * full; k < maxlen; k += 2)
	{
		T * p = val + vb + sell_pair_slot(k, maxlen, lane, full);
		const T a = k < len ? (T) sv(k) : (T) 0;
		if (k + 1 < maxlen)
		{
			T2 w;
			w.x = a;
			w.y = k + 1 < len ? (T) sv(k + 1) : (T) 0;
			*reinterpret_cast<T2 *>(p) = w;
		}
		else
			*p = a;
	}
}

// ------------------------------------------------------------------------------------------------ SELL LDS-window layout
// slices padded to whole groups of 4 steps (sellw_val_pos): fp64 in pairs of steps, fp32 a lane's 4 steps side by side
template <typename T, bool STAGE>
__global__ __launch_bounds__(UPD_BLOCK) void
update_window_kernel(const int * __restrict__ rp, const double * __restrict__ va, const int * __restrict__ row_of_sorted, long m,
		long num_slices, const int64_t * __restrict__ desc, T * __restrict__ val)
{
	UPD_LDS_STRIP(STAGE, strip)
	const long sl = ((long) blockIdx.x * UPD_BLOCK + threadIdx.x) / WAVE;
	const int lane = threadIdx.x % WAVE;
	int start = 0, len = 0;
	if (sl < num_slices)
		sell_lane_row(rp, row_of_sorted, m, sl, lane, start, len);
	const SliceValues sv = slice_values<STAGE>(va, strip, start, len, lane);
	if (sl >= num_slices)
		return;
	const int64_t b = desc[2 * sl];
	const int width = (int) ((desc[2 * sl + 2] - b) / WAVE);          // a multiple of 4, >= every len of the slice (checked by prepare)
	for (int k0 = 0; k0 < width; k0 += 4)
	{
		T v[4];
		#pragma unroll
		for (int u = 0; u < 4; u++)
			v[u] = k0 + u < len ? (T) sv(k0 + u) : (T) 0;
		if constexpr (sizeof(T) == 8)
		{
			typedef T T2 __attribute__((ext_vector_type(2)));
			T2 w0, w1;
			w0.x = v[0];
			w0.y = v[1];
			w1.x = v[2];
			w1.y = v[3];
			*reinterpret_cast<T2 *>(val + b + sellw_val_pos(k0, lane, false)) = w0;
			*reinterpret_cast<T2 *>(val + b + sellw_val_pos(k0 + 2, lane, false)) = w1;
		}
		else
		{
			typedef T T4 __attribute__((ext_vector_type(4)));
			T4 w;
			w.x = v[0];
			w.y = v[1];
			w.z = v[2];
			w.w = v[3];
			*reinterpret_cast<T4 *>(val + b + sellw_val_pos(k0, lane, true)) = w;
		}
	}
}

// ------------------------------------------------------------------------------------------------ plain SELL (C = 16 / 32 / 64 / 256)
// one thread per (slice, row), column-major: slice_ptr + k * C + lane, as plain_fill_kernel of the builder
template <typename T>
__global__ __launch_bounds__(UPD_BLOCK) void
update_plain_kernel(const int * __restrict__ rp, const double * __restrict__ va, const int * __restrict__ row_of_sorted, long m,
		long num_slices, int C, const int64_t * __restrict__ ptr, T * __restrict__ val)
{
	const long t = (long) blockIdx.x * UPD_BLOCK + threadIdx.x;
	const long sl = t / C;
	const int r = (int) (t % C);
	if (sl >= num_slices)
		return;
	const int64_t base = ptr[sl];
	const long width = (ptr[sl + 1] - base) / C;
	const long i = sl * C + r;
	long js = 0, len = 0;
	if (i < m)
	{
		const int o = row_of_sorted[i];
		js = rp[o];
		len = rp[o + 1] - js;
	}
	for (long k = 0; k < width; k++)
		val[base + k * C + r] = k < len ? (T) va[js + k] : (T) 0;
}

// ------------------------------------------------------------------------------------------------ prepare: row pointer against layout
// one thread per slice: the stored width against the longest of the slice's rows under the handle's row_of_sorted.
// layout 0 = plain (ptr = slice_ptr, widths rounded up to `round`), 1 = LDS-window (ptr = desc, rounded up to 4), 2 = delta (ptr = desc)
__global__ __launch_bounds__(UPD_BLOCK) void
check_widths_kernel(const int * __restrict__ rp, const int * __restrict__ row_of_sorted, long m, long num_slices, int C, int round,
		int layout, const int64_t * __restrict__ ptr, int * __restrict__ bad)
{
	const long sl = (long) blockIdx.x * UPD_BLOCK + threadIdx.x;
	if (sl >= num_slices)
		return;
	long w = 0;
	const long i1 = (sl + 1) * C < m ? (sl + 1) * C : m;
	for (long i = sl * C; i < i1; i++)
	{
		const int o = row_of_sorted[i];
		const long l = rp[o + 1] - rp[o];
		w = l > w ? l : w;
	}
	long stored;
	if (layout == 2)
		stored = sell_slice_width(ptr[2 * sl + 2] - ptr[2 * sl], sell_desc_v7(ptr[2 * sl + 1]));
	else
	{
		w = (w + round - 1) / round * round;
		stored = layout == 1 ? (ptr[2 * sl + 2] - ptr[2 * sl]) / C : (ptr[sl + 1] - ptr[sl]) / C;
	}
	if (stored != w)
		*bad = 1;
}

// ------------------------------------------------------------------------------------------------ host side

struct DevScratch {
	std::vector<void *> ptrs;
	~DevScratch()
	{
		for (void * p : ptrs)
			(void) hipFree(p);
	}
	template <typename P>
	int get(P ** out, size_t bytes)
	{
		void * p = nullptr;
		HIP_TRY(hipMalloc(&p, bytes ? bytes : 16));
		ptrs.push_back(p);
		*out = (P *) p;
		return 0;
	}
};

static bool
is_sell(const spmv_mi355x_matrix * A)
{
	return A->format == SPMV_MI355X_SELL_C_SIGMA;
}

// why this handle's values cannot be replaced in place whatever map it is given (nullptr: they can)
static const char *
update_refusal_of_layout(const spmv_mi355x_matrix * A)
{
	if (A->upd_col_filter)
		return "the handle was created with a column filter (col_filter_mode): its entries are a subset of the caller's";
	if (A->upd_symmetric)
		return "the handle was created with symmetric_input = 1: its entries are not the caller's CSR entries";
	if (A->coob_ranges > 0 || A->d_coob_ent)
		return "the column-blocked layout (col_blocks) stores its entries sorted by column";
	if (A->cfg.unit)
		return "the handle dropped its value stream because its values were uniform (a _unit layout)";
	return nullptr;
}

static const char * const TRANSPOSED_UNMAPPED = "the handle was created with transpose = 1: its entries are not in the caller's order "
                                                "(call spmv_mi355x_update_values_prepare_transposed with the pattern of A)";

// why this handle takes no update as it is: a transposed handle needs its entry map first (update_values_prepare_transposed)
static const char *
update_refusal(const spmv_mi355x_matrix * A)
{
	if (A->transposed && !A->d_upd_src)
		return TRANSPOSED_UNMAPPED;
	return update_refusal_of_layout(A);
}

// What prepare keeps. d_rp: a device row pointer of rows() + 1 entries from 0 to nnz(), checked against the layout (SELL: every slice's
// stored width against the longest of its rows). d_src: the entry map that goes with it (transposed handles), or nullptr.
// 0 = both are the handle's now, what it kept before is freed; 1 = error set (`what: subject does not match ...`), both still the caller's.
static int
keep_row_ptr(spmv_mi355x_matrix * A, int * d_rp, unsigned * d_src, long count, const char * what, const char * subject)
{
	const long m = A->m;
	if (is_sell(A) && A->sell_slices > 0)
	{
		DevScratch guard;
		int * flag;
		if (guard.get(&flag, 4))
			return 1;
		HIP_TRY(hipMemset(flag, 0, 4));
		const int C = A->sell_c;
		const int layout = A->sell_window ? 1 : A->sell_delta ? 2 : 0;
		const int round = layout == 1 ? 4 : layout == 2 ? 1 : (C >= WAVE ? 1 : WAVE / C);
		const int64_t * ptr = layout == 0 ? A->d_slice_ptr : A->d_sell_desc;
		hipLaunchKernelGGL(check_widths_kernel, dim3((unsigned) ((A->sell_slices + UPD_BLOCK - 1) / UPD_BLOCK)), dim3(UPD_BLOCK), 0, 0, d_rp, A->d_row_of_sorted, m,
				A->sell_slices, C, round, layout, ptr, flag);
		HIP_TRY(hipGetLastError());
		int flag_host = 0;
		HIP_TRY(hipMemcpy(&flag_host, flag, 4, hipMemcpyDeviceToHost));
		if (flag_host)
		{
			set_error("%s: %s does not match the pattern this handle was built from", what, subject);
			return 1;
		}
	}
	size_t cap = 0;
	if (A->d_val && hipMemPtrGetInfo(A->d_val, &cap) != hipSuccess)
	{
		(void) hipGetLastError();
		cap = 0;                                           // unknown: the first update that needs room allocates
	}
	if (A->d_upd_row_ptr)
		(void) hipFree(A->d_upd_row_ptr);
	if (A->d_upd_src)
		(void) hipFree(A->d_upd_src);
	A->d_upd_row_ptr = d_rp;
	A->d_upd_src = d_src;
	A->upd_count = d_src ? count : 0;
	A->val_capacity = cap;
	return 0;
}

static unsigned
slice_grid(long num_slices_and_terminator)
{
	return (unsigned) ((num_slices_and_terminator * WAVE + UPD_BLOCK - 1) / UPD_BLOCK);
}

// CSR family / row-sorted COO
static int
update_csr_ordered(spmv_mi355x_matrix * A, const double * va, hipStream_t st)
{
	const long n = A->nnz;
	const bool merge = A->format == SPMV_MI355X_CSR_MERGE;
	DevScratch tmp;
	int * differs = nullptr;
	if (merge)
	{
		if (tmp.get(&differs, 4))
			return 1;
		HIP_TRY(hipMemsetAsync(differs, 0, 4, st));
	}
	const bool aligned = (reinterpret_cast<uintptr_t>(va) & 15) == 0;
	const dim3 grid((unsigned) ((n + 4L * UPD_BLOCK - 1) / (4L * UPD_BLOCK))), block(UPD_BLOCK);
	if (A->val_f32)
	{
		if (aligned)
			hipLaunchKernelGGL((stream_values_kernel<float, true>), grid, block, 0, st, va, (float *) A->d_val, n, differs);
		else
			hipLaunchKernelGGL((stream_values_kernel<float, false>), grid, block, 0, st, va, (float *) A->d_val, n, differs);
	}
	else
	{
		if (aligned)
			hipLaunchKernelGGL((stream_values_kernel<double, true>), grid, block, 0, st, va, (double *) A->d_val, n, differs);
		else
			hipLaunchKernelGGL((stream_values_kernel<double, false>), grid, block, 0, st, va, (double *) A->d_val, n, differs);
	}
	HIP_TRY(hipGetLastError());
	if (!merge)
	{
		HIP_TRY(hipStreamSynchronize(st));
		return 0;
	}
	// the merge path's one choice from the values (build_csr_merge): uniform values -> the constant is kept, the stream dropped
	int differs_host = 0;
	double v0 = 0;
	HIP_TRY(hipMemcpyAsync(&differs_host, differs, 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(&v0, va, 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	if (A->val_f32)
		v0 = (double) (float) v0;
	if (!differs_host && v0 == v0)
	{
		(void) hipFree(A->d_val);
		A->d_val = nullptr;
		A->val_capacity = 0;
		A->cfg.unit = 1;
		A->cfg.unit_value = v0;
		A->mem_footprint -= (double) n * A->vbytes;
		snprintf(A->format_name, sizeof(A->format_name), "MI355X_CSR_MERGE_i%d_unit_%s", A->merge_ipt, A->f32 ? "f" : "d");
	}
	return 0;
}

template <typename T>
static int
update_sell_fixed(spmv_mi355x_matrix * A, const double * va, hipStream_t st, bool stage)
{
	const long ns = A->sell_slices;
	const int * rp = A->d_upd_row_ptr;
	T * val = (T *) A->d_val;
	if (A->sell_window)
	{
		if (stage)
			hipLaunchKernelGGL((update_window_kernel<T, true>), dim3(slice_grid(ns)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, A->d_sell_desc, val);
		else
			hipLaunchKernelGGL((update_window_kernel<T, false>), dim3(slice_grid(ns)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, A->d_sell_desc, val);
	}
	else if (A->sell_delta)
	{
		if (stage)
			hipLaunchKernelGGL((update_delta_kernel<T, false, true>), dim3(slice_grid(ns)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, nullptr, nullptr,
					A->d_sell_desc, val);
		else
			hipLaunchKernelGGL((update_delta_kernel<T, false, false>), dim3(slice_grid(ns)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, nullptr, nullptr,
					A->d_sell_desc, val);
	}
	else
	{
		const unsigned grid = (unsigned) ((ns * A->sell_c + UPD_BLOCK - 1) / UPD_BLOCK);
		hipLaunchKernelGGL((update_plain_kernel<T>), dim3(grid), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, A->sell_c, A->d_slice_ptr, val);
	}
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	return 0;
}

// the delta layout of an fp64 handle that looks for 7-byte slices: selection, offsets, (re)allocation, descriptors and values
static int
update_sell_v7(spmv_mi355x_matrix * A, const double * va, hipStream_t st, bool stage)
{
	const long ns = A->sell_slices;
	const int * rp = A->d_upd_row_ptr;
	DevScratch tmp;
	int * v7_e0;
	int64_t * val_count, * val_ptr;
	void * scan_tmp;
	size_t scan_bytes = 0;
	HIP_TRY(hipcub::DeviceScan::ExclusiveSum(nullptr, scan_bytes, (int64_t *) nullptr, (int64_t *) nullptr, (int) (ns + 1), st));
	if (tmp.get(&v7_e0, (size_t) ns * 4) || tmp.get(&val_count, (size_t) (ns + 1) * 8) || tmp.get(&val_ptr, (size_t) (ns + 1) * 8) ||
	    tmp.get(&scan_tmp, scan_bytes))
		return 1;
	if (stage)
		hipLaunchKernelGGL((update_v7_select_kernel<true>), dim3(slice_grid(ns + 1)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, v7_e0, val_count);
	else
		hipLaunchKernelGGL((update_v7_select_kernel<false>), dim3(slice_grid(ns + 1)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, v7_e0, val_count);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipcub::DeviceScan::ExclusiveSum(scan_tmp, scan_bytes, val_count, val_ptr, (int) (ns + 1), st));
	std::vector<int64_t> val_ptr_host((size_t) ns + 1);
	std::vector<int> e0_host((size_t) ns);
	HIP_TRY(hipMemcpyAsync(val_ptr_host.data(), val_ptr, (size_t) (ns + 1) * 8, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipMemcpyAsync(e0_host.data(), v7_e0, (size_t) ns * 4, hipMemcpyDeviceToHost, st));
	HIP_TRY(hipStreamSynchronize(st));
	const int64_t val_words = val_ptr_host[(size_t) ns];
	long v7_slices = 0;
	for (long sl = 0; sl < ns; sl++)
		v7_slices += e0_host[(size_t) sl] != 0;
	// a selection that stores more words than the allocation holds: a new allocation (its size depends on the values)
	const size_t need = ((size_t) val_words + STREAM_SLACK) * 8;
	if (need > A->val_capacity)
	{
		void * fresh = nullptr;
		HIP_TRY(hipMalloc(&fresh, need));
		(void) hipFree(A->d_val);
		A->d_val = fresh;
		A->val_capacity = need;
	}
	HIP_TRY(hipMemsetAsync((char *) A->d_val + (size_t) val_words * 8, 0, (size_t) STREAM_SLACK * 8, st));
	if (stage)
		hipLaunchKernelGGL((update_delta_kernel<double, true, true>), dim3(slice_grid(ns + 1)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, val_ptr, v7_e0,
				A->d_sell_desc, (double *) A->d_val);
	else
		hipLaunchKernelGGL((update_delta_kernel<double, true, false>), dim3(slice_grid(ns + 1)), dim3(UPD_BLOCK), 0, st, rp, va, A->d_row_of_sorted, A->m, ns, val_ptr, v7_e0,
				A->d_sell_desc, (double *) A->d_val);
	HIP_TRY(hipGetLastError());
	HIP_TRY(hipStreamSynchronize(st));
	sell_delta_values_changed(A, val_ptr_host.data(), v7_slices);
	return 0;
}

static int
update_state(const spmv_mi355x_matrix * A)
{
	if (!A)
	{
		set_error("update_values_state: NULL handle");
		return 0;
	}
	if (const char * why = update_refusal(A))
	{
		set_error("update_values: %s", why);
		return 0;
	}
	return A->d_upd_row_ptr ? 2 : 1;
}

}  // namespace spmv

using namespace spmv;

extern "C" {

int
spmv_mi355x_update_values_state(const spmv_mi355x_matrix * A)
{
	return update_state(A);
}

int
spmv_mi355x_update_values_prepare(spmv_mi355x_matrix * A, const int32_t * row_ptr)
{
	if (!A || !row_ptr)
	{
		set_error("update_values_prepare: NULL %s", !A ? "handle" : "row_ptr");
		return 1;
	}
	if (const char * why = A->transposed ? TRANSPOSED_UNMAPPED : update_refusal(A))
	{
		set_error("update_values_prepare: %s", why);
		return 1;
	}
	const long m = A->m;
	long bad = -1;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(max : bad)
	for (long i = 0; i < m; i++)
		if (row_ptr[i + 1] < row_ptr[i])
			bad = std::max(bad, i);
	if (row_ptr[0] != 0 || bad >= 0 || (long) row_ptr[m] != A->nnz)
	{
		if (row_ptr[0] != 0)
			set_error("update_values_prepare: row_ptr must be the LOCAL row pointer, starting at 0 (got %d)", row_ptr[0]);
		else if (bad >= 0)
			set_error("update_values_prepare: row_ptr is not monotone at row %ld", bad);
		else
			set_error("update_values_prepare: row_ptr[rows] = %ld does not match the handle's nnz = %ld", (long) row_ptr[m], A->nnz);
		return 1;
	}
	HIP_TRY(hipSetDevice(A->device));
	int * d_rp = nullptr;
	if (dev_alloc(&d_rp, (size_t) m + 1))
		return 1;
	DevScratch guard;
	guard.ptrs.push_back(d_rp);
	HIP_TRY(hipMemcpy(d_rp, row_ptr, ((size_t) m + 1) * 4, hipMemcpyHostToDevice));
	if (keep_row_ptr(A, d_rp, nullptr, 0, "update_values_prepare", "row_ptr"))
		return 1;
	guard.ptrs.clear();                                    // the copy stays with the handle
	return 0;
}

// A handle built with transpose = 1, from values in A's entry order: the pattern of A once more -> the entry map (transpose_csr.hip)
int
spmv_mi355x_update_values_prepare_transposed(spmv_mi355x_matrix * At, long m, long n, const int32_t * row_ptr, const int32_t * col_idx)
{
	const char * const what = "update_values_prepare_transposed";
	if (!At || !row_ptr || (!col_idx && At->t_nnz > 0))
	{
		set_error("%s: NULL %s", what, !At ? "handle" : !row_ptr ? "row_ptr" : "col_idx");
		return 1;
	}
	if (!At->transposed)
	{
		set_error("%s: the handle was not created with transpose = 1 (its entries are the caller's: spmv_mi355x_update_values_prepare)", what);
		return 1;
	}
	if (const char * why = update_refusal_of_layout(At))
	{
		set_error("%s: %s", what, why);
		return 1;
	}
	if (m != At->n || n != At->t_rows)
	{
		set_error("%s: the pattern is %ld x %ld, the handle was created from a matrix of %ld x %ld", what, m, n, At->n, At->t_rows);
		return 1;
	}
	if (row_ptr[0] != 0)
	{
		set_error("%s: row_ptr must start at 0 (got %d)", what, row_ptr[0]);
		return 1;
	}
	long bad = -1;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(max : bad)
	for (long i = 0; i < m; i++)
		if (row_ptr[i + 1] < row_ptr[i])
			bad = std::max(bad, i);
	if (bad >= 0)
	{
		set_error("%s: row_ptr is not monotone at row %ld", what, bad);
		return 1;
	}
	const long nnz = row_ptr[m];
	if (nnz != At->t_nnz)
	{
		set_error("%s: row_ptr[m] = %ld does not match the nnz = %ld of the matrix the handle was created from", what, nnz, At->t_nnz);
		return 1;
	}
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(max : bad)
	for (long j = 0; j < nnz; j++)
		if (col_idx[j] < 0 || col_idx[j] >= n)
			bad = std::max(bad, j);
	if (bad >= 0)
	{
		set_error("%s: column index %d out of range [0,%ld) at entry %ld", what, col_idx[bad], n, bad);
		return 1;
	}
	HIP_TRY(hipSetDevice(At->device));
	int * d_lrp = nullptr;
	unsigned * d_src = nullptr;
	long lnnz = 0;
	if (transpose_entry_map(At->convert_on_device, m, n, nnz, row_ptr, col_idx, At->t_row_begin, At->t_row_end, &d_lrp, &d_src, &lnnz))
		return 1;
	DevScratch guard;
	guard.ptrs = {d_lrp, d_src};
	if (lnnz != At->nnz)
	{
		set_error("%s: the rows [%ld,%ld) of the transposed pattern hold %ld entries, the handle's nnz = %ld: the pattern does not match the pattern "
		          "this handle was built from", what, At->t_row_begin, At->t_row_end, lnnz, At->nnz);
		return 1;
	}
	if (keep_row_ptr(At, d_lrp, d_src, nnz, what, "the pattern"))
		return 1;
	guard.ptrs.clear();                                    // both stay with the handle
	return 0;
}

long
spmv_mi355x_update_values_count(const spmv_mi355x_matrix * A)
{
	return !A ? -1 : A->d_upd_src ? A->upd_count : A->nnz;
}

int
spmv_mi355x_update_values_device(spmv_mi355x_matrix * A, const double * values_dev, void * hip_stream)
{
	if (!A || (!values_dev && spmv_mi355x_update_values_count(A) > 0))
	{
		set_error("update_values_device: NULL %s", !A ? "handle" : "values");
		return 1;
	}
	if (const char * why = update_refusal(A))
	{
		set_error("update_values_device: %s", why);
		return 1;
	}
	if (!A->d_upd_row_ptr)
	{
		set_error("update_values_device: spmv_mi355x_update_values_prepare has not been called on this handle");
		return 1;
	}
	if (reinterpret_cast<uintptr_t>(values_dev) & 7)
	{
		set_error("update_values_device: the values must be 8-byte aligned");
		return 1;
	}
	hipStream_t st = (hipStream_t) hip_stream;
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != A->device)
		HIP_TRY(hipSetDevice(A->device));
	// a transposed handle: the values arrive in A's entry order; one gather through the entry map puts them in the handle's local CSR
	// order, and everything below runs on that transient array as on a caller's
	DevScratch mapped;
	if (A->d_upd_src && A->nnz > 0)
	{
		double * va_t = nullptr;
		if (mapped.get(&va_t, (size_t) A->nnz * 8) || transpose_gather_values(A->d_upd_src, values_dev, A->nnz, va_t, st))
			return 1;
		values_dev = va_t;
	}
	int rc = 0;
	if (A->nnz == 0)
		HIP_TRY(hipStreamSynchronize(st));
	else if (!is_sell(A))
		rc = update_csr_ordered(A, values_dev, st);
	else if (A->sell_delta && !A->sell_window && A->sell_v7_active)
		rc = update_sell_v7(A, values_dev, st, update_stage_setting());
	else if (A->val_f32)
		rc = update_sell_fixed<float>(A, values_dev, st, update_stage_setting());
	else
		rc = update_sell_fixed<double>(A, values_dev, st, update_stage_setting());
	if (rc)
		return 1;
	A->y_downloaded = false;                               // the next host-buffer spmv downloads the new product
	return 0;
}

int
spmv_mi355x_update_values(spmv_mi355x_matrix * A, const double * values_host)
{
	const long count = spmv_mi355x_update_values_count(A);
	if (!A || (!values_host && count > 0))
	{
		set_error("update_values: NULL %s", !A ? "handle" : "values");
		return 1;
	}
	if (const char * why = update_refusal(A))
	{
		set_error("update_values: %s", why);
		return 1;
	}
	if (!A->d_upd_row_ptr)
	{
		set_error("update_values: spmv_mi355x_update_values_prepare has not been called on this handle");
		return 1;
	}
	HIP_TRY(hipSetDevice(A->device));
	DevScratch tmp;
	double * d_va = nullptr;
	if (tmp.get(&d_va, (size_t) count * 8))
		return 1;
	if (count)
		HIP_TRY(hipMemcpy(d_va, values_host, (size_t) count * 8, hipMemcpyHostToDevice));
	return spmv_mi355x_update_values_device(A, d_va, nullptr);
}

}  // extern "C"

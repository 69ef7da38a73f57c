// CSR of A (m x n) -> CSR of A^t (n x m), where the matrix already is: in device memory (include/spmv_mi355x.h "transposed handles",
// opts.transpose). The engine then builds a handle of A^t in A^t's own best layout, and every kernel, spmm, the solvers and the value
// stores serve the transposed product unchanged. There is deliberately no y = A^t x over A's layout: that is one scattered fp64 atomic
// per entry (24 G updates/s scattered, 178 G/s at best: profiles/r01_atomic_bench.txt) and a result that changes from run to run.
//
// THE ORDER (the contract): the rows of A^t in order; inside a row the entries in ascending row of A; entries of equal (row, column)
// in their input order = a stable counting sort of the entries by column. Nothing here depends on the order in which atomics land:
//   1. one lane per entry: its row, by binary search of the entry number in row_ptr (neighbouring lanes walk the same cache lines);
//   2. one stable radix sort of (column, entry number) over the ceil(log2 n) bits a column takes (hipcub);
//   3. row_ptr of A^t = the first sorted position of every column: a lower-bound search in the sorted keys, one lane per column;
//   4. one gather: col_t[e] = row[id[e]], val_t[e] = val[id[e]] — a bandwidth kernel with two scattered reads per entry (4 + 8 bytes;
//      inside one column of A the ids ascend, so a column that many consecutive rows own reads whole lines), four entries per lane
//      and step, the sorted ids read once as 16 bytes with the nt policy, both results stored as 16 bytes, a grid sized from the CUs.
// Transient: the row marks, the ids and the sort's second pair of buffers (16 bytes per entry + the sort's own scratch), freed before
// this returns; the three output arrays are the caller's to free (before the format builder allocates its own, csr_stream.hip).
// transpose_csr_host is the same order on the host (OpenMP) and stays as the checker (opts.convert_on = 2): same bytes.
//
// Steps 1 to 3 are transpose_order(): THE ORDER has this one definition. Its sorted ids are also the ENTRY MAP of the transposition —
// entry e of the CSR of A^t is entry ids[e] of the CSR of A — which transpose_entry_map() keeps (for a row block of A^t: that stretch,
// with the row pointer rebased to 0) so that update_values can refresh a transposed handle from values in A's entry order
// (update_values.hip, spmv_mi355x_update_values_prepare_transposed): one launch of values_gather_kernel, step 4 without the rows.
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <vector>

#include "handle.hpp"

namespace spmv {

namespace {

constexpr int TB = 256;

struct Scratch {
	std::vector<void *> ptrs;
	~Scratch() { release(); }
	void release()
	{
		for (void * p : ptrs)
			(void) hipFree(p);
		ptrs.clear();
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

// row[e] = the row of entry e (the last i with rp[i] <= e: empty rows never own an entry), ids[e] = e
__global__ __launch_bounds__(TB) void
transpose_mark_kernel(const int * __restrict__ rp, long m, long nnz, int * __restrict__ row, unsigned * __restrict__ ids)
{
	for (long e = (long) blockIdx.x * TB + threadIdx.x; e < nnz; e += (long) gridDim.x * TB)
	{
		long lo = 0, hi = m - 1;
		while (lo < hi)
		{
			const long mid = (lo + hi + 1) / 2;
			if (rp[mid] <= e)
				lo = mid;
			else
				hi = mid - 1;
		}
		row[e] = (int) lo;
		ids[e] = (unsigned) e;
	}
}

// rp_t[c] = the first sorted entry whose column is >= c, c = 0 .. n (rp_t[n] = nnz)
__global__ __launch_bounds__(TB) void
transpose_start_kernel(const unsigned * __restrict__ key, long nnz, long n, int * __restrict__ rp_t)
{
	const long c = (long) blockIdx.x * TB + threadIdx.x;
	if (c > n)
		return;
	long lo = 0, hi = nnz;
	while (lo < hi)
	{
		const long mid = (lo + hi) / 2;
		if ((long) key[mid] < c)
			lo = mid + 1;
		else
			hi = mid;
	}
	rp_t[c] = (int) lo;
}

// ci_t[e] = row[ids[e]], va_t[e] = va[ids[e]]; ids, ci_t and va_t are allocations of this file (16-byte aligned)
__global__ __launch_bounds__(TB) void
transpose_gather_kernel(const unsigned * __restrict__ ids, const int * __restrict__ row, const double * __restrict__ va, long nnz,
		int * __restrict__ ci_t, double * __restrict__ va_t)
{
	typedef unsigned U4 __attribute__((ext_vector_type(4)));
	typedef int I4 __attribute__((ext_vector_type(4)));
	typedef double D2 __attribute__((ext_vector_type(2)));
	const long quads = nnz / 4;
	for (long q = (long) blockIdx.x * TB + threadIdx.x; q < quads; q += (long) gridDim.x * TB)
	{
		const U4 id = __builtin_nontemporal_load(reinterpret_cast<const U4 *>(ids) + q);
		I4 r;
		D2 a, b;
		r.x = row[id.x];
		r.y = row[id.y];
		r.z = row[id.z];
		r.w = row[id.w];
		a.x = va[id.x];
		a.y = va[id.y];
		b.x = va[id.z];
		b.y = va[id.w];
		reinterpret_cast<I4 *>(ci_t)[q] = r;
		reinterpret_cast<D2 *>(va_t)[2 * q] = a;
		reinterpret_cast<D2 *>(va_t)[2 * q + 1] = b;
	}
	// the last nnz % 4 entries
	if (blockIdx.x == 0 && threadIdx.x < nnz - 4 * quads)
	{
		const long e = 4 * quads + threadIdx.x;
		const unsigned id = ids[e];
		ci_t[e] = row[id];
		va_t[e] = va[id];
	}
}

// va_t[e] = va[src[e]]: step 4 for new values alone (12 bytes read, 8 written per entry). src and va_t are allocations of the library
// (16-byte aligned); va is the caller's, 8-byte aligned, and is read one value at a time
__global__ __launch_bounds__(TB) void
values_gather_kernel(const unsigned * __restrict__ src, const double * __restrict__ va, long nnz, double * __restrict__ va_t)
{
	typedef unsigned U4 __attribute__((ext_vector_type(4)));
	typedef double D2 __attribute__((ext_vector_type(2)));
	const long quads = nnz / 4;
	for (long q = (long) blockIdx.x * TB + threadIdx.x; q < quads; q += (long) gridDim.x * TB)
	{
		const U4 id = __builtin_nontemporal_load(reinterpret_cast<const U4 *>(src) + q);
		D2 a, b;
		a.x = va[id.x];
		a.y = va[id.y];
		b.x = va[id.z];
		b.y = va[id.w];
		reinterpret_cast<D2 *>(va_t)[2 * q] = a;
		reinterpret_cast<D2 *>(va_t)[2 * q + 1] = b;
	}
	// the last nnz % 4 entries
	if (blockIdx.x == 0 && threadIdx.x < nnz - 4 * quads)
	{
		const long e = 4 * quads + threadIdx.x;
		va_t[e] = va[src[e]];
	}
}

// step 4 for the pattern alone: ci_t[e] = row[ids[e]], and the ids copied out of the sort's scratch
__global__ __launch_bounds__(TB) void
transpose_rows_kernel(const unsigned * __restrict__ ids, const int * __restrict__ row, long nnz, int * __restrict__ ci_t, unsigned * __restrict__ ids_out)
{
	for (long e = (long) blockIdx.x * TB + threadIdx.x; e < nnz; e += (long) gridDim.x * TB)
	{
		const unsigned id = ids[e];
		ci_t[e] = row[id];
		ids_out[e] = id;
	}
}

// lrp[i] = rp_t[r0 + i] - rp_t[r0], i = 0 .. rows: the row pointer of the row block [r0, r0 + rows) of A^t, from 0
__global__ __launch_bounds__(TB) void
transpose_block_kernel(const int * __restrict__ rp_t, long r0, long rows, int * __restrict__ lrp)
{
	const long i = (long) blockIdx.x * TB + threadIdx.x;
	if (i <= rows)
		lrp[i] = rp_t[r0 + i] - rp_t[r0];
}

static unsigned
bandwidth_grid(long items)
{
	int dev = 0, cus = 256;
	if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus < 1)
	{
		(void) hipGetLastError();
		cus = 256;
	}
	const long want = (items + TB - 1) / TB, cap = (long) cus * 8;
	return (unsigned) std::max<long>(1, std::min(want, cap));
}

static bool
transpose_sizes_bad(long m, long n, long nnz)
{
	if (m < 0 || n < 0 || nnz < 0 || n + nnz >= 0x7fffffffL || (nnz > 0 && (m < 1 || n < 1)))
	{
		set_error("transpose: sizes out of range (m=%ld n=%ld nnz=%ld)", m, n, nnz);
		return true;
	}
	return false;
}

// Steps 1 to 3 of THE ORDER for nnz > 0, enqueued on the null stream: rp_t (n + 1 entries, the caller's allocation) is written;
// *row_out (the row of every entry of A) and *ids_out (the sorted entry numbers) are allocations of `tmp`, like the sort's buffers.
static int
transpose_order(long m, long n, long nnz, const int * rp, const int * ci, Scratch & tmp, int * rp_t, int ** row_out, unsigned ** ids_out)
{
	int * row;
	unsigned * ids, * ids_sorted, * key_sorted;
	if (tmp.get(&row, (size_t) nnz * 4) || tmp.get(&ids, (size_t) nnz * 4) || tmp.get(&ids_sorted, (size_t) nnz * 4) || tmp.get(&key_sorted, (size_t) nnz * 4))
		return 1;
	hipLaunchKernelGGL(transpose_mark_kernel, dim3(bandwidth_grid(nnz)), dim3(TB), 0, 0, rp, m, nnz, row, ids);
	HIP_TRY(hipGetLastError());
	int bits = 1;
	while ((1L << bits) < n)
		bits++;
	const unsigned * key = reinterpret_cast<const unsigned *>(ci);        // columns are in [0, n): non-negative
	size_t bytes = 0;
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, key, key_sorted, ids, ids_sorted, (int) nnz, 0, bits, (hipStream_t) 0));
	void * sort_tmp;
	if (tmp.get(&sort_tmp, bytes))
		return 1;
	HIP_TRY(hipcub::DeviceRadixSort::SortPairs(sort_tmp, bytes, key, key_sorted, ids, ids_sorted, (int) nnz, 0, bits, (hipStream_t) 0));
	hipLaunchKernelGGL(transpose_start_kernel, dim3((unsigned) ((n + 1 + TB - 1) / TB)), dim3(TB), 0, 0, key_sorted, nnz, n, rp_t);
	HIP_TRY(hipGetLastError());
	*row_out = row;
	*ids_out = ids_sorted;
	return 0;
}

}  // namespace

// rp, ci, va: device pointers of an m x n CSR with row_ptr[0] = 0, row_ptr[m] = nnz and columns in [0, n) (the caller has checked).
// Outputs: device allocations of n + 1, max(nnz, 1) and max(nnz, 1) elements, the caller's to hipFree. 0 = done, 1 = error set.
int
transpose_csr_device(long m, long n, long nnz, const int * rp, const int * ci, const double * va, int ** rp_t_out, int ** ci_t_out, double ** va_t_out)
{
	*rp_t_out = nullptr;
	*ci_t_out = nullptr;
	*va_t_out = nullptr;
	if (transpose_sizes_bad(m, n, nnz))
		return 1;
	Scratch out, tmp;
	int * rp_t, * ci_t;
	double * va_t;
	if (out.get(&rp_t, (size_t) (n + 1) * 4) || out.get(&ci_t, (size_t) nnz * 4) || out.get(&va_t, (size_t) nnz * 8))
		return 1;
	if (nnz == 0)
		HIP_TRY(hipMemset(rp_t, 0, (size_t) (n + 1) * 4));
	else
	{
		int * row;
		unsigned * ids_sorted;
		if (transpose_order(m, n, nnz, rp, ci, tmp, rp_t, &row, &ids_sorted))
			return 1;
		hipLaunchKernelGGL(transpose_gather_kernel, dim3(bandwidth_grid((nnz + 3) / 4)), dim3(TB), 0, 0, ids_sorted, row, va, nnz, ci_t, va_t);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipDeviceSynchronize());
	tmp.release();
	out.ptrs.clear();
	*rp_t_out = rp_t;
	*ci_t_out = ci_t;
	*va_t_out = va_t;
	return 0;
}

// The pattern alone, for a device-resident pattern (color.hip: the graph of A + A^t, and the two transpositions behind P A P^t):
// steps 1 to 3 and the row gather of step 4. *ids_out = the sorted entry numbers, the entry map of the transposition. Outputs: device
// allocations of n + 1, max(nnz, 1) and max(nnz, 1) words, the caller's to hipFree. 0 = done, 1 = error set.
int
transpose_pattern_device(long m, long n, long nnz, const int * rp, const int * ci, int ** rp_t_out, int ** ci_t_out, unsigned ** ids_out)
{
	*rp_t_out = nullptr;
	*ci_t_out = nullptr;
	*ids_out = nullptr;
	if (transpose_sizes_bad(m, n, nnz))
		return 1;
	Scratch out, tmp;
	int * rp_t, * ci_t;
	unsigned * ids;
	if (out.get(&rp_t, (size_t) (n + 1) * 4) || out.get(&ci_t, (size_t) nnz * 4) || out.get(&ids, (size_t) nnz * 4))
		return 1;
	if (nnz == 0)
		HIP_TRY(hipMemset(rp_t, 0, (size_t) (n + 1) * 4));
	else
	{
		int * row;
		unsigned * ids_sorted;
		if (transpose_order(m, n, nnz, rp, ci, tmp, rp_t, &row, &ids_sorted))
			return 1;
		hipLaunchKernelGGL(transpose_rows_kernel, dim3(bandwidth_grid(nnz)), dim3(TB), 0, 0, ids_sorted, row, nnz, ci_t, ids);
		HIP_TRY(hipGetLastError());
	}
	HIP_TRY(hipDeviceSynchronize());
	tmp.release();
	out.ptrs.clear();
	*rp_t_out = rp_t;
	*ci_t_out = ci_t;
	*ids_out = ids;
	return 0;
}

// The entry map of the transposition for the rows [r0, r1) of A^t, from the (validated) host pattern of A: *d_lrp_out = the block's row
// pointer from 0 (r1 - r0 + 1 entries), *d_src_out = for every entry of the block the number of that entry in the CSR of A
// (*lnnz_out entries, 16-byte aligned), both device allocations the caller frees. on_device: transpose_order() on the uploaded pattern;
// otherwise transpose_csr_host() carries the entry numbers in place of the values (the checker: the same bytes).
// Transient device memory: the pattern of A, the row pointer of A^t, and on the device what the transposition takes without its value
// arrays (16 bytes per non-zero + the sort's scratch).
int
transpose_entry_map(bool on_device, long m, long n, long nnz, const int * rp, const int * ci, long r0, long r1, int ** d_lrp_out, unsigned ** d_src_out,
		long * lnnz_out)
{
	*d_lrp_out = nullptr;
	*d_src_out = nullptr;
	*lnnz_out = 0;
	if (transpose_sizes_bad(m, n, nnz))
		return 1;
	if (r0 < 0 || r1 > n || r0 > r1)
	{
		set_error("transpose: bad row block [%ld,%ld) for %ld rows", r0, r1, n);
		return 1;
	}
	Scratch out, tmp;
	int * d_rp_t, * d_lrp;
	unsigned * d_src = nullptr, * d_ids = nullptr;
	if (tmp.get(&d_rp_t, (size_t) (n + 1) * 4) || out.get(&d_lrp, (size_t) (r1 - r0 + 1) * 4))
		return 1;
	if (nnz == 0)
		HIP_TRY(hipMemset(d_rp_t, 0, (size_t) (n + 1) * 4));
	else if (on_device)
	{
		int * d_rp, * d_ci, * row;
		if (tmp.get(&d_rp, (size_t) (m + 1) * 4) || tmp.get(&d_ci, (size_t) nnz * 4))
			return 1;
		HIP_TRY(hipMemcpy(d_rp, rp, (size_t) (m + 1) * 4, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_ci, ci, (size_t) nnz * 4, hipMemcpyHostToDevice));
		if (transpose_order(m, n, nnz, d_rp, d_ci, tmp, d_rp_t, &row, &d_ids))
			return 1;
	}
	else
	{
		std::vector<double> number((size_t) nnz), number_t;
		#pragma omp parallel for num_threads(spmv::host_threads())
		for (long e = 0; e < nnz; e++)
			number[(size_t) e] = (double) e;                    // exact: nnz < 2^31
		std::vector<int> rp_t, ci_t;
		transpose_csr_host(m, n, nnz, rp, ci, number.data(), rp_t, ci_t, number_t);
		std::vector<unsigned> ids((size_t) nnz);
		#pragma omp parallel for num_threads(spmv::host_threads())
		for (long e = 0; e < nnz; e++)
			ids[(size_t) e] = (unsigned) number_t[(size_t) e];
		if (tmp.get(&d_ids, (size_t) nnz * 4))
			return 1;
		HIP_TRY(hipMemcpy(d_rp_t, rp_t.data(), (size_t) (n + 1) * 4, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_ids, ids.data(), (size_t) nnz * 4, hipMemcpyHostToDevice));
	}
	int ends[2] = {0, 0};
	HIP_TRY(hipMemcpy(&ends[0], d_rp_t + r0, 4, hipMemcpyDeviceToHost));         // null stream: behind the kernels above
	HIP_TRY(hipMemcpy(&ends[1], d_rp_t + r1, 4, hipMemcpyDeviceToHost));
	const long lnnz = (long) ends[1] - ends[0];
	if (ends[0] < 0 || lnnz < 0 || ends[1] > nnz)
	{
		set_error("transpose: row pointer of the transposed matrix out of range (%d, %d of %ld)", ends[0], ends[1], nnz);
		return 1;
	}
	if (out.get(&d_src, (size_t) lnnz * 4))
		return 1;
	hipLaunchKernelGGL(transpose_block_kernel, dim3((unsigned) ((r1 - r0 + 1 + TB - 1) / TB)), dim3(TB), 0, 0, d_rp_t, r0, r1 - r0, d_lrp);
	HIP_TRY(hipGetLastError());
	if (lnnz)
		HIP_TRY(hipMemcpy(d_src, d_ids + ends[0], (size_t) lnnz * 4, hipMemcpyDeviceToDevice));
	HIP_TRY(hipDeviceSynchronize());
	tmp.release();
	out.ptrs.clear();
	*d_lrp_out = d_lrp;
	*d_src_out = d_src;
	*lnnz_out = lnnz;
	return 0;
}

// va_t[e] = va[src[e]] for the nnz entries of a map transpose_entry_map() made, enqueued on st. src and va_t are 16-byte aligned
// device allocations; every src[e] indexes va.
int
transpose_gather_values(const unsigned * src, const double * va, long nnz, double * va_t, hipStream_t st)
{
	if (nnz <= 0)
		return 0;
	hipLaunchKernelGGL(values_gather_kernel, dim3(bandwidth_grid((nnz + 3) / 4)), dim3(TB), 0, st, src, va, nnz, va_t);
	HIP_TRY(hipGetLastError());
	return 0;
}

// create(): the caller's (validated) host CSR, row_ptr from 0 -> the host CSR of A^t, transposed on the device. One upload and one
// download of 12 bytes per non-zero around it: accepted, so that the row block, the column filter and every builder family keep
// working from one local CSR.
int
transpose_csr_upload(long m, long n, long nnz, const int * rp, const int * ci, const double * va, std::vector<int> & rp_t, std::vector<int> & ci_t,
		std::vector<double> & va_t)
{
	Scratch in, out;
	int * d_rp, * d_ci, * d_rp_t = nullptr, * d_ci_t = nullptr;
	double * d_va, * d_va_t = nullptr;
	if (in.get(&d_rp, (size_t) (m + 1) * 4) || in.get(&d_ci, (size_t) nnz * 4) || in.get(&d_va, (size_t) nnz * 8))
		return 1;
	HIP_TRY(hipMemcpy(d_rp, rp, (size_t) (m + 1) * 4, hipMemcpyHostToDevice));
	if (nnz)
	{
		HIP_TRY(hipMemcpy(d_ci, ci, (size_t) nnz * 4, hipMemcpyHostToDevice));
		HIP_TRY(hipMemcpy(d_va, va, (size_t) nnz * 8, hipMemcpyHostToDevice));
	}
	if (transpose_csr_device(m, n, nnz, d_rp, d_ci, d_va, &d_rp_t, &d_ci_t, &d_va_t))
		return 1;
	out.ptrs = {d_rp_t, d_ci_t, d_va_t};
	in.release();
	rp_t.resize((size_t) n + 1);
	ci_t.resize((size_t) std::max<long>(nnz, 1));
	va_t.resize((size_t) std::max<long>(nnz, 1));
	HIP_TRY(hipMemcpy(rp_t.data(), d_rp_t, (size_t) (n + 1) * 4, hipMemcpyDeviceToHost));
	if (nnz)
	{
		HIP_TRY(hipMemcpy(ci_t.data(), d_ci_t, (size_t) nnz * 4, hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(va_t.data(), d_va_t, (size_t) nnz * 8, hipMemcpyDeviceToHost));
	}
	return 0;
}

// The checker of the above (opts.convert_on = 2): the same stable counting sort by column on the host. Counts through atomics (integer
// sums do not depend on their order); for the fill every thread owns a range of columns of about equal non-zeros and walks the whole
// matrix in entry order, so a column's entries land in ascending entry number whatever the thread count.
void
transpose_csr_host(long m, long n, long nnz, const int * rp, const int * ci, const double * va, std::vector<int> & rp_t, std::vector<int> & ci_t,
		std::vector<double> & va_t)
{
	rp_t.assign((size_t) n + 1, 0);
	ci_t.assign((size_t) std::max<long>(nnz, 1), 0);
	va_t.assign((size_t) std::max<long>(nnz, 1), 0.0);
	if (nnz == 0)
		return;
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(static, 4096)
	for (long e = 0; e < nnz; e++)
	{
		#pragma omp atomic
		rp_t[(size_t) ci[e] + 1]++;
	}
	for (long c = 0; c < n; c++)
		rp_t[(size_t) c + 1] += rp_t[(size_t) c];
	const int T = std::max(1, spmv::host_threads());
	std::vector<long> cut((size_t) T + 1, n);
	cut[0] = 0;
	for (int t = 1; t < T; t++)
		cut[(size_t) t] = std::lower_bound(rp_t.begin(), rp_t.end(), (int) (nnz * t / T)) - rp_t.begin();
	for (int t = 1; t <= T; t++)
		cut[(size_t) t] = std::min<long>(n, std::max(cut[(size_t) t], cut[(size_t) t - 1]));
	std::vector<int> pos(rp_t.begin(), rp_t.end() - 1);
	#pragma omp parallel for num_threads(T) schedule(static, 1)
	for (int t = 0; t < T; t++)
	{
		const long c0 = cut[(size_t) t], c1 = cut[(size_t) t + 1];
		if (c0 >= c1)
			continue;
		for (long i = 0; i < m; i++)
			for (long e = rp[i]; e < rp[i + 1]; e++)
			{
				const long c = ci[e];
				if (c < c0 || c >= c1)
					continue;
				const int k = pos[(size_t) c]++;
				ci_t[(size_t) k] = (int) i;
				va_t[(size_t) k] = va[e];
			}
	}
}

}  // namespace spmv

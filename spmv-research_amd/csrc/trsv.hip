// Sparse triangular solve handles (include/spmv_mi355x.h "sparse triangular solve"): the host analysis (levels and launch plan), the
// level-sliced layout of trsv.hpp, and the C ABI. Host code only; the kernels are in kernels_trsv.hip.
//
// THE PLAN. level[i] = 0 when row i has no kept off-diagonal entry, else 1 + the largest level among the rows those entries name;
// LOWER walks the rows upwards, UPPER downwards. A level of at most chain_rows rows is THIN. A maximal run of consecutive thin
// levels is one launch of one workgroup (trsv_chain_kernel), every other level is one launch with one lane per row
// (trsv_level_kernel). The launches of a solve go to one stream in level order and that order is the only thing that orders
// workgroups: no flag is spun on, there is no grid barrier, no cooperative or persistent kernel and no captured graph. A workgroup
// never waits for another one, so a solve cannot hang whatever else runs on the device.
//
// THE BLOCKED PLAN (trsv_create_blocked). Block b owns the rows [b B, min(n, (b + 1) B)); a kept entry (i, j) whose column lies in
// another block is dropped, and the level rule runs over what is left, block by block. No row of a block depends on a row of another
// one, so all blocks are solved by ONE launch with one workgroup per block (trsv_blocked_kernel), and again no workgroup waits for
// another one. What is lost is the dropped couplings: the handle solves the block-diagonal part of the triangle, exactly.

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "handle.hpp"
#include "solvers_common.hpp"
#include "trsv.hpp"

namespace spmv {

static bool
trsv_scalars_ok(const char * what, int uplo, const int * diag, const int * precision, long n, long chain_rows, bool blocked = false)
{
	if (uplo != SPMV_MI355X_LOWER && uplo != SPMV_MI355X_UPPER)
		set_error("%s: uplo must be SPMV_MI355X_LOWER (0) or SPMV_MI355X_UPPER (1) (got %d)", what, uplo);
	else if (diag && *diag != SPMV_MI355X_DIAG_STORED && *diag != SPMV_MI355X_DIAG_UNIT)
		set_error("%s: diag must be SPMV_MI355X_DIAG_STORED (0) or SPMV_MI355X_DIAG_UNIT (1) (got %d)", what, *diag);
	else if (precision && *precision != SPMV_MI355X_F64 && *precision != SPMV_MI355X_F32)
		set_error("%s: unknown precision %d", what, *precision);
	else if (n < 0 || n >= 0x7fffffffL)
		set_error("%s: n = %ld out of range [0, 2^31 - 1)", what, n);
	else if (blocked && (chain_rows < 0 || chain_rows > TRSV_BLOCK_ROWS_MAX))
		set_error("%s: block_rows must be 0 (the default) or 1 .. %d (got %ld)", what, TRSV_BLOCK_ROWS_MAX, chain_rows);
	else if (!blocked && (chain_rows < 0 || chain_rows > TRSV_CHAIN_ROWS_MAX))
		set_error("%s: chain_rows must be 0 (the default) or 1 .. %d (got %ld)", what, TRSV_CHAIN_ROWS_MAX, chain_rows);
	else
		return true;
	return false;
}

// row_ptr from 0 and monotone, columns in [0, n): the checks and the messages of spmv_mi355x_create
int
trsv_check_pattern(const char * what, long n, const int32_t * rp, const int32_t * ci)
{
	if (rp[0] != 0)
	{
		set_error("%s: row_ptr must start at 0 (got %d)", what, rp[0]);
		return 1;
	}
	long bad = -1;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(max : bad)
	for (long i = 0; i < n; i++)
		if (rp[i + 1] < rp[i])
			bad = std::max(bad, i);
	if (bad >= 0)
	{
		set_error("%s: row_ptr is not monotone at row %ld", what, bad);
		return 1;
	}
	const long nnz = rp[n];
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(max : bad)
	for (long j = 0; j < nnz; j++)
		if (ci[j] < 0 || ci[j] >= n)
			bad = std::max(bad, j);
	if (bad >= 0)
	{
		set_error("%s: column index %d out of range [0,%ld) at entry %ld", what, ci[bad], n, bad);
		return 1;
	}
	return 0;
}

// is entry (i, c) an off-diagonal entry of the chosen triangle?
static inline bool
trsv_dep(int uplo, long i, long c)
{
	return uplo == SPMV_MI355X_LOWER ? c < i : c > i;
}

// is it kept, i.e. a dependency of row i? B = block_rows of a blocked handle (the column must lie in the row's block), 0 otherwise
static inline bool
trsv_dep(int uplo, long i, long c, long B)
{
	return trsv_dep(uplo, i, c) && (B == 0 || c / B == i / B);
}

// O(nnz). The pattern has been checked.
void
trsv_analysis(int uplo, long n, const int32_t * rp, const int32_t * ci, int chain_rows, TrsvAnalysis & an)
{
	an.chain_rows = chain_rows ? chain_rows : TRSV_CHAIN_ROWS_DEFAULT;
	an.level_of_row.assign((size_t) n, 0);
	int32_t * level = an.level_of_row.data();
	int32_t top = -1;
	const bool lower = uplo == SPMV_MI355X_LOWER;
	for (long t = 0; t < n; t++)
	{
		const long i = lower ? t : n - 1 - t;
		int32_t lv = 0;
		for (long j = rp[i]; j < rp[i + 1]; j++)
			if (trsv_dep(uplo, i, ci[j]))
				lv = std::max(lv, level[ci[j]] + 1);
		level[i] = lv;
		top = std::max(top, lv);
	}
	an.levels = (long) top + 1;
	an.level_ptr.assign((size_t) an.levels + 1, 0);
	an.level_slice.assign((size_t) an.levels + 1, 0);
	for (long i = 0; i < n; i++)
		an.level_ptr[level[i] + 1]++;
	an.max_level_rows = 0;
	for (long l = 0; l < an.levels; l++)
	{
		const int32_t rows = an.level_ptr[l + 1];
		an.max_level_rows = std::max<long>(an.max_level_rows, rows);
		an.level_ptr[l + 1] = an.level_ptr[l] + rows;
		an.level_slice[l + 1] = an.level_slice[l] + (rows + TRSV_SLICE - 1) / TRSV_SLICE;
	}
	an.plan.clear();
	for (long l = 0; l < an.levels;)
	{
		const int rows = an.level_ptr[l + 1] - an.level_ptr[l];
		TrsvStep s;
		memset(&s, 0, sizeof(s));
		s.l0 = (int) l;
		if (rows > an.chain_rows)
		{
			s.l1 = (int) l + 1;
			s.pos0 = an.level_ptr[l];
			s.rows = rows;
			s.slice0 = an.level_slice[l];
			l++;
		}
		else
		{
			// the maximal run of thin levels from l on; its workgroup is as wide as the widest of them, in whole waves
			int widest = 0;
			long e = l;
			for (; e < an.levels && an.level_ptr[e + 1] - an.level_ptr[e] <= an.chain_rows; e++)
				widest = std::max(widest, an.level_ptr[e + 1] - an.level_ptr[e]);
			s.chain = 1;
			s.l1 = (int) e;
			s.block = std::min(TRSV_CHAIN_BLOCK_MAX, (widest + WAVE - 1) / WAVE * WAVE);
			l = e;
		}
		an.plan.push_back(s);
	}
}

// The blocked plan, O(nnz); block_rows = 0 is the default. The blocks are independent of each other.
void
trsv_analysis_blocked(int uplo, long n, const int32_t * rp, const int32_t * ci, long block_rows, TrsvAnalysis & an)
{
	const long B = block_rows ? block_rows : TRSV_BLOCK_ROWS_DEFAULT;
	const long blocks = (n + B - 1) / B;
	const bool lower = uplo == SPMV_MI355X_LOWER;
	an.block_rows = B;
	an.blocks = blocks;
	an.level_of_row.assign((size_t) n, 0);
	an.block_level.assign((size_t) blocks + 1, 0);
	int32_t * level = an.level_of_row.data();
	long dropped = 0;
	// the level of a row WITHIN its block, and the levels of every block
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(+ : dropped) schedule(dynamic, 16)
	for (long blk = 0; blk < blocks; blk++)
	{
		const long r0 = blk * B, r1 = std::min(n, r0 + B);
		int32_t top = -1;
		for (long t = r0; t < r1; t++)
		{
			const long i = lower ? t : r1 - 1 - (t - r0);
			int32_t lv = 0;
			for (long j = rp[i]; j < rp[i + 1]; j++)
				if (trsv_dep(uplo, i, ci[j], B))
					lv = std::max(lv, level[ci[j]] + 1);
				else if (trsv_dep(uplo, i, ci[j]))
					dropped++;
			level[i] = lv;
			top = std::max(top, lv);
		}
		an.block_level[blk + 1] = top + 1;
	}
	an.nnz_dropped = dropped;
	an.max_block_levels = 0;
	for (long blk = 0; blk < blocks; blk++)
	{
		an.max_block_levels = std::max<long>(an.max_block_levels, an.block_level[blk + 1]);
		an.block_level[blk + 1] += an.block_level[blk];
	}
	an.levels = blocks ? an.block_level[blocks] : 0;
	// from here on level_of_row numbers the levels through all blocks; the callers that report it subtract block_level again
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(static, 4096)
	for (long i = 0; i < n; i++)
		level[i] += an.block_level[i / B];
	an.level_ptr.assign((size_t) an.levels + 1, 0);
	an.level_slice.assign((size_t) an.levels + 1, 0);
	for (long i = 0; i < n; i++)
		an.level_ptr[level[i] + 1]++;
	an.max_level_rows = 0;
	for (long l = 0; l < an.levels; l++)
	{
		const int32_t rows = an.level_ptr[l + 1];
		an.max_level_rows = std::max<long>(an.max_level_rows, rows);
		an.level_ptr[l + 1] = an.level_ptr[l] + rows;
		an.level_slice[l + 1] = an.level_slice[l] + (rows + TRSV_SLICE - 1) / TRSV_SLICE;
	}
}

}  // namespace spmv

using namespace spmv;

namespace spmv {

// STORED: the diagonal of row i is the first stored entry with column i (the rule of jacobi_diagonal); it must exist, be finite and
// non-zero after narrowing to the handle's precision, and be the only entry with column i. The first bad row is reported.
// va == nullptr checks the pattern alone (a diagonal in every row, stored once): what update_values_prepare can know.
template <typename T>
static int
trsv_check_diagonal(const char * what, long n, const int32_t * rp, const int32_t * ci, const double * va)
{
	long bad = n;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(min : bad) schedule(static, 4096)
	for (long i = 0; i < n; i++)
	{
		long at = -1;
		bool twice = false;
		for (long j = rp[i]; j < rp[i + 1]; j++)
			if (ci[j] == i)
			{
				twice = twice || at >= 0;
				if (at < 0)
					at = j;
			}
		const T d = at >= 0 && va ? (T) va[at] : (T) (va ? 0 : 1);
		if (at < 0 || twice || !std::isfinite(d) || d == 0)
			bad = std::min(bad, i);
	}
	if (bad == n)
		return 0;
	long at = -1, count = 0;
	for (long j = rp[bad]; j < rp[bad + 1]; j++)
		if (ci[j] == bad)
		{
			if (at < 0)
				at = j;
			count++;
		}
	if (at < 0)
		set_error("%s: row %ld has no diagonal entry (SPMV_MI355X_DIAG_STORED needs one in every row)", what, bad);
	else if (count > 1)
		set_error("%s: row %ld stores %ld entries with column %ld: the diagonal must be stored once", what, bad, count, bad);
	else
		set_error("%s: the diagonal of row %ld is %g in the handle's precision (from %g): it must be finite and non-zero", what, bad,
				(double) (T) va[at], va[at]);
	return 1;
}

// THE LAYOUT OF trsv.hpp, WRITTEN ONCE: everything trsv_build stores except the numbers. Instead of values it yields where every
// stored value comes from: slot_src[e] = the entry of the caller's CSR in slot e of val (-1: padding), diag_src[p] = the first stored
// entry of row perm[p] with column perm[p] (-1: none; filled under STORED only). trsv_build narrows the values through these maps and
// update_values (below) uploads them, so a handle updated on the GPU holds what create would have built.
struct TrsvLayout {
	std::vector<int32_t> perm, len, col, slot_src, diag_src;
	std::vector<int32_t> slice_pos;       // slices + 1: slice s holds the positions [slice_pos[s], slice_pos[s + 1])
	std::vector<int64_t> slice_ptr;       // slices + 1
	long slices = 0, kept = 0;
};

static void
trsv_layout(int uplo, bool stored, long B /* 0: a global handle */, long n, const TrsvAnalysis & an, const int32_t * rp,
		const int32_t * ci, TrsvLayout & L)
{
	const long levels = an.levels;
	const long slices = levels ? an.level_slice[levels] : 0;
	L.slices = slices;
	L.perm.assign((size_t) n, 0);
	L.len.assign((size_t) n, 0);
	L.diag_src.assign(stored ? (size_t) n : 0, -1);
	std::vector<int32_t> & perm = L.perm, & len = L.len;
	{
		std::vector<int32_t> next(an.level_ptr.begin(), an.level_ptr.end());
		for (long i = 0; i < n; i++)                 // ascending rows: (level, row) order
			perm[next[an.level_of_row[i]]++] = (int32_t) i;
	}
	long kept = 0;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(+ : kept) schedule(static, 4096)
	for (long p = 0; p < n; p++)
	{
		const long i = perm[p];
		int32_t c = 0;
		bool have = false;
		for (long j = rp[i]; j < rp[i + 1]; j++)
		{
			c += trsv_dep(uplo, i, ci[j], B);
			if (stored && !have && ci[j] == i)
			{
				L.diag_src[p] = (int32_t) j;
				have = true;
			}
		}
		len[p] = c;
		kept += c;
	}
	L.kept = kept;
	L.slice_pos.assign((size_t) slices + 1, 0);
	std::vector<int32_t> & slice_pos = L.slice_pos;
	for (long l = 0; l < levels; l++)
		for (long s = an.level_slice[l]; s < an.level_slice[l + 1]; s++)
			slice_pos[s] = an.level_ptr[l] + (int32_t) (s - an.level_slice[l]) * TRSV_SLICE;
	slice_pos[slices] = (int32_t) n;
	// the last slice of a level ends where the level ends
	L.slice_ptr.assign((size_t) slices + 1, 0);
	std::vector<int64_t> & slice_ptr = L.slice_ptr;
	auto slice_end = [&](long s, long l) { return std::min<long>(slice_pos[s] + TRSV_SLICE, an.level_ptr[l + 1]); };
	for (long l = 0; l < levels; l++)
		for (long s = an.level_slice[l]; s < an.level_slice[l + 1]; s++)
		{
			int32_t w = 0;
			for (long p = slice_pos[s]; p < slice_end(s, l); p++)
				w = std::max(w, len[p]);
			slice_ptr[s + 1] = (int64_t) w * (slice_end(s, l) - slice_pos[s]);     // prefix-summed below
		}
	for (long s = 0; s < slices; s++)
		slice_ptr[s + 1] += slice_ptr[s];
	const size_t stored_entries = (size_t) slice_ptr[slices];
	L.col.assign(stored_entries, 0);
	L.slot_src.assign(stored_entries, -1);
	std::vector<int32_t> level_of_slice((size_t) slices);
	for (long l = 0; l < levels; l++)
		for (long s = an.level_slice[l]; s < an.level_slice[l + 1]; s++)
			level_of_slice[s] = (int32_t) l;
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(dynamic, 64)
	for (long s = 0; s < slices; s++)
	{
		const long p0 = slice_pos[s], lanes = slice_end(s, level_of_slice[s]) - p0;
		for (long r = 0; r < lanes; r++)
		{
			const long i = perm[p0 + r];
			int64_t e = slice_ptr[s] + r;
			for (long j = rp[i]; j < rp[i + 1]; j++)
				if (trsv_dep(uplo, i, ci[j], B))
				{
					L.slot_src[e] = (int32_t) j;
					L.col[e] = B ? (int32_t) (ci[j] - i / B * B) : ci[j];     // blocked: the column within the block
					e += lanes;
				}
		}
	}
}

template <typename T>
static int
trsv_build(spmv_mi355x_trsv * H, const TrsvAnalysis & an, const int32_t * rp, const int32_t * ci, const double * va)
{
	const long n = H->n;
	const bool stored = H->diag == SPMV_MI355X_DIAG_STORED;
	const long B = H->block_rows;         // 0: a global handle
	TrsvLayout L;
	trsv_layout(H->uplo, stored, B, n, an, rp, ci, L);
	const std::vector<int32_t> & perm = L.perm, & len = L.len, & col = L.col;
	const std::vector<int64_t> & slice_ptr = L.slice_ptr;
	const size_t stored_entries = L.slot_src.size();
	H->nnz_kept = L.kept + (stored ? n : 0);
	H->slices = L.slices;
	H->slots = (long) stored_entries;
	H->nnz_csr = rp[n];
	// the numbers, through the maps; narrowed as spmv_mi355x_create narrows. Padding stays zero.
	std::vector<T> val(stored_entries, (T) 0), diag(stored ? (size_t) n : 0);
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(static, 4096)
	for (size_t e = 0; e < stored_entries; e++)
		if (L.slot_src[e] >= 0)
			val[e] = (T) va[L.slot_src[e]];
	#pragma omp parallel for num_threads(spmv::host_threads()) schedule(static, 4096)
	for (size_t p = 0; p < diag.size(); p++)
		diag[p] = (T) va[L.diag_src[p]];              // trsv_check_diagonal has seen a diagonal in every row
	struct Up { const void * src; size_t bytes; } ups[9] = {
		{val.data(), stored_entries * sizeof(T)}, {col.data(), stored_entries * sizeof(int32_t)},
		{slice_ptr.data(), slice_ptr.size() * sizeof(int64_t)}, {len.data(), (size_t) n * sizeof(int32_t)},
		{perm.data(), (size_t) n * sizeof(int32_t)}, {diag.data(), diag.size() * sizeof(T)},
		{an.level_ptr.data(), an.level_ptr.size() * sizeof(int32_t)}, {an.level_slice.data(), an.level_slice.size() * sizeof(int32_t)},
		{an.block_level.data(), an.block_level.size() * sizeof(int32_t)}};
	H->mem_footprint = 0;
	for (int k = 0; k < 9; k++)
	{
		if ((k == 5 && !stored) || (k == 8 && !B))
			continue;
		if (upload_bytes(ups[k].src, ups[k].bytes, 0, &H->owned[k]))
			return 1;
		H->mem_footprint += (double) ups[k].bytes;
	}
	H->arr.val = H->owned[0];
	H->arr.col = (const int *) H->owned[1];
	H->arr.slice_ptr = (const int64_t *) H->owned[2];
	H->arr.len = (const int *) H->owned[3];
	H->arr.perm = (const int *) H->owned[4];
	H->arr.diag = H->owned[5];
	H->arr.level_ptr = (const int *) H->owned[6];
	H->arr.level_slice = (const int *) H->owned[7];
	H->arr.block_level = (const int *) H->owned[8];
	return 0;
}

static void
trsv_free(spmv_mi355x_trsv * H)
{
	for (void * p : H->owned)
		if (p)
			(void) hipFree(p);
	if (H->d_b)
		(void) hipFree(H->d_b);
	if (H->d_x)
		(void) hipFree(H->d_x);
	if (H->d_bk)
		(void) hipFree(H->d_bk);
	if (H->d_xk)
		(void) hipFree(H->d_xk);
	for (void * p : {(void *) H->upd_slot_src, (void *) H->upd_diag_src, (void *) H->upd_status, (void *) H->upd_values,
			(void *) H->swp_slice_pos, H->swp_keep, H->swp_buf})
		if (p)
			(void) hipFree(p);
	if (H->upd_done)
		(void) hipEventDestroy(H->upd_done);
	delete H;
}

// The checks 1 to 3 and the analysis of both analyze entries; rows = chain_rows, or block_rows of the blocked form. level_of_row_out
// receives the levels as the caller counts them: within the row's block for the blocked form.
static int
trsv_analyze_checked(const char * what, bool blocked, int uplo, long n, const int32_t * row_ptr, const int32_t * col_idx, long rows,
		int32_t ** level_of_row_out, TrsvAnalysis & an)
{
	if (level_of_row_out)
		*level_of_row_out = nullptr;
	if (!trsv_scalars_ok(what, uplo, nullptr, nullptr, n, rows, blocked))
		return 1;
	if (!row_ptr || (!col_idx && row_ptr[n] > 0))
	{
		set_error("%s: NULL argument (%s%s )", what, !row_ptr ? " row_ptr" : "", !col_idx ? " col_idx" : "");
		return 1;
	}
	if (trsv_check_pattern(what, n, row_ptr, col_idx))
		return 1;
	if (blocked)
		trsv_analysis_blocked(uplo, n, row_ptr, col_idx, rows, an);
	else
		trsv_analysis(uplo, n, row_ptr, col_idx, (int) rows, an);
	if (level_of_row_out)
	{
		int32_t * lv = (int32_t *) malloc(std::max<size_t>((size_t) n, 1) * sizeof(int32_t));
		if (!lv)
		{
			set_error("%s: out of host memory (%ld levels of rows)", what, n);
			return 1;
		}
		for (long i = 0; i < n; i++)
			lv[i] = an.level_of_row[i] - (blocked ? an.block_level[i / an.block_rows] : 0);
		*level_of_row_out = lv;
	}
	return 0;
}

// both create entries; rows = chain_rows, or block_rows of the blocked form
static int
trsv_create(const char * what, bool blocked, spmv_mi355x_trsv ** out, int uplo, int diag, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values, long rows, int device)
{
	if (out)
		*out = nullptr;
	// 1. scalars, 2. NULL pointers, 3. the pattern, 4. the diagonal: all on the host; 5. the device
	if (!trsv_scalars_ok(what, uplo, &diag, &precision, n, rows, blocked))
		return 1;
	const bool entries = row_ptr && row_ptr[n] > 0;
	if (!out || !row_ptr || (entries && (!col_idx || !values)))
	{
		set_error("%s: NULL argument (%s%s%s%s )", what, !out ? " out" : "", !row_ptr ? " row_ptr" : "",
				entries && !col_idx ? " col_idx" : "", entries && !values ? " values" : "");
		return 1;
	}
	if (trsv_check_pattern(what, n, row_ptr, col_idx))
		return 1;
	const bool f32 = precision == SPMV_MI355X_F32;
	if (diag == SPMV_MI355X_DIAG_STORED && (f32 ? trsv_check_diagonal<float>(what, n, row_ptr, col_idx, values)
	                                            : trsv_check_diagonal<double>(what, n, row_ptr, col_idx, values)))
		return 1;
	int ndev = 0;
	spmv_mi355x_device_count(&ndev);
	if (ndev < 1)
	{
		set_error("%s: no HIP device available: this engine has no CPU fallback", what);
		return 1;
	}
	if (device < 0)
		HIP_TRY(hipGetDevice(&device));
	if (device >= ndev)
	{
		set_error("%s: device %d out of range (%d devices)", what, device, ndev);
		return 1;
	}
	HIP_TRY(hipSetDevice(device));
	TrsvAnalysis an;
	if (blocked)
		trsv_analysis_blocked(uplo, n, row_ptr, col_idx, rows, an);
	else
		trsv_analysis(uplo, n, row_ptr, col_idx, (int) rows, an);
	spmv_mi355x_trsv * H = new spmv_mi355x_trsv();
	H->uplo = uplo;
	H->diag = diag;
	H->precision = precision;
	H->f32 = f32;
	H->device = device;
	H->n = n;
	H->levels = blocked ? an.max_block_levels : an.levels;
	H->levels_total = an.levels;
	H->max_level_rows = an.max_level_rows;
	H->chain_rows = an.chain_rows;
	H->plan = an.plan;
	H->block_rows = an.block_rows;
	H->blocks = an.blocks;
	H->nnz_dropped = an.nnz_dropped;
	// one width for the whole launch: the widest level of any block in whole waves, at least one wave
	H->threads = (int) std::min<long>(TRSV_BLOCKED_THREADS_MAX, std::max<long>(WAVE, (an.max_level_rows + WAVE - 1) / WAVE * WAVE));
	if (f32 ? trsv_build<float>(H, an, row_ptr, col_idx, values) : trsv_build<double>(H, an, row_ptr, col_idx, values))
	{
		trsv_free(H);
		return 1;
	}
	*out = H;
	return 0;
}

// Jacobi sweeps (below): what the solve entries run in the place of the exact plan after trsv_set_sweeps
static int trsv_sweeps_run(spmv_mi355x_trsv * T, int sweeps, int k, const void * b, long ldb, void * x, long ldx, hipStream_t st);

}  // namespace spmv

extern "C" {

int
spmv_mi355x_trsv_analyze(int uplo, long n, const int32_t * row_ptr, const int32_t * col_idx, int chain_rows,
		int32_t ** level_of_row_out, long * levels_out, long * launches_out, long * max_level_rows_out, int * chain_rows_used_out)
{
	TrsvAnalysis an;
	if (trsv_analyze_checked("trsv_analyze", false, uplo, n, row_ptr, col_idx, chain_rows, level_of_row_out, an))
		return 1;
	if (levels_out)
		*levels_out = an.levels;
	if (launches_out)
		*launches_out = (long) an.plan.size();
	if (max_level_rows_out)
		*max_level_rows_out = an.max_level_rows;
	if (chain_rows_used_out)
		*chain_rows_used_out = an.chain_rows;
	return 0;
}

int
spmv_mi355x_trsv_analyze_blocked(int uplo, long n, const int32_t * row_ptr, const int32_t * col_idx, long block_rows,
		int32_t ** level_of_row_out, long * blocks_out, long * max_block_levels_out, long * max_level_rows_out, long * nnz_dropped_out,
		long * block_rows_used_out)
{
	TrsvAnalysis an;
	if (trsv_analyze_checked("trsv_analyze_blocked", true, uplo, n, row_ptr, col_idx, block_rows, level_of_row_out, an))
		return 1;
	if (blocks_out)
		*blocks_out = an.blocks;
	if (max_block_levels_out)
		*max_block_levels_out = an.max_block_levels;
	if (max_level_rows_out)
		*max_level_rows_out = an.max_level_rows;
	if (nnz_dropped_out)
		*nnz_dropped_out = an.nnz_dropped;
	if (block_rows_used_out)
		*block_rows_used_out = an.block_rows;
	return 0;
}

int
spmv_mi355x_trsv_create(spmv_mi355x_trsv ** out, int uplo, int diag, int precision, long n, const int32_t * row_ptr,
		const int32_t * col_idx, const double * values, int chain_rows, int device)
{
	return trsv_create("trsv_create", false, out, uplo, diag, precision, n, row_ptr, col_idx, values, chain_rows, device);
}

int
spmv_mi355x_trsv_create_blocked(spmv_mi355x_trsv ** out, int uplo, int diag, int precision, long n, const int32_t * row_ptr,
		const int32_t * col_idx, const double * values, long block_rows, int device)
{
	return trsv_create("trsv_create_blocked", true, out, uplo, diag, precision, n, row_ptr, col_idx, values, block_rows, device);
}

int
spmv_mi355x_trsv_block_info(const spmv_mi355x_trsv * T, long * block_rows_out, long * blocks_out, long * max_block_levels_out,
		long * nnz_dropped_out)
{
	if (!T)
	{
		set_error("trsv_block_info: NULL handle");
		return 1;
	}
	if (block_rows_out)
		*block_rows_out = T->block_rows;
	if (blocks_out)
		*blocks_out = T->blocks;
	if (max_block_levels_out)
		*max_block_levels_out = T->block_rows ? T->levels : 0;
	if (nnz_dropped_out)
		*nnz_dropped_out = T->nnz_dropped;
	return 0;
}

int
spmv_mi355x_trsv_destroy(spmv_mi355x_trsv * T)
{
	if (!T)
		return 0;
	(void) hipSetDevice(T->device);
	trsv_free(T);
	return 0;
}

int
spmv_mi355x_trsv_solve_device_async(spmv_mi355x_trsv * T, const void * b_dev, void * x_dev, void * hip_stream)
{
	if (!T || (T->n > 0 && (!b_dev || !x_dev)))
	{
		set_error("trsv_solve: NULL argument (%s%s%s )", !T ? " T" : "", T && !b_dev ? " b" : "", T && !x_dev ? " x" : "");
		return 1;
	}
	if (T->block_rows ? T->n == 0 : T->plan.empty())
		return 0;
	if (T->sweeps > 0)        // trsv_set_sweeps: the Jacobi-sweep approximation in the place of the exact plan
		return trsv_sweeps_run(T, T->sweeps, 1, b_dev, 1, x_dev, 1, (hipStream_t) hip_stream);
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != T->device)
		HIP_TRY(hipSetDevice(T->device));
	hipStream_t st = (hipStream_t) hip_stream;
	const bool unit = T->diag == SPMV_MI355X_DIAG_UNIT;
	if (T->block_rows)
		return launch_trsv_blocked(T->f32, unit, T->arr, T->blocks, T->threads, T->block_rows, T->n, b_dev, x_dev, st);
	for (const TrsvStep & s : T->plan)
		s.chain ? launch_trsv_chain(T->f32, unit, T->arr, s, b_dev, x_dev, st) : launch_trsv_level(T->f32, unit, T->arr, s, b_dev, x_dev, st);
	HIP_TRY(hipGetLastError());
	return 0;
}

int
spmv_mi355x_trsv_solve(spmv_mi355x_trsv * T, const void * b_host, void * x_host)
{
	if (!T || (T->n > 0 && (!b_host || !x_host)))
	{
		set_error("trsv_solve: NULL argument (%s%s%s )", !T ? " T" : "", T && !b_host ? " b" : "", T && !x_host ? " x" : "");
		return 1;
	}
	if (T->n == 0)
		return 0;
	HIP_TRY(hipSetDevice(T->device));
	const size_t bytes = (size_t) T->n * (T->f32 ? 4 : 8);
	if (!T->d_b && (dev_alloc_bytes(&T->d_b, bytes) || dev_alloc_bytes(&T->d_x, bytes)))
		return 1;
	HIP_TRY(hipMemcpyAsync(T->d_b, b_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (spmv_mi355x_trsv_solve_device_async(T, T->d_b, T->d_x, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(x_host, T->d_x, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

int
spmv_mi355x_trsv_info(const spmv_mi355x_trsv * T, long * n_out, long * nnz_kept_out, long * levels_out, long * launches_out,
		long * max_level_rows_out, int * chain_rows_out)
{
	if (!T)
	{
		set_error("trsv_info: NULL handle");
		return 1;
	}
	if (n_out)
		*n_out = T->n;
	if (nnz_kept_out)
		*nnz_kept_out = T->nnz_kept;
	if (levels_out)
		*levels_out = T->levels;
	if (launches_out)
		*launches_out = T->block_rows ? (T->n > 0 ? 1 : 0) : (long) T->plan.size();
	if (max_level_rows_out)
		*max_level_rows_out = T->max_level_rows;
	if (chain_rows_out)
		*chain_rows_out = T->block_rows ? 0 : T->chain_rows;
	return 0;
}

double
spmv_mi355x_trsv_mem_footprint(const spmv_mi355x_trsv * T)
{
	return T ? T->mem_footprint : 0;
}

int
spmv_mi355x_time_trsv_device(spmv_mi355x_trsv * T, const void * b_dev, void * x_dev, int iters, void * hip_stream, double * ms_out)
{
	if (!T || !ms_out)
	{
		set_error("time_trsv_device: NULL %s", !T ? "handle" : "ms_per_iter_out");
		return 1;
	}
	HIP_TRY(hipSetDevice(T->device));
	hipStream_t st = (hipStream_t) hip_stream;
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	HIP_TRY(hipEventCreate(&e1));
	HIP_TRY(hipEventRecord(e0, st));
	for (int i = 0; i < iters; i++)
		if (spmv_mi355x_trsv_solve_device_async(T, b_dev, x_dev, hip_stream))
			return 1;
	HIP_TRY(hipEventRecord(e1, st));
	HIP_TRY(hipEventSynchronize(e1));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	*ms_out = iters > 0 ? (double) ms / iters : 0;
	return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ k columns

namespace spmv {

// The passes of a k-column solve. A global handle: column_chunks(k), 8s and then the binary remainder. A blocked handle: the same
// with Kmax = trsv_blocked_kmax() in the place of 8, since a workgroup keeps its rows of the chunk in LDS.
static std::vector<Chunk>
trsv_multi_chunks(const spmv_mi355x_trsv * T, int k)
{
	if (!T->block_rows)
		return column_chunks(k);
	const int kmax = trsv_blocked_kmax(T->block_rows, T->n, T->f32);
	std::vector<Chunk> out;
	int c0 = 0;
	for (; k - c0 >= kmax; c0 += kmax)
		out.push_back({c0, kmax});
	for (int w = kmax / 2; w >= 1; w /= 2)
		if (k - c0 >= w)
		{
			out.push_back({c0, w});
			c0 += w;
		}
	return out;
}

// the refusals of the k-column solve entries, all on the host, in the header's order
static bool
trsv_multi_arguments_ok(const char * what, const spmv_mi355x_trsv * T, int k, const void * b, long ldb, const void * x, long ldx)
{
	if (!T)
		set_error("%s: NULL argument ( T )", what);
	else if (k < 1)
		set_error("%s: k = %d: at least one column is needed", what, k);
	else if (ldb < k || ldx < k)
		set_error("%s: ldb = %ld, ldx = %ld: a leading dimension must be at least k = %d", what, ldb, ldx, k);
	else if (b == x && ldb != ldx)
		set_error("%s: b == x (in place) needs ldb == ldx (got %ld and %ld)", what, ldb, ldx);
	else if (T->n > 0 && (!b || !x))
		set_error("%s: NULL argument (%s%s )", what, !b ? " b" : "", !x ? " x" : "");
	else
		return true;
	return false;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_trsv_solve_multi_device_async(spmv_mi355x_trsv * T, int k, const void * b_dev, long ldb, void * x_dev, long ldx,
		void * hip_stream)
{
	if (!trsv_multi_arguments_ok("trsv_solve_multi", T, k, b_dev, ldb, x_dev, ldx))
		return 1;
	if (T->n == 0)
		return 0;
	if (T->sweeps > 0)
		return trsv_sweeps_run(T, T->sweeps, k, b_dev, ldb, x_dev, ldx, (hipStream_t) hip_stream);
	// One contiguous column is a vector: the single solve with its kernels, so k = 1 costs what the single call costs. The KC = 1
	// kernels serve a column of a wider block (ld > 1), such as the last one of k = 9; profiles/r28_trsv_multi.txt has their cost.
	if (k == 1 && ldb == 1 && ldx == 1)
		return spmv_mi355x_trsv_solve_device_async(T, b_dev, x_dev, hip_stream);
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != T->device)
		HIP_TRY(hipSetDevice(T->device));
	hipStream_t st = (hipStream_t) hip_stream;
	const bool unit = T->diag == SPMV_MI355X_DIAG_UNIT;
	for (const Chunk & ch : trsv_multi_chunks(T, k))
	{
		const TrsvCols cols = {b_dev, x_dev, ldb, ldx, ch.c0, ch.kc};
		if (T->block_rows)
		{
			if (launch_trsv_blocked_multi(T->f32, unit, T->arr, T->blocks, T->threads, T->block_rows, T->n, cols, st))
				return 1;
			continue;
		}
		for (const TrsvStep & s : T->plan)
			s.chain ? launch_trsv_chain_multi(T->f32, unit, T->arr, s, cols, st) : launch_trsv_level_multi(T->f32, unit, T->arr, s, cols, st);
	}
	HIP_TRY(hipGetLastError());
	return 0;
}

}  // extern "C"

namespace spmv {

// The blocking host form of a k-column solve, arguments checked, n > 0: the two device blocks (ld = k), the copies, and between them
// the solve under the handle's setting (sweeps = 0) or `sweeps` Jacobi sweeps whatever the setting is.
static int
trsv_solve_multi_staged(spmv_mi355x_trsv * T, int sweeps, int k, const void * B_host, void * X_host)
{
	HIP_TRY(hipSetDevice(T->device));
	if (k > T->block_k)
	{
		// the blocks of an earlier, smaller k may still be read by a solve in flight
		HIP_TRY(hipDeviceSynchronize());
		for (void ** p : {&T->d_bk, &T->d_xk})
		{
			if (*p)
				(void) hipFree(*p);
			*p = nullptr;
		}
		T->block_k = 0;
		const size_t grown = (size_t) T->n * (size_t) k * (T->f32 ? 4 : 8);
		if (dev_alloc_bytes(&T->d_bk, grown) || dev_alloc_bytes(&T->d_xk, grown))
			return 1;
		T->block_k = k;
	}
	const size_t bytes = (size_t) T->n * (size_t) k * (T->f32 ? 4 : 8);
	HIP_TRY(hipMemcpyAsync(T->d_bk, B_host, bytes, hipMemcpyHostToDevice, nullptr));
	if (sweeps > 0 ? trsv_sweeps_run(T, sweeps, k, T->d_bk, k, T->d_xk, k, nullptr)
	               : spmv_mi355x_trsv_solve_multi_device_async(T, k, T->d_bk, k, T->d_xk, k, nullptr))
		return 1;
	HIP_TRY(hipMemcpyAsync(X_host, T->d_xk, bytes, hipMemcpyDeviceToHost, nullptr));
	HIP_TRY(hipStreamSynchronize(nullptr));
	return 0;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_trsv_solve_multi(spmv_mi355x_trsv * T, int k, const void * B_host, void * X_host)
{
	if (!trsv_multi_arguments_ok("trsv_solve_multi", T, k, B_host, k, X_host, k))
		return 1;
	if (T->n == 0)
		return 0;
	return trsv_solve_multi_staged(T, 0, k, B_host, X_host);
}

int
spmv_mi355x_trsv_solve_multi_plan(const spmv_mi355x_trsv * T, int k, long * matrix_passes_out, long * launches_out, int * max_chunk_out)
{
	if (!T)
	{
		set_error("trsv_solve_multi_plan: NULL argument ( T )");
		return 1;
	}
	if (k < 1)
	{
		set_error("trsv_solve_multi_plan: k = %d: at least one column is needed", k);
		return 1;
	}
	long passes = 0, launches = 0;
	int widest = 0;                   // the widest chunk the handle serves, whatever k is
	if (T->n > 0)
	{
		passes = (long) trsv_multi_chunks(T, k).size();
		launches = T->block_rows ? passes : passes * (long) T->plan.size();
		widest = T->block_rows ? trsv_blocked_kmax(T->block_rows, T->n, T->f32) : MAX_KC;
	}
	if (matrix_passes_out)
		*matrix_passes_out = passes;
	if (launches_out)
		*launches_out = launches;
	if (max_chunk_out)
		*max_chunk_out = widest;
	return 0;
}

int
spmv_mi355x_time_trsv_multi_device(spmv_mi355x_trsv * T, int k, const void * b_dev, long ldb, void * x_dev, long ldx, int iters,
		void * hip_stream, double * ms_out)
{
	if (!T || !ms_out)
	{
		set_error("time_trsv_multi_device: NULL %s", !T ? "handle" : "ms_per_iter_out");
		return 1;
	}
	if (!trsv_multi_arguments_ok("trsv_solve_multi", T, k, b_dev, ldb, x_dev, ldx))
		return 1;
	HIP_TRY(hipSetDevice(T->device));
	hipStream_t st = (hipStream_t) hip_stream;
	hipEvent_t e0, e1;
	HIP_TRY(hipEventCreate(&e0));
	HIP_TRY(hipEventCreate(&e1));
	HIP_TRY(hipEventRecord(e0, st));
	for (int i = 0; i < iters; i++)
		if (spmv_mi355x_trsv_solve_multi_device_async(T, k, b_dev, ldb, x_dev, ldx, hip_stream))
			return 1;
	HIP_TRY(hipEventRecord(e1, st));
	HIP_TRY(hipEventSynchronize(e1));
	float ms = 0;
	HIP_TRY(hipEventElapsedTime(&ms, e0, e1));
	(void) hipEventDestroy(e0);
	(void) hipEventDestroy(e1);
	*ms_out = iters > 0 ? (double) ms / iters : 0;
	return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ Jacobi sweeps

namespace spmv {

// min(sweeps, levels): from `levels` sweeps on no bit changes, so more are never run. 0 at n = 0.
static long
trsv_sweeps_effective(const spmv_mi355x_trsv * T, long sweeps)
{
	return std::min<long>(sweeps, T->levels);
}

static bool
trsv_sweeps_in_range(const char * what, int sweeps, int lowest)
{
	if (sweeps >= lowest && sweeps <= TRSV_SWEEPS_MAX)
		return true;
	set_error("%s: sweeps = %d: must be in %d .. %d", what, sweeps, lowest, TRSV_SWEEPS_MAX);
	return false;
}

// The slice -> position map (at the first sweep solve) and the scratch of a chunk of kc columns (at the first solve of more than
// one sweep, regrown for a wider chunk): two n x kc blocks with ld = kc, `keep` for the b of an in-place solve and `buf` for the
// sweeps that do not write x.
static int
trsv_sweeps_prepare(spmv_mi355x_trsv * T, int kc, bool scratch, hipStream_t st)
{
	if (!T->swp_slice_pos)
	{
		const size_t bytes = (size_t) (T->slices + 1) * sizeof(int);
		void * p = nullptr;
		if (dev_alloc_bytes(&p, bytes))
			return 1;
		if (launch_trsv_sweep_map(T->arr, T->levels_total, T->slices, T->n, (int *) p, st))
		{
			(void) hipFree(p);
			return 1;
		}
		// once per handle: a later solve may come on another stream
		const hipError_t built = hipStreamSynchronize(st);
		if (built != hipSuccess)
		{
			(void) hipFree(p);
			set_error("trsv_solve_sweeps: the slice map could not be built: %s", hipGetErrorString(built));
			return 1;
		}
		T->swp_slice_pos = (int *) p;
		T->swp_bytes += (double) bytes;
	}
	if (scratch && kc > T->swp_k)
	{
		const size_t esz = T->f32 ? 4 : 8;
		// the blocks of an earlier, narrower chunk may still be read by a solve in flight
		HIP_TRY(hipDeviceSynchronize());
		for (void ** p : {&T->swp_keep, &T->swp_buf})
		{
			if (*p)
				(void) hipFree(*p);
			*p = nullptr;
		}
		T->swp_bytes -= 2.0 * (double) T->n * T->swp_k * esz;
		T->swp_k = 0;
		const size_t grown = (size_t) T->n * (size_t) kc * esz;
		if (dev_alloc_bytes(&T->swp_keep, grown) || dev_alloc_bytes(&T->swp_buf, grown))
			return 1;
		T->swp_k = kc;
		T->swp_bytes += 2.0 * (double) grown;
	}
	return 0;
}

// The sweep solve of k columns, arguments checked, n > 0. THE BUFFERS: sweep m of S writes x when S - m is even and buf otherwise,
// and reads what sweep m - 1 wrote, so no sweep reads the block it writes and the last one writes x; x doubles as the second
// ping-pong buffer, and only the k columns of x are ever written in the caller's memory. b is read by every sweep: in place
// (b == x) the first sweep copies it to keep in the pass that reads it, and the later sweeps read keep.
static int
trsv_sweeps_run(spmv_mi355x_trsv * T, int sweeps, int k, const void * b, long ldb, void * x, long ldx, hipStream_t st)
{
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != T->device)
		HIP_TRY(hipSetDevice(T->device));
	const long S = trsv_sweeps_effective(T, sweeps);
	const std::vector<Chunk> chunks = column_chunks(k);
	if (trsv_sweeps_prepare(T, chunks[0].kc, S > 1, st))
		return 1;
	const bool unit = T->diag == SPMV_MI355X_DIAG_UNIT, in_place = b == x;
	const size_t esz = T->f32 ? 4 : 8;
	for (const Chunk & ch : chunks)
	{
		const void * bc = (const char *) b + (size_t) ch.c0 * esz;
		void * xc = (char *) x + (size_t) ch.c0 * esz;
		TrsvSweep s = {};
		s.kc = ch.kc;
		for (long m = 1; m <= S; m++)
		{
			const bool to_x = (S - m) % 2 == 0;
			s.first = m == 1;
			s.src = s.dst;
			s.lds = s.ldd;
			s.dst = to_x ? xc : T->swp_buf;
			s.ldd = to_x ? ldx : ch.kc;
			s.keep = s.first && in_place && S > 1 ? T->swp_keep : nullptr;
			s.b = !s.first && in_place ? T->swp_keep : bc;
			s.ldb = !s.first && in_place ? ch.kc : ldb;
			if (launch_trsv_sweep(T->f32, unit, T->arr, T->swp_slice_pos, T->slices, T->block_rows, s, st))
				return 1;
		}
	}
	return 0;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_trsv_solve_sweeps_multi_device_async(spmv_mi355x_trsv * T, int sweeps, int k, const void * b_dev, long ldb, void * x_dev,
		long ldx, void * hip_stream)
{
	if (!T)
	{
		set_error("trsv_solve_sweeps: NULL argument ( T )");
		return 1;
	}
	if (!trsv_sweeps_in_range("trsv_solve_sweeps", sweeps, 1) || !trsv_multi_arguments_ok("trsv_solve_sweeps", T, k, b_dev, ldb, x_dev, ldx))
		return 1;
	if (T->n == 0)
		return 0;
	return trsv_sweeps_run(T, sweeps, k, b_dev, ldb, x_dev, ldx, (hipStream_t) hip_stream);
}

int
spmv_mi355x_trsv_solve_sweeps_device_async(spmv_mi355x_trsv * T, int sweeps, const void * b_dev, void * x_dev, void * hip_stream)
{
	return spmv_mi355x_trsv_solve_sweeps_multi_device_async(T, sweeps, 1, b_dev, 1, x_dev, 1, hip_stream);
}

int
spmv_mi355x_trsv_solve_sweeps_multi(spmv_mi355x_trsv * T, int sweeps, int k, const void * B_host, void * X_host)
{
	if (!T)
	{
		set_error("trsv_solve_sweeps: NULL argument ( T )");
		return 1;
	}
	if (!trsv_sweeps_in_range("trsv_solve_sweeps", sweeps, 1) || !trsv_multi_arguments_ok("trsv_solve_sweeps", T, k, B_host, k, X_host, k))
		return 1;
	if (T->n == 0)
		return 0;
	return trsv_solve_multi_staged(T, sweeps, k, B_host, X_host);       // the staging of trsv_solve_multi; the setting is not touched
}

int
spmv_mi355x_trsv_solve_sweeps(spmv_mi355x_trsv * T, int sweeps, const void * b_host, void * x_host)
{
	return spmv_mi355x_trsv_solve_sweeps_multi(T, sweeps, 1, b_host, x_host);
}

int
spmv_mi355x_trsv_set_sweeps(spmv_mi355x_trsv * T, int sweeps)
{
	if (!T)
	{
		set_error("trsv_set_sweeps: NULL argument ( T )");
		return 1;
	}
	if (!trsv_sweeps_in_range("trsv_set_sweeps", sweeps, 0))
		return 1;
	T->sweeps = sweeps;
	return 0;
}

int
spmv_mi355x_trsv_sweeps_info(const spmv_mi355x_trsv * T, int k, int * sweeps_out, long * effective_out, long * launches_out,
		double * bytes_out)
{
	if (!T)
	{
		set_error("trsv_sweeps_info: NULL argument ( T )");
		return 1;
	}
	if (k < 1)
	{
		set_error("trsv_sweeps_info: k = %d: at least one column is needed", k);
		return 1;
	}
	const long S = trsv_sweeps_effective(T, T->sweeps);
	if (sweeps_out)
		*sweeps_out = T->sweeps;
	if (effective_out)
		*effective_out = S;
	if (launches_out)
		*launches_out = S * (long) column_chunks(k).size();
	if (bytes_out)
		*bytes_out = T->swp_bytes;
	return 0;
}

}  // extern "C"

// ------------------------------------------------------------------------------------------------ update_values

namespace spmv {

// What update_map and update_values_prepare share: the pattern checks of create that need no values, the analysis and the layout.
// block_rows < 0: the global form with chain_rows; else the blocked form.
static int
trsv_layout_checked(const char * what, int uplo, int diag, long n, const int32_t * rp, const int32_t * ci, long chain_rows, long block_rows,
		TrsvLayout & L)
{
	const bool stored = diag == SPMV_MI355X_DIAG_STORED;
	if (trsv_check_pattern(what, n, rp, ci))
		return 1;
	if (stored && trsv_check_diagonal<double>(what, n, rp, ci, nullptr))
		return 1;
	TrsvAnalysis an;
	if (block_rows >= 0)
		trsv_analysis_blocked(uplo, n, rp, ci, block_rows, an);
	else
		trsv_analysis(uplo, n, rp, ci, (int) chain_rows, an);
	trsv_layout(uplo, stored, block_rows >= 0 ? an.block_rows : 0, n, an, rp, ci, L);
	return 0;
}

// The recomputed layout against the handle's device arrays. 0 = the same pattern; 1 = error set, naming the lowest row whose
// position or length differs, else a row of the first slice whose extent differs, else the lowest row whose kept columns differ.
static int
trsv_same_layout(const char * what, const spmv_mi355x_trsv * T, const int32_t * rp, const TrsvLayout & L)
{
	const long n = T->n;
	std::vector<int32_t> len((size_t) n), perm((size_t) n), col((size_t) T->slots);
	std::vector<int64_t> slice_ptr((size_t) T->slices + 1);
	if (n)
	{
		HIP_TRY(hipMemcpy(len.data(), T->arr.len, (size_t) n * sizeof(int32_t), hipMemcpyDeviceToHost));
		HIP_TRY(hipMemcpy(perm.data(), T->arr.perm, (size_t) n * sizeof(int32_t), hipMemcpyDeviceToHost));
	}
	HIP_TRY(hipMemcpy(slice_ptr.data(), T->arr.slice_ptr, slice_ptr.size() * sizeof(int64_t), hipMemcpyDeviceToHost));
	if (T->slots)
		HIP_TRY(hipMemcpy(col.data(), T->arr.col, (size_t) T->slots * sizeof(int32_t), hipMemcpyDeviceToHost));
	long bad = n;
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(min : bad) schedule(static, 4096)
	for (long p = 0; p < n; p++)
		if (perm[p] != L.perm[p])
			bad = std::min<long>(bad, std::min(perm[p], L.perm[p]));
		else if (len[p] != L.len[p])
			bad = std::min<long>(bad, perm[p]);
	if (bad < n)
	{
		set_error("%s: the pattern is not the one the handle was created with: row %ld has another place in the level order or "
				"another count of kept entries", what, bad);
		return 1;
	}
	const long common = std::min(T->slices, L.slices);
	long s = 0;
	while (s <= common && slice_ptr[s] == L.slice_ptr[s])
		s++;
	if (s <= common || T->slices != L.slices)
	{
		const long at = std::min(std::max<long>(s - 1, 0), std::max<long>(L.slices - 1, 0));
		set_error("%s: the pattern is not the one the handle was created with: the slice of row %ld has another extent (the levels "
				"differ)", what, L.slices ? (long) L.perm[L.slice_pos[at]] : 0L);
		return 1;
	}
	#pragma omp parallel for num_threads(spmv::host_threads()) reduction(min : bad) schedule(static, 4096)
	for (long e = 0; e < T->slots; e++)
		if (col[e] != L.col[e])
			bad = std::min<long>(bad, std::upper_bound(rp, rp + n + 1, L.slot_src[e]) - rp - 1);
	if (bad < n)
	{
		set_error("%s: the pattern is not the one the handle was created with: row %ld keeps other columns", what, bad);
		return 1;
	}
	return 0;
}

// the host-side refusals of the update entries, in the header's order
static bool
trsv_update_arguments_ok(const spmv_mi355x_trsv * T, const void * values, bool takes_values = true)
{
	if (!T)
		set_error("trsv_update_values: NULL handle");
	else if (takes_values && !values && T->nnz_csr > 0)
		set_error("trsv_update_values: NULL argument ( values )");
	else if (T->upd_state == 1)
		set_error("trsv_update_values: spmv_mi355x_trsv_update_values_prepare has not been called for this handle");
	else
		return true;
	return false;
}

}  // namespace spmv

extern "C" {

int
spmv_mi355x_trsv_update_map(int uplo, int diag, long n, const int32_t * row_ptr, const int32_t * col_idx, int chain_rows, long block_rows,
		int32_t ** slot_src_out, long * slots_out, int32_t ** diag_src_out)
{
	const char * what = "trsv_update_map";
	if (slot_src_out)
		*slot_src_out = nullptr;
	if (diag_src_out)
		*diag_src_out = nullptr;
	if (block_rows < -1)
	{
		set_error("%s: block_rows must be -1 (the global form), 0 (the default) or 1 .. %d (got %ld)", what, TRSV_BLOCK_ROWS_MAX, block_rows);
		return 1;
	}
	const bool blocked = block_rows >= 0;
	if (!trsv_scalars_ok(what, uplo, &diag, nullptr, n, blocked ? block_rows : (long) chain_rows, blocked))
		return 1;
	if (!row_ptr || (!col_idx && row_ptr[n] > 0))
	{
		set_error("%s: NULL argument (%s%s )", what, !row_ptr ? " row_ptr" : "", !col_idx ? " col_idx" : "");
		return 1;
	}
	TrsvLayout L;
	if (trsv_layout_checked(what, uplo, diag, n, row_ptr, col_idx, chain_rows, block_rows, L))
		return 1;
	const size_t slots = L.slot_src.size();
	int32_t * ss = slot_src_out ? (int32_t *) malloc(std::max<size_t>(slots, 1) * sizeof(int32_t)) : nullptr;
	const bool want_diag = diag_src_out && diag == SPMV_MI355X_DIAG_STORED;
	int32_t * ds = want_diag ? (int32_t *) malloc(std::max<size_t>((size_t) n, 1) * sizeof(int32_t)) : nullptr;
	if ((slot_src_out && !ss) || (want_diag && !ds))
	{
		free(ss);
		free(ds);
		set_error("%s: out of host memory (%zu slots, %ld rows)", what, slots, n);
		return 1;
	}
	if (ss)
		memcpy(ss, L.slot_src.data(), slots * sizeof(int32_t));
	if (ds)
		memcpy(ds, L.diag_src.data(), (size_t) n * sizeof(int32_t));
	if (slot_src_out)
		*slot_src_out = ss;
	if (diag_src_out)
		*diag_src_out = ds;
	if (slots_out)
		*slots_out = (long) slots;
	return 0;
}

int
spmv_mi355x_trsv_update_values_prepare(spmv_mi355x_trsv * T, long n, const int32_t * row_ptr, const int32_t * col_idx)
{
	const char * what = "trsv_update_values_prepare";
	if (!T)
	{
		set_error("%s: NULL handle", what);
		return 1;
	}
	if (T->upd_state != 1)
		return 0;             // a second prepare does nothing
	if (!row_ptr)
	{
		set_error("%s: NULL argument ( row_ptr )", what);
		return 1;
	}
	if (n != T->n)
	{
		set_error("%s: the pattern is not the one the handle was created with: n = %ld, the handle has %ld rows", what, n, T->n);
		return 1;
	}
	if (!col_idx && row_ptr[n] > 0)
	{
		set_error("%s: NULL argument ( col_idx )", what);
		return 1;
	}
	TrsvLayout L;
	if (trsv_layout_checked(what, T->uplo, T->diag, n, row_ptr, col_idx, T->chain_rows, T->block_rows ? T->block_rows : -1, L))
		return 1;
	HIP_TRY(hipSetDevice(T->device));
	if (trsv_same_layout(what, T, row_ptr, L))
		return 1;
	const bool stored = T->diag == SPMV_MI355X_DIAG_STORED;
	void * slot_src = nullptr, * diag_src = nullptr, * status = nullptr;
	hipEvent_t done = nullptr;
	const size_t slot_bytes = L.slot_src.size() * sizeof(int32_t), diag_bytes = L.diag_src.size() * sizeof(int32_t);
	if (upload_bytes(L.slot_src.data(), slot_bytes, 0, &slot_src) || (stored && upload_bytes(L.diag_src.data(), diag_bytes, 0, &diag_src))
			|| dev_alloc_bytes(&status, 16) || hipEventCreateWithFlags(&done, hipEventDisableTiming) != hipSuccess)
	{
		for (void * p : {slot_src, diag_src, status})
			if (p)
				(void) hipFree(p);
		if (status && !done)
			set_error("%s: hipEventCreate failed", what);           // the allocations have set their own message
		return 1;
	}
	T->upd_slot_src = (int *) slot_src;
	T->upd_diag_src = (int *) diag_src;
	T->upd_status = (unsigned *) status;
	T->upd_done = done;
	if (stored)
	{
		// by row, for the message of a refusal
		T->upd_diag_entry.assign((size_t) n, 0);
		for (long p = 0; p < n; p++)
			T->upd_diag_entry[L.perm[p]] = L.diag_src[p];
	}
	T->nnz_csr = row_ptr[n];
	T->upd_bytes = (double) slot_bytes + (stored ? (double) diag_bytes : 0) + 16;
	T->upd_state = 2;
	return 0;
}

double
spmv_mi355x_trsv_update_values_bytes(const spmv_mi355x_trsv * T)
{
	return T ? T->upd_bytes : 0;
}

int
spmv_mi355x_trsv_update_values_state(const spmv_mi355x_trsv * T)
{
	return T ? T->upd_state : 0;
}

int
spmv_mi355x_trsv_update_values_device_async(spmv_mi355x_trsv * T, const double * values_dev, void * hip_stream)
{
	if (!trsv_update_arguments_ok(T, values_dev))
		return 1;
	T->upd_pending = false;
	if (T->n == 0)
	{
		T->upd_bad_row = -1;
		T->upd_state = 2;
		return 0;
	}
	int cur = -1;
	HIP_TRY(hipGetDevice(&cur));
	if (cur != T->device)
		HIP_TRY(hipSetDevice(T->device));
	hipStream_t st = (hipStream_t) hip_stream;
	const bool stored = T->diag == SPMV_MI355X_DIAG_STORED;
	HIP_TRY(hipMemsetAsync(T->upd_status, 0xff, 16, st));
	if (stored && launch_trsv_update_check(T->f32, T->upd_diag_src, T->arr.perm, values_dev, T->upd_status, T->n, st))
		return 1;
	if (launch_trsv_update_write(T->f32, T->upd_slot_src, stored ? T->upd_diag_src : nullptr, values_dev, T->owned[0], T->owned[5],
			T->upd_status, T->slots, T->n, st))
		return 1;
	HIP_TRY(hipEventRecord(T->upd_done, st));
	T->upd_last = values_dev;
	T->upd_pending = true;
	return 0;
}

int
spmv_mi355x_trsv_update_values_result(spmv_mi355x_trsv * T, long * bad_row_out)
{
	if (bad_row_out)
		*bad_row_out = -1;
	if (!trsv_update_arguments_ok(T, nullptr, false))
		return 1;
	if (T->upd_pending)
	{
		HIP_TRY(hipSetDevice(T->device));
		HIP_TRY(hipEventSynchronize(T->upd_done));
		unsigned word = TRSV_UPDATE_FINE;
		HIP_TRY(hipMemcpy(&word, T->upd_status, sizeof(word), hipMemcpyDeviceToHost));
		T->upd_pending = false;
		T->upd_bad_row = word == TRSV_UPDATE_FINE ? -1 : (long) word;
		if (T->upd_bad_row >= 0)
			HIP_TRY(hipMemcpy(&T->upd_bad_value, T->upd_last + T->upd_diag_entry[T->upd_bad_row], sizeof(double), hipMemcpyDeviceToHost));
		T->upd_state = T->upd_bad_row >= 0 ? 3 : 2;
	}
	if (T->upd_bad_row < 0 || T->upd_state != 3)
		return 0;
	if (bad_row_out)
		*bad_row_out = T->upd_bad_row;
	const double v = T->upd_bad_value;
	set_error("trsv_update_values: the diagonal of row %ld is %g in the handle's precision (from %g): it must be finite and non-zero",
			T->upd_bad_row, T->f32 ? (double) (float) v : v, v);
	return 1;
}

int
spmv_mi355x_trsv_update_values_device(spmv_mi355x_trsv * T, const double * values_dev, void * hip_stream)
{
	return spmv_mi355x_trsv_update_values_device_async(T, values_dev, hip_stream) || spmv_mi355x_trsv_update_values_result(T, nullptr);
}

int
spmv_mi355x_trsv_update_values(spmv_mi355x_trsv * T, const double * values_host)
{
	if (!trsv_update_arguments_ok(T, values_host))
		return 1;
	HIP_TRY(hipSetDevice(T->device));
	const size_t bytes = (size_t) T->nnz_csr * sizeof(double);
	if (!T->upd_values && dev_alloc_bytes((void **) &T->upd_values, bytes))
		return 1;
	if (bytes)
		HIP_TRY(hipMemcpyAsync(T->upd_values, values_host, bytes, hipMemcpyHostToDevice, nullptr));
	return spmv_mi355x_trsv_update_values_device(T, T->upd_values, nullptr);
}

int
spmv_mi355x_trsv_update_values_staged(spmv_mi355x_trsv * T, const double ** values_dev_out)
{
	if (values_dev_out)
		*values_dev_out = nullptr;
	if (!T || !values_dev_out || !T->upd_values)
	{
		set_error("trsv_update_values_staged: %s", !T ? "NULL handle" : !values_dev_out ? "NULL argument ( values_dev_out )"
				: "the handle has taken no host values yet (spmv_mi355x_trsv_update_values)");
		return 1;
	}
	*values_dev_out = T->upd_values;
	return 0;
}

int
spmv_mi355x_trsv_stored_values(spmv_mi355x_trsv * T, void * val_host, long * slots_out, void * diag_host)
{
	if (!T)
	{
		set_error("trsv_stored_values: NULL handle");
		return 1;
	}
	if (slots_out)
		*slots_out = T->slots;
	if (!val_host)
		return 0;
	HIP_TRY(hipSetDevice(T->device));
	HIP_TRY(hipDeviceSynchronize());          // an update in flight on any stream is in the bytes returned
	const size_t size = T->f32 ? 4 : 8;
	if (T->slots)
		HIP_TRY(hipMemcpy(val_host, T->arr.val, (size_t) T->slots * size, hipMemcpyDeviceToHost));
	if (diag_host && T->diag == SPMV_MI355X_DIAG_STORED && T->n)
		HIP_TRY(hipMemcpy(diag_host, T->arr.diag, (size_t) T->n * size, hipMemcpyDeviceToHost));
	return 0;
}

}  // extern "C"

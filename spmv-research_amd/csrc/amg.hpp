// Smoothed-aggregation AMG (include/spmv_mi355x.h "AMG"): what amg.hip (the checks, the hierarchy, the C ABI), kernels_amg.hip (the
// setup kernels of steps 1 to 5, the cycle's vector kernels, the dense coarsest solve) and solver_pcg_tri.hip (pcg_amg) share.
//
// THE MAPPING. Every setup kernel is one lane per row of A_l, AMG_TB lanes per workgroup, at most AMG_MAX_GRID workgroups which walk
// the rows with a grid stride: beyond AMG_TB * AMG_MAX_GRID = 262 144 rows a workgroup takes a second trip. A lane walks its row in
// stored order; rows of A_l hold a handful of entries (a stencil, a Galerkin product of one), so a wave per row would idle. The
// cycle's vector kernels are the solvers' (VB lanes, solver_blocks workgroups, GRID_STRIDE). The dense solve is one workgroup of
// AMG_DENSE_MAX lanes, lane a owning y_a; its loops hold one barrier per column and run n trips in every lane.
// THE CYCLE FOR k COLUMNS (amg_apply_multi*): the same schedule over row-major blocks, every SpMV one SpMM, every vector launch one
// launch per chunk of KC in {8, 4, 2, 1} columns (k = 8s, then the binary remainder); a thread owns row i of its chunk. The dense
// solve is one workgroup per chunk: the triangle (66 048 B) goes into LDS once, piv is [AMG_DENSE_MAX][KC] (8 KiB at KC = 8), lane a
// keeps y_a of every column, and there is one barrier per column of L in each direction whatever KC is. The hierarchy owns the
// per-level blocks (mb, mx, mt below); the first multi apply allocates them and a larger k replaces them, which synchronises the device.
// No atomics on values (the one atomic is the integer count of undecided nodes, one add per workgroup), no flags, nothing spins; a
// launch boundary is the only ordering between workgroups.
//     kernel                     VGPRs   LDS        scratch
//     amg_diag_kernel              20    2 048 B       0
//     amg_mis_init_kernel          13        0         0
//     amg_mis_sweep_kernel         18        0         0
//     amg_mis_decide_kernel        18    1 024 B       0
//     amg_root_flag_kernel         16        0         0
//     amg_agg_pass1_kernel         18        0         0
//     amg_agg_pass2_kernel         24        0         0
//     amg_prolong_kernel           24        0         0
//     amg_first / sweep / residual <= 22     0         0
//     amg_dense_solve_kernel       20   67 072 B       0
//     amg_diag_check_kernel        22    3 072 B       0
//     amg_weights_kernel           16        0         0
//     amg_dense_factor_kernel      46   66 056 B       0
//     amg_filter_count_kernel      22        0         0
//     amg_filter_fill_kernel       30    2 048 B       0
//     amg_filter_values_kernel     21    3 072 B       0
//     amg_agg_norm_kernel          14        0         0
//     amg_tentative_kernel         20        0         0
//     amg_prolong_t_kernel         24        0         0
//     amg_first / sweep / residual_multi <KC = 8 / 4 / 2 / 1>, the largest of fp32 and fp64
//                          62 / 38 / 26 / 26     0         0
//     amg_dense_solve_multi_kernel <KC = 8 / 4 / 2 / 1>
//                          40 / 30 / 26 / 20   74 240 / 70 144 / 68 096 / 67 072 B   0
//     amg_fold_tail_kernel <KC = 8 / 4 / 2 / 1>, fp32 / fp64, 1024 lanes (at most 128 VGPRs)
//            55 / 44 / 38 / 31 and 80 / 56 / 45 / 36     74 240 / 70 144 / 68 096 / 67 072 B   0
//     amg_fold_narrow_kernel        8        0         0
// (-Rpass-analysis=kernel-resource-usage, gfx950; profiles/r23_amg.txt, profiles/r24_amg_update.txt,
// profiles/r25_amg_prolongator.txt and profiles/r33_amg_fold.txt have the compiler's own table.)
// THE FOLDED TAIL (amg_set_fold; kernels_amg_fold.hip; the header's "AMG: the small levels as one launch"). ONE workgroup of
// AMG_FOLD_TB = 1024 lanes runs the cycle from the first folded level down and back up, once per chunk of KC columns. A row of A_l is
// walked by G_l = amg_fold_lanes(n_l, nnz_l) adjacent lanes of one wave (lane g takes the entries g, g + G, ..., a shuffle tree adds the
// partials), a row of P_l or R_l by one lane; rows are dealt to the lanes in trips of 1024 / G rows, and every lane runs the same
// number of trips. The elementwise steps are one lane per row with a stride of 1024. The dense solve is amg_dense_solve_multi_kernel's
// with lanes 128.. idle: lane a owns y_a, one barrier per column in each direction, n trips in every lane. The vectors stay in global
// memory (the hierarchy's b, x, t or mb, mx, mt), ordered by __syncthreads(); LDS holds the packed factor and piv alone.
// STEPS 5a TO 5c (amg_create_with; the header's "AMG: a caller's near-null vector and filtered prolongator smoothing"). Filtered: a
// count pass (kept entries, the lump and the fall-back per row), hipcub's exclusive scan over n + 1 counts, a fill pass (A_F's columns,
// values, the int32 map into A_l, the partials of rho_p). Near-null: the device transposition of T's pattern with b as its values
// lists every aggregate's members in ascending order (its sort by column is stable); one lane per aggregate sums b * b sequentially,
// one lane per row divides. amg_prolong_t_kernel reads t and dF. A handle built with the defaults runs none of them and launches what
// amg_create launches. An update keeps A_F's pattern, the map, the fall-back rows and t, and runs amg_filter_values_kernel (lump, dF,
// A_F's values, the partials, the count of bad lumped diagonals) before the plan of A_F T.
// AN UPDATE OF THE VALUES (amg_update_values*) keeps, from prepare on, what AmgUpdate below lists: per coarsened level the three SpGEMM
// plans (their device patterns serve step 1 and launch_amg_prolong too), agg, the entry map P -> R and the value arrays. An update is
// per level amg_diag_check_kernel (the host reads one count and amg_grid(n) partials), amg_weights_kernel, the numeric passes of the
// plans, amg_prolong_kernel, the gather into R's order and the handles' update_values_device; a dense last level is factorised by
// amg_dense_factor_kernel, one workgroup of AMG_DENSE_MAX lanes with the packed triangle in LDS, two barriers per column, n trips in
// every lane, a failed pivot raised by a plain store.
#pragma once

#include <vector>

#include "common.hpp"
#include "../../include/spmv_mi355x.h"

namespace spmv {

constexpr int AMG_TB = 256;
constexpr int AMG_MAX_GRID = 1024;                        // workgroups per setup launch; more rows are walked with a grid stride
constexpr int AMG_DENSE_MAX = 128;                        // rows of a dense coarsest level: 128 * 129 / 2 doubles = 66 048 B of LDS
constexpr int AMG_MIS_ROUND_CAP = 1024;                   // every round decides a node, real counts are below 20: a bug becomes a message
constexpr unsigned AMG_HASH_MUL = 0x9E3779B1u;            // SPGEMM_HASH_MUL
constexpr int AMG_FOLD_TB = 1024;                         // lanes of the one workgroup that runs the folded tail
constexpr int AMG_FOLD_MAX_ROWS = 65536;                  // the largest fold_rows
constexpr int AMG_FOLD_MAX_LANES = 64;                    // lanes per row of A_l inside the tail: at most a wave

// A_l on the device
struct AmgCsr {
	const int * rp;
	const int * ci;
	const double * va;
	long n;
};

inline int
amg_grid(long n)
{
	return (int) std::min<long>(AMG_MAX_GRID, std::max<long>(1, (n + AMG_TB - 1) / AMG_TB));
}

// step 1: d[i] = the first stored a_ii; part[workgroup] = the workgroup's max of (sum_j |a_ij|) / d_i; amg_grid(n) partials
int launch_amg_diag(const AmgCsr & a, double * d, double * part, hipStream_t st);
// step 3: state = 1 and key0 = the key of every node
int launch_amg_mis_init(long n, int * state, unsigned long long * key0, hipStream_t st);
// out[i] = max(in[i], in[j] for j in S(i))
int launch_amg_mis_sweep(const AmgCsr & a, const double * d, double theta2, const unsigned long long * in, unsigned long long * out,
		hipStream_t st);
// the verdicts of a round: state and key0 of every undecided node; *undecided += the nodes still undecided (zeroed by the caller)
int launch_amg_mis_decide(long n, int * state, unsigned long long * key0, const unsigned long long * key2, int * undecided, hipStream_t st);
// step 4: id = the exclusive scan of (state == 2); scan_tmp / scan_bytes as hipcub wants them (amg_scan_bytes)
size_t amg_scan_bytes(long n);
int launch_amg_number_roots(long n, const int * state, int * flag, int * id, void * scan_tmp, size_t scan_bytes, hipStream_t st);
int launch_amg_agg_pass1(const AmgCsr & a, const double * d, double theta2, const int * state, const int * id, int * agg1, hipStream_t st);
int launch_amg_agg_pass2(const AmgCsr & a, const double * d, double theta2, const int * agg1, int * agg2, hipStream_t st);
// step 5: p_va from the CSR of A T
int launch_amg_prolong(long n, const int * at_rp, const int * at_ci, const double * at_va, const int * agg, const double * d, double omega,
		double * p_va, hipStream_t st);
// step 5a, count: kept[i] entries stay in row i of A_F, fb[i] = the row fell back to all its entries, df[i] = the lumped diagonal
int launch_amg_filter_count(const AmgCsr & a, const double * d, double theta2, int * kept, int * fb, double * df, hipStream_t st);
// out = the exclusive scan of in[0 .. count); scan_tmp / scan_bytes as hipcub wants them (amg_scan_bytes(count))
int launch_amg_offsets(long count, const int * in, int * out, void * scan_tmp, size_t scan_bytes, hipStream_t st);
// step 5a, fill: A_F's columns, values and entry map into A_l, and amg_grid(n) partials of (sum_j |aF_ij|) / dF_i
int launch_amg_filter_fill(const AmgCsr & a, const double * d, double theta2, const int * f_rp, const int * fb, const double * df, int * f_ci,
		double * f_va, int * map, double * part, hipStream_t st);
// step 5a for an update on the frozen kept pattern: df, f_va (NULL: not written) and the partials; *bad += the rows filtered at create
// whose lumped diagonal is not finite or not > 0 (zeroed by the caller)
int launch_amg_filter_values(const AmgCsr & a, const double * d, const int * f_rp, const int * map, const int * fb, double * df, double * f_va,
		double * part, int * bad, hipStream_t st);
// step 5b: nrm[g] over the members of aggregate g (m_rp, m_b: the transposition of T's pattern with b as its values); t = b / nrm[agg]
int launch_amg_agg_norm(long nc, const int * m_rp, const double * m_b, double * nrm, hipStream_t st);
int launch_amg_tentative(long n, const double * b, const int * agg, const double * nrm, double * t, hipStream_t st);
// step 5c: p_va from the CSR of A_F T, t and dF
int launch_amg_prolong_t(long n, const int * at_rp, const int * at_ci, const double * at_va, const int * agg, const double * t, const double * df,
		double omega_p, double * p_va, hipStream_t st);
// the cycle: x = w o b;  x += w o (b - t);  t = b - t
int launch_amg_first(bool f32, const void * w, const void * b, void * x, long n, hipStream_t st);
int launch_amg_sweep(bool f32, const void * w, const void * b, const void * t, void * x, long n, hipStream_t st);
int launch_amg_residual(bool f32, const void * b, void * t, long n, hipStream_t st);
// x = (L L^t)^-1 b for the packed factor L of n <= AMG_DENSE_MAX rows (row-major lower triangle, fp64)
int launch_amg_dense_solve(bool f32, const double * L, const void * b, void * x, int n, hipStream_t st);
// the same four for the k columns of row-major blocks (row i at ptr + i * ld), one launch per chunk of 8, 4, 2 or 1 columns
int launch_amg_first_multi(bool f32, int k, const void * w, const void * b, long ldb, void * x, long ldx, long n, hipStream_t st);
int launch_amg_sweep_multi(bool f32, int k, const void * w, const void * b, long ldb, const void * t, long ldt, void * x, long ldx, long n,
		hipStream_t st);
int launch_amg_residual_multi(bool f32, int k, const void * b, long ldb, void * t, long ldt, long n, hipStream_t st);
int launch_amg_dense_solve_multi(bool f32, int k, const double * L, const void * b, long ldb, void * x, long ldx, int n, hipStream_t st);

// an update: step 1 with *bad += the rows whose diagonal is absent, not finite or <= 0 (zeroed by the caller); d and part as above
int launch_amg_diag_check(const AmgCsr & a, double * d, double * part, int * bad, hipStream_t st);
// w[i] = omega / d[i] in fp64, narrowed to the handle's precision
int launch_amg_weights(bool f32, long n, const double * d, double omega, void * w, hipStream_t st);
// the packed factor of a.n <= AMG_DENSE_MAX rows into F; *failed = 1 at a pivot that is <= 0 or not finite (zeroed by the caller)
int launch_amg_dense_factor(const AmgCsr & a, double * F, int * failed, hipStream_t st);

// ---- the folded tail (amg_set_fold; kernels_amg_fold.hip) -----------------------------------------------------------------------------
// One level as the tail kernel reads it, an array of `levels` of them on the device (entries above the first folded level are zero):
// the fold's own int32 CSR copies of A_l, P_l and R_l with values of the handle's precision (P and R NULL on the last level), the
// level's w, and the level's vectors: b, x, t of the single apply or mb, mx, mt of the k-column apply (x is NULL on level 0).
struct AmgFoldLevel {
	const int * a_rp, * a_ci;
	const void * a_va;
	const int * p_rp, * p_ci;
	const void * p_va;
	const int * r_rp, * r_ci;
	const void * r_va;
	const void * w;
	void * b, * x, * t;
	int n, lg;                                            // rows; log2 of the lanes per row of A_l
};

// THE RULE of the lanes per row (the header's): the largest power of two that is <= min(64, nnz / n, 1024 / n) in integer division,
// and 1 where that minimum is 0. It depends on the CSR of A_l alone.
inline int
amg_fold_lanes(long n, long nnz)
{
	const long cap = n > 0 ? std::min<long>(AMG_FOLD_MAX_LANES, std::min(nnz / n, (long) AMG_FOLD_TB / n)) : 1;
	int g = 1;
	while (2L * g <= cap)
		g *= 2;
	return g;
}

struct AmgFold {
	int first = 0;                                        // the first folded level
	std::vector<AmgFoldLevel> host;                       // the descriptors with the single apply's vectors
	std::vector<void *> va, p_va, r_va;                   // per level the fold's value arrays: what an update rewrites
	AmgFoldLevel * d_single = nullptr, * d_multi = nullptr;
	std::vector<void *> owned;
	double bytes = 0;
};

// the tail from level `first` to `last` and back for k columns (one launch per chunk of 8, 4, 2 or 1): rhs `in` and solution `out` of
// level `first` with their own ld, the other vectors the descriptors' with ld; factor NULL = the last level takes cs - 1 sweeps
int launch_amg_fold_tail(bool f32, int k, const AmgFoldLevel * lv, int first, int last, const void * in, long ldin, void * out, long ldout, long ld,
		int nu, int cs, const double * factor, hipStream_t st);
// dst = src narrowed to the handle's precision (a copy in fp64)
int launch_amg_fold_values(bool f32, const double * src, void * dst, long count, hipStream_t st);

// what amg_update_values_prepare keeps of level l, all on the device
struct AmgUpdateLevel {
	spmv_mi355x_spgemm * at = nullptr, * ap = nullptr, * ac = nullptr;   // A T, A P, R (A P); NULL on the last level
	const int * d_rp = nullptr, * d_ci = nullptr;         // A_l's pattern: the plan's copy, or the level's own on the last level
	int * d_agg = nullptr;
	unsigned * d_src = nullptr;                           // entry e of R is entry d_src[e] of P
	double * d_va = nullptr, * d_d = nullptr;             // A_l's values (level 0: a copy of the caller's), the diagonal
	double * d_ones = nullptr, * d_at = nullptr, * d_p = nullptr, * d_r = nullptr, * d_ap = nullptr;
	// a hierarchy of amg_create_with: A_F's row pointer, its entry map into A_l and the rows that fell back (filtered); A_F's values and
	// the lumped diagonal; t of a near-null vector (else d_ones serves)
	const int * d_f_rp = nullptr;
	int * d_map = nullptr, * d_fb = nullptr;
	double * d_fva = nullptr, * d_df = nullptr, * d_t = nullptr;
};

struct AmgUpdate {
	std::vector<AmgUpdateLevel> lev;
	std::vector<void *> owned;                            // every device allocation but the plans'
	double * d_part = nullptr, * d_factor = nullptr;      // step 1's partials; the factor before it is known to be one
	int * d_count = nullptr;                              // the bad diagonals of every level, then the pivot flag
	double bytes = 0, prepare_seconds = 0;
	long updates = 0;
	double update_seconds = 0, spgemm_seconds = 0, handle_seconds = 0;   // of the last update
	bool host_stale = false;                              // the host copies of the values lag behind the device's
};

struct AmgLevel {
	long n = 0, nnz = 0, nnz_p = 0, aggregates = 0;
	int mis_rounds = 0;
	double omega = 0, rho = 0;
	std::vector<int32_t> rp, ci, p_rp, p_ci, agg;         // the host copies level_csr and aggregates return
	std::vector<double> va, p_va;
	// amg_create_with: A_F of a coarsened level (filtered), its map into A_l and the rows that fell back; b_l and t (near_null)
	long nnz_f = 0, unfiltered_rows = 0;
	double omega_p = 0, rho_p = 0;
	std::vector<int32_t> f_rp, f_ci, f_map, f_fb;
	std::vector<double> f_va, nn, tv;
	spmv_mi355x_matrix * A = nullptr, * P = nullptr, * R = nullptr;
	void * w = nullptr, * b = nullptr, * x = nullptr, * t = nullptr;   // n values of the handle's precision each; x is NULL on level 0
};

}  // namespace spmv

struct spmv_mi355x_amg {
	int precision = 0, device = 0, format = 0;
	bool f32 = false;
	long n = 0;
	spmv_mi355x_amg_opts opts = {};
	int levels = 0, coarse_kind = 0, stalled = 0;
	bool filtered = false, has_nn = false;                // spmv_mi355x_amg_prolongator_opts
	std::vector<spmv::AmgLevel> lev;
	double * d_factor = nullptr;                          // the packed Cholesky factor of a dense last level
	void * d_in = nullptr, * d_out = nullptr;             // the vectors of the host-buffer apply, allocated at its first call
	long spmvs = 0, launches = 0;
	double setup_seconds = 0, coarsen_seconds = 0, spgemm_seconds = 0, transpose_seconds = 0, create_seconds = 0, download_seconds = 0;
	double vector_bytes = 0;
	// apply_multi: per level the blocks b, x and t, room for rows x multi_k values each, used with ld = k of the call (x is NULL on level 0, whose b serves an
	// apply in place); allocated at the first multi apply, regrown (after a device synchronisation) when a larger k arrives
	std::vector<void *> mb, mx, mt;
	int multi_k = 0, multi_host_k = 0;
	double multi_bytes = 0;                               // of mb, mx and mt: part of vector_bytes
	void * d_in_multi = nullptr, * d_out_multi = nullptr; // the blocks of the host-buffer apply_multi, n x multi_host_k
	spmv::AmgUpdate * upd = nullptr;                      // amg_update_values_prepare's; NULL before it
	bool update_failed = false;                           // the last update stopped below level 0: apply refuses
	int fold_rows = 0;                                    // amg_set_fold's; 0 = off
	spmv::AmgFold * fold = nullptr;                       // NULL while no level has rows <= fold_rows
};

/* spmv_mi355x.h — C ABI of the MI355X (gfx950 / CDNA4) SpMV engine.
 *
 * This is the drop-in boundary for the SpMV hot path of LiHaoxu/SpMV-Research: the shared object
 * libspmv_mi355x.so (hand-written HIP, hipcc --offload-arch=gfx950) exports exactly what a backend TU of the
 * reference harness needs behind its plug-in API
 *
 *     struct Matrix_Format * csr_to_format(INT_T * row_ptr, INT_T * col_ind, ValueTypeReference * values,
 *                                          long m, long n, long nnz, long symmetric, long symmetry_expanded);
 *     virtual void Matrix_Format::spmv(ValueType * x, ValueType * y);
 *         (benchmark_code/BENCH/src/spmv_kernels/spmv_kernel.h:8-29)
 *
 * with plain pointers, sizes and opaque handles, so the host TU is compiled by g++ with no HIP header
 * (precedent for the split: GPU_clean/csr_rocm_vector.cpp:215,239 `extern "C" launch_kernel_wrapper`).
 * The adapter TU that binds this ABI to Matrix_Format is spmv-research_amd/host/spmv_kernel_mi355x.cpp;
 * INTEGRATION.md shows the Makefile_in rule a maintainer would add.
 *
 * Conventions
 *   - every function returns 0 on success, non-zero on failure; spmv_mi355x_last_error() gives the message
 *     (the Matrix_Format adapter turns a failure into the reference's error()+exit behaviour, lib/debug.h:83-135);
 *   - single caller thread per handle, blocking on return unless the name ends in _async / takes a stream;
 *   - indices are int32 (INT_T, make.sh:166), values arrive as fp64 regardless of precision (Q3, bench.cpp:601)
 *     and are narrowed on upload when precision == SPMV_MI355X_F32 (csr.cpp:72 does the same);
 *   - inputs are deep-copied: the caller may free them right after create (bench.cpp:605-629);
 *   - there is NO CPU fallback: without a usable gfx950 device create() fails.
 */
#ifndef SPMV_MI355X_H
#define SPMV_MI355X_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct spmv_mi355x_matrix spmv_mi355x_matrix;   /* opaque */

/* storage format + kernel of y = A*x */
enum {
	SPMV_MI355X_CSR_SCALAR   = 0,  /* one lane per row; bit-identical to the reference CPU kernel (csr.cpp:334-350)      */
	SPMV_MI355X_CSR_VECTOR   = 1,  /* one group of 2..64 lanes per row (64 = one wavefront per row); replaces
	                                  GPU_clean/spmv_subkernel_csr_rocm_vector.cpp:5-54 / CPU analogue csr_vec.cpp:182-213 */
	SPMV_MI355X_CSR_MERGE    = 2,  /* merge-path CSR; replaces merge.cpp:256-319 / GPU_clean/merge_cuda.cu:249-261        */
	SPMV_MI355X_SELL_C_SIGMA = 3,  /* sliced ELL, C rows per slice, sigma-window sort; replaces sell_sorted.cpp:112-419 /
	                                  sell_c_s.cpp:39-131                                                                  */
	SPMV_MI355X_COO          = 4,  /* row-sorted COO, segmented reduction; replaces mkl_coo.cpp:58-106 /
	                                  GPU_clean/rocsparse_coo.cpp:88-104,294                                               */
	SPMV_MI355X_CSR_STREAM   = 5,  /* one wavefront per block of R consecutive rows, products staged in LDS (CSR-Stream);
	                                  replaces the row-block CSR kernels GPU_clean/spmv_subkernel_csr_rocm_adaptive.cpp:76-153 */
	SPMV_MI355X_NUM_FORMATS  = 6
};

enum { SPMV_MI355X_F64 = 0, SPMV_MI355X_F32 = 1 };

/* Tunables. Zero-initialise, set struct_size = sizeof(spmv_mi355x_opts); 0 / unset = engine default. */
typedef struct {
	int  struct_size;
	int  device;            /* HIP device ordinal; -1 = the current device                                        */
	int  lanes_per_row;     /* CSR_VECTOR: 2,4,8,16,32,64; 0 = chosen from mean nnz/row                            */
	                        /* CSR_STREAM: the same field holds ROWS PER WAVEFRONT (4,8,16,32,64); 0 = auto          */
	int  sell_split;        /* SELL delta format: wavefronts sharing one 64-row slice (1, 2 or 4); 0 = auto by slice count */
	int  sell_c;            /* SELL: rows per slice (16, 32, 64, or 256 = the BSC library's, sell_c_s.cpp:58-60); 0 = 64         */
	int  sell_sigma;        /* SELL: sort window in rows (multiple of sell_c); 0 = 16384 (sell_c_s.cpp:58-60)      */
	int  merge_items;       /* MERGE: merge items per thread (5,7,9,11,13); COO: entries per lane (2,4,8); 0 = default */
	int  xcd_remap;         /* tile order over the 8 XCDs: 0 = auto, 1 = contiguous work-balanced ranges, 2 = off,
	                           3 = chunks of 64 tiles dealt round-robin to the XCDs                                */
	int  nontemporal;       /* matrix streams loaded with the nt policy: 0 = auto (by footprint), 1 = on, 2 = off  */
	int  stream_mode;       /* CSR_STREAM: 0 = auto (3); 1 = products staged in LDS (row-major x gather); 2 = (value,column)
	                           pairs staged in LDS through registers, lanes walk rows (coalesced x gathers); 3 = the same with
	                           the global->LDS copy done by LDS-DMA (global_load_lds). With 64 rows per wave 2 and 3 are
	                           bit-exact; 4 = nnz-balanced row blocks whose window of x is copied into LDS (up to 128 KiB) and
	                           gathered from there, lanes_per_row lanes per row (8..64), merge_items = blocks per CU (0 auto);
	                           for matrices whose row blocks touch a narrow column range (FEM / banded)                   */
	long row_begin;         /* row block [row_begin,row_end) of the GLOBAL CSR to keep on this device (row-partitioned */
	long row_end;           /*   multi-GPU, §8e); 0,0 = all rows. x stays full length n; y has row_end-row_begin rows. */
	long col_begin;         /* optional column filter [col_begin,col_end) used for the local/remote split that lets    */
	long col_end;           /*   the local part run while allgather(x) is in flight; 0,0 = no filter                   */
	int  col_filter_mode;   /* 0 = keep all, 1 = keep columns inside [col_begin,col_end), 2 = keep columns outside     */
	int  sell_delta;        /* SELL with 64-row slices: column indices stored as one base per step + 8/16-bit deltas per lane
	                           where they fit (lossless, bit-identical results): 0 = auto (on when sell_c = 64), 1 = on, 2 = off */
	int  convert_on;        /* where the layouts with a GPU builder (SELL plain / delta / LDS-window: csrc/convert_sell.hip; the entry arrays of
	                           the column-blocked layout: csrc/convert_coo.hip) are built from the CSR: 0 = auto (GPU), 1 = GPU,
	                           2 = host (OpenMP; kept as the checker — both produce the same bytes)                    */
	int  symmetric_input;   /* 1 = the CSR arrays hold ONE triangle of a symmetric matrix (KEEP_SYMMETRY builds of the harness:
	                           csr_to_format(..., symmetric = 1, symmetry_expanded = 0), csr_sym.cpp:118-123); the product is
	                           y = (T + T^t - diag T) x; rows()/nnz() report the expanded matrix. SELL_C_SIGMA on a banded matrix
	                           (every slice group's window of rows + columns fits LDS: (w + 1) * (sizeof(V) + 8) <= 152 KiB) keeps the
	                           triangle and multiplies without expanding it — half the matrix stream, the mirrored additions as LDS
	                           atomics (csrc/kernels_sell_window.hip) — on its own when the expanded stream exceeds the 256 MiB
	                           Infinity Cache, always with sell_window = 1. Everything else expands the triangle at create().        */
	int  rows_per_group;    /* CSR_VECTOR: consecutive rows a lane group keeps in flight together (1, 2 or 4; 2 and 4 need
	                           lanes_per_row >= 8); 0 = auto                                                        */
	int  col_blocks;        /* COO: 0 = row-sorted COO (the reference's layout); -1 = column-blocked layout for graph matrices: the rows are
	                           dealt to workgroups that keep their y in LDS, a workgroup's entries are sorted by column and stored as one
	                           dword each in full batches (csrc/kernels_coo.hip); > 0 = the same with a wave instruction's 64 entries kept
	                           inside ceil(n / col_blocks) columns (tests). LDS atomics: sums to the tolerance, not bit-reproducible.
	                           CSR_MERGE: 0 / -2 = the CSR-order merge path (deterministic); -1 / > 0 = the same column-blocked layout
	                           with merge-path-balanced row ranges — never chosen unless asked for                                  */
	int  sell_window;       /* SELL, 64-row slices: a workgroup owns a group of consecutive slices, copies the group's column window of
	                           x into LDS and gathers from there; column indices are 16-bit offsets into the window (for banded /
	                           FEM matrices; csrc/kernels_sell_window.hip). 0 = auto (when sell_sigma, sell_delta and convert_on are at their defaults
	                           and every group's window fits; rows are then sorted inside a slice group: sigma = 64 * sell_group), 1 = on, 2 = off.
	                           spmv_mi355x_sell_layout() does not decode this layout: name a sell_sigma (or sell_window = 2) for layout parity */
	int  kahan;             /* CSR_SCALAR: 1 = Kahan-compensated row sums, the reference's CUSTOM_KAHAN build (csr.cpp:353-373); same
	                           operations in the same order -> bit-identical to it                                             */
	int  sell_group;        /* sell_window: slices per workgroup (1, 2, 4, 8 or 16; times sell_split at most 16 wavefronts); 0 = auto */
	int  placement;         /* where the handle's vectors live relative to its value array ("vectors placed by the engine" below):
	                           0 = off (default: plain allocations), 1 = on (slices of the device's vector pools; the first handle
	                           of a process that asks makes ONE walk through the device's free memory to find them), 2 = off,
	                           3 = 1 + a search over the handle's matrix arrays (worth 1-5 %, ~500 launches).
	                           SPMV_MI355X_PLACEMENT in the environment overrides: 0 off, 1 on, 2 on + log on stderr, 3, 4 (diagnostic) */
	int  placement_budget_gib;  /* transient memory the walk may hold, GiB (0 = 160; it never takes the device's last 8 GiB)             */
	int  sell_values;       /* SELL delta layout, fp64: slices whose values (in their full groups of 4 steps) are all +-0 / denormal or finite
	                           normals within 7 binades store each value in 7 bytes (sign, 3-bit exponent code against a per-slice base,
	                           52-bit mantissa; lossless, bit-identical results; csrc/launch.hpp). 0 = auto (on when the plain value array
	                           exceeds the 256 MiB Infinity Cache), 1 = on, 2 = off. SPMV_MI355X_SELL_VALUES in the environment overrides */
	int  value_storage;     /* how the matrix VALUES are stored, independent of the precision of x and y:
	                           0 = in the handle's precision (default), 1 = fp32. See "mixed precision" below.                  */
	int  transpose;         /* 0 = a handle of A (default), 1 = a handle of A^t, transposed on the GPU from the CSR of A. See "transposed
	                           handles" below. (The field took the struct's tail padding: sizeof did not change, and a caller that
	                           zero-initialises as asked above has 0 here.)                                                       */
} spmv_mi355x_opts;

/* ---- mixed precision: fp64 vectors over fp32-stored values (opts.value_storage = 1) ------------------------------------- */
/* With precision SPMV_MI355X_F64 and value_storage = 1 the values are narrowed to fp32 on upload, exactly as an F32 handle narrows
 * them, while x, y, every product and every row sum stay fp64: the kernel widens each stored value (exactly) and runs the fp64
 * kernel's FMAs in the fp64 kernel's order. The value stream is half as long: about 4.3 instead of 8.3 bytes per non-zero in the
 * delta layout's index-free modes.
 *   - LOSSY, and therefore never chosen automatically: the product is that of the ROUNDED matrix, bit-identical to what an fp64
 *     handle (sell_values = 2) built from (double) (float) values gives, on every variant of the layout and for spmm of any k.
 *     Each stored value is off by at most half an fp32 ulp (2^-24 relative); a value outside fp32's range becomes +-inf or is
 *     flushed, as in an F32 handle.
 *   - served by SPMV_MI355X_SELL_C_SIGMA in the delta layout only (spmv_mi355x_create and spmv_mi355x_create_from_stream). The
 *     stored arrays are byte for byte those of the F32 handle of the same matrix and options. With the field set the automatic
 *     choices go to that layout: sell_window auto = off, sell_values auto = off (7-byte records are fp64 only), and
 *     symmetric_input = 1 always expands the triangle at create(). Row blocks and column filters work as always.
 *   - rc 1, with a last_error that names value_storage and before any device is touched, for: another format, sell_window = 1,
 *     sell_delta = 2, sell_c other than 0 or 64, sell_values = 1; and for any value_storage other than 0 or 1.
 *   - with precision SPMV_MI355X_F32 value_storage = 1 is accepted and changes nothing (whatever the format and layout).
 *   - format_name() of a mixed handle ends in "_v4" (4-byte values under fp64 vectors: MI355X_SELLD_64_16384_d_v4);
 *     spmv_mi355x_precision() keeps meaning the precision of x and y, spmv_mi355x_value_storage() tells that of the stored values;
 *     mem_footprint() counts the stored bytes, csr_mem_footprint() keeps normalising by the vector precision (the fp64 problem);
 *     spmv_mi355x_sell_layout() returns the stored values widened to fp64.
 *   - the solvers (pcg, pbicgstab, their _multi forms) run on a mixed handle unchanged, with fp64 vectors.
 * A caller whose struct_size ends before the field gets value_storage = 0. */

/* ---- transposed handles: y = A^t x from the CSR of A (opts.transpose = 1) ------------------------------------------------------- */
/* Callers that need both products (A D A^t of interior-point steps, CGLS / LSQR, BiCG / QMR, restriction with R = P^t) create a second
 * handle with transpose = 1 from the same arrays: spmv_mi355x_create(m, n, nnz, row_ptr, col_idx, values) and
 * spmv_mi355x_create_from_stream then build a handle of A^t: rows() is n, cols() is m, x has m values and y has n. The CSR is
 * transposed in device memory (csrc/transpose_csr.hip) and the handle is built in A^t's own best layout, so every kernel, spmm, the
 * solvers, the 7-byte and fp32 value stores and placement serve it unchanged and deterministically. There is no y = A^t x over the
 * layout of A: that would be one scattered fp64 atomic per entry (profiles/r01_atomic_bench.txt) and not reproducible.
 * THE CONTRACT: a handle built from (A, opts with transpose = 1) is indistinguishable from the handle create() builds from the CSR of
 * A^t with transpose = 0 and otherwise equal opts, where that CSR has the rows of A^t in order, inside a row its entries in ascending
 * row of A, and entries of equal (row, column) in their input order (a stable counting sort by column). Indistinguishable: every array
 * of spmv_mi355x_stored_array is byte-identical, format_name (no suffix) / mem_footprint / csr_mem_footprint / nnz / sell_layout /
 * kernel_info / spmm_plan answer the same, and spmv, spmm and the solvers give the same bits on every deterministic layout.
 * spmv_mi355x_transposed() tells the two apart.
 *   - order of the input stage: the caller's arrays are validated as they are (row_ptr monotone, columns in [0, n), the int32 limits
 *     — same messages — plus n + nnz < 2^31 for the transposed shape), then transposed; EVERY other option sees the n x m matrix A^t:
 *     row_begin / row_end are rows of A^t, the column filter bounds are columns of A^t, and the automatic layout choices (LDS window,
 *     7-byte values, nontemporal) are made on A^t. convert_on = 2 transposes on the host (the checker of the GPU routine; same bytes).
 *   - create() uploads the CSR, transposes it on the device and downloads the result (12 bytes per non-zero each way) so that the row
 *     block, the column filter and every format's builder run from one local CSR; create_from_stream transposes the resident arrays
 *     and nothing passes through the host. Transient device memory: 16 bytes per non-zero + the sort's scratch, next to the CSR of
 *     A^t (12 bytes per non-zero); all of it is freed before the format is built (the stream's own arrays too).
 *   - rc 1 with a last_error that names transpose, before any device is touched: a value other than 0 or 1; transpose = 1 with
 *     symmetric_input = 1 (the transpose of a symmetric matrix is the matrix itself); spmv_mi355x_create_partitioned with
 *     transpose = 1 (its parts would each transpose the whole matrix).
 *   - update_values / update_values_device refuse a transposed handle (rc 1, update_values_state 0: its entries are not in the
 *     caller's order) until spmv_mi355x_update_values_prepare_transposed has derived the entry map from the pattern of A; from then
 *     on they take new values in A's entry order ("new values for an existing handle"). The map is not made at create(): it is 4 bytes
 *     per entry that only a caller who updates needs, and a transposed handle's footprint is that of the handle of A^t.
 *   - the solvers read the Jacobi diagonal from the host CSR they are given: on a transposed handle pass the CSR create() was given
 *     (that of A) — the diagonal of A^t is that of A.
 * A caller whose struct_size ends before the field gets transpose = 0. */

/* ---- library / device ------------------------------------------------------------------------------------ */
const char * spmv_mi355x_last_error(void);
int  spmv_mi355x_device_count(int * count_out);
int  spmv_mi355x_device_info(int device, char * name_out, long name_n, int * compute_units_out, long * hbm_bytes_out);

/* ---- construction = csr_to_format() (csr.cpp:221-240 and the per-format constructors) ------------------------ */
int  spmv_mi355x_create(spmv_mi355x_matrix ** out, int format, int precision,
		long m, long n, long nnz,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const spmv_mi355x_opts * opts /* may be NULL */);
int  spmv_mi355x_destroy(spmv_mi355x_matrix * A);

/* Matrix_Format fields (spmv_kernel.h:10-15,23) */
const char * spmv_mi355x_format_name(const spmv_mi355x_matrix * A);
double spmv_mi355x_mem_footprint(const spmv_mi355x_matrix * A);      /* bytes of the device-side format            */
double spmv_mi355x_csr_mem_footprint(const spmv_mi355x_matrix * A);  /* nnz*(sizeof(V)+4)+(m+1)*4                  */
long   spmv_mi355x_rows(const spmv_mi355x_matrix * A);               /* local rows (row block)                      */
long   spmv_mi355x_cols(const spmv_mi355x_matrix * A);
long   spmv_mi355x_nnz(const spmv_mi355x_matrix * A);                /* local non-zeros after row/column filtering  */
int    spmv_mi355x_precision(const spmv_mi355x_matrix * A);          /* SPMV_MI355X_F64 / SPMV_MI355X_F32 of x and y */
int    spmv_mi355x_value_storage(const spmv_mi355x_matrix * A);      /* ... of the stored values (opts.value_storage); NULL: -1 */
int    spmv_mi355x_device(const spmv_mi355x_matrix * A);             /* HIP device ordinal the handle lives on      */
int    spmv_mi355x_transposed(const spmv_mi355x_matrix * A);         /* 1 = built with opts.transpose = 1, else 0; NULL: -1 */

/* ---- a handle from a CSR that arrives in pieces ---------------------------------------------------------------------- */
/* spmv_mi355x_create() needs the whole CSR in host memory at once. A caller that generates or reads its rows piece by piece (a rank
 * of a multi-GPU run: bench.py --gpus N) appends them to a CSR kept in DEVICE memory — every piece is checked like create() checks a
 * matrix (row_ptr from 0 and monotone, columns in [0, n)) — and gets ONE handle converted on the GPU from the resident CSR; the host
 * never holds more than a piece. nnz_capacity: an upper bound of the non-zeros to come (device arrays of that size live until
 * create_from_stream). Pieces are consecutive rows in order; a piece's row_ptr has rows + 1 entries starting at 0.
 * create_from_stream consumes the stream (also on failure). Formats: SPMV_MI355X_SELL_C_SIGMA with 64-row slices and the delta
 * layout (what create() picks for large matrices; same arrays, same results); opts fields of other layouts are rejected.
 * No reference counterpart: csr_to_format() receives complete arrays (spmv_kernel.h:8-29). */
typedef struct spmv_mi355x_csr_stream spmv_mi355x_csr_stream;
int  spmv_mi355x_csr_stream_begin(spmv_mi355x_csr_stream ** out, int device /* -1: current */, long m, long n, long nnz_capacity);
int  spmv_mi355x_csr_stream_append(spmv_mi355x_csr_stream * s, long rows, const int32_t * row_ptr, const int32_t * col_idx,
		const double * values);
int  spmv_mi355x_create_from_stream(spmv_mi355x_matrix ** out, spmv_mi355x_csr_stream * s, int format, int precision,
		const spmv_mi355x_opts * opts);
int  spmv_mi355x_csr_stream_discard(spmv_mi355x_csr_stream * s);

/* ---- new values for an existing handle --------------------------------------------------------------------------------- */
/* Same pattern, new numbers: a Newton / interior-point / time-stepping caller changes the values of its matrix between solves and
 * never its pattern. update_values rewrites the stored value array in place and keeps everything create() derived from the pattern
 * (row sort, index encodings, LDS-window groups, tile maps, the uploaded column indices, the placement of the arrays).
 * THE CONTRACT: a handle created from (pattern, V1, opts) and updated with V2 is indistinguishable from one freshly created from
 * (pattern, V2, opts): every array spmv_mi355x_stored_array exposes is byte-identical, format_name / mem_footprint / sell_layout /
 * kernel_info / spmm_plan answer the same, and spmv, spmm and the solvers give the same bits on every deterministic layout.
 *   - values: nnz() fp64 values, values[e] belonging to entry e of the handle's LOCAL CSR (for a row block created with
 *     opts.row_begin / row_end: that contiguous stretch of the caller's array), narrowed to the handle's value storage as create()
 *     narrows them (fp32 for an F32 handle and for value_storage = 1). NaN and Inf pass through, as in create().
 *   - prepare, once per handle before the first update: row_ptr = the local row pointer the handle was built from (host, rows() + 1
 *     entries from 0). It is checked (starts at 0, monotone, ends at nnz(); SELL layouts: every slice's stored width against the
 *     longest of its rows — a mismatch is "row_ptr does not match the pattern this handle was built from") and a device copy is kept
 *     (4 * (rows() + 1) bytes, not counted in mem_footprint(), freed at destroy). THE COLUMNS CANNOT BE VERIFIED: values passed in the
 *     order of another pattern with the same row lengths are stored as given. CSR-ordered layouts need no map, but prepare is required
 *     all the same (one protocol). Calling it again replaces the copy.
 *   - update_values_device orders its work on hip_stream behind what is enqueued there and WAITS for it (blocking, as every entry
 *     without _async): with 7-byte values the host-side counts of the handle change. update_values is the same through a transient
 *     device copy of the host array.
 *   - what create() chooses from the values is chosen again: the slices of a delta handle that store 7-byte values (sell_values on, or
 *     auto on a large matrix), with the value offsets, descriptors, tile map, footprint, nontemporal rule and the _v7 suffix that follow
 *     (the value array is reallocated when the new selection needs more room); and the merge path's dropping of a uniform value
 *     stream: a merge handle updated with uniform values becomes the _unit handle create() would build — and, like it, takes no
 *     further update.
 *   - kept: the handle's x / y device buffers and its cached-x state, its spmm scratch, arrays moved by placement level 3 (they are
 *     written where they live). The next host-buffer spmv downloads y again.
 *   - rc 1, a last_error naming update_values, the handle untouched: a NULL handle or pointer; update before prepare; a handle created
 *     with opts.transpose = 1 that has no entry map yet (see below), with a column filter (col_filter_mode != 0: its entries
 *     are a subset of the caller's) or with symmetric_input = 1 (expanded or
 *     kept as a triangle: its entries are not the caller's); the column-blocked layout (col_blocks != 0: entries sorted by column); a
 *     handle without a value stream (the _unit layouts of uniform values). spmv_mi355x_partitioned handles have no such entry (their
 *     parts carry column filters).
 *   - update_values_state, host-only: 0 = this handle cannot be updated (last_error says why), 1 = it can, prepare is still missing,
 *     2 = ready. NULL: 0.
 * TRANSPOSED HANDLES (opts.transpose = 1): the caller holds the CSR of A, the handle the entries of A^t in the order of the
 * transposition. update_values_prepare_transposed, once per handle before its first update, takes the PATTERN of A as create() or the
 * stream was given it (m, n, row_ptr of m + 1 and col_idx of row_ptr[m] entries, host arrays, row_ptr from 0; no values) and derives
 * the ENTRY MAP src: entry e of the handle's local CSR is entry src[e] of the CSR of A. From then on update_values and
 * update_values_device read update_values_count() = nnz(A) fp64 values, values[e] belonging to entry e of the CSR of A — all of A's
 * values, also when the handle holds a row block of A^t — so ONE array of new values refreshes the handle of A and the handle of A^t.
 * THE CONTRACT: a handle created from (pattern of A, V1, opts with transpose = 1), prepared and updated with V2, is indistinguishable
 * (as above) from the handle create() builds from (pattern of A, V2, the same opts), and so from the handle of the CSR of A^t with V2.
 *   - the pattern is checked as create() checks it (row_ptr from 0 and monotone, columns in [0, n): same messages) and against what
 *     the handle recorded at create: m == cols(At), n == the rows of the whole A^t, row_ptr[m] == nnz(A) (a mismatch names both
 *     numbers). It is uploaded and ordered on the GPU by the transposition's own stable sort by column (csrc/transpose_csr.hip:
 *     one definition of the order); the sorted entry numbers are the map, for a row block [row_begin, row_end) of A^t that stretch of
 *     them with the row pointer rebased to 0. A handle created with convert_on = 2 (or SPMV_MI355X_HOST_CONVERT) derives the map on the
 *     host with the order's host form instead: the checker, same bytes. The derived local row pointer then passes the checks of
 *     update_values_prepare: it ends at nnz(), and on SELL layouts every slice's stored width equals the longest of its rows — else
 *     "the pattern does not match the pattern this handle was built from". NOT CHECKABLE: a pattern with the same number of entries
 *     per column (row of A^t) within every slice but other row positions: its values are stored as the map orders them.
 *   - kept with the handle until destroy or the next prepare_transposed, neither counted in mem_footprint(): the local row pointer
 *     (4 * (rows() + 1) bytes) and the map (4 * nnz() bytes). Transient device memory during the call: the pattern of A (4 bytes per
 *     row and per non-zero), the row pointer of A^t, and what the transposition takes without its value arrays: 16 bytes per non-zero
 *     + the sort's scratch.
 *   - an update gathers va_t[e] = values[src[e]] into a transient device array of nnz() doubles (one launch, 12 bytes read and 8
 *     written per entry) and then runs the update above unchanged, 7-byte re-selection, reallocation and the merge path's _unit rule
 *     included. Everything is ordered on hip_stream and the call blocks; the host form uploads update_values_count() doubles first.
 *   - state: 0 before prepare_transposed (last_error names transpose), 2 after. update_values_prepare keeps refusing a transposed
 *     handle, prepared or not (a prepared one stays prepared). prepare_transposed returns rc 1 with a last_error naming
 *     update_values_prepare_transposed, the handle untouched, for a NULL handle or array, a handle created with transpose = 0, a
 *     handle no map can serve (column filter, col_blocks, a _unit layout), a shape or nnz mismatch, a bad pattern; the NULL and argument
 *     errors come before any device is touched.
 *   - update_values_count, host-only: the values an update of this handle reads: nnz(), and nnz(A) once prepare_transposed has run.
 *     NULL: -1.
 * SPMV_MI355X_UPDATE_STAGE = 0 makes the SELL kernels read every row straight from global memory instead of staging a slice's
 * contiguous stretch of the CSR array through LDS. */
int  spmv_mi355x_update_values_prepare(spmv_mi355x_matrix * A, const int32_t * row_ptr);
int  spmv_mi355x_update_values(spmv_mi355x_matrix * A, const double * values_fp64_host);
int  spmv_mi355x_update_values_device(spmv_mi355x_matrix * A, const double * values_fp64_dev, void * hip_stream);
int  spmv_mi355x_update_values_state(const spmv_mi355x_matrix * A);
int  spmv_mi355x_update_values_prepare_transposed(spmv_mi355x_matrix * At, long m, long n,
		const int32_t * row_ptr, const int32_t * col_idx);
long spmv_mi355x_update_values_count(const spmv_mi355x_matrix * A);

/* ---- Matrix_Format::spmv(x, y) with HOST buffers --------------------------------------------------------- */
/* Reference GPU-backend semantics (GPU_clean/csr_rocm_vector.cpp:224-257): x is uploaded when the host
 * pointer is new (or always_copy is set), one launch + device sync, y is downloaded on the first call (or when
 * always_copy is set). x: n values, y: rows values, both of the handle's precision. */
int  spmv_mi355x_spmv(spmv_mi355x_matrix * A, const void * x_host, void * y_host);
int  spmv_mi355x_set_always_copy(spmv_mi355x_matrix * A, int on);   /* for callers whose x changes (bench_cg.cpp)  */
int  spmv_mi355x_upload_x(spmv_mi355x_matrix * A, const void * x_host);
int  spmv_mi355x_download_y(spmv_mi355x_matrix * A, void * y_host);

/* ---- device-pointer entry points (solvers, multi-GPU, benchmarks) ---------------------------------------- */
/* y_dev = A * x_dev (beta == 0) or y_dev += A * x_dev (beta == 1), enqueued on hip_stream (a hipStream_t passed
 * as void*, NULL = the default stream); returns after enqueue. */
int  spmv_mi355x_spmv_device_async(spmv_mi355x_matrix * A, const void * x_dev, void * y_dev, int beta, void * hip_stream);
/* Special values (y = A x and y += A x; every format, layout, precision and value storage; the host-buffer call and spmm alike):
 *   1. confinement: y[i] is non-finite exactly for the rows i that STORE an entry in a column j whose x[j] is Inf or NaN — a
 *      stored value times Inf or NaN is never finite, a stored 0.0 gives NaN as in the sequential loop — or that store a
 *      non-finite value (a value may also narrow to Inf in fp32 storage). Every other row is finite and as accurate as on finite
 *      input (bit-identical to the sequential CSR loop for the row-sequential kernels). The padding of the SELL layouts (a 0.0 at a
 *      valid column) never multiplies the x of a column the row does not store — an empty row's sum
 *      is dropped, the delta layout masks the padding steps of the slices that hold rows of different lengths, the LDS-window
 *      layout points its padding at a zero of its own. Whether a reached row holds +Inf, -Inf or NaN is not specified.
 *   2. beta == 0 overwrites y whatever it held, NaN included; beta == 1 adds to it.
 *   3. subnormal inputs and products are computed, not flushed, in fp64 and fp32, the atomic layouts included.
 * The triangular solves propagate likewise: a non-finite b[i] reaches x[i] and the rows that depend on it, nothing else.
 * (tests/test_gpu_special_values.py) */
/* Time `iters` back-to-back launches with HIP events recorded on the stream the kernels run on; ms per iteration. */
int  spmv_mi355x_time_device(spmv_mi355x_matrix * A, const void * x_dev, void * y_dev, int iters,
		void * hip_stream, double * ms_per_iter_out);
/* ---- Y = A X for k vectors at once ------------------------------------------------------------------------------------ */
/* Y = A X (beta == 0) or Y += A X (beta == 1) for k >= 1 vectors at once, enqueued on hip_stream.
 * X: cols() rows of k values, row i at X_dev + i*ldx (ldx >= k, counted in values of the handle's precision);
 * Y: rows() rows, row i at Y_dev + i*ldy (ldy >= k). Only Y[i*ldy + j], i < rows(), j < k is written.
 * Column j of Y is bit-identical to spmv_mi355x_spmv_device_async(A, x_j, y_j, beta, ...) on the contiguous column x_j
 * whenever that product is deterministic (every layout without LDS / global atomics).
 * The SELL-C-sigma delta layout reads the matrix once per PASS of up to 8 columns: k runs as passes of the largest power of two
 * <= min(8, columns left) (k = 7: 4 + 2 + 1, k = 16: 8 + 8). The SELL-C-sigma LDS-window layout (MI355X_SELLW_*, not its
 * symmetric-storage form) does the same with Kmax in place of 8: a pass of K columns keeps the slice group's window of X in LDS,
 *     need(K) = align16((wmax + 1) * K * sizeof(value)) + (waves per slice > 1 ? threads per workgroup * K * sizeof(value) : 0)
 * bytes (wmax = the widest window of the handle's groups), and Kmax is the largest K in {8, 4, 2, 1} with need(K) <= 163 840, the
 * LDS one workgroup may declare (Kmax = 2: k = 5 runs as 2 + 2 + 1). Its kernel reads strided X and writes strided Y itself, also
 * when Kmax = 1. On both layouts k == 1 with ldx == ldy == 1 is the single-vector kernel itself. Every other layout runs the
 * single-vector product once per column, through a column of scratch the handle owns (allocated at its first such call), so one
 * handle serves one spmm at a time. spmv_mi355x_spmm_plan tells which of these a handle does.
 * rc 1 without touching memory for k < 1, ldx < k, ldy < k, a NULL handle, or a NULL X / Y where columns / rows exist. */
int  spmv_mi355x_spmm_device_async(spmv_mi355x_matrix * A, int k, const void * X_dev, long ldx, void * Y_dev, long ldy,
		int beta, void * hip_stream);
/* How spmm_device_async serves k columns on this handle: times the matrix arrays are streamed, and the most columns one pass serves
 * (1 = one column per pass). Host-only: touches no device. rc 1 for a NULL handle, k < 1 or a NULL out pointer. */
int  spmv_mi355x_spmm_plan(const spmv_mi355x_matrix * A, int k, int * matrix_passes_out, int * max_cols_per_pass_out);
/* HIP-event timing of `iters` back-to-back spmm launches (beta 0), like spmv_mi355x_time_device */
int  spmv_mi355x_time_spmm_device(spmv_mi355x_matrix * A, int k, const void * X_dev, long ldx, void * Y_dev, long ldy,
		int iters, void * hip_stream, double * ms_per_iter_out);
/* blocking host-buffer form: X is cols() x k, Y is rows() x k, both dense row-major (ld = k) */
int  spmv_mi355x_spmm(spmv_mi355x_matrix * A, int k, const void * X_host, void * Y_host);

/* Name and launch shape of the dominant kernel (for matching rocprofv3 kernel-trace rows). */
int  spmv_mi355x_kernel_info(const spmv_mi355x_matrix * A, char * name_out, long name_n, long * grid_out, int * block_out);

/* dst_dev[0..bytes) = src_dev[0..bytes), enqueued on hip_stream: lets a caller without HIP headers (the ctypes / cgo side of
 * the distributed solver callbacks) move a vector slice into its exchange buffer. */
int  spmv_mi355x_copy_device_async(void * dst_dev, const void * src_dev, long bytes, void * hip_stream);

/* Device buffers owned by the handle (allocated lazily by the host-buffer entry points): x has n values, y has rows + 64
 * (the reference driver's slack, bench_spmv.cpp:606-609). With opts.placement = 1 both are placed by the engine (below). */
void * spmv_mi355x_x_device(spmv_mi355x_matrix * A);
void * spmv_mi355x_y_device(spmv_mi355x_matrix * A);
int  spmv_mi355x_upload_y(spmv_mi355x_matrix * A, const void * y_host);      /* rows values into the handle's y (for y += A x) */

/* ---- vectors placed by the engine --------------------------------------------------------------------------------- */
/* The 288 GiB of an MI355X behave as 32 GiB blocks that fall into classes, and the same kernel on the same matrix and x takes 1.28 or
 * 1.46 ms (nlpkkt240 twin) depending only on whether y lives in a block of the same class as the value array; which memory an
 * allocation gets is the driver's choice (profiles/r02_placement.md). With opts.placement = 1 (or SPMV_MI355X_PLACEMENT
 * >= 1) the engine keeps, per process and device, two to four VECTOR POOLS (1-4 GiB each) in blocks of different class: the first
 * handle that needs a vector of 8 MiB or more walks the device's free memory once — candidates 16 GiB of ballast apart, timed with the
 * handle's own kernel; one that differs by 1.5 % from every candidate kept so far is kept; the walk ends three candidates after the
 * last new class; at most opts.placement_budget_gib (160) of ballast, returned when the walk ends — and every later vector of any
 * handle is a slice of the pool in which that handle's kernel runs fastest (one trial of six launches per pool). The handle's own pair (spmv_mi355x_x_device / y_device, used by spmv_mi355x_spmv) is placed this way; output_alloc /
 * input_alloc give callers of the device-pointer entry points the same for vectors the handle's SpMV writes / reads (bytes >= (rows +
 * 64) resp. cols values; smaller, under 8 MiB or with placement off: a plain allocation). Zero-filled. Free with output_free.
 * OFF by default: the walk holds tens of GiB for a fraction of a second, its free-memory check is racy against other processes on the
 * same GPU, and the driver clears the returned ballast in the background for a few seconds, during which any process's kernels on that
 * GPU run up to 5 % slower (profiles/r02_placement.md §6). placement_release frees a device's pools (no vector of them may be live).
 * No reference counterpart (the reference's GPU backends hipMalloc their vectors in the constructor, GPU_clean/csr_rocm_vector.cpp:77-86). */
int  spmv_mi355x_output_alloc(spmv_mi355x_matrix * A, size_t bytes, void ** out);
int  spmv_mi355x_input_alloc(spmv_mi355x_matrix * A, size_t bytes, void ** out);
int  spmv_mi355x_output_free(void * p);
/* The search over the handle's MATRIX arrays that opts.placement = 3 runs for the handle's own vector pair, for a caller's pair: every
 * array of 16 MiB .. 8 GiB is tried at up to ten sites 16 GiB of ballast apart (a device copy and six launches of y = A x per trial; y is
 * overwritten) and stays where the kernel ran fastest if that beats where it was by 2 %. Same budget and the same caveats as the walk. */
int  spmv_mi355x_place_arrays(spmv_mi355x_matrix * A, const void * x_dev, void * y_dev);
int  spmv_mi355x_placement_release(int device /* -1: every device */);
/* what the walk of a device found: state 0 = none made yet, 1 = pools of different block class kept, 2 = no contrast inside the budget
 * (plain allocations); candidates timed, GiB of ballast held at its deepest, the number of pools, the walking handle's kernel time (us)
 * with y in each */
int  spmv_mi355x_placement_info(int device, int * state_out, int * candidates_out, long * walked_gib_out, int * pools_out, double us_out[4]);

/* ---- solver callers of spmv() ---------------------------------------------------------------- */
/* Device-resident replacements for the reference's two Krylov drivers, which call MF->spmv() with a vector that changes
 * every iteration:  spmv_mi355x_pcg       = preconditioned_cg()        benchmark_code/BENCH/src/bench_cg.cpp:93-322
 *                   spmv_mi355x_pbicgstab = preconditioned_bicgstab()  benchmark_code/BENCH/src/bench_bicg.cpp:149-459
 * Arguments as in the reference: the handle (MF), the host CSR arrays the Jacobi preconditioner K = diag(A) is read from
 * (values in fp64 = ValueTypeReference, like spmv_mi355x_create), b and x_res_out as HOST arrays of the handle's
 * precision, max_iterations (CG_MAX_NUM_ITERS). Same semantics: x0 = 0, eps = 1e-15*|b|, explicit residual every 100
 * iterations with best-x tracking, CG restart rule and `err < eps` break, BiCGSTAB never breaks; errors "bad K, zero in
 * diagonal" and "the matrix must be square" are returned (rc 1 + last_error) instead of exit(1).
 * history_out (may be NULL): 3*max_iterations doubles; row k = error, error_explicit, error_best as the reference prints
 * them at iteration k (bench_cg.cpp:249); rows >= info->iterations stay 0. */
typedef struct {
	unsigned struct_size;      /* in: sizeof(spmv_mi355x_solver_info) */
	long   iterations;         /* num_loops_out (bench_cg.cpp:315) */
	double error;              /* |b - A*x_res_out|, the CSV "error" column (bench_cg.cpp:412-418) */
	double error_best;         /* err_best: smallest explicit residual seen = the one of x_res_out */
	double eps, eps_counter;   /* 1e-15*|b|, 1e-7*|b| (bench_cg.cpp:159-174) */
	long   restarts;           /* CG restarts taken (bench_cg.cpp:219-235) */
	long   spmv_calls;         /* SpMV launches the solver made */
	double seconds;            /* wall time of the whole call = the CSV "time" column */
} spmv_mi355x_solver_info;
int  spmv_mi355x_pcg(spmv_mi355x_matrix * A, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * b_host, void * x_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info);
int  spmv_mi355x_pbicgstab(spmv_mi355x_matrix * A, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * b_host, void * x_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info);

/* Multi-RHS form of the same two solvers: k independent systems A x_j = b_j on one handle. Column j returns exactly (bit for
 * bit) what spmv_mi355x_pcg / _pbicgstab return for b_j on the same handle whenever the handle's SpMV is deterministic; the
 * k recurrences stay independent (no shared Krylov subspace). What is shared: one spmv_mi355x_spmm_device_async pass over
 * the matrix per SpMV of the single solver, every kernel launch, the Jacobi diagonal.
 * B_host is rows() x k, row-major (ld = k), in the handle's precision; X_res_out_host has the same shape and receives each
 * column's x_best. history_out (may be NULL): k * 3 * max_iterations doubles, column j's block at
 * history_out + j * 3 * max_iterations, laid out as the single solver's. info (may be NULL): an array of k elements whose
 * stride is the caller's info[0].struct_size; every element is written with that size. iterations, error, error_best, eps,
 * eps_counter and restarts are per column; spmv_calls counts the SpMM launches of the call and seconds is its wall time
 * (both the same in every element). The host stops enqueueing once every column has reached its `err < eps` break (with
 * the single solver's polling lag); until then a broken column stays frozen. Errors as the single solvers, plus k < 1;
 * argument errors return before any device is touched. */
int  spmv_mi355x_pcg_multi(spmv_mi355x_matrix * A, int k, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * B_host, void * X_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info);
int  spmv_mi355x_pbicgstab_multi(spmv_mi355x_matrix * A, int k, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const void * B_host, void * X_res_out_host, long max_iterations, double * history_out, spmv_mi355x_solver_info * info);

/* ---- CGLS: least squares over a handle of A and a handle of A^t ------------------------------------------------------------ */
/* min |A x - b|^2 + damp * |x|^2 (damp >= 0, Tikhonov) for ANY m x n matrix — tall, wide, rank-deficient — from x0 = 0, so that an
 * underdetermined system with damp = 0 returns its minimum-norm solution. The CGLS recurrences, A^t A never formed, every vector
 * resident in device memory (csrc/solver_cgls.hip; 2 SpMV + 4 vector launches per iteration):
 *     r = b; s = A^t r; p = s; gamma = s.s; gamma0 = gamma
 *     loop k: q = A p;  delta = q.q + damp * p.p;  alpha = gamma / delta;  x += alpha p;  r -= alpha q;
 *             s = A^t r - damp * x;  gamma' = s.s;  beta = gamma' / gamma;  p = s + beta p;  gamma = gamma'
 *             stop when sqrt(gamma') <= tol * sqrt(gamma0)
 *   - A is m x n; At is a handle of its transpose (n x m), built with opts.transpose = 1 or from the caller's own CSR of A^t;
 *     spmv_mi355x_transposed() is not consulted. CHECKED: rows(At) == cols(A), cols(At) == rows(A), the same precision, the same
 *     device. NOT CHECKABLE: that At really holds A^t — with another n x m matrix the recurrences run on and mean nothing.
 *   - b_host: m values, x_out_host: n values, both of the handles' precision. Scalars and dot products are fp64 in both precisions.
 *   - any format and layout serves (the solver only calls spmv_mi355x_spmv_device_async), value_storage = 1, 7-byte values and row
 *     blocks of At's own rules included; on handles whose SpMV is deterministic the whole solve is, bit for bit. The solver's vectors
 *     are plain allocations (placement is not used, as in pcg).
 *   - tol == 0 is legal and means "never stop on the tolerance". max_iterations == 0 returns x = 0, stop 2 and the norms of x = 0.
 *   - history_out (may be NULL): 2 * max_iterations doubles; row k = (|r_{k+1}|, |s_{k+1}|) after loop body k, both the RECURSIVE
 *     quantities; rows >= info->iterations stay 0.
 *   - after a stop the iteration is frozen on the device: x, iterations and the history are those of the iteration at which the
 *     rule fired, however far the host had run ahead (at most 64 iterations).
 *   - rc 1, a last_error that names cgls, before any device is touched and with every caller buffer untouched: a NULL A, At, b or
 *     x_out; info->struct_size < 8; damp or tol negative or not finite; max_iterations < 0; a shape (the message gives both),
 *     precision or device mismatch between the two handles. */
typedef struct {
	unsigned struct_size;   /* in: sizeof(spmv_mi355x_lsq_info) */
	long   iterations;      /* completed loop bodies */
	int    stop;            /* 1 = |s_k| <= tol*|s_0|, 2 = max_iterations reached, 3 = A^t b == 0 (x = 0 returned, 0 iterations),
	                           4 = breakdown: delta = |q|^2 + damp*|p|^2 was 0 or not finite (x of the last good iteration returned) */
	double rnorm;           /* |b - A x_out|, EXPLICIT (one SpMV with A after the loop) */
	double arnorm;          /* |A^t (b - A x_out) - damp * x_out|, EXPLICIT (one SpMV with At after the loop) */
	double arnorm0;         /* |A^t b| */
	double xnorm;           /* |x_out| */
	long   spmv_calls;      /* SpMV launches of the whole call, both handles, setup and the two explicit ones included */
	double seconds;         /* wall time of the call */
} spmv_mi355x_lsq_info;
int  spmv_mi355x_cgls(spmv_mi355x_matrix * A, spmv_mi355x_matrix * At,
		const void * b_host, void * x_out_host, double damp, double tol, long max_iterations,
		double * history_out /* may be NULL: 2*max_iterations doubles */, spmv_mi355x_lsq_info * info /* may be NULL */);

/* ---- MINRES: symmetric indefinite systems over one handle ------------------------------------------------------------------- */
/* (A - shift * I) x = b from x0 = 0 for a square SYMMETRIC matrix: indefinite, singular-but-consistent, saddle-point (KKT) matrices
 * with a zero diagonal block included — what pcg / pbicgstab refuse ("zero in diagonal") and what CG is not defined for. Paige and
 * Saunders' MINRES with an optional DIAGONAL preconditioner given as its inverse, M^-1 = diag(minv): one SpMV per iteration, short
 * recurrences, the residual (in the M^-1 norm) never increases, the diagonal of A is never needed. Every vector is resident in
 * device memory (csrc/solver_minres.hip; 1 SpMV + 3 vector launches per iteration). The recurrences are scipy's
 * minres without its norm-estimate stopping tests, every scalar fp64:
 *     r1 = b; y = M^-1 b; beta1 = sqrt(b.y)                                        (b.y == 0: stop 3; < 0 or not finite: stop 4)
 *     oldb = 0; beta = beta1; dbar = 0; epsln = 0; phibar = beta1; cs = -1; sn = 0; w = w2 = 0; r2 = r1
 *     loop itn = 1, 2, ...:
 *         v = y / beta;  y = A v - shift v;  if itn >= 2: y -= (beta/oldb) r1
 *         alfa = v.y;    y -= (alfa/beta) r2;  r1 = r2;  r2 = y;  y = M^-1 r2
 *         oldb = beta;   beta^2 = r2.y                        (negative or not finite: stop 4, x untouched by this iteration)
 *         beta = sqrt(beta^2)
 *         oldeps = epsln; delta = cs dbar + sn alfa; gbar = sn dbar - cs alfa; epsln = sn beta; dbar = -cs beta
 *         gamma = max(hypot(gbar, beta), DBL_EPSILON); cs = gbar/gamma; sn = beta/gamma; phi = cs phibar; phibar = sn phibar
 *         w1 = w2; w2 = w; w = (v - oldeps w1 - delta w2) / gamma;  x += phi w
 *         history[itn-1] = phibar
 *         if tol > 0 and phibar <= tol beta1: stop 1;  else if beta == 0: stop 5
 *   - b_host, x_out_host and minv_host: rows() values of the handle's precision. Scalars and dot products are fp64 in both precisions.
 *   - minv_host (may be NULL): every entry finite and > 0. NULL = no preconditioner: no extra vector is stored and no multiply is
 *     issued. The library derives no preconditioner itself: the caller knows whether 1/|a_ii|, a row norm or nothing suits its zero
 *     block.
 *   - any format and layout serves (the solver only calls spmv_mi355x_spmv_device_async): value_storage = 1, 7-byte values and
 *     symmetric_input = 1 handles included; on handles whose SpMV is deterministic the whole solve is, bit for bit. The solver's
 *     vectors are plain allocations (placement is not used, as in pcg and cgls).
 *   - tol == 0 is legal and means "never stop on the tolerance". max_iterations == 0 returns x = 0, stop 2 and rnorm = rnorm0.
 *     On stop 3 x = 0 and every norm is 0.
 *   - history_out (may be NULL): max_iterations doubles; entry k = phibar after loop body k + 1, the RECURSIVE residual in the M^-1
 *     norm; entries >= info->iterations stay 0.
 *   - after a stop the iteration is frozen on the device: x, iterations and the history are those of the iteration at which the
 *     rule fired, however far the host had run ahead (at most 64 iterations).
 *   - rc 1, a last_error that names minres, every caller buffer and info untouched. First the scalars, before any device is touched
 *     and before the NULL checks: info->struct_size < 8; shift not finite; tol negative or not finite; max_iterations < 0. Then a
 *     NULL A, b or x_out. Then rows() != cols() (the message gives both; this also refuses row-block handles). Then a minv entry
 *     that is not finite or is <= 0 (the message names the first such index): a host pass over the n values before any launch.
 *   - NOT CHECKABLE: that A is symmetric — on an unsymmetric matrix the recurrences run on and mean nothing; that a
 *     symmetric_input = 1 handle holds what the caller thinks it holds.
 *   - NOT BUILT: multi-RHS and row-partitioned forms, device-pointer b / x, scipy's Anorm / Acond estimates and the stopping tests
 *     built on them. */
typedef struct {
	unsigned struct_size;   /* in: sizeof(spmv_mi355x_minres_info) */
	long   iterations;      /* completed loop bodies */
	int    stop;            /* 1 = phibar_k <= tol * beta1 (tol > 0)
	                           2 = max_iterations reached
	                           3 = b == 0 (beta1 == 0): x = 0, 0 iterations
	                           4 = breakdown: r.(M^-1 r) negative or any scalar not finite;
	                               x of the last good iteration is returned
	                           5 = the Lanczos process ended (beta_{k+1} == 0) */
	double rnorm;           /* |b - (A - shift I) x_out|, EXPLICIT (one SpMV after the loop) */
	double rnorm0;          /* |b| */
	double prnorm;          /* phibar at the stop: recursive residual in the M^-1 norm */
	double prnorm0;         /* beta1 = sqrt(b . M^-1 b) */
	double xnorm;           /* |x_out| */
	long   spmv_calls;      /* the one explicit SpMV included */
	double seconds;
} spmv_mi355x_minres_info;
int  spmv_mi355x_minres(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host,
		double shift, const void * minv_host /* may be NULL */, double tol, long max_iterations,
		double * history_out /* may be NULL: max_iterations doubles */, spmv_mi355x_minres_info * info /* may be NULL */);

/* ---- GMRES(m): general square systems over one handle ----------------------------------------------------------------------- */
/* A x = b from x0 = 0 for ANY square matrix, symmetric or not, a zero on the diagonal included: restarted GMRES with restart length
 * m = `restart`, classical Gram-Schmidt applied twice (CGS2: the dots of a pass are independent, so they are one launch, and two
 * passes keep the basis orthogonal to working precision), Givens rotations on the Hessenberg column, and an optional DIAGONAL RIGHT
 * preconditioner given as its inverse: the solver runs GMRES on A diag(minv) and returns x = diag(minv) u, so the residual it
 * minimises, reports and stops on is the true 2-norm |b - A x|, which never increases within a cycle. Every vector is resident in
 * device memory (csrc/solver_gmres.hip; 1 SpMV + 6 launches per inner step). The recurrences, every scalar and every
 * dot fp64, vectors in the handle's precision, M v = minv v (or v):
 *     x = 0; beta0 = |b|                                                        (beta0 == 0: stop 3; not finite: stop 4)
 *     r = b; beta = beta0; it = 0
 *     cycle:  v_0 = r / beta;  g = (beta, 0, ..., 0);  j = 0
 *       inner step, while j < m and it < max_iterations:
 *         w = A M v_j;  h = 0
 *         twice:  c_i = v_i.w for i <= j, all from the same w;  w -= c_0 v_0, ..., w -= c_j v_j in that order;  h_i += c_i
 *         hn = h_{j+1} = |w|
 *         for i < j:  (h_i, h_{i+1}) = (cs_i h_i + sn_i h_{i+1}, -sn_i h_i + cs_i h_{i+1})
 *         rho = hypot(h_j, h_{j+1})                  (not finite or 0: stop 4; this column is dropped: j, it and x as before it)
 *         cs_j = h_j / rho;  sn_j = h_{j+1} / rho;  h_j = rho;  R[0..j, j] = h[0..j]
 *         g_{j+1} = -sn_j g_j;  g_j = cs_j g_j;  it += 1;  j += 1;  history[it-1] = |g_j|
 *         if tol > 0 and |g_j| <= tol beta0: stop 1;  else if hn == 0: stop 5;  else v_j = w / hn
 *       cycle end:  R[0..j, 0..j] y = g[0..j] by back substitution;  u = y_0 v_0 + ... + y_{j-1} v_{j-1} in that order;  x += M u
 *       if stopped or it >= max_iterations: return
 *       r = b - A x;  beta = |r|;  restarts += 1                                 (beta not finite: stop 4; beta == 0: stop 5)
 *   - b_host, x_out_host and minv_host: rows() values of the handle's precision.
 *   - restart: 1 .. 128. The cap covers three things: the basis of (restart + 1) * rows() values in device memory, the serial
 *     rotation chain that one thread walks in every inner step, and the restart + 4 slots of partial sums.
 *   - minv_host (may be NULL): every entry finite and > 0. NULL = no preconditioner: no extra vector is stored and no multiply is
 *     issued. The library derives no preconditioner itself.
 *   - any format and layout serves (the solver only calls spmv_mi355x_spmv_device_async): value_storage = 1 and 7-byte values
 *     included; on handles whose SpMV is deterministic the whole solve is, bit for bit. The solver's vectors are plain allocations.
 *   - tol == 0 is legal and means "never stop on the tolerance". max_iterations == 0 returns x = 0, stop 2 and rnorm = rnorm0.
 *     On stop 3 x = 0 and every norm is 0.
 *   - history_out (may be NULL): max_iterations doubles; entry k = |g| after inner step k + 1, the RECURSIVE residual; entries >=
 *     info->iterations stay 0.
 *   - after a stop the solve is frozen on the device: x, iterations and the history are those of the step at which the rule fired
 *     (the columns of its unfinished cycle applied once), however far the host had run ahead (at most 64 inner steps).
 *   - rc 1, a last_error that names gmres, every caller buffer and info untouched. First the scalars, before any device is touched
 *     and before the NULL checks: info->struct_size < 8; restart < 1 or > 128; tol negative or not finite; max_iterations < 0. Then a
 *     NULL A, b or x_out. Then rows() != cols() (the message gives both; this also refuses row-block handles). Then a minv entry
 *     that is not finite or is <= 0 (the message names the first such index): a host pass over the n values before any launch.
 *   - NOT BUILT: multi-RHS and row-partitioned forms, device-pointer b / x, left preconditioning, flexible GMRES (a preconditioner
 *     that changes from step to step), a non-zero x0. */
typedef struct {
	unsigned struct_size;   /* in: sizeof(spmv_mi355x_gmres_info) */
	long   iterations;      /* completed inner steps (one SpMV each), over all cycles */
	int    stop;            /* 1 = |g_{j+1}| <= tol * |b| (tol > 0)
	                           2 = max_iterations reached
	                           3 = b == 0: x = 0, 0 iterations
	                           4 = breakdown: a scalar not finite, or rho == 0; x of the last good step's columns is returned
	                           5 = the Krylov space ended: h_{j+1,j} == 0 with rho != 0, or an explicit restart residual == 0 */
	long   restarts;        /* restarts taken = cycles begun after the first */
	double rnorm;           /* |b - A x_out|, EXPLICIT (one SpMV after the loop) */
	double rnorm0;          /* |b| */
	double prnorm;          /* |g_{j+1}| at the stop: the recursive residual (right preconditioning: the true 2-norm one) */
	double xnorm;           /* |x_out| */
	long   spmv_calls;      /* every launch: inner steps incl. the host's run-ahead, one per restart, the explicit one */
	double seconds;
} spmv_mi355x_gmres_info;
int  spmv_mi355x_gmres(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, int restart,
		const void * minv_host /* may be NULL */, double tol, long max_iterations,
		double * history_out /* may be NULL: max_iterations doubles */, spmv_mi355x_gmres_info * info /* may be NULL */);

/* ---- sparse triangular solve: level-scheduled L x = b and U x = b handles --------------------------------------------------------- */
/* What applies Gauss-Seidel / SSOR (A's own triangles) and ILU(0) / IC(0) (the caller's factors, or spmv_mi355x_ilu0's): T x = b for one triangle T of a
 * square n x n matrix given as CSR (csrc/trsv.hip, csrc/kernels_trsv.hip). spmv_mi355x_gmres_tri and
 * spmv_mi355x_pcg_tri (below) are the solvers that call it.
 * WHICH TRIANGLE. uplo = SPMV_MI355X_LOWER keeps the entries with column <= row, SPMV_MI355X_UPPER those with column >= row; entries
 * on the other side are ignored, so one CSR array holding both ILU factors (unit L below, U on and above the diagonal) serves two
 * handles, and the CSR of A serves both halves of a Gauss-Seidel sweep. diag = SPMV_MI355X_DIAG_STORED reads d_i from row i;
 * SPMV_MI355X_DIAG_UNIT takes d_i = 1 and ignores every stored entry with column i, a zero or a missing one included.
 * THE SOLVE, PINNED TO THE BIT. For every row i
 *     s = b[i]
 *     for each kept off-diagonal entry (i, j, a) of row i, in STORED order:   s = fma(-a, x[j], s)
 *     x[i] = s / d_i     (STORED: an IEEE division, never a multiplication by a reciprocal)     |     x[i] = s     (UNIT)
 * with every operation, every value and both vectors in the handle's precision (fma and / on double, fmaf and / on float); values are
 * narrowed on upload exactly as spmv_mi355x_create narrows them. Duplicate off-diagonal entries are separate fmas, stored explicit
 * zeros count as dependencies, padding of the stored layout never contributes an operation. A row's result does not depend on the
 * order in which rows are processed, so every level schedule and launch plan gives the bits of the sequential CPU loop
 * (tests/trsv_reference.c), run after run.
 * THE ANALYSIS (host, O(nnz)). level[i] = 0 when row i has no kept off-diagonal entry, else 1 + the largest level[j] over those
 * entries; LOWER walks the rows in ascending order, UPPER in descending order. A level with at most chain_rows rows is THIN. A
 * maximal run of consecutive thin levels is ONE launch of ONE workgroup, which walks the run with a workgroup barrier between levels;
 * every other level is one launch with one lane per row. launches = (levels that are not thin) + (maximal thin runs); n = 0 gives 0
 * levels and 0 launches. chain_rows: 1 .. 65536, 0 = the default (256, from the sweep in
 * profiles/r16_trsv.txt). The order of the launches on the stream is the only ordering
 * between workgroups: nothing spins on a flag, there is no grid barrier and no cooperative or persistent kernel.
 * spmv_mi355x_trsv_analyze returns what create() derives from the pattern without touching a device (create() runs the same
 * routine; trsv_info agrees with it): level_of_row_out receives a malloc'ed array of n levels (at least one element; free with
 * spmv_mi355x_free), any out pointer may be NULL.
 *   - create() deep-copies its inputs. Stored: the rows permuted by (level, row) in column-major slices of up to 64 rows that never
 *     straddle a level, each with its own width and a per-row length (a long row pads its own slice only), the permutation, and the
 *     diagonal itself. trsv_mem_footprint() is the bytes of these device arrays. nnz_kept of trsv_info counts the entries a solve
 *     reads: the kept off-diagonal ones, plus n diagonal ones under DIAG_STORED.
 *   - solve_device_async: b_dev and x_dev hold n values of the handle's precision on the handle's device; the launches are enqueued
 *     on hip_stream (NULL = the default stream) and the call returns. b_dev == x_dev (in place) is legal; any other overlap is not.
 *     Only x[0 .. n) is written. trsv_solve is the blocking host-buffer form (its two device vectors are allocated at the first
 *     call and kept). n = 0: rc 0, nothing read or written. One solve at a time per handle and vector pair.
 *   - time_trsv_device: HIP-event timing of `iters` back-to-back solves, like spmv_mi355x_time_device.
 *   - rc 1 with a last_error that names trsv, checked in this order, everything but the last on the host before any device is touched:
 *     1. scalars: uplo, diag, precision, n < 0 (or beyond the int32 range), chain_rows < 0 or > 65536;
 *     2. NULL pointers: out, row_ptr; col_idx / values when row_ptr[n] > 0;
 *     3. the pattern, as spmv_mi355x_create checks it and with its messages: row_ptr from 0 and monotone, columns in [0, n);
 *     4. with DIAG_STORED the diagonal of every row, the message naming the first bad row: the diagonal is the first stored entry
 *        with column i (the rule the solvers' Jacobi diagonal uses); it must exist, be finite and be non-zero AFTER narrowing to the
 *        handle's precision; a second entry with column i in the same row is refused;
 *     5. the device: without a usable one the library's "no HIP device available" message; `device` out of range.
 *     trsv_analyze makes the checks 1 to 3 that apply to its arguments. The solve entries refuse a NULL handle and, for n > 0, a NULL
 *     vector; trsv_info a NULL handle; trsv_mem_footprint(NULL) is 0; trsv_destroy(NULL) is rc 0.
 *   - NOT CHECKABLE: that b_dev / x_dev hold n values on the right device.
 *   - NOT BUILT: wiring into pbicgstab / minres (gmres and CG have it: spmv_mi355x_gmres_tri, spmv_mi355x_pcg_tri); a solve
 *     with T^t over T's layout (k right-hand sides ARE served: "K COLUMNS" below; new values for the same pattern too: "UPDATE_VALUES"
 *     below); GPU-side analysis;
 *     graph capture; a row-partitioned form;
 *     a "sync-free" variant in which workgroups wait for each other inside one launch. */
typedef struct spmv_mi355x_trsv spmv_mi355x_trsv;   /* opaque */
enum { SPMV_MI355X_LOWER = 0, SPMV_MI355X_UPPER = 1 };
enum { SPMV_MI355X_DIAG_STORED = 0, SPMV_MI355X_DIAG_UNIT = 1 };
int  spmv_mi355x_trsv_analyze(int uplo, long n, const int32_t * row_ptr, const int32_t * col_idx, int chain_rows /* 0 = default */,
		int32_t ** level_of_row_out /* malloc'ed, spmv_mi355x_free; may be NULL */, long * levels_out, long * launches_out,
		long * max_level_rows_out, int * chain_rows_used_out);
int  spmv_mi355x_trsv_create(spmv_mi355x_trsv ** out, int uplo, int diag, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64, int chain_rows, int device /* -1 = current */);
int  spmv_mi355x_trsv_destroy(spmv_mi355x_trsv * T);
int  spmv_mi355x_trsv_solve_device_async(spmv_mi355x_trsv * T, const void * b_dev, void * x_dev, void * hip_stream);
int  spmv_mi355x_trsv_solve(spmv_mi355x_trsv * T, const void * b_host, void * x_host);          /* blocking */
int  spmv_mi355x_trsv_info(const spmv_mi355x_trsv * T, long * n_out, long * nnz_kept_out, long * levels_out, long * launches_out,
		long * max_level_rows_out, int * chain_rows_out);                                      /* any pointer may be NULL */
double spmv_mi355x_trsv_mem_footprint(const spmv_mi355x_trsv * T);
int  spmv_mi355x_time_trsv_device(spmv_mi355x_trsv * T, const void * b_dev, void * x_dev, int iters, void * hip_stream, double * ms_per_iter_out);

/* THE BLOCKED FORM: the block-Jacobi variant of the same solve, ONE launch per solve. The global plan above is
 * launch-bound (hundreds to thousands of launches, or one workgroup walking thousands of levels through global memory). Here the
 * rows are cut into contiguous blocks of B = block_rows rows, block b owning the rows [b B, min(n, (b + 1) B)) whatever uplo is, and
 * an entry (i, j, a) is kept when the rule above keeps it (LOWER: j < i, UPPER: j > i) AND floor(j / B) == floor(i / B). Every other
 * off-diagonal entry is ignored, exactly as the other triangle is. The diagonal rule (STORED / UNIT, the first stored entry with
 * column i, its checks and messages), the narrowing of the values and the per-row arithmetic are those of the global handle, so x is
 * bit for bit what tests/trsv_reference.c returns for the CSR with the dropped entries removed, and with B >= n, where nothing is
 * dropped, bit for bit what the global handle returns. What is lost is the dropped couplings: as a preconditioner the blocked
 * handle is weaker than the global one and far cheaper to apply.
 * No row depends on a row of another block, so one workgroup solves each block with the block's own level schedule (the level rule
 * above over the kept entries) and all blocks run in one launch; the block's part of x lives in LDS, which is why B is capped. No
 * workgroup reads what another one writes: nothing waits for anything, nothing can hang.
 *   - block_rows: 1 .. 16384 (16384 fp64 values = 128 KiB of the 160 KiB of LDS a workgroup may declare; the same cap for fp32),
 *     0 = the default (4096, NOT yet from a sweep: profiles/r18_trsv_blocked.txt).
 *   - trsv_analyze_blocked: level_of_row_out receives the level of each row WITHIN its block; blocks = ceil(n / B);
 *     max_block_levels = the most levels of any block; max_level_rows = the widest level of any block; nnz_dropped = the off-diagonal
 *     entries of the chosen triangle that cross a block boundary; block_rows_used = B. Any out pointer may be NULL.
 *   - trsv_solve_device_async, trsv_solve, time_trsv_device, trsv_mem_footprint and trsv_destroy serve a blocked handle unchanged.
 *     trsv_info returns n, nnz_kept = the kept in-block entries (+ n under STORED), levels = max_block_levels, launches = 1 (0 when
 *     n == 0), max_level_rows as above, chain_rows = 0. trsv_block_info on a global handle gives block_rows 0, blocks 0, levels 0,
 *     dropped 0.
 *   - Stored: the layout of the global handle with the positions ordered by (block, level within the block, row), the first level
 *     of every block, and the columns block-local in 32 bits: 12 (fp64) / 8 (fp32) bytes per kept entry plus the slices' padding.
 *   - rc 1 in trsv_create's order and with its messages, the prefixes being trsv_create_blocked / trsv_analyze_blocked; block_rows
 *     takes the place of chain_rows in step 1: "block_rows must be 0 (the default) or 1 .. 16384 (got N)".
 *   - NOT BUILT: overlapping blocks, a reordering that would shrink what is dropped, 16-bit columns. */
int  spmv_mi355x_trsv_analyze_blocked(int uplo, long n, const int32_t * row_ptr, const int32_t * col_idx, long block_rows /* 0 = default */,
		int32_t ** level_of_row_out /* level WITHIN the row's block; malloc'ed, spmv_mi355x_free; may be NULL */,
		long * blocks_out, long * max_block_levels_out, long * max_level_rows_out, long * nnz_dropped_out, long * block_rows_used_out);
int  spmv_mi355x_trsv_create_blocked(spmv_mi355x_trsv ** out, int uplo, int diag, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64, long block_rows, int device /* -1 = current */);
int  spmv_mi355x_trsv_block_info(const spmv_mi355x_trsv * T, long * block_rows_out, long * blocks_out, long * max_block_levels_out,
		long * nnz_dropped_out);                                                               /* any out pointer may be NULL */

/* K COLUMNS: T X = B for k right-hand sides over the same handle. Any handle serves, global or blocked, without
 * being rebuilt: there is no new layout and no new analysis. B and X are row-major blocks, row i at ptr + i * ld, ld >= k counted in
 * values of the handle's precision. The columns are solved in chunks of KC = 8, 4, 2 or 1; one chunk is one pass over the plan in
 * which a lane still owns one row, loads the row's length, position, diagonal and every (value, column) pair ONCE, gathers the KC
 * values of x[column] as one row of the block and runs KC fma chains in stored order and KC IEEE divisions. Per column that is
 * exactly the expression of "THE SOLVE, PINNED TO THE BIT", so column j returns the bits of trsv_solve_device_async on column j (and
 * of tests/trsv_reference.c) whatever k, ld and chunk it sits in. The ordering between levels is that of the single solve: launch
 * boundaries, and workgroup barriers inside the one-workgroup launches. Nothing spins, nothing waits on another workgroup.
 *   - chunks. A global handle: k = 8s and then the binary remainder (k = 11: 8 + 2 + 1), each chunk the plan's launches once more.
 *     A blocked handle: the same with Kmax in the place of 8, Kmax being the largest KC in {8, 4, 2, 1} with min(block_rows, n) * KC
 *     values <= 160 KiB, since a workgroup keeps its rows of the chunk in LDS; each chunk is one launch. At block_rows = 16384 in fp64
 *     Kmax is 1 and k columns take k launches: served, not refused.
 *   - k = 1 with ldb = ldx = 1 is a vector: the call is handed to trsv_solve_device_async and costs what it costs. A single column
 *     of a wider block (ld > 1) runs the KC = 1 form of the k-column kernels.
 *   - rows of the blocks are read and written with one vector access where ld % KC == 0, the chunk's first column is a multiple of
 *     KC and the block's base is aligned to KC values, else value by value; the bits do not depend on it.
 *   - solve_multi_device_async: enqueued on hip_stream. b_dev == x_dev (in place) is legal when ldb == ldx; any other overlap is not.
 *     Only the k columns of the n rows of X are written: the ld - k padding columns of X are not touched, those of B are not read.
 *   - trsv_solve_multi: the blocking host form with ld = k; the two device blocks are allocated at the first call and replaced when
 *     a larger k arrives, which synchronises the device.
 *   - trsv_solve_multi_plan (host only, touches no device): matrix_passes = the number of chunks, launches = passes * the launches
 *     of trsv_info (so = passes for a blocked handle), max_chunk = Kmax of the handle (8 for a global one). All three are 0 at n = 0.
 *   - time_trsv_multi_device: HIP-event timing of `iters` back-to-back k-column solves.
 *   - rc 1 with the prefix "trsv_solve_multi:" ("trsv_solve_multi_plan:" for the plan, which makes the first two checks), on the
 *     host before any device is touched, in this order: 1. a NULL handle; 2. k < 1; 3. ldb < k or ldx < k; 4. b == x with
 *     ldb != ldx; 5. for n > 0 a NULL block. n = 0 is rc 0 with nothing launched.
 *   - NOT BUILT: a chunk width other than 8 / 4 / 2 / 1 (k = 3 is two passes), column-major blocks, T^t. */
int  spmv_mi355x_trsv_solve_multi_device_async(spmv_mi355x_trsv * T, int k, const void * b_dev, long ldb, void * x_dev, long ldx,
		void * hip_stream);
int  spmv_mi355x_trsv_solve_multi(spmv_mi355x_trsv * T, int k, const void * B_host, void * X_host);          /* blocking, ld = k */
int  spmv_mi355x_trsv_solve_multi_plan(const spmv_mi355x_trsv * T, int k, long * matrix_passes_out, long * launches_out,
		int * max_chunk_out);                                                                  /* any out pointer may be NULL */
int  spmv_mi355x_time_trsv_multi_device(spmv_mi355x_trsv * T, int k, const void * b_dev, long ldb, void * x_dev, long ldx, int iters,
		void * hip_stream, double * ms_per_iter_out);

/* JACOBI SWEEPS: T^-1 b approximated by a fixed number of sweeps, each ONE full-width launch (csrc/trsv.hip,
 * csrc/kernels_trsv_sweeps.hip). With T = D + N (D the diagonal, 1 under DIAG_UNIT):
 *     x(1) = D^-1 b,    x(m + 1) = D^-1 (b - N x(m)),    x = x(sweeps)
 * Every sweep is one launch over all n rows, one lane per row, over the arrays the handle already stores: no levels, no chains, no
 * ordering inside the launch, no new copy of the values, no new analysis. Any handle serves, global or blocked (a blocked handle
 * drops the entries that couple two blocks, as in its exact solve). A fixed sweep count is a fixed linear operator, so CG and GMRES
 * may be given it as a preconditioner.
 * PINNED TO THE BIT (tests/trsv_sweeps_reference.c): per row and sweep, s = b[i]; from the second sweep on, for each kept
 * off-diagonal entry (i, j, a) in stored order s = fma(-a, x(m)[j], s); x(m + 1)[i] = s / d_i (s under DIAG_UNIT), in the handle's
 * precision with an IEEE division. The first sweep reads no entry at all. This is the row expression of the exact solve, so a row
 * of level l holds the exact solve's bits from sweep l + 1 on, and sweeps >= levels returns THE BITS OF trsv_solve.
 * EFFECTIVE SWEEPS. Because of that the library runs min(sweeps, levels) sweeps, `levels` being the figure of trsv_info
 * (max_block_levels for a blocked handle; 0 at n = 0, where nothing is launched): a large sweep count is an exact solve in `levels`
 * full-width launches, and the work is bounded.
 *   - trsv_solve_sweeps_device_async(T, sweeps, b, x, stream): enqueued on hip_stream; b_dev == x_dev (in place) is legal. Only
 *     x[0 .. n) is written in the caller's memory, but x ALSO HOLDS INTERMEDIATE SWEEPS until the solve has finished; b is never
 *     modified (in place it is x). trsv_solve_sweeps is the blocking host form (the vectors of trsv_solve).
 *   - trsv_solve_sweeps_multi_device_async / trsv_solve_sweeps_multi: k columns of row-major blocks, the arguments and the rules of
 *     trsv_solve_multi (ld >= k, in place needs ldb == ldx, the ld - k padding columns are neither read nor written). Chunks of
 *     8, 4, 2, 1 columns (k = 11: 8 + 2 + 1) for EVERY handle, a blocked one included: no LDS bounds the chunk here. A chunk is
 *     `effective sweeps` launches; column j returns the bits of the single sweep solve on column j.
 *   - THE HANDLE OWNS ITS SCRATCH: a map of slices + 1 ints (the first position of every slice), built on the GPU at the handle's
 *     first sweep solve (that one call synchronises the stream), and, from the first solve of more than one sweep on, two n x KC
 *     blocks (KC = the widest chunk so far; replaced when a wider one arrives, which synchronises the device). None of it is
 *     allocated by create, none of it counts in trsv_mem_footprint(): trsv_sweeps_info reports it, the rule of the update_values
 *     maps. CONSEQUENCE: the sweep solves of ONE handle must not run on two streams at the same time.
 *   - trsv_set_sweeps(T, s), s > 0: from now on trsv_solve_device_async, trsv_solve, trsv_solve_multi_device_async,
 *     trsv_solve_multi, time_trsv_device and time_trsv_multi_device of THIS handle run s sweeps in the place of the exact plan
 *     (their refusals and prefixes stay theirs). That is how every solver that takes a spmv_mi355x_tri_precond (pcg_tri,
 *     pcg_trsm_multi, gmres_tri) uses sweeps with no change to the struct. s = 0 (the default) restores the exact plan. trsv_info,
 *     trsv_solve_multi_plan and trsv_mem_footprint keep describing the EXACT plan whatever the setting; a handle on which
 *     set_sweeps was never called behaves bit for bit and launch for launch as before. update_values needs nothing new.
 *   - SYMMETRY. The swept operator is p_s(T) = sum_{j < s} (-D^-1 N)^j D^-1 and p_s(T^t) = p_s(T)^t, so an SGS or IC(0) triple
 *     whose two handles run the SAME sweep count is a symmetric positive definite M^-1 for a positive diagonal. Unequal counts make
 *     M nonsymmetric and CG must not be given it; the library cannot check this. Jacobi sweeps on a factor that is far from
 *     diagonally dominant can GROW before the nilpotency bound ends them; this is not checked either.
 *   - trsv_sweeps_info(T, k, ...) (host only): the setting of set_sweeps, effective = min(setting, levels) (0 while the setting is 0),
 *     launches = effective * the number of chunks of k columns, bytes = the map and scratch allocated so far (0 before any sweep solve).
 *   - rc 1 on the host before any device is touched, prefix "trsv_solve_sweeps:", in this order: 1. a NULL handle; 2. sweeps
 *     outside 1 .. 1048576; then the checks of trsv_solve_multi: 3. k < 1; 4. ldb < k or ldx < k; 5. b == x with ldb != ldx; 6. for
 *     n > 0 a NULL vector (the single forms make 1, 2 and 6). "trsv_set_sweeps:": a NULL handle, sweeps outside 0 .. 1048576.
 *     "trsv_sweeps_info:": a NULL handle, k < 1. n = 0 is rc 0 with nothing launched and nothing written.
 *   - NOT BUILT: damped or weighted sweeps, a residual-based stop, asynchronous (chaotic) sweeps, fusing sweeps 1 and 2, skipping
 *     the rows that are already final, sweeps inside the AMG smoother. */
int  spmv_mi355x_trsv_solve_sweeps_device_async(spmv_mi355x_trsv * T, int sweeps, const void * b_dev, void * x_dev, void * hip_stream);
int  spmv_mi355x_trsv_solve_sweeps(spmv_mi355x_trsv * T, int sweeps, const void * b_host, void * x_host);       /* blocking */
int  spmv_mi355x_trsv_solve_sweeps_multi_device_async(spmv_mi355x_trsv * T, int sweeps, int k, const void * b_dev, long ldb,
		void * x_dev, long ldx, void * hip_stream);
int  spmv_mi355x_trsv_solve_sweeps_multi(spmv_mi355x_trsv * T, int sweeps, int k, const void * B_host, void * X_host);  /* blocking, ld = k */
int  spmv_mi355x_trsv_set_sweeps(spmv_mi355x_trsv * T, int sweeps /* 0 = exact (the default) */);
int  spmv_mi355x_trsv_sweeps_info(const spmv_mi355x_trsv * T, int k, int * sweeps_out, long * effective_out, long * launches_out,
		double * bytes_out);                                                                   /* any out pointer may be NULL */

/* UPDATE_VALUES: new numbers for the pattern a trsv handle was created with, scattered on the GPU. The rule of
 * spmv_mi355x_update_values: same pattern, new numbers, no rebuild, and the handle comes out BYTE FOR BYTE what trsv_create /
 * trsv_create_blocked builds from the new values: every stored value, the padding (never written: it keeps create's zeros) and the
 * diagonal, narrowed to the handle's precision by the conversion create makes (round to nearest even). Nothing that depends on the
 * pattern alone is redone: no analysis, no layout, no upload of the other eight arrays. What it is for: the Newton and time-stepping
 * loops in which ilu0_factor_device_async leaves a new f on the device: f goes into the two handles without a host copy.
 * THE ENTRY MAP (host, pattern only, once per handle). slot_src[e], one int32 per stored slot of the value array (slots of them,
 * padding included): the entry of the CALLER'S CSR that create puts in slot e, -1 for padding. Slice s of `lanes` positions stores
 * entry k of its lane r at slice_ptr[s] + k * lanes + r; a row's kept entries keep their stored order, duplicates are separate
 * entries, the other triangle, the diagonal and (blocked) the entries that leave the row's block never appear. diag_src[p], one
 * int32 per position under DIAG_STORED: the first stored entry of row perm[p] with column perm[p]. create and the map are ONE walk of
 * the pattern in the library (csrc/trsv.hip: trsv_layout), not two statements of the layout.
 *   - trsv_update_map: that derivation alone, no device touched and no handle needed, as trsv_analyze exposes the analysis.
 *     block_rows = -1 gives the global form (chain_rows is checked, it does not change the layout), 0 the default block size, 1 ..
 *     16384 that size. slot_src_out and diag_src_out are malloc'ed (at least one element; free with spmv_mi355x_free), diag_src_out
 *     receives NULL under DIAG_UNIT; any out pointer may be NULL. rc 1 with the prefix "trsv_update_map:" in trsv_create's order and
 *     with its messages: 1. scalars, 2. NULL pointers, 3. the pattern, 4. under DIAG_STORED a row without a diagonal entry or with two.
 *   - trsv_update_values_prepare(T, n, row_ptr, col_idx): once per handle; a second call does nothing. Derives the map from the CSR
 *     given, which must have the handle's pattern, uploads it and allocates one 16-byte status block and an event. The CSR fixes the
 *     ENTRY ORDER of every later values array. The bytes (4 per slot, 4 n under DIAG_STORED, 16) are not in trsv_mem_footprint(), the
 *     rule of the maps of spmv_mi355x_update_values_prepare; trsv_update_values_bytes() reports them (0 before prepare). n = 0 is legal.
 *     rc 1 with the prefix "trsv_update_values_prepare:", the handle untouched and its state still 1, in this order: 1. a NULL handle;
 *     2. a NULL row_ptr; 3. n other than the handle's; 4. a NULL col_idx when row_ptr[n] > 0; 5. the pattern checks of trsv_create
 *     and, under DIAG_STORED, a diagonal in every row, stored once; 6. the recomputed len, perm, slice_ptr and col against the handle's
 *     device arrays, downloaded once: the message names the lowest row whose place in the level order or whose count of kept entries
 *     differs, else a row of the first slice whose extent differs, else the lowest row whose kept columns differ; 7. the device.
 *   - trsv_update_values_device_async(T, values_dev, hip_stream): values_dev holds row_ptr[n] doubles in the order of the CSR given to
 *     prepare: ALL entries, both triangles, exactly the array spmv_mi355x_ilu0_values_device returns. Enqueues one 16-byte memset (the
 *     status word), under DIAG_STORED one check kernel, and one write kernel, then returns. The check kernel narrows every new
 *     diagonal and reports a zero or non-finite one by atomicMin of its ROW on the status word (ILU(0)'s breakdown idiom: the result
 *     does not depend on thread order, nothing spins); the write kernel reads the word first and writes NOTHING when it names a row,
 *     so a refused update leaves the previous values in place, bit for bit. A DIAG_UNIT handle has no check and cannot refuse.
 *     Ordering against solves of the same handle is the caller's job through the stream: an update and a solve of one handle are
 *     ordered when they are enqueued on the same stream (or on streams the caller has ordered), never otherwise; one update at a
 *     time per handle. values_dev must stay valid until the result has been taken.
 *   - trsv_update_values_result(T, &bad_row): waits for the last async update; rc 0 with bad_row = -1, or rc 1 with the LOWEST
 *     refused row and create's message: "trsv_update_values: the diagonal of row R is X in the handle's precision (from Y): it must
 *     be finite and non-zero" (the one offending double is copied back for it). Asked again, it answers the same.
 *   - trsv_update_values_device = async + result. trsv_update_values = the host form: uploads row_ptr[n] doubles into a staging buffer
 *     that is allocated at the first call and kept (as the vectors of trsv_solve are), then the same. trsv_update_values_staged
 *     returns that buffer (refused before the first host-form update; valid until destroy, overwritten by the next host-form update):
 *     a second handle of the same CSR, the other half of an SGS pair, updates from it without a second upload.
 *   - trsv_update_values_state (host only): 0 = cannot be updated (a NULL handle), 1 = prepare is missing, 2 = ready, 3 = the last
 *     update whose result was taken was refused and the handle holds the values from before it. A later accepted update gives 2.
 *   - trsv_stored_values (blocking, synchronises the device): the stored value array (slots values of the handle's precision, padding
 *     included) into val_host and the n diagonals by position into diag_host (ignored under DIAG_UNIT, may be NULL); slots_out
 *     receives slots. val_host = NULL only queries slots. Two handles with equal stored_values solve alike: the tests compare them.
 *   - rc 1 from the update entries with the prefix "trsv_update_values:", the handle untouched, checked on the host in this order:
 *     1. a NULL handle; 2. a NULL values array when row_ptr[n] > 0; 3. an update (or a result) before prepare; then the device.
 *     trsv_update_values_bytes(NULL) is 0. Every earlier entry behaves as before; a handle that never calls prepare allocates
 *     nothing more and solves exactly as before.
 *   - NOT CHECKABLE: that values_dev holds row_ptr[n] doubles on the handle's device, in the order of prepare's CSR.
 *   - NOT BUILT: GPU-side analysis (create still analyses on the host); update_values for FSAI; a pattern change (a new handle);
 *     the row-partitioned form. */
int  spmv_mi355x_trsv_update_map(int uplo, int diag, long n, const int32_t * row_ptr, const int32_t * col_idx, int chain_rows,
		long block_rows /* -1 = global */, int32_t ** slot_src_out /* malloc'ed, spmv_mi355x_free */, long * slots_out,
		int32_t ** diag_src_out /* malloc'ed; NULL under DIAG_UNIT */);
int  spmv_mi355x_trsv_update_values_prepare(spmv_mi355x_trsv * T, long n, const int32_t * row_ptr, const int32_t * col_idx);
double spmv_mi355x_trsv_update_values_bytes(const spmv_mi355x_trsv * T);
int  spmv_mi355x_trsv_update_values_state(const spmv_mi355x_trsv * T);
int  spmv_mi355x_trsv_update_values_device_async(spmv_mi355x_trsv * T, const double * values_fp64_dev, void * hip_stream);
int  spmv_mi355x_trsv_update_values_result(spmv_mi355x_trsv * T, long * bad_row_out /* may be NULL */);
int  spmv_mi355x_trsv_update_values_device(spmv_mi355x_trsv * T, const double * values_fp64_dev, void * hip_stream);   /* blocking */
int  spmv_mi355x_trsv_update_values(spmv_mi355x_trsv * T, const double * values_fp64_host);                             /* blocking */
int  spmv_mi355x_trsv_update_values_staged(spmv_mi355x_trsv * T, const double ** values_dev_out);
int  spmv_mi355x_trsv_stored_values(spmv_mi355x_trsv * T, void * val_host, long * slots_out, void * diag_host);         /* blocking */

/* ---- ILU(0): factorize A on the GPU for the triangular preconditioners ------------------------------------------------------------ */
/* The incomplete LU factorization of a square matrix on its own pattern, computed on the device, so that the strongest preconditioner
 * the triangular solves apply no longer has to come from the caller (csrc/ilu0.hip, csrc/kernels_ilu0.hip). The handle
 * is built from the PATTERN (create), takes numbers any number of times (factor: same pattern, new numbers, the rule of
 * spmv_mi355x_update_values) and returns ONE value array f in A's entry order: its strictly lower part is L (unit diagonal implied),
 * its diagonal and upper part is U. That array goes to two trsv handles, LOWER / UNIT and UPPER / STORED, with no scale in between:
 * the "caller's ILU(0)" row of spmv_mi355x_gmres_tri. For a symmetric positive definite A, U = D L^t, so M = L U is the M of IC(0)
 * and the same triple preconditions spmv_mi355x_pcg_tri and spmv_mi355x_pcg_trsm_multi: there is no Cholesky variant and nothing is
 * transposed.
 * THE FACTORIZATION, PINNED TO THE BIT. Input: int32 CSR, n x n, columns strictly ascending in every row, a stored diagonal in every
 * row, fp64 values. The factorization is always fp64 (the trsv handles narrow f as they narrow any values). f = a copy of the values;
 *     for i = 0 .. n-1
 *       for each entry p of row i with column k < i, ascending k
 *           f[p] = f[p] / f[diag(k)]                                        (an IEEE division)
 *           for each entry q of row k with column j > k
 *               if row i stores column j at r:   f[r] = fma(-f[p], f[q], f[r])
 * Every f[r] receives its fmas in ascending k and no two entries q of one k step touch the same r, so the result does not depend on
 * how the j loop or the rows of a level are spread over lanes: every plan gives the bits of the sequential loop
 * (tests/ilu0_reference.c), run after run. A pivot f[diag(i)] that is zero or not finite once row i is finished is a BREAKDOWN: the
 * arithmetic goes on as IEEE gives it, the lowest such row is reported by get_info (breakdown_row, -1: none), nothing spins and
 * nothing is refused at factor time. trsv_create then refuses the bad diagonal, naming the row.
 * THE BLOCKED FORM (block_rows >= 0): the same loop on the CSR without the off-diagonal entries that couple two blocks of B =
 * block_rows rows, block b owning the rows [b B, min(n, (b + 1) B)). Dropped entries keep A's value in f; blocked trsv handles with
 * the same B ignore them anyway. block_rows: -1 = global, 0 = the trsv default (4096), 1 .. 16384.
 * THE SCHEDULE. Row i needs the finished rows k of every stored k < i of row i: the level rule of trsv_analyze(LOWER) on A's pattern,
 * and the levels come from that routine (trsv_analyze_blocked for the blocked form, where the level WITHIN the block is the launch
 * index, so all blocks share max_block_levels launches). Level 0 has no k step and gets no launch: launches = levels - 1 (0 when
 * n = 0). Every factor call also enqueues one 16-byte memset (the breakdown word) and one copy kernel (f = values, and the pivots of
 * level 0) ahead of them. The order of the launches on the stream is the only ordering between levels: no flag, no grid barrier, no
 * persistent kernel. Inside a level the rows are independent; a row belongs to a group of 4 .. 64 lanes (chosen per level on its mean
 * row width, as csr_vector chooses) that walks the row's k steps in order, strides over row k's entries beyond the diagonal and finds
 * column j in row i by binary search. Step k writes what step k' > k reads through other lanes: a workgroup barrier after every step
 * orders them, and a group never leaves its workgroup.
 *   - create() is pattern only and deep-copies it. Stored: A's columns, per row the positions of its first kept entry, its diagonal
 *     and its end, the rows sorted by (level, row) (level pointers on the host), f, and the breakdown word; 12 nnz + 16 n + 16 bytes,
 *     which is ilu0_mem_footprint().
 *   - factor (blocking, host values) and factor_device_async (device values, enqueued on hip_stream, returns at once) may be called
 *     any number of times; each overwrites f. values_dev may be the handle's own f. One factorization at a time per handle.
 *   - ilu0_values copies f to the host (nnz doubles) after a device synchronise; ilu0_values_device returns the device pointer, valid
 *     until destroy and overwritten by the next factor. Both are refused before the first factor.
 *   - get_info reads the breakdown word and therefore synchronises the device. levels / launches as above; max_level_rows = the most
 *     rows of one launch (for a blocked handle: of one level over all blocks); nnz_dropped = the entries of A, of both triangles,
 *     whose column lies outside the row's block (0 for a global handle); block_rows = B used and blocks = ceil(n / B), both 0 for a
 *     global handle; factorizations = the factor calls so far. info->struct_size in: sizeof; out: the bytes written.
 *   - rc 1 with the prefix "ilu0_create:" / "ilu0_factor:" / "ilu0_values:" / "ilu0_get_info:", everything but the last on the host
 *     before any device is touched, in this order:
 *     1. scalars: n < 0 (or beyond the int32 range), block_rows outside -1 .. 16384; for get_info an unset info->struct_size;
 *     2. NULL pointers: out, row_ptr; col_idx when row_ptr[n] > 0; the handle; values for nnz > 0;
 *     3. the pattern, as spmv_mi355x_trsv_create checks it and with its messages: row_ptr from 0 and monotone, columns in [0, n);
 *     4. a row whose columns are not strictly ascending (the lowest such row and its first offending column are named);
 *     5. a row without a stored diagonal (the lowest such row is named);
 *     6. the device: without a usable one the library's "no HIP device available" message; `device` out of range.
 *     n = 0 is rc 0 with nothing launched; ilu0_destroy(NULL) is rc 0; ilu0_mem_footprint(NULL) is 0.
 *   - NOT CHECKABLE: that values_dev holds nnz doubles on the handle's device; that the values are those of the pattern given to create.
 *   - NOT BUILT: IC(0) with a square-root diagonal (the same M for symmetric positive definite input); MILU and shifted variants;
 *     ILU(k) / ILUT; pivoting; GPU-side analysis; the row-partitioned form (a refactorization no longer rebuilds the two trsv
 *     handles: spmv_mi355x_trsv_update_values_device_async takes f where ilu0_values_device leaves it); running a run of thin levels as one workgroup chain, as the solve
 *     does (every level is its own launch). */
typedef struct spmv_mi355x_ilu0 spmv_mi355x_ilu0;   /* opaque */
typedef struct {
	size_t struct_size;           /* in: sizeof(spmv_mi355x_ilu0_info); out: the bytes written */
	long n, nnz, nnz_dropped, levels, launches, max_level_rows, block_rows, blocks;
	long breakdown_row;           /* -1: none */
	long factorizations;
} spmv_mi355x_ilu0_info;
int  spmv_mi355x_ilu0_create(spmv_mi355x_ilu0 ** out, long n, const int32_t * row_ptr, const int32_t * col_idx,
		long block_rows /* -1 = global, 0 = default (the trsv default), 1 .. 16384 */, int device /* -1 = current */);
int  spmv_mi355x_ilu0_factor(spmv_mi355x_ilu0 * F, const double * values_host);                 /* blocking */
int  spmv_mi355x_ilu0_factor_device_async(spmv_mi355x_ilu0 * F, const double * values_dev, void * hip_stream);
int  spmv_mi355x_ilu0_values(spmv_mi355x_ilu0 * F, double * out_host /* nnz, A's entry order */); /* blocking */
int  spmv_mi355x_ilu0_values_device(spmv_mi355x_ilu0 * F, const double ** f_dev_out);
int  spmv_mi355x_ilu0_get_info(spmv_mi355x_ilu0 * F, spmv_mi355x_ilu0_info * info);             /* reads the breakdown word: synchronises */
double spmv_mi355x_ilu0_mem_footprint(const spmv_mi355x_ilu0 * F);
int  spmv_mi355x_ilu0_destroy(spmv_mi355x_ilu0 * F);

/* ---- multicolour ordering: colour, permute, SGS / ILU(0) in as many launches as colours -------------------------------------------- */
/* An exact global triangular solve, and the ILU(0) factorization, cost one launch per LEVEL of the triangle, and the natural ordering
 * of a grid or a stencil has hundreds to thousands of levels. Under a multicolouring every row of colour c depends only on rows of
 * lower colours, so the matrix B = P A P^t, whose rows are sorted by colour, has as many levels as colours: a handful, whatever n is.
 * This handle colours the graph of a square CSR pattern on the GPU, derives the permutation, forms B with an entry map, and moves
 * vectors and value arrays between the two orderings (csrc/color.hip, csrc/kernels_color.hip, csrc/color.hpp).
 * Everything downstream is the existing API applied to B: trsv_create, ilu0_create, the preconditioner triples of pcg_tri,
 * pcg_trsm_multi and gmres_tri, update_values. No solver changes. The solve of A x = b becomes B (P x) = P b.
 * THE GRAPH. The vertices are the rows; i and j (i != j) are adjacent when a_ij OR a_ji is stored (a Gauss-Seidel or ILU ordering
 * needs both directions: the pattern of A^t comes from the device transposition of "transposed handles"). Stored zeros count;
 * duplicates and a missing diagonal are harmless; the columns of a row need not be sorted.
 * THE COLOURING, PINNED. key(i) = ((uint64) (h >> 1) << 31) | i with h = (uint32) (i * 0x9E3779B1u), the keys of the AMG's
 * independent set. Rounds are synchronous (each reads one colour array and writes another): an uncoloured vertex whose key exceeds
 * the key of every UNCOLOURED neighbour takes the smallest colour >= 0 that none of its coloured neighbours holds. A neighbour of
 * lower key is never coloured first, so the result EQUALS first-fit greedy colouring in descending key order
 * (tests/color_reference.c), run after run, and every vertex of colour c > 0 has a neighbour of every colour below c. The rounds
 * needed are the longest chain of ascending keys + 1: 6 on a 5-point grid, about 20 on a 27-point stencil, m ON A CLIQUE OF m ROWS.
 * The host reads one counter per round; 4096 rounds are refused with a message. Nothing spins and nothing is ordered between
 * workgroups except by the launch boundary. One lane per row; the smallest free colour is searched in windows of 64 colours (a
 * 64-bit mask), so no row is refused for its width or its colour count.
 * THE PERMUTATION. perm[p] = the old row at new position p, sorted by (colour, old row) (a stable radix sort on the device);
 * rank = its inverse; color_ptr[c] .. color_ptr[c + 1] are the positions of colour c (num_colors + 1 entries).
 * THE PERMUTED MATRIX. B(p, q) = A(perm[p], perm[q]): row p of B holds the entries of row perm[p] of A with columns rank[j], in
 * ASCENDING NEW COLUMN order, equal columns in their stored order (so a sorted A with a diagonal gives a B that ilu0_create takes).
 * entry_map[e_B] = e_A, int32, nnz entries; values_B = values_A[entry_map] is one gather.
 *   - create is pattern only and blocking; it deep-copies the pattern to the device. The colours, perm, rank and color_ptr are kept on
 *     the host for the getters and perm / rank on the device for the vector kernels.
 *   - permute_csr (host outputs, blocking; values_host may be NULL, then values_out is not written) and permute_csr_device (device
 *     pointers the handle owns, valid until destroy) form B's pattern and the map at their first call, on the device, by two stable
 *     transpositions of the relabelled pattern; A's own pattern is dropped then. Later calls copy.
 *   - permute_values_device_async is the gather alone, enqueued on hip_stream (after a first call that formed B; the first call
 *     synchronises). Its output is what spmv_mi355x_update_values_device of a handle of B, spmv_mi355x_ilu0_factor_device_async and
 *     spmv_mi355x_trsv_update_values_device_async take: a Newton loop refreshes the whole permuted preconditioner on one stream
 *     without the host. permute_values is its blocking host form.
 *   - permute_vectors_device_async: direction SPMV_MI355X_COLOR_FORWARD out[p] = in[perm[p]], SPMV_MI355X_COLOR_BACKWARD out[i] =
 *     in[rank[i]] (the inverse), for the k columns of row-major n x k blocks (row i at ptr + i * ld), one launch per chunk of 8 / 4 /
 *     2 / 1 columns; precision 0 = fp64, 1 = fp32 (the handle has none of its own). permute_vectors is the blocking host form; what
 *     lies between k and ld in out stays as it was.
 *   - info->struct_size in: sizeof; out: the bytes written. symmetric = 1 when row_ptr and col_idx of A^t equal A's array for array
 *     (then one walk per row serves; a symmetric pattern with unsorted rows or duplicates may report 0 and is walked twice, with the
 *     same result); max_class / min_class = the most and fewest rows of one colour; the seconds of the transposition (with the
 *     comparison), of the rounds, of the sort (with the downloads) and of forming B (0 before the first permute call).
 *   - mem_footprint: the pattern (4 (n + 1) + 4 nnz) and perm and rank (8 n); 4 nnz more once B and the map are formed.
 *   - rc 1 with the prefix "color_create:" / "color_info:" / "color_permute_csr:" / "color_permute_values:" /
 *     "color_permute_vectors:", in this order, 1 to 3 on the host before any device is touched:
 *     1. scalars: n < 0 (or beyond the int32 range); for permute_vectors direction, precision, then k < 1 or ld < k; for info an
 *        unset struct_size;
 *     2. NULL pointers: out, row_ptr; col_idx when row_ptr[n] > 0; the handle; the arrays of a call when n (nnz) > 0;
 *     3. the pattern, as spmv_mi355x_trsv_create checks it and with its messages: row_ptr from 0 and monotone, columns in [0, n);
 *        then n + nnz beyond the int32 range (the transposition's limit);
 *     4. in == out of permute_vectors and of permute_values (neither can run in place);
 *     5. the device: without a usable one the library's "no HIP device available" message; `device` out of range;
 *     6. more than 4096 rounds.
 *     n = 0 is rc 0 with nothing launched (0 colours, color_ptr = {0}); color_destroy(NULL) is rc 0; color_mem_footprint(NULL) is 0.
 *   - NOT CHECKABLE: that device pointers hold what the call says on the handle's device; that in and out of a device call do not
 *     overlap in part; that the values are those of the pattern given to create.
 *   - NOT BUILT: distance-2 colouring; balancing the colour classes; fewer colours than greedy gives (greedy finds 5 on the 5-point
 *     grid, where 2 exist); a multicolour smoother inside the AMG cycle; applying P^t M^-1 P around an unpermuted A (the caller
 *     permutes b and x once per solve instead); the blocked and the row-partitioned forms. */
typedef struct spmv_mi355x_color spmv_mi355x_color;   /* opaque */
enum { SPMV_MI355X_COLOR_FORWARD = 0, SPMV_MI355X_COLOR_BACKWARD = 1 };
typedef struct {
	size_t struct_size;           /* in: sizeof(spmv_mi355x_color_stats); out: the bytes written */
	long n, nnz, symmetric, num_colors, rounds, max_class, min_class;
	double transpose_seconds, round_seconds, sort_seconds, permute_seconds;
} spmv_mi355x_color_stats;
int  spmv_mi355x_color_create(spmv_mi355x_color ** out, long n, const int32_t * row_ptr, const int32_t * col_idx, int device /* -1 = current */);
int  spmv_mi355x_color_destroy(spmv_mi355x_color * C);
int  spmv_mi355x_color_info(const spmv_mi355x_color * C, spmv_mi355x_color_stats * stats);
int  spmv_mi355x_color_colors(const spmv_mi355x_color * C, int32_t * colors_host /* n */);
int  spmv_mi355x_color_perm(const spmv_mi355x_color * C, int32_t * perm_host /* n, may be NULL */, int32_t * rank_host /* n, may be NULL */);
int  spmv_mi355x_color_color_ptr(const spmv_mi355x_color * C, int32_t * color_ptr_host /* num_colors + 1 */);
double spmv_mi355x_color_mem_footprint(const spmv_mi355x_color * C);
int  spmv_mi355x_color_permute_csr(spmv_mi355x_color * C, const double * values_host /* nnz, may be NULL */, int32_t * row_ptr_out /* n + 1 */,
		int32_t * col_idx_out /* nnz */, double * values_out /* nnz, with values_host */, int32_t * entry_map_out /* nnz */);   /* blocking */
int  spmv_mi355x_color_permute_csr_device(spmv_mi355x_color * C, const int32_t ** row_ptr_dev_out, const int32_t ** col_idx_dev_out,
		const int32_t ** entry_map_dev_out);
int  spmv_mi355x_color_permute_values(spmv_mi355x_color * C, const double * values_host, double * values_out_host);      /* blocking */
int  spmv_mi355x_color_permute_values_device_async(spmv_mi355x_color * C, const double * values_dev, double * values_out_dev, void * hip_stream);
int  spmv_mi355x_color_permute_vectors(spmv_mi355x_color * C, int direction, int precision, int k, const void * in_host, long ldin,
		void * out_host, long ldout);                                                                                 /* blocking */
int  spmv_mi355x_color_permute_vectors_device_async(spmv_mi355x_color * C, int direction, int precision, int k, const void * in_dev, long ldin,
		void * out_dev, long ldout, void * hip_stream);

/* ---- GMRES(m) right-preconditioned by triangular solves ------------------------------------------------------------------------ */
/* spmv_mi355x_gmres with M^-1 v = second^-1 ( scale o ( first^-1 v ) ) for "M v" (csrc/solver_gmres.hip): each of
 * the three parts may be NULL, the two solves are spmv_mi355x_trsv handles of any kind, blocked or global, and scale is a vector.
 * The recurrences, the stop codes, the freeze, history and info are exactly those of spmv_mi355x_gmres. Two ways to fill it:
 *     SGS of A:               first = LOWER / STORED handle of A's CSR, scale = diag(A), second = UPPER / STORED handle of A's CSR
 *     the caller's ILU(0):    first = LOWER / UNIT, second = UPPER / STORED, no scale (spmv_mi355x_ilu0 above computes the factor)
 *   - per inner step: the launches of the two solves and one scale kernel on top of spmv_mi355x_gmres's; one scratch vector.
 *   - scale_host: rows() values of the handle's precision. M = (NULL, s, NULL) with s > 0 returns bit for bit what
 *     spmv_mi355x_gmres returns with minv = s.
 *   - the handles are used, not owned: they must outlive the call, and one handle serves one solve at a time.
 *   - rc 1 with a last_error that names gmres_tri, caller buffers and info untouched: first the checks of spmv_mi355x_gmres in its
 *     order (info->struct_size, restart, tol, max_iterations; NULL A, b or x_out; rows() != cols()), then
 *     1. M is NULL or M->struct_size < sizeof(spmv_mi355x_tri_precond);
 *     2. first, scale_host and second are all NULL (the message points to spmv_mi355x_gmres);
 *     3. a handle's n differs from rows(), or its precision or its device from A's (first before second);
 *     4. a scale entry that is not finite or is zero (the message names the first such index).
 *   - NOT BUILT: the same for pbicgstab / minres (CG has it: spmv_mi355x_pcg_tri below), left preconditioning, a preconditioner
 *     that changes between steps. */
typedef struct {
	unsigned struct_size;         /* in: sizeof(spmv_mi355x_tri_precond) */
	spmv_mi355x_trsv * first;     /* may be NULL */
	const void * scale_host;      /* may be NULL: rows() values of the handle's precision, finite and non-zero */
	spmv_mi355x_trsv * second;    /* may be NULL */
} spmv_mi355x_tri_precond;
int  spmv_mi355x_gmres_tri(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, int restart,
		const spmv_mi355x_tri_precond * M, double tol, long max_iterations,
		double * history_out /* may be NULL: max_iterations doubles */, spmv_mi355x_gmres_info * info /* may be NULL */);

/* ---- CG preconditioned by triangular solves (SGS / IC(0)), tol-based ------------------------------------------------------------- */
/* A x = b from x0 = 0 for a square SYMMETRIC POSITIVE DEFINITE matrix by preconditioned conjugate gradients, the CG member of the
 * tol-based family (cgls, minres, gmres: `tol`, stop codes, explicit norms in info, frozen on the device at the stop, any handle),
 * with M^-1 v = second^-1 ( scale o ( first^-1 v ) ) given as the spmv_mi355x_tri_precond that spmv_mi355x_gmres_tri takes: each of
 * the three parts may be NULL, the two solves are spmv_mi355x_trsv handles of any kind, blocked or global, and scale is a vector
 * (csrc/solver_pcg_tri.hip). M == NULL, or a struct with three NULL parts, means z = r: no z vector is stored, no
 * extra launch is issued and r.z is r.r, the plain CG. spmv_mi355x_pcg (above) is another solver: the reference harness's
 * preconditioned_cg() to the letter, Jacobi only, no tol. The recurrences, every scalar and every dot fp64, vectors in the handle's
 * precision:
 *     x = 0; r = b; rnorm0 = |b|                     (0: stop 3, x = 0, every norm 0; not finite: stop 4)
 *     z = M^-1 r; p = z; rz = r.z                    (not finite or <= 0: stop 4, 0 iterations, x = 0)
 *     loop k = 1, 2, ... while k <= max_iterations:
 *         q = A p; pq = p.q                          (not finite or <= 0: stop 4; x, iterations, history as before this body)
 *         alpha = rz / pq; x += alpha p; r -= alpha q; rr = r.r; history[k-1] = sqrt(rr); iterations = k
 *         if tol > 0 and sqrt(rr) <= tol rnorm0: stop 1;  else if rr == 0: stop 5
 *         z = M^-1 r; rz' = r.z                      (not finite or <= 0: stop 4; this body's x is kept)
 *         beta = rz' / rz; rz = rz'; p = z + beta p
 * Two ways to fill M:
 *     SGS of an SPD A:        first = LOWER / STORED handle of A's CSR, scale = diag(A), second = UPPER / STORED handle of A's CSR
 *     the caller's IC(0):     first = LOWER / STORED handle of L, no scale, second = UPPER / STORED handle of the CSR of L^t
 *     spmv_mi355x_ilu0's f:   first = LOWER / UNIT, second = UPPER / STORED, both over f, no scale (IC(0)'s M for an SPD A)
 *   - per iteration: 1 SpMV, the launches of the two solves and at most one scale kernel, and 4 vector kernels (3 without M).
 *   - b_host, x_out_host and M->scale_host: rows() values of the handle's precision.
 *   - any format and layout serves (the solver only calls spmv_mi355x_spmv_device_async): value_storage = 1, 7-byte values and
 *     symmetric_input = 1 included; on handles whose SpMV is deterministic the whole solve is, bit for bit. The solver's vectors
 *     are plain allocations. M = (NULL, ones, NULL) returns the bits of M = NULL.
 *   - the handles of M are used, not owned: they must outlive the call, and one handle serves one solve at a time.
 *   - tol == 0 is legal and means "never stop on the tolerance". max_iterations == 0 returns x = 0, stop 2 and rnorm = rnorm0.
 *   - history_out (may be NULL): max_iterations doubles; entry k = |r| of the recurrence after body k + 1; entries >=
 *     info->iterations stay 0.
 *   - after a stop the solve is frozen on the device: x, iterations and the history are those of the body at which the rule fired,
 *     however far the host had run ahead (at most 64 bodies).
 *   - rc 1 with a last_error that names pcg_tri, caller buffers and info untouched, in this order, the first three before any
 *     device is touched and before the NULL checks:
 *     1. info->struct_size < 8;
 *     2. tol negative or not finite;
 *     3. max_iterations < 0;
 *     4. A, b or x_out is NULL;
 *     5. rows() != cols() (the message gives both; this also refuses row-block handles);
 *     6. M is not NULL and M->struct_size < sizeof(spmv_mi355x_tri_precond);
 *     7. a handle's n differs from rows(), or its precision or its device from A's (first before second);
 *     8. a scale entry that is not finite or is zero (the message names the first such index). A negative one is legal and ends
 *        in stop 4.
 *   - NOT CHECKABLE: that A and M are symmetric positive definite. Blocked handles give a symmetric M only when both use the same
 *     block_rows (a global handle counts as block_rows >= n). Stop 4 catches only what the two inner products reveal.
 *   - NOT BUILT: the row-partitioned form, device-pointer b / x, a non-zero x0 (k right-hand sides with any M:
 *     spmv_mi355x_pcg_trsm_multi below). */
typedef struct {
	unsigned struct_size;   /* in: sizeof(spmv_mi355x_pcg_tri_info) */
	long   iterations;      /* completed loop bodies */
	int    stop;            /* 1 = |r| <= tol * |b| (tol > 0)
	                           2 = max_iterations reached
	                           3 = b == 0: x = 0, 0 iterations
	                           4 = breakdown: |b|, r.z or p.q not finite, or r.z or p.q <= 0
	                           5 = r == 0 exactly */
	double rnorm;           /* |b - A x_out|, EXPLICIT (one SpMV after the loop) */
	double rnorm0;          /* |b| */
	double prnorm;          /* |r| of the recurrence at the stop */
	double xnorm;           /* |x_out| */
	long   spmv_calls;      /* every launch, the host's run-ahead and the explicit one included */
	double seconds;
} spmv_mi355x_pcg_tri_info;
int  spmv_mi355x_pcg_tri(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host,
		const spmv_mi355x_tri_precond * M /* may be NULL */, double tol, long max_iterations,
		double * history_out /* may be NULL: max_iterations doubles */, spmv_mi355x_pcg_tri_info * info /* may be NULL */);

/* ---- FSAI: a factorized sparse approximate inverse built on the GPU, applied as two SpMVs ---------------------------------------- */
/* For a square SYMMETRIC POSITIVE DEFINITE A and a lower triangular pattern P the handle holds the sparse lower triangular G on P with
 * G A G^t ~ I and diag(G A G^t) = 1 (Kolotilina-Yeremin), and applies M^-1 v = G^t (G v): two SpMVs over two ordinary handles, G built
 * by spmv_mi355x_create and G^t by the same call with opts.transpose = 1. No triangular solve, no level schedule, no ordering between
 * workgroups (csrc/fsai.hip, csrc/kernels_fsai.hip). Rows of G do not depend on each other.
 * THE ARITHMETIC, fp64 whatever the handle's precision. Of A only the entries with column <= row are read. For row i with pattern
 * columns J = (j_1 < ... < j_s = i):
 *     gather   S[a][b] = A(j_a, j_b) for b <= a, taken from row j_a of A at column j_b; an absent entry is 0, a stored 0 is a 0
 *     Cholesky for k = 1..s, for a = k..s:  for p = 1..k-1 ascending  S[a][k] = fma(-C[a][p], C[k][p], S[a][k]);
 *                                           then C[k][k] = sqrt(S[k][k]) and C[a][k] = S[a][k] / C[k][k] (IEEE division)
 *     solve    C^t g = e_s:  g_s = 1 / C[s][s];  for k = s-1..1:  t = 0; for a = k+1..s ascending t = fma(C[a][k], g_a, t);
 *                                                                 g_k = -t / C[k][k]
 * Row i of G is g on the columns J (the textbook g^ / sqrt(g^_s) with S g^ = e_s). Every S[a][k] has its own sequential chain, so
 * the bits do not depend on how lanes are mapped to elements: tests/fsai_reference.c is the same arithmetic as one loop.
 * BREAKDOWN: a pivot S[k][k] that is <= 0 or not finite. The whole row then becomes g_i = 1 / sqrt(A(i, i)) with an explicit 0 in every
 * other entry, and the row is counted in fallback_rows. Nothing aborts.
 *   - the pattern: pat_row_ptr / pat_col_idx, a CSR whose rows hold strictly ascending columns, all <= the row, the last one the row
 *     itself, at most SPMV_MI355X_FSAI_MAX_ROW entries each (the packed triangle of a row lives in LDS: 66 KiB at 128). Both NULL =
 *     the lower triangle of A's own pattern, each row sorted by the library. spmv_mi355x_fsai_pattern (host only, O(work) with a
 *     marker array) returns the pattern of tril(A~)^power for power 1..3, A~ = the pattern of A's lower triangle with the diagonal
 *     added: columns ascending, arrays malloc'ed, released with spmv_mi355x_free. It refuses n out of range, power outside 1..3, NULL
 *     arrays and a bad CSR (create's checks), with the prefix fsai_pattern.
 *   - stored: G's fp64 values on the host in the pattern's entry order (spmv_mi355x_fsai_values), the two handles (values narrowed as
 *     create narrows them; format and opts are the caller's, for both) and one scratch vector of n values for G v.
 *     spmv_mi355x_fsai_matrices lends the two handles: they belong to F and die with it (both NULL when n == 0).
 *   - fsai_apply_device_async: out = G^t (G in) enqueued on the stream; in == out is legal (G in is in the scratch vector before out is
 *     written). One apply at a time per handle. fsai_apply is the blocking form on host vectors of the handle's precision.
 *   - fsai_info: n, nnz of the pattern, max_row = its longest row, fallback_rows, the seconds of the row kernel and of the whole
 *     setup; fsai_setup_split: the kernel, the download of G and the two creates, in seconds. Any out pointer may be NULL.
 *   - n == 0 is legal everywhere: no handle is built, apply does nothing.
 *   - rc 1 with a last_error that starts with "fsai_create:", in this order, all but the last on the host before any device is touched:
 *     1. the scalars: an unknown precision or format, n < 0 or n >= 2^31 - 1, opts->struct_size not set, and opts that set transpose,
 *        symmetric_input or a row block / column filter (row_begin, row_end, col_filter_mode); opts->value_storage under create's rule;
 *     2. NULL pointers: out, row_ptr, col_idx or values of a matrix with entries, a pattern given as one array of the two;
 *     3. A's pattern, as create checks it: row_ptr from 0 and monotone, columns in [0, n);
 *     4. a column stored twice in one row of A's lower triangle (which value A(i, j) has would not be defined);
 *     5. the pattern: pat_row_ptr from 0 and monotone, columns in [0, row], strictly ascending, the last column equal to the row,
 *        and a row with more than SPMV_MI355X_FSAI_MAX_ROW entries (the message gives the row and its count);
 *     6. the diagonal of A: the first stored entry with column i must exist, be finite and be > 0 (the message names the first bad row);
 *     7. the device, and whatever spmv_mi355x_create refuses for the format and opts (its message after the prefix).
 *   - NOT CHECKABLE: that A is symmetric and positive definite. Only the lower triangle is read; an indefinite A shows, if at all, as
 *     fallback_rows > 0.
 *   - NOT BUILT: update_values for an fsai handle (new values of A need a new handle), gmres / minres / pbicgstab wiring,
 *     the row-partitioned form, adaptive patterns, a pattern with entries above the diagonal.
 * spmv_mi355x_pcg_fsai is spmv_mi355x_pcg_tri with z = M^-1 r = fsai_apply_device_async: the same recurrences, kernels, stop codes,
 * history, spmv_mi355x_pcg_tri_info and freeze (the two SpMVs of an apply write only F's scratch vector and z, scratch that only the
 * predicated kernels read). info.spmv_calls counts the products with A, not those with G and G^t. Per iteration: 3 SpMVs and 4
 * vector kernels. rc 1 with a last_error that starts with "pcg_fsai:": first items 1 to 5 of spmv_mi355x_pcg_tri, then F == NULL (the
 * message points to spmv_mi355x_pcg_tri), then F's n, precision or device differing from A's, in that order. */
#define SPMV_MI355X_FSAI_MAX_ROW 128
typedef struct spmv_mi355x_fsai spmv_mi355x_fsai;   /* opaque */
int  spmv_mi355x_fsai_pattern(long n, const int32_t * row_ptr, const int32_t * col_idx, int power,
		int32_t ** row_ptr_out, int32_t ** col_idx_out /* malloc'ed; spmv_mi355x_free */);
int  spmv_mi355x_fsai_create(spmv_mi355x_fsai ** out, int format, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const int32_t * pat_row_ptr, const int32_t * pat_col_idx /* both NULL = tril(A) */, const spmv_mi355x_opts * opts /* may be NULL */);
int  spmv_mi355x_fsai_destroy(spmv_mi355x_fsai * F);
int  spmv_mi355x_fsai_apply_device_async(spmv_mi355x_fsai * F, const void * in_dev, void * out_dev, void * hip_stream);
int  spmv_mi355x_fsai_apply(spmv_mi355x_fsai * F, const void * in_host, void * out_host);       /* blocking */
int  spmv_mi355x_fsai_values(const spmv_mi355x_fsai * F, double * out /* nnz doubles, pattern order */);
int  spmv_mi355x_fsai_matrices(const spmv_mi355x_fsai * F, spmv_mi355x_matrix ** G_out, spmv_mi355x_matrix ** Gt_out);   /* borrowed */
int  spmv_mi355x_fsai_info(const spmv_mi355x_fsai * F, long * n_out, long * nnz_out, long * max_row_out, long * fallback_rows_out,
		double * kernel_seconds_out, double * setup_seconds_out);                                /* any out pointer may be NULL */
int  spmv_mi355x_fsai_setup_split(const spmv_mi355x_fsai * F, double * kernel_seconds_out, double * download_seconds_out,
		double * create_g_seconds_out, double * create_gt_seconds_out);                          /* any out pointer may be NULL */
double spmv_mi355x_fsai_mem_footprint(const spmv_mi355x_fsai * F);    /* the two handles and the scratch vector, bytes */
int  spmv_mi355x_pcg_fsai(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, spmv_mi355x_fsai * F, double tol,
		long max_iterations, double * history_out /* may be NULL: max_iterations doubles */,
		spmv_mi355x_pcg_tri_info * info /* may be NULL */);

/* ---- SpGEMM: C = A B on the GPU, the pattern once, the values per value set ---------------------------------------------------- */
/* C = A B for A m x k and B k x n, both int32 CSR with fp64 values. A plan finds the pattern of C once (spgemm_create, "symbolic")
 * and recomputes C's values for every new set of A's and B's values on the same patterns (spgemm_multiply, "numeric"): update_values'
 * rule, same pattern, new numbers, no rebuild. The values come out in the entry order of C's CSR, so they are what
 * spmv_mi355x_update_values_device of a handle of C takes. Row-wise (Gustavson) with a hash table per row of C, in LDS where it fits
 * and in a per-workgroup slab of global memory where it does not (csrc/spgemm.hip, csrc/kernels_spgemm.hip).
 * THE PATTERN. Column j is stored in row i of C exactly when some stored A(i, l) meets a stored B(l, j). Stored zeros and numerical
 * cancellation do not remove an entry. Columns ascend within a row; c_row_ptr[0] = 0.
 * THE VALUES. acc = +0.0 for every entry of row i; then for the entries p of row i of A in STORED order, for every entry q of B's
 * row col(p):  acc[col(q)] = fma(a_p, b_q, acc[col(q)]). Each C(i, j) is one fma chain in the order of A's entries, so the product is
 * deterministic and bit-identical to that loop run sequentially (tests/spgemm_reference.c), whatever lane takes which entry.
 * THE INPUTS. A's rows may be unsorted and may hold a column twice: both occurrences are steps of the chain. B's rows may be unsorted
 * but must not hold a column twice (the products of one step must land on distinct entries): such a B is refused at create.
 * LIMITS. m, k, n < 2^31 - 1 and nnz(C) < 2^31. No cap on the width of a row; empty rows and empty matrices are legal.
 *   - spgemm_create(device = -1: the current one): the plan keeps A's, B's and C's patterns on the device, the numeric bins' row lists
 *     and, if C has rows wider than 2048, the slab of their tables. The values never stay: spgemm_multiply stages them for the call.
 *   - spgemm_pattern: c_row_ptr (m + 1) and c_col_idx (nnz_c, from spgemm_info) into the caller's arrays.
 *   - spgemm_multiply: host arrays, blocking. spgemm_multiply_device_async: device arrays of nnz_a, nnz_b and nnz_c doubles, enqueued
 *     on the stream; one multiply at a time per plan. Where C has no entries both return at once and touch no pointer (NULL is legal).
 *   - spgemm_info: struct_size is set by the caller, at most that many bytes are written. products = the sum over A's entries of the
 *     length of the row of B they meet; max_row_products and max_row_c = the largest per row; the rows per bin of csrc/spgemm.hpp on
 *     min(products, n) (symbolic_bin_rows: the counting pass) and on C's true width (numeric_bin_rows: the pass that writes the
 *     columns, and the numeric one); symbolic_probes = the probes beyond the first over all insertions
 *     of the counting pass; symbolic_seconds = the device part of create, multiply_seconds = the kernels of the last spgemm_multiply;
 *     device_bytes = what the plan holds. (The struct is spmv_mi355x_spgemm_stats: C has one name space for functions and typedefs.)
 *   - rc 1 with a last_error that starts with "spgemm_create:", in this order, all but the last two on the host before any HIP call:
 *     1. m, k or n < 0 or >= 2^31 - 1;
 *     2. NULL: out, a_row_ptr, b_row_ptr, and the col_idx of a matrix that has entries;
 *     3. a pattern: row_ptr from 0 and monotone, A's columns in [0, k), B's in [0, n) (A first, then B);
 *     4. a column twice in a row of B (the message names the row and the column);
 *     5. the device;
 *     6. symbolic: nnz(C) >= 2^31, before C is allocated; "spgemm: internal: table overflow in row ..." if a probe ever found its
 *        table full (tables hold at least twice the row's bound, so it cannot; the bound on the probes makes a bug a message).
 *   - NOT BUILT: fsai_pattern on the device, a fused triple product, fp32 accumulation, the row-partitioned form, numerical
 *     dropping, C = A B + D. */
#define SPMV_MI355X_SPGEMM_BINS 7
typedef struct spmv_mi355x_spgemm spmv_mi355x_spgemm;   /* opaque */
typedef struct {
	unsigned struct_size;   /* in: sizeof of the caller's struct; out: bytes written */
	long   m, k, n, nnz_a, nnz_b, nnz_c;
	long   products, max_row_products, max_row_c;
	long   symbolic_bin_rows[SPMV_MI355X_SPGEMM_BINS], numeric_bin_rows[SPMV_MI355X_SPGEMM_BINS];
	long   symbolic_probes;
	double symbolic_seconds, multiply_seconds;
	double device_bytes;
} spmv_mi355x_spgemm_stats;
int  spmv_mi355x_spgemm_create(spmv_mi355x_spgemm ** out, int device /* -1: current */, long m, long k, long n,
		const int32_t * a_row_ptr, const int32_t * a_col_idx, const int32_t * b_row_ptr, const int32_t * b_col_idx);   /* symbolic */
int  spmv_mi355x_spgemm_destroy(spmv_mi355x_spgemm * P);
int  spmv_mi355x_spgemm_pattern(const spmv_mi355x_spgemm * P, int32_t * c_row_ptr_out /* m+1 */, int32_t * c_col_idx_out /* nnz_c */);
int  spmv_mi355x_spgemm_multiply(spmv_mi355x_spgemm * P, const double * a_values, const double * b_values,
		double * c_values_out);                                                                   /* host, blocking */
int  spmv_mi355x_spgemm_multiply_device_async(spmv_mi355x_spgemm * P, const double * a_values_dev, const double * b_values_dev,
		double * c_values_dev, void * hip_stream);
int  spmv_mi355x_spgemm_info(const spmv_mi355x_spgemm * P, spmv_mi355x_spgemm_stats * info /* struct_size first */);

/* ---- AMG: a smoothed-aggregation multilevel preconditioner built on the GPU -------------------------------------------------------- */
/* For a square SYMMETRIC POSITIVE DEFINITE A (int32 CSR, both triangles) the handle holds a hierarchy A_0 = A, A_1, ... with
 * prolongators P_l and restrictions R_l = P_l^t, and applies one V(nu, nu) cycle z = M^-1 v, M symmetric positive definite. The
 * products are SpGEMM plans, the restriction is the device transposition, every operator is an ordinary handle in the caller's
 * format, opts and precision (csrc/amg.hip, csrc/kernels_amg.hip).
 * THE HIERARCHY, fp64 whatever the handle's precision, the arithmetic exactly as written (no contraction), so that the sequential
 * loops of tests/amg_reference.c reproduce it bit for bit. For level l = 0, 1, ... with A_l of n_l rows:
 *   1. d_i = the first stored a_ii;  rho = max_i (sum_j |a_ij|, in stored order) / d_i;  omega = 4 / (3 rho).
 *   2. strength: for j != i, j in S(i) iff a_ij * a_ij >= (theta * theta) * (d_i * d_j).
 *   3. roots = a maximal independent set at distance 2 in S, in synchronous rounds. A node's state is 0 (out), 1 (undecided) or 2
 *      (root), its key (state << 62) | ((h >> 1) << 31) | i with h = (uint32) (i * 0x9E3779B1u). A round takes the max key over
 *      {i} + S(i) twice (each sweep reads one buffer and writes another); an undecided node whose result is its own key becomes a
 *      root, one whose result carries state 2 goes out. Rounds repeat until no node is undecided (the host reads one counter per
 *      round; more than 1024 rounds are an error). A node without strong neighbours becomes a root of its own.
 *   4. aggregates: roots are numbered in index order. Pass 1: a node with a root in S(i) takes that root's aggregate. Pass 2: a node
 *      still free takes the aggregate of the strong neighbour assigned in pass 1 with the largest |a_ij|, ties to the smallest j.
 *   5. T_ij = 1 iff agg(i) = j;  AT = A_l T by an SpGEMM plan;  P_ij = (agg(i) == j ? 1.0 : 0.0) - (omega / d_i) * AT_ij on AT's
 *      pattern (the stored diagonal puts T's pattern inside AT's).
 *   6. R = P^t in the transposition's contractual order;  A_{l+1} = R (A_l P) by two SpGEMM plans.
 * Level l is the last when n_l <= coarse_rows, or l + 1 == max_levels, or step 4 returned more than 0.9 n_l aggregates (a stall:
 * steps 5 and 6 are not run). A last level of at most 128 rows is factorised once, A = L L^t, packed and dense in fp64:
 *      for k = 0..n-1, for a = k..n-1:  s = A(a, k);  for p = 0..k-1 ascending  s = fma(-L(a, p), L(k, p), s);
 *                                       then L(k, k) = sqrt(s) for a = k and L(a, k) = s / L(k, k) below it
 * (an absent entry is 0). A pivot s that is <= 0 or not finite abandons the factor: the level takes the sweeps, coarse_kind = 2.
 * THE CYCLE, vectors in the handle's precision, w = (omega / d) narrowed, nu = sweeps. Below the last level:
 *      x = w o b;  nu - 1 times x = x + w o (b - A x);  r = b - A x;  b_{l+1} = R r;  x += P cycle(l + 1)  (y += A x of the handle);
 *      nu times x = x + w o (b - A x)
 * and on the last level either L y = b, L^t x = y in fp64, column by column,
 *      for k = 0..n-1:   y_k = y_k / L(k, k);  for a > k  y_a = fma(-L(a, k), y_k, y_a)
 *      for k = n-1..0:   x_k = y_k / L(k, k);  for a < k  y_a = fma(-L(k, a), x_k, y_a)
 * or x = w o b and coarse_sweeps - 1 of the same sweep. One level with nu = 1 costs 4 SpMVs and 3 vector launches.
 *   - amg_create: amg_opts NULL = the defaults below; opts NULL = create's defaults. The handle of A_0 is built here and lent by
 *     amg_level_matrices, so a caller keeps one copy of A. n == 0 is legal: no level, apply does nothing.
 *   - amg_apply_device_async: out = M^-1 in, enqueued on the stream; in == out is legal (in is copied first). One apply at a time per
 *     handle. amg_apply is the blocking form on host vectors of the handle's precision.
 *   - amg_info: struct_size is set by the caller, at most that many bytes are written. Per level rows, nnz of A_l, nnz of P_l (0 on
 *     the last), omega, rho, MIS rounds and aggregates (0 where step 3 was not run); operator complexity = sum nnz(A_l) / nnz(A_0),
 *     grid complexity = sum n_l / n_0; coarse_kind SPMV_MI355X_AMG_COARSE_*; stalled; SpMVs and launches (SpMVs included) of one
 *     apply; the seconds of the setup, split into coarsening (steps 1 to 5's kernels), SpGEMM, transposition, handle creation and
 *     downloads. (The struct is spmv_mi355x_amg_stats: C has one name space for functions and typedefs.)
 *   - amg_level_matrices: borrowed handles of A_l, P_l, R_l (P and R NULL on the last level); they die with M.
 *     amg_aggregates: n_l int32, empty (nothing written) where step 3 was not run. amg_level_csr: the fp64 CSR the handles of
 *     A_l (which = SPMV_MI355X_AMG_A) or P_l (SPMV_MI355X_AMG_P) were built from, sizes from amg_info; any out pointer may be NULL.
 *   - rc 1 with a last_error that starts with "amg_create:", in this order, all but the last on the host before any device is touched:
 *     1. the scalars: opts->struct_size or amg_opts->struct_size not set, an unknown precision or format, n < 0 or n >= 2^31 - 1,
 *        opts that set transpose, symmetric_input or a row block / column filter, opts->value_storage under create's rule; then
 *        theta not finite or outside [0, 1], max_levels outside 1..16, coarse_rows outside 1..128, sweeps outside 1..4,
 *        coarse_sweeps outside 1..64;
 *     2. NULL pointers: out, row_ptr, col_idx or values of a matrix with entries;
 *     3. A's pattern, as create checks it: row_ptr from 0 and monotone, columns in [0, n);
 *     4. a column stored twice in a row (the message names the row and the column);
 *     5. the diagonal: every row must store a_ii, finite and > 0 (the message names the first bad row);
 *     6. the device, whatever spmv_mi355x_create and spmv_mi355x_spgemm_create refuse (their message after the prefix), a coarse
 *        diagonal that is not positive and a MIS that did not end.
 *   - NOT CHECKABLE: that A is symmetric and positive definite. An indefinite A shows, if at all, as a coarse diagonal that is not
 *     positive, as coarse_kind = 2, or as stop 4 of the solver.
 *   - NOT BUILT: update_values for a hierarchy that re-aggregates (what is built keeps the aggregates and redoes the numeric
 *     passes: "new values for a hierarchy" below), W- and K-cycles, more than one near-null vector (block coarse unknowns,
 *     elasticity), filtering with a threshold of its own, gmres / minres / multi-RHS wiring other than CG's (k right-hand sides
 *     through the cycle and through CG: spmv_mi355x_amg_apply_multi and spmv_mi355x_pcg_amg_multi below), the row-partitioned
 *     form. (The small levels as one launch are built, opt-in: "AMG: the small levels as one launch" below.) The setup routes patterns
 *     through the host (spgemm_create and create take host arrays); the split in amg_info shows what that costs.
 * spmv_mi355x_pcg_amg is spmv_mi355x_pcg_tri with z = M^-1 r = amg_apply_device_async: the same recurrences, kernels, stop codes,
 * history, spmv_mi355x_pcg_tri_info and freeze (the SpMVs and vector kernels of a cycle write only the hierarchy's own vectors and
 * z). info.spmv_calls counts the products with A of the recurrence, not those of the cycle. rc 1 with a last_error that starts with
 * "pcg_amg:": first items 1 to 5 of spmv_mi355x_pcg_tri, then M == NULL (the message points to spmv_mi355x_pcg_tri), then M's n,
 * precision or device differing from A's, in that order. */
#define SPMV_MI355X_AMG_MAX_LEVELS 16
enum { SPMV_MI355X_AMG_COARSE_DENSE = 0, SPMV_MI355X_AMG_COARSE_SWEEPS = 1, SPMV_MI355X_AMG_COARSE_SWEEPS_AFTER_PIVOT = 2 };
enum { SPMV_MI355X_AMG_A = 0, SPMV_MI355X_AMG_P = 1, SPMV_MI355X_AMG_AF = 2 };
typedef struct spmv_mi355x_amg spmv_mi355x_amg;   /* opaque */
typedef struct {
	int    struct_size;    /* sizeof(spmv_mi355x_amg_opts) */
	double theta;          /* strength threshold, default 0.08, in [0, 1] */
	int    max_levels;     /* default 10, 1..16 */
	int    coarse_rows;    /* default 128, 1..128: a level of at most this many rows is the last */
	int    sweeps;         /* nu, default 1, 1..4 */
	int    coarse_sweeps;  /* default 4, 1..64: damped-Jacobi sweeps of a last level that is not factorised */
} spmv_mi355x_amg_opts;
typedef struct {
	unsigned struct_size;   /* in: sizeof of the caller's struct; out: bytes written */
	int    levels, coarse_kind, stalled;
	long   rows[SPMV_MI355X_AMG_MAX_LEVELS], nnz[SPMV_MI355X_AMG_MAX_LEVELS], nnz_p[SPMV_MI355X_AMG_MAX_LEVELS];
	long   aggregates[SPMV_MI355X_AMG_MAX_LEVELS], mis_rounds[SPMV_MI355X_AMG_MAX_LEVELS];
	double omega[SPMV_MI355X_AMG_MAX_LEVELS], rho[SPMV_MI355X_AMG_MAX_LEVELS];
	double operator_complexity, grid_complexity;
	long   spmvs_per_apply, launches_per_apply;
	double setup_seconds, coarsen_seconds, spgemm_seconds, transpose_seconds, create_seconds, download_seconds;
} spmv_mi355x_amg_stats;
int  spmv_mi355x_amg_create(spmv_mi355x_amg ** out, int format, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const spmv_mi355x_amg_opts * amg_opts /* NULL = defaults */, const spmv_mi355x_opts * opts /* may be NULL */);
int  spmv_mi355x_amg_destroy(spmv_mi355x_amg * M);
int  spmv_mi355x_amg_apply_device_async(spmv_mi355x_amg * M, const void * in_dev, void * out_dev, void * hip_stream);
int  spmv_mi355x_amg_apply(spmv_mi355x_amg * M, const void * in_host, void * out_host);          /* blocking */
int  spmv_mi355x_amg_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_stats * info /* struct_size first */);
int  spmv_mi355x_amg_level_matrices(const spmv_mi355x_amg * M, int level, spmv_mi355x_matrix ** A_out, spmv_mi355x_matrix ** P_out,
		spmv_mi355x_matrix ** R_out);                                                             /* borrowed */
int  spmv_mi355x_amg_aggregates(const spmv_mi355x_amg * M, int level, int32_t * out /* rows[level] */);
int  spmv_mi355x_amg_level_csr(const spmv_mi355x_amg * M, int level, int which, int32_t * row_ptr_out, int32_t * col_idx_out,
		double * values_out);
double spmv_mi355x_amg_mem_footprint(const spmv_mi355x_amg * M);     /* the handles, the vectors and the dense factor, bytes */
int  spmv_mi355x_pcg_amg(spmv_mi355x_matrix * A, const void * b_host, void * x_out_host, spmv_mi355x_amg * M, double tol,
		long max_iterations, double * history_out /* may be NULL: max_iterations doubles */,
		spmv_mi355x_pcg_tri_info * info /* may be NULL */);

/* ---- AMG: new values for a hierarchy --------------------------------------------------------------------------------------------- */
/* update_values' rule for the hierarchy: same pattern, new numbers, the SAME AGGREGATES, no rebuild. prepare once, then update any
 * number of times; a caller who never updates pays nothing. values are nnz(A_0) fp64 numbers in the entry order of the CSR amg_create
 * was given.
 * FROZEN, exactly what amg_create found from the first values: the number of levels and their rows, stalled, the aggregates, the
 * patterns of A_l, P_l and R_l, theta, sweeps and coarse_sweeps.
 * RECOMPUTED from the new values by steps 1, 5 and 6 above in the same pinned fp64 arithmetic: d, rho and omega of every level,
 * w = omega / d narrowed to the handle's precision, P_l, R_l = P_l^t, A_{l+1} = R (A_l P), the dense factor of a last level of at most
 * 128 rows and with it coarse_kind (only DENSE <-> SWEEPS_AFTER_PIVOT can flip); spmvs_per_apply and launches_per_apply follow.
 * THE CONTRACT.
 *   1. Same structure: a hierarchy created from V1 and updated with V2 is indistinguishable from amg_create on V2 whenever amg_create
 *      on V2 would find the same levels and aggregates: amg_level_csr's values and amg_info's omega and rho are equal to the bit,
 *      amg_apply gives the same bits, and every handle is byte for byte the created one (update_values' own contract).
 *   2. Otherwise the hierarchy is, bit for bit, that of the sequential loops of tests/amg_update_reference.c, which take the
 *      aggregates as given.
 * amg_level_csr returns the new values afterwards (they are downloaded when asked for), amg_aggregates what it returned before; the
 * level-0 handle stays the lent one, same pointer, and holds V2; amg_info's seconds stay those of create.
 *   - amg_update_values_prepare, once (a second call does nothing): first every handle's update_values_state; one that takes no update
 *     (the _unit merge layout of uniform values, col_blocks) gives rc 1, "amg_update_values_prepare: level l: A|P|R: <the handle's
 *     reason>", the hierarchy untouched and usable. Then per coarsened level the three SpGEMM plans (A T, A P, R (A P)) are rebuilt
 *     from the host patterns and aggregates the hierarchy keeps, the entry map P -> R is derived by the transposition's own order,
 *     update_values_prepare runs on A_l, P_l and R_l, and the value arrays of A_l, A T, P, R and A P are allocated. None of it is
 *     counted in amg_mem_footprint (as the handles' maps are not); amg_update_info reports the bytes and the seconds. n == 0 and
 *     one-level hierarchies are legal.
 *   - amg_update_values_device: ordered on hip_stream, blocking (as update_values_device). Per level one kernel computes d, the row
 *     sums over d and the count of bad diagonals (the host reads the count and at most 1024 partial maxima), one computes w, the
 *     handle of A_l is refreshed, and below the last level the plans' numeric passes, step 5's kernel, the gather into R's order and
 *     the refresh of P_l and R_l follow. A dense last level is factorised on the device; a failed pivot sets coarse_kind = 2, as
 *     create does. amg_update_values uploads the values once and calls it.
 *   - rc 1 with a last_error that starts with "amg_update_values:" and the hierarchy untouched: a NULL handle or values; update before
 *     prepare; a handle that takes no update; values that are not 8-byte aligned; a diagonal of level 0 that is not positive and
 *     finite ("the diagonal of row i of level 0 ...").
 *   - a bad diagonal or a rho that is not finite on a COARSER level is found after the finer levels were rewritten: rc 1 and state 3.
 *     amg_apply, amg_apply_device_async and pcg_amg then refuse (rc 1, a message naming the failed update) until an update succeeds.
 *   - amg_update_values_state, host-only: 0 = cannot (last_error says why; NULL: 0), 1 = prepare is missing, 2 = ready, 3 = the last
 *     update failed below level 0.
 *   - amg_update_info: struct_size is set by the caller. prepared, failed, the updates so far, the bytes prepare keeps and its
 *     seconds, and of the last update its seconds, split into the SpGEMM numeric passes and the handles' update_values_device
 *     (the rest: steps 1 and 5, the weights, the gather, the factor and the host's reads).
 *   - NOT BUILT: re-aggregating when the strength pattern drifts (the caller decides and calls amg_create), update_values for fsai
 *     handles (trsv handles have it: "UPDATE_VALUES" of the triangular solve), an asynchronous update, the row-partitioned form, W- and K-cycles. */
typedef struct {
	unsigned struct_size;   /* in: sizeof of the caller's struct; out: bytes written */
	int    prepared, failed;
	long   updates;
	double prepare_bytes, prepare_seconds;
	double update_seconds, spgemm_seconds, handle_seconds;   /* of the last update */
} spmv_mi355x_amg_update_stats;
int  spmv_mi355x_amg_update_values_prepare(spmv_mi355x_amg * M);
int  spmv_mi355x_amg_update_values(spmv_mi355x_amg * M, const double * values_fp64_host);
int  spmv_mi355x_amg_update_values_device(spmv_mi355x_amg * M, const double * values_fp64_dev, void * hip_stream);
int  spmv_mi355x_amg_update_values_state(const spmv_mi355x_amg * M);
int  spmv_mi355x_amg_update_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_update_stats * info /* struct_size first */);

/* ---- AMG: a caller's near-null vector and filtered prolongator smoothing -------------------------------------------------------- */
/* spmv_mi355x_amg_create_with is amg_create with two options for step 5, the prolongator. prolongator_opts NULL, or
 * {filtered = 0, near_null = NULL}, gives the hierarchy of amg_create bit for bit, with the same launches. Steps 1 to 4 and 6, the
 * stopping rules, the cycle and its weights w = omega / d of step 1 are untouched; the Galerkin product stays R (A_l P) with the
 * unfiltered A_l. The arithmetic is fp64, every product and sum rounded on its own (tests/amg_prolongator_reference.c):
 *   5a. filter (filtered = 1; otherwise A_F = A_l, dF = d, omega_p = omega). Row i keeps, in stored order, the first stored a_ii and
 *       every j in S(i) of step 2; lump = +0.0, then lump = lump + a_ij over every other entry in stored order; dF_i = d_i + lump.
 *       A dF_i that is not finite or not > 0 sends the row back to ALL its entries and dF_i = d_i (counted in unfiltered_rows).
 *       A_F has the kept entries in A's stored order with dF_i at the diagonal's position;
 *       rho_p = max_i (sum_j |aF_ij|, stored order) / dF_i;  omega_p = 4 / (3 rho_p).
 *   5b. tentative prolongator (near_null given; otherwise t_i = 1.0 and nothing is carried down). With b the level's vector
 *       (b_0 = near_null), for aggregate a over its members in ascending i: s = +0.0; s = s + b_i * b_i; nrm_a = sqrt(s);
 *       t_i = b_i / nrm_agg(i), an IEEE division; b_{l+1}[a] = nrm_a. T has the pattern of step 5 and the values t.
 *   5c. AT = A_F T by an SpGEMM plan; P_ij = (agg(i) == j ? t_i : 0.0) - (omega_p / dF_i) * AT_ij on AT's pattern.
 *   - everything of "AMG" above works on such a handle; amg_level_csr takes which = SPMV_MI355X_AMG_AF, the filtered operator of a
 *     coarsened level (refused where filtered = 0 and on a level without a prolongator; its entry count is nnz_filtered).
 *   - amg_prolongator_info: struct_size is set by the caller. filtered, has_near_null, and per coarsened level nnz_filtered,
 *     unfiltered_rows, omega_p, rho_p (with filtered = 0: nnz, 0, omega, rho; 0 on a level without a prolongator).
 *   - amg_near_null: b_l, rows[level] doubles; nothing is written where no near-null vector was given.
 *   - rc 1 with a last_error that starts with "amg_create_with:", in amg_create's order. Among the scalars, after the amg_opts ones:
 *     prolongator_opts->struct_size not set, then filtered outside 0..1. After item 5: every near_null[i] must be finite and not 0
 *     (the message names the first row). Under item 6: a rho_p that is not a positive finite number, and an aggregate whose norm is
 *     not a positive finite number (b * b underflowed to 0 or overflowed; the message names the level and the aggregate).
 *   - new values (amg_update_values*): frozen in addition are the kept pattern of every A_F, fall-back rows included, its entry map
 *     into A_l, and t and b_l of every level (they depend on near_null and the aggregates only). Recomputed: lump, dF, rho_p,
 *     omega_p, A_F's values, P, R, A_{l+1}. A lumped diagonal that is not finite or not > 0 on a row that was filtered at create is a
 *     bad diagonal of that level: on level 0 it is found before anything is written, below it gives state 3. The updated hierarchy
 *     equals amg_create_with on the new values bit for bit whenever that would find the same aggregates AND the same kept patterns;
 *     otherwise it equals the update loops of tests/amg_prolongator_reference.c. */
typedef struct {
	int            struct_size;  /* sizeof(spmv_mi355x_amg_prolongator_opts) */
	int            filtered;     /* 0 (default) or 1 */
	const double * near_null;    /* n fp64 values on the host, or NULL (default): the constant, un-normalised */
} spmv_mi355x_amg_prolongator_opts;
typedef struct {
	unsigned struct_size;   /* in: sizeof of the caller's struct; out: bytes written */
	int    filtered, has_near_null;
	long   nnz_filtered[SPMV_MI355X_AMG_MAX_LEVELS], unfiltered_rows[SPMV_MI355X_AMG_MAX_LEVELS];
	double omega_p[SPMV_MI355X_AMG_MAX_LEVELS], rho_p[SPMV_MI355X_AMG_MAX_LEVELS];
} spmv_mi355x_amg_prolongator_stats;
int  spmv_mi355x_amg_create_with(spmv_mi355x_amg ** out, int format, int precision, long n,
		const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const spmv_mi355x_amg_opts * amg_opts /* NULL = defaults */,
		const spmv_mi355x_amg_prolongator_opts * prolongator_opts /* NULL = defaults */, const spmv_mi355x_opts * opts /* may be NULL */);
int  spmv_mi355x_amg_prolongator_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_prolongator_stats * info /* struct_size first */);
int  spmv_mi355x_amg_near_null(const spmv_mi355x_amg * M, int level, double * out /* rows[level] */);

/* ---- k right-hand sides through one AMG or FSAI cycle and one tol-based CG -------------------------------------------------------- */
/* k independent systems A x_j = b_j on one handle. Not block CG: every column keeps the recurrences, the stop codes
 * 1 to 5, the breakdown rules and the freeze of spmv_mi355x_pcg_tri. What the columns share is one spmv_mi355x_spmm_device_async per
 * SpMV of the single call, every launch, and every pass over A_l, R_l and P_l of a hierarchy.
 * THE CONTRACT of every call below: on handles whose SpMV is deterministic, column j returns the bits of the single-vector call on
 * column j. No single-vector entry point goes through the SpMM or a k-column apply; the vector kernels of the solve are one set, of
 * which the single-vector solve is k = 1.
 * Every k-column block is row-major: row i at ptr + i * ld, ld >= k counted in values of the handle's precision.
 *   - amg_apply_multi_device_async: out = M^-1 in for the k columns, the schedule of amg_apply_device_async with every SpMV as one
 *     SpMM (beta = 1 for the prolongation) and every vector launch as one launch per chunk of 8, 4, 2 or 1 columns (k = 8s, then the
 *     binary remainder, as the SpMM splits it). A dense last level is solved by one workgroup per chunk, which loads the packed factor
 *     into LDS once for up to 8 columns. Level 0 reads `in` and writes `out` through their own ld; in == out needs ldin == ldout and
 *     works on a copy. The hierarchy owns the per-level blocks: they are allocated at the first multi apply, counted in
 *     amg_mem_footprint, and replaced when a larger k arrives, WHICH SYNCHRONISES THE DEVICE. One multi apply per hierarchy at a time.
 *     amg_update_values* keeps working: the blocks hold no matrix data. amg_apply_multi is the blocking host form with ld = k.
 *     rc 1 with "amg_apply_multi:": a NULL argument, k < 1, ld < k, in == out with ldin != ldout, a hierarchy whose last update failed.
 *     n == 0 returns 0.
 *   - amg_apply_multi_plan (host only, touches no device): matrix_passes_out = the sum over the cycle's products of what
 *     spmv_mi355x_spmm_plan reports for that level's handle and k; launches_out = those passes plus the vector and dense launches
 *     (the single cycle's, once per chunk). k = 1 reports spmvs_per_apply and launches_per_apply.
 *   - fsai_apply_multi_device_async / fsai_apply_multi: out = G^t (G in) as two SpMMs with an n x k scratch block that grows on demand
 *     (growing synchronises); in == out is legal with ldin == ldout.
 *   - pcg_tri_multi / pcg_fsai_multi / pcg_amg_multi: B_host and X_out_host are rows() x k, ld = k. history_out (may be NULL):
 *     k * max_iterations doubles, column j's rows at history_out + j * max_iterations. infos (may be NULL): k spmv_mi355x_pcg_tri_info,
 *     EACH with struct_size set. Per column they carry what the single solve carries; the explicit |b - A x| and |x| come from one
 *     final SpMM; spmv_calls (SpMM calls) and seconds are the call's, equal in every element. pcg_tri_multi serves M = NULL and an M
 *     with a scale alone (Jacobi); an M with first or second set is REFUSED there, with the message it has always had:
 *     spmv_mi355x_pcg_trsm_multi is the entry that serves it.
 *   - pcg_trsm_multi: pcg_tri_multi for ANY M: NULL, a scale alone, or any mix of blocked and global trsv handles (SGS of A, the
 *     caller's IC(0)). Z = second^-1 (scale o (first^-1 R)) on the n x k block, the triangular parts by spmv_mi355x_trsv_solve_multi_
 *     device_async ("K COLUMNS" of the triangular solve), which reads every (value, column) pair of a factor once per chunk of
 *     columns. The same signature, infos and history as pcg_tri_multi and its checks in its order without the triangular refusal;
 *     then M->struct_size and the parts of M as spmv_mi355x_pcg_tri checks them (6 to 8). On a handle with a deterministic SpMV
 *     column j returns the bits of spmv_mi355x_pcg_tri on b_j with the same M: x, history and every info field but spmv_calls and
 *     seconds; with M = NULL or a scale alone the bits of pcg_tri_multi. The triangular solves know nothing of a column's stop:
 *     they write only Z.
 *     A stopped column is frozen while the others run: its x, r, p, state and history are stored back unchanged or not at all. b_j = 0
 *     stops with 3, a NaN in b_j with 4 at 0 iterations and x_j = 0; neither disturbs its neighbours. The host stops enqueueing once
 *     every column has stopped (with the single solve's polling lag). Per iteration: 1 SpMM, M's own launches, 4 vector launches per
 *     chunk (3 without a preconditioner, when no z is stored).
 *     rc 1 before any device is touched, in this order: k < 1; an infos[j].struct_size < 8; tol negative or not finite;
 *     max_iterations < 0; (pcg_tri_multi) M with a triangular part; A, B or X_out NULL; then the single entries' checks in their order.
 *   - NOT BUILT: block CG, k-column GMRES (gmres_tri stays single-vector), routing the single triangular solve through the k-column
 *     kernels. */
int  spmv_mi355x_amg_apply_multi_device_async(spmv_mi355x_amg * M, int k, const void * in_dev, long ldin, void * out_dev, long ldout,
		void * hip_stream);
int  spmv_mi355x_amg_apply_multi(spmv_mi355x_amg * M, int k, const void * in_host, void * out_host);          /* blocking, ld = k */
int  spmv_mi355x_amg_apply_multi_plan(const spmv_mi355x_amg * M, int k, long * matrix_passes_out, long * launches_out);
int  spmv_mi355x_fsai_apply_multi_device_async(spmv_mi355x_fsai * F, int k, const void * in_dev, long ldin, void * out_dev, long ldout,
		void * hip_stream);
int  spmv_mi355x_fsai_apply_multi(spmv_mi355x_fsai * F, int k, const void * in_host, void * out_host);        /* blocking, ld = k */
int  spmv_mi355x_pcg_tri_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host,
		const spmv_mi355x_tri_precond * M /* may be NULL; a scale alone */, double tol, long max_iterations,
		double * history_out /* may be NULL: k * max_iterations doubles */, spmv_mi355x_pcg_tri_info * infos /* may be NULL: k of them */);
int  spmv_mi355x_pcg_trsm_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host,
		const spmv_mi355x_tri_precond * M /* may be NULL; any parts */, double tol, long max_iterations,
		double * history_out /* may be NULL: k * max_iterations doubles */, spmv_mi355x_pcg_tri_info * infos /* may be NULL: k of them */);
int  spmv_mi355x_pcg_fsai_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, spmv_mi355x_fsai * F, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos);
int  spmv_mi355x_pcg_amg_multi(spmv_mi355x_matrix * A, int k, const void * B_host, void * X_out_host, spmv_mi355x_amg * M, double tol,
		long max_iterations, double * history_out, spmv_mi355x_pcg_tri_info * infos);

/* ---- AMG: the small levels as one launch (opt-in fold) ---------------------------------------------------------------------------- */
/* The cycle of a large hierarchy is bound by its launches, and most of them belong to levels that hold almost none of its entries.
 * spmv_mi355x_amg_set_fold(M, fold_rows) is a setter on a built hierarchy (as trsv_set_sweeps is): fold_rows = 0, the state after
 * create, is off; the range is 0..65536. With fold_rows > 0 let f be the first level, level 0 included, with rows[f] <= fold_rows.
 * Levels 0 .. f-1 run exactly as before: same handles, same launches. The whole rest of the V cycle from level f down to the last
 * level and back up to level f (smoothing, residual, restriction, the coarse solve or the coarse sweeps, prolongation, smoothing) is
 * ONE launch of ONE workgroup of 1024 lanes (csrc/kernels_amg_fold.hip). If no level qualifies nothing folds and
 * apply is the unfolded apply bit for bit. f depends on fold_rows and rows[] alone: never on k, the precision or LDS capacity. With
 * the fold off every entry point does what it did, bit for bit and launch for launch.
 * THE DATA. The fold owns plain int32 CSR copies of A_l, P_l and R_l of the folded levels, values narrowed to the handle's
 * precision as the handles' are, uploaded at set_fold from the host copies the hierarchy keeps. R_l is the stable transposition of
 * P_l's CSR (rows ascending within a column: the device transposition's order). w_l is the level's own w, the dense factor the
 * hierarchy's own. The vectors are the hierarchy's level vectors in global memory, ordered by workgroup barriers; LDS holds the
 * packed factor and the pivots of the dense solve alone. No atomics, no flags, no grid barrier, nothing spins; every barrier sits
 * outside the row loops, whose trip counts are uniform. The copies are counted in amg_mem_footprint and freed at destroy.
 * THE ARITHMETIC OF THE TAIL, pinned (tests/amg_fold_reference.c states it as sequential loops), in the handle's precision T, every
 * product and sum rounded on its own, the only fused operations the fma() written here:
 *      a row's product: s = +0, then s = fma(a_e, x_col(e), s) for the row's entries e in stored order;
 *      x = w o b;   t = A x, x = x + w o (b - t);   t = b - A x;   b_{l+1} = R t;   x = x + P x_{l+1}
 * in the cycle's order ("THE CYCLE" of "AMG" above). LANES PER ROW: the rows of A_l are split over G_l lanes, G_l = the largest
 * power of two that is <= min(64, nnz(A_l) / n_l, 1024 / n_l) in integer division, and 1 where that minimum is 0. Lane g of a row
 * takes the entries g, g + G, g + 2 G, ... of the row as its own fma chain from +0, and the G partial sums are combined by the
 * halving tree s_g = s_g + s_{g + h} for h = G / 2, G / 4, ..., 1; the product is s_0. G_l depends on the CSR of A_l alone, never
 * on k, T or the launch; amg_fold_info reports it. The rows of P_l and R_l are walked by one lane. A dense last level is solved
 * inside the tail with the bits of the dense solve of "AMG" above: fp64, the same column order. The tail sums a row in another order
 * than a handle's SpMV does: a folded apply differs from the unfolded one by rounding, and stays within the cycle's bound of it.
 * K COLUMNS: amg_apply_multi launches the tail once per chunk of 8, 4, 2 or 1 columns; a lane loads a (value, column) pair once
 * and keeps one partial sum per column; column j of amg_apply_multi has the bits of amg_apply on column j, fold on or off.
 *   - amg_set_fold: blocking (it synchronises the device); not to be called while an apply is in flight. rc 1 with "amg_set_fold:":
 *     a NULL handle; fold_rows outside 0..65536; a hierarchy whose last update failed. n == 0 is legal: no level, nothing folds.
 *   - amg_fold_info: struct_size is set by the caller. fold_rows; first_level (= levels when nothing folds); folded_levels;
 *     launches_per_apply and spmvs_per_apply (the handle SpMVs left) of one apply; tail_products, the matrix products inside the tail
 *     and tail_entries, their entry visits per apply; lanes_per_row[l] = G_l of the folded levels (0 above them); bytes of the copies.
 *     amg_info's spmvs_per_apply and launches_per_apply and amg_apply_multi_plan(k) follow the fold (one tail launch per chunk).
 *   - amg_apply_level_device_async: out = cycle(level, in) for one column of rows[level] values under the current fold setting,
 *     in == out legal. rc 1 with "amg_apply_level:": a NULL handle; a hierarchy whose last update failed; a level outside
 *     0..levels-1; NULL in or out.
 *   - amg_apply*, amg_apply_multi*, pcg_amg and pcg_amg_multi pick the fold up through apply.
 *   - new values: amg_update_values* on a folded hierarchy refreshes the fold's value arrays on the device (narrowed from the
 *     update's arrays, which are in the same entry order); w and the factor are the hierarchy's own; a last level that flips between
 *     dense and sweeps is followed. The result is what set_fold gives on a hierarchy created from the new values (contract 1 of
 *     "new values for a hierarchy"). set_fold before or after amg_update_values_prepare both work.
 *   - NOT BUILT: a multi-workgroup tail (one CU bounds what is worth folding), folding by entries instead of rows, a fold for FSAI,
 *     W-cycles inside the tail.
 * MEASURED (one MI355X, fp64, every leg beside fold_rows = 0 on the same hierarchy; profiles/r33_amg_fold.txt): the fold LOSES unless
 * the tail is tiny. Unfolded, the small levels cost 3.5 us per launch; one workgroup walks the tail at 1.1 ns per entry visit. On
 * the 2000 x 2000 grid (theta 0.08, last levels of 37, 164, 301 entries per row) fold_rows = 1024 takes the apply from 0.553 to
 * 1.603 ms, 8192 to 2.18 ms, 65536 to 5.65 ms; with filtered smoothing (tails of 9 222 to 27 453 entry visits) 1024 is level or 2 %
 * ahead. The default stays 0 and no value is recommended as one. */
typedef struct {
	unsigned struct_size;   /* set by the caller */
	int    fold_rows, first_level, folded_levels;
	long   launches_per_apply, spmvs_per_apply, tail_products, tail_entries;
	int    lanes_per_row[SPMV_MI355X_AMG_MAX_LEVELS];
	double bytes;
} spmv_mi355x_amg_fold_stats;
int  spmv_mi355x_amg_set_fold(spmv_mi355x_amg * M, int fold_rows);                                           /* blocking */
int  spmv_mi355x_amg_fold_info(const spmv_mi355x_amg * M, spmv_mi355x_amg_fold_stats * info /* struct_size first */);
int  spmv_mi355x_amg_apply_level_device_async(spmv_mi355x_amg * M, int level, const void * in_dev, void * out_dev, void * hip_stream);

/* Row-partitioned (multi-GPU) form of the same two solvers: one process per GPU owns the row block [row_offset,
 * row_offset + m_local) of A, b and x. The solver keeps every vector device-resident and local; the two things that cross
 * ranks are handed to the caller, who has the communicator (torch.distributed / RCCL in bench-level code):
 *   spmv(ctx, in_dev, out_dev)           out_local = (A * in)_local where `in` is this rank's slice of the global vector
 *                                        (exchange of the slices + the local SpMV launches, e.g. §8e's allgather(x) scheme)
 *   allreduce_sum(ctx, reduce_buf_dev, count)   in-place sum over the ranks of `count` doubles in reduce_buf_dev
 * Both are called on the host between kernel launches and must ENQUEUE their work on the NULL stream (or order against
 * it); nothing waits for the host. Per iteration: CG 1 spmv + 2 all-reduces (1 and 2 doubles), BiCGSTAB 2 spmv + 3
 * all-reduces. All ranks compute identical scalars, take the `err < eps` break at the same iteration and return the same
 * history/info; the values equal the single-GPU solver's up to the summation order of the dots.
 * row_ptr_local has m_local+1 entries starting at 0; col_idx_global holds GLOBAL column indices (the Jacobi diagonal of
 * local row i is the first entry with column row_offset + i); b / x are the local slices (host, handle precision). */
typedef struct {
	unsigned struct_size;      /* sizeof(spmv_mi355x_dist_ops) */
	long   row_offset;
	int  (*spmv)(void * ctx, const void * in_dev, void * out_dev);
	int  (*allreduce_sum)(void * ctx, double * reduce_buf_dev, int count);
	double * reduce_buf_dev;   /* device scratch of >= 4 doubles owned by the caller (so it can be a tensor of its framework) */
	void * ctx;
} spmv_mi355x_dist_ops;
int  spmv_mi355x_pcg_dist(const spmv_mi355x_dist_ops * ops, int precision, long m_local, const int32_t * row_ptr_local,
		const int32_t * col_idx_global, const double * values_fp64, const void * b_local_host, void * x_local_out_host,
		long max_iterations, double * history_out, spmv_mi355x_solver_info * info);
int  spmv_mi355x_pbicgstab_dist(const spmv_mi355x_dist_ops * ops, int precision, long m_local, const int32_t * row_ptr_local,
		const int32_t * col_idx_global, const double * values_fp64, const void * b_local_host, void * x_local_out_host,
		long max_iterations, double * history_out, spmv_mi355x_solver_info * info);

/* ---- several GPUs of one node behind ONE handle (SURVEY §8b "create_partitioned", §8e) ------------------------------------- */
/* What the reference's single-process driver can call: csr_to_format() hands over the whole matrix (bench.cpp:600-603), the
 * library cuts it into `nparts` nnz-balanced contiguous row blocks — loop_partitioner_balance_prefix_sums
 * (lib/parallel_util.h:156-184, what csr.cpp:140 does per thread) with one worker per GPU — puts block p on devices[p]
 * (NULL: device p modulo the device count) and keeps x on every device as nparts equal padded slices. Per SpMV the x slices
 * are exchanged (RCCL allgather over xGMI; peer / device copies where RCCL is unavailable or several parts share a device)
 * while each device computes the part of its block whose columns lie in its own slice; the remote-column part is accumulated
 * once the exchange has landed. y comes back in global row order. Square matrices only.
 * exchange: 0 = auto (RCCL when the devices are distinct and librccl.so.1 loads, else copies), 1 = RCCL, 2 = copies. */
typedef struct spmv_mi355x_partitioned spmv_mi355x_partitioned;   /* opaque */
int  spmv_mi355x_create_partitioned(spmv_mi355x_partitioned ** out, int nparts, const int * devices, int exchange, int format,
		int precision, long m, long n, long nnz, const int32_t * row_ptr, const int32_t * col_idx, const double * values_fp64,
		const spmv_mi355x_opts * opts /* may be NULL; device / row block / column filter fields are set per part */);
int  spmv_mi355x_destroy_partitioned(spmv_mi355x_partitioned * P);
/* Matrix_Format::spmv(x, y) with host buffers (n and m values of the handle's precision), same caching convention as
 * spmv_mi355x_spmv: x is uploaded when its pointer is new, y is downloaded on the first call after an upload. */
int  spmv_mi355x_spmv_partitioned(spmv_mi355x_partitioned * P, const void * x_host, void * y_host);
int  spmv_mi355x_partitioned_set_always_copy(spmv_mi355x_partitioned * P, int on);
/* `iters` SpMVs back to back on the resident x (exchange forced every time): wall-clock ms per SpMV between all-device syncs. */
int  spmv_mi355x_time_partitioned(spmv_mi355x_partitioned * P, int iters, double * ms_per_iter_out);
int  spmv_mi355x_partitioned_parts(const spmv_mi355x_partitioned * P);
int  spmv_mi355x_partitioned_offsets(const spmv_mi355x_partitioned * P, long * offsets_out /* [nparts+1] */);
const char * spmv_mi355x_partitioned_format_name(const spmv_mi355x_partitioned * P);
const char * spmv_mi355x_partitioned_exchange(const spmv_mi355x_partitioned * P);     /* "RCCL allgather" | "peer copies" | ... */
double spmv_mi355x_partitioned_mem_footprint(const spmv_mi355x_partitioned * P);

/* ---- format introspection for parity tests (host copies of the converted arrays) -------------------------- */
/* One stored array of the plain SELL layout ("val", "col", "slice_ptr", "row_of_sorted"), of the LDS-window SELL layout ("val", "idx",
 * "desc", "row_of_sorted", "groups") or of the column-blocked layout
 * ("entries", "val", "batch_base", "batch_ptr", "chunk_ptr", "chunk_row", "wg_rows", "range_row", "range_long", "long_row") exactly as it
 * lies in device memory: a malloc'ed copy (free with spmv_mi355x_free). For the tests that hold the host and the GPU builder of a
 * layout to the same bytes, and for diagnostics. */
int  spmv_mi355x_stored_array(const spmv_mi355x_matrix * A, const char * name, void ** out, size_t * bytes_out);

/* SELL-C-sigma layout: any out pointer may be NULL. Arrays are malloc'ed copies; free with spmv_mi355x_free().
 * For delta-compressed handles the column array is DECODED back to the plain column-major layout. */
int  spmv_mi355x_sell_layout(const spmv_mi355x_matrix * A, long * C_out, long * sigma_out, long * num_slices_out,
		long * nnz_ext_out, int64_t ** slice_ptr_out, int32_t ** col_out, double ** val_as_f64_out,
		int32_t ** row_of_sorted_out);
/* merge-path tile start coordinates (row, nnz) — num_tiles+1 pairs */
int  spmv_mi355x_merge_tiles(const spmv_mi355x_matrix * A, long * num_tiles_out, long * tile_items_out, int32_t ** coords_out);
void spmv_mi355x_free(void * p);

#ifdef __cplusplus
}
#endif
#endif /* SPMV_MI355X_H */

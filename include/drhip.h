/*
 * drhip.h -- C-ABI of libdrhip.so, the MI355X (gfx950) device layer and
 * algorithm kernels behind the Distributed Ranges `shp` API.
 *
 * The reference (sudhirverma/distributed-ranges, header-only C++20/SYCL) has
 * no FFI of its own: its device layer is SYCL queues + USM
 * (include/dr/shp/{init,allocators,copy,device_ref}.hpp) and its per-segment
 * arithmetic is oneDPL (reduce_async / inclusive_scan_async / for_each_async)
 * plus SYCL parallel_for kernels.  Each entry point below replaces one of
 * those call sites; the replaced reference interface is cited per function.
 * The C++ drop-in layer (distributed-ranges_amd/include/dr/shp/...) and the
 * Python binding (distributed-ranges_amd/drhip.py) both call only this ABI.
 *
 * Conventions
 *   - Every function returns int: 0 = success, otherwise a drhip_status code
 *     (hip errors are mapped to DRHIP_ERR_HIP and the hipError_t text is
 *     kept for drhip_last_error()).
 *   - A "segment" (seg) is one entry of the ordered device list given to
 *     drhip_init -- the reference's segment rank (shp/init.hpp:40-50).  Each
 *     segment owns one HIP stream; duplicated device ids are allowed
 *     (the reference test harness's --devicesCount duplication,
 *     test/gtest/shp/shp-tests.cpp:34-39).
 *   - Kernel entry points are ASYNCHRONOUS on the segment's stream; buffers
 *     are owned by the caller and must be device-visible (device memory,
 *     peer memory with P2P enabled, or pinned host memory).  `*_host`
 *     arguments are plain host pointers read during the call.
 *   - "ACC" is the accumulation type of an element type: double for F32/F64,
 *     the element type itself for integers (wrapping two's-complement
 *     arithmetic).  Reduce results, scan carries and totals are ACC.
 */
#ifndef DRHIP_H
#define DRHIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum {
  DRHIP_I32 = 0, DRHIP_U32 = 1, DRHIP_I64 = 2, DRHIP_U64 = 3, DRHIP_F32 = 4, DRHIP_F64 = 5
} drhip_dtype;

typedef enum { DRHIP_PLUS = 0, DRHIP_MUL = 1, DRHIP_MIN = 2, DRHIP_MAX = 3 } drhip_op;

typedef enum {
  DRHIP_OK = 0,
  DRHIP_ERR_HIP = 1,          /* a HIP runtime call failed */
  DRHIP_ERR_NOT_INIT = 2,     /* drhip_init not called */
  DRHIP_ERR_BAD_SEG = 3,      /* segment index out of range */
  DRHIP_ERR_BAD_ARG = 4,      /* null pointer, unsupported dtype/op, bad size */
  DRHIP_ERR_NO_DEVICE = 5,    /* no HIP device visible */
  DRHIP_ERR_TIMEOUT = 6,      /* a bounded in-kernel spin gave up */
  DRHIP_ERR_UNSUPPORTED = 7,
  DRHIP_ERR_COMM = 8,         /* an RCCL call failed (text has the ncclResult_t) */
  DRHIP_ERR_ALLOC = 9         /* the allocator returned memory overlapping a live block,
                                 or a guard red zone was overwritten (DRHIP_ALLOC_GUARD) */
} drhip_status;

/* ------------------------------------------------------------ runtime --
 * Replaces shp::init/finalize/devices/nprocs/context (shp/init.hpp:16-52)
 * and get_numa_devices/get_duplicated_devices (shp/util.hpp:77-136). */

/* Registers `nsegs` segments on HIP devices dev_ids[0..nsegs) (ids may
 * repeat), creates one non-blocking stream per segment, enables peer access
 * between distinct devices, and allocates per-segment workspaces.  Calling
 * it again re-initialises (finalize + init). */
int drhip_init(const int *dev_ids, int nsegs);
int drhip_finalize(void);
int drhip_device_count(int *count);           /* visible HIP devices */
int drhip_nprocs(int *nsegs);                 /* shp::nprocs() */
int drhip_device_of(int seg, int *dev_id);    /* shp::devices()[seg] */
int drhip_stream(int seg, void **hip_stream); /* the segment's hipStream_t */
int drhip_sync(int seg);                      /* wait for the segment's stream */
int drhip_sync_all(void);
const char *drhip_last_error(void);           /* text of the last failure */
const char *drhip_version(void);
/* HIP graphs of a segment's work (no counterpart in the reference, whose
 * every algorithm call builds new sycl::queues, e.g. reduce.hpp:63): the
 * drhip calls (and RCCL collectives) issued between drhip_graph_begin and
 * drhip_graph_end on seg's stream are captured, not run; drhip_graph_launch
 * replays them on seg's stream with one launch.  For a step repeated with
 * the same buffers and sizes -- e.g. the strong-scaled reduce + scan whose
 * per-rank kernels take ~0.3 ms, where launch gaps are SURVEY.md 7's "per-
 * call overhead <= 10 us" budget.  Every kernel launched by the C-ABI keeps
 * its state on the device (single-pass reduce counters reset by their last
 * block, scan status words re-zeroed by a memset node), so a replay
 * recomputes everything.  Between begin and end, no call may allocate
 * (warm the workspaces with one eager call first) or synchronise.
 * Lifetime: a graph holds raw pointers to seg's workspace and tile-prefix
 * buffer, so from drhip_graph_begin until every graph of seg is destroyed
 * (drhip_graph_destroy) a call that would GROW either buffer fails with
 * DRHIP_ERR_UNSUPPORTED instead of freeing memory a graph still uses.  A
 * drhip_reduce_tiles inside a graph takes effect at drhip_graph_launch: an
 * eager drhip_inclusive_scan_tiles after a replay must name the captured
 * range.  A graph launches only on the segment it was captured on. */
int drhip_graph_begin(int seg);
int drhip_graph_end(int seg, void **graph_exec);
int drhip_graph_launch(int seg, void *graph_exec);
int drhip_graph_destroy(void *graph_exec);

/* ------------------------------------------------------------- memory --
 * device_allocator::allocate/deallocate (shp/allocators.hpp:45-72) and
 * shp::copy/copy_async/fill_async (shp/copy.hpp:19-173), device_ref
 * element access (shp/device_ref.hpp:23-44). */
/* drhip_malloc: device memory on seg's device, valid on every stream and
 * peer device.  Default (DRHIP_ALLOC=cache, read at drhip_init): a caching
 * allocator over hipMalloc -- drhip_free keeps the block, whole, in seg's
 * cache behind fences recorded on every segment stream and the device's NULL
 * stream (no host sync), and drhip_malloc hands it out again for a request
 * of the same size class (powers of two below 1 MiB, 2 MiB multiples above)
 * once every fence has completed; work a caller queued on OTHER streams of
 * its own is not fenced (drain those before freeing memory they use).  The
 * cache is released at drhip_finalize and when hipMalloc runs out of memory.
 * DRHIP_ALLOC=hipmalloc: plain hipMalloc / hipFree (hipFree synchronises the
 * device).  DRHIP_ALLOC=pool: the device's stream-ordered pool
 * (hipMallocAsync), kept for diagnosis only -- on ROCm 7.2 / gfx950 a pool
 * block filled by a copy can read differently from a kernel
 * (profiles/r06_pool_diagnosis.txt; DRHIP_POOL=private|noreuse variants).
 * Every live block is tracked: one the allocator returns overlapping a live
 * block is refused (DRHIP_ERR_ALLOC), and drhip_free refuses
 * (DRHIP_ERR_BAD_ARG) a pointer that is not a live drhip_malloc block.
 * DRHIP_ALLOC_GUARD=1: red zones around every block, checked by drhip_free
 * and drhip_sync (DRHIP_ERR_ALLOC names the block); DRHIP_ALLOC_TRACE=path:
 * one line per allocation / free. */
int drhip_malloc(int seg, size_t bytes, void **ptr);
int drhip_free(int seg, void *ptr);
int drhip_host_alloc(size_t bytes, void **ptr);        /* pinned, device-visible host memory */
int drhip_host_free(void *ptr);
/* Async on the segment stream for device / pinned host buffers; with a
 * pageable host buffer the copy still goes on the segment stream (the
 * runtime stages it; DRHIP_COPY=staged: through a pinned 64 MiB buffer of
 * the segment's) and the call blocks until it has landed. */
int drhip_memcpy_h2d(int seg, void *dst, const void *src, size_t bytes);
int drhip_memcpy_d2h(int seg, void *dst, const void *src, size_t bytes);
int drhip_memcpy_d2d(int seg, void *dst, const void *src, size_t bytes);  /* async, may cross devices */
/* dst[i] = *value_host, i < n, element size 1/2/4/8 bytes (copy.hpp:147-168) */
int drhip_fill(int seg, void *dst, size_t n, const void *value_host, size_t elem_size);
/* dst[i] = start + i (std::iota over a segment; test/gtest/shp/algorithms.cpp:11-19) */
int drhip_iota(int seg, int dtype, void *dst, size_t n, const void *start_host);

/* ------------------------------------------------------- elementwise --
 * Fixed-function forms of shp::for_each (shp/algorithms/for_each.hpp:14-92)
 * for callers that cannot compile user lambdas with hipcc; the C++ layer
 * has a header-only template path for arbitrary callables. */
/* out[i] = op(in[i], scalar)   (out may alias in) */
int drhip_transform_scalar(int seg, int dtype, int op, const void *in, void *out, size_t n,
                           const void *scalar_host);
/* out[i] = op(a[i], b[i]) */
int drhip_transform_binary(int seg, int dtype, int op, const void *a, const void *b, void *out,
                           size_t n);
/* x[i] = -x[i]  (the ForEach test's negate, algorithms.cpp:21-37) */
int drhip_negate(int seg, int dtype, void *x, size_t n);

/* ------------------------------------------------------------ reduce --
 * Replaces the per-segment oneDPL reduce_async of shp::reduce
 * (shp/algorithms/reduce.hpp:22-34,74-78).  *out_acc (ACC, device-visible)
 * = op-reduction of x[0..n); n == 0 writes the identity of op.  One kernel
 * launch: the last block to finish folds the block partials. */
int drhip_reduce(int seg, int dtype, int op, const void *x, size_t n, void *out_acc);
/* Cross-segment combine (shp/algorithms/reduce.hpp:81-83 fold in segment
 * order; inclusive_scan.hpp:108-116 scan of the partials) of w gathered
 * segment results partials[0..w) (ACC values of dtype, device-visible, e.g.
 * the output of drhip_allgather): *result = p[0] op p[1] op ... op p[w-1]
 * and, when rank > 0, *carry = p[0] op ... op p[rank-1] -- both folded left
 * to right by one device thread (floats combine in the reference's order).
 * result / carry nullable; asynchronous on seg's stream. */
int drhip_fold_partials(int seg, int dtype, int op, const void *partials, int w, int rank, void *result,
                        void *carry);
/* transform_reduce / dot: sum_i x[i]*y[i] (examples/shp/dot_product.cpp:11-18,
 * reduce(zip(x,y) | transform(a*b), 0, plus)). */
int drhip_dot(int seg, int dtype, const void *x, const void *y, size_t n, void *out_acc);

/* ------------------------------------------------------------- scan ----
 * Replaces phases 1 and 3 of shp::inclusive_scan
 * (shp/algorithms/inclusive_scan.hpp:77-83 oneDPL inclusive_scan_async,
 * :118-143 for_each_async carry pass) with ONE single-pass decoupled-
 * lookback kernel:
 *     out[i] = carry op init op in[0] op ... op in[i]
 * init_host  (nullable, element type): the reference's piece-0 init (:77-80)
 * carry_host (nullable, ACC):          carry read at call time
 * carry_dev  (nullable, ACC):          carry read by the kernel (device-visible),
 *                                      e.g. the output of an RCCL exchange
 * total_acc  (nullable, ACC):          receives carry op init op (all of in),
 *                                      the value phase 2 (:108-116) scans.
 * Supported ops are commutative, so carry placement (the reference applies
 * op(x, carry), :132-134) is value-identical; fp32 inter-tile carries are
 * kept in fp64.  in == out (in-place) is allowed. */
int drhip_inclusive_scan(int seg, int dtype, int op, const void *in, void *out, size_t n,
                         const void *init_host, const void *carry_host, const void *carry_dev,
                         void *total_acc);
/* The N > 1 step of a reduce + scan in one kernel after the exchange:
 * partials[0..w) are the w gathered segment totals (ACC of dtype, device
 * memory, e.g. drhip_allgather's output); the scan of in[0..n) gets as carry
 * the fold of partials[0..rank) and, if result is not null, *result = the
 * fold of all w (the reduce's answer) -- both folded left to right exactly
 * as drhip_fold_partials does, by tile 0 of the scan kernel, so the step
 * runs one kernel fewer (reduce.hpp:81-83, inclusive_scan.hpp:108-143). */
int drhip_inclusive_scan_gathered(int seg, int dtype, int op, const void *in, void *out, size_t n,
                                  const void *partials, int w, int rank, void *result);
/* Reduce + scan over the SAME range (the C2 step, and the shp scan's piece
 * totals): drhip_reduce_tiles is drhip_reduce (the ACC op-reduction of
 * x[0..n) to *out_acc) that also leaves, in the segment, every scan tile's
 * exclusive prefix; drhip_inclusive_scan_tiles then scans that same range
 * (in == x, same n, dtype, op: checked, DRHIP_ERR_BAD_ARG otherwise) with
 * those prefixes -- no look-back, no status words: a streaming pass.  x must
 * not be written between the two calls (the prefixes describe its contents
 * at the reduce; DRHIP_CHECK_TILES=1 at drhip_init hashes the range at both
 * calls and makes drhip_sync return DRHIP_ERR_BAD_ARG on a change -- a debug
 * mode, 4 B/elem more per call), and another drhip_reduce_tiles on the same
 * segment replaces the prefixes.  Its
 * carry is *carry_dev (nullable) and/or the fold of partials[0..rank) of the
 * w gathered segment totals (nullable; *result = fold of all w, nullable),
 * as drhip_inclusive_scan_gathered (also when n == 0: an empty segment still
 * writes *result).  Bytes: 4 + 8 per element, as a reduce
 * followed by drhip_inclusive_scan; the reduce's tile pass replaces the
 * scan's inter-tile look-back (reduce.hpp:40-88 then inclusive_scan.hpp:
 * 22-148 over one range). */
int drhip_reduce_tiles(int seg, int dtype, int op, const void *x, size_t n, void *out_acc);
int drhip_inclusive_scan_tiles(int seg, int dtype, int op, const void *in, void *out, size_t n,
                               const void *carry_dev, const void *partials, int w, int rank, void *result);

/* ------------------------------------------------------------- gemv ----
 * Replaces the gemv nonzero loop (shp/algorithms/gemv.hpp:45-66) with a
 * CSR-vector SpMV over one row tile:  y[i] += sum_k vals[k] * x[colind[k]]
 * for rows i < m, rowptr/colind int32 (idtype DRHIP_I32) or int64
 * (DRHIP_I64), vals/x/y of vdtype (F32 or F64).  The reference's racy
 * `c_v += a_v*b_v` (:62) becomes one owner per row -- no atomics.
 * colind/vals hold nnz entries; rowptr values index them (0 <= rowptr[i]
 * <= nnz) and every colind entry is a valid column of x: the kernel reads
 * whole 16-byte vectors of colind/vals that may straddle row-tile edges. */
int drhip_spmv_csr(int seg, int vdtype, int idtype, size_t m, size_t nnz, const void *rowptr,
                   const void *colind, const void *vals, const void *x, void *y);
/* Device-side synthetic CSR generator for rows [row0, row0+nrows) of an
 * ncols-wide matrix (kind 0 = banded offsets -4..+5, kind 1 = k random
 * distinct sorted columns).  Same hash definition as oracle.c, so a tile
 * generated here equals orc_csr_gen_*.  rowptr is tile-local (starts at 0).
 * Replaces sparse_matrix::init_random_ (containers/sparse_matrix.hpp:286-336),
 * whose host std::map generator cannot build 2^26-row matrices. */
int drhip_csr_nnz(int kind, size_t row0, size_t nrows, size_t ncols, int k, size_t *nnz);
int drhip_csr_gen(int seg, int kind, size_t row0, size_t nrows, size_t ncols, int k,
                  uint64_t seed, void *rowptr, void *colind, void *vals);
/* Density generator for rows [row0, row0+nrows) of an m x ncols matrix:
 * floor(density*m*ncols) nonzeros in total (util/generate_random.hpp:37),
 * spread evenly over rows, one column per equal-width stratum of each row
 * (distinct, sorted), values U[0,1) (float/double) or {0,1} (integers).
 * Replaces generate_random_csr (util/generate_random.hpp:29-90) as called by
 * sparse_matrix(shape, density[, partition]) (containers/sparse_matrix.hpp:
 * 157-166, 286-336), which ignores density and reseeds every tile with 0.
 * Equals orc_csr_gen_density.  rowptr is tile-local. */
int drhip_csr_density_nnz(size_t row0, size_t nrows, size_t m, size_t ncols, double density, size_t *nnz);
int drhip_csr_gen_density(int seg, int vdtype, int idtype, size_t row0, size_t nrows, size_t m, size_t ncols,
                          double density, uint64_t seed, void *rowptr, void *colind, void *vals);

/* ------------------------------------------------------------- sort ----
 * shp::sort is absent from the reference; defined with
 * std::ranges::sort semantics (ascending, std::less).  LSD radix sort of
 * 4- or 8-byte keys (I32/U32/F32 order-preserving bit transforms).
 * From 256 MiB of 4-byte keys the passes are persistent kernels (a grid of
 * the device's resident capacity, tiles claimed per XCD).  Segments of ONE
 * process sharing a device are serialised by the runtime; sorts from
 * SEPARATE processes must not run on one device at the same time (their
 * resident grids can starve each other until the bounded spin reports
 * DRHIP_ERR_TIMEOUT): run them one after the other, or set
 * DRHIP_SORT_OS_PT=0 (the one-shot kernels) in those processes. */
int drhip_sort_workspace(int seg, int dtype, size_t n, size_t *bytes);
int drhip_sort(int seg, int dtype, void *keys, size_t n, void *tmp, size_t tmp_bytes);
/* Distributed-sort helpers: the regular samples samples[j] = sorted[j *
 * stride] (j < ceil(n / stride)) of a sorted run, and per-bucket counts of a
 * sorted run against nsplit sorted splitters (bucket b = [splitter[b-1],
 * splitter[b])). */
int drhip_sort_sample(int seg, int dtype, const void *sorted, size_t n, size_t stride,
                      void *samples);
int drhip_sort_bucket_counts(int seg, int dtype, const void *sorted, size_t n,
                             const void *splitters, int nsplit, uint64_t *counts);
/* Exact splitting of the distributed sort (host functions, csrc/split.hip;
 * SURVEY.md 8e "sort": one samples allgather, one slices allgather, then
 * the all-to-all).  Keys are radix-order bits widened to uint64.  p ranks
 * with n[i] sorted keys; rank i's regular samples (stride[i], nsamples[i]
 * of them) concatenated in `samples`; nb boundaries g[k] (global sorted
 * ranks, normally the prefix sums of n).  drhip_split_windows writes, for
 * each boundary, a value bracket [lo[k], hi[k]] holding the key of global
 * rank g[k], and win[2 (i nb + k) + {0,1}] = the slice [a, b) of rank i's
 * sorted keys holding every key of that bracket.  drhip_split_exact takes
 * every slice's keys concatenated in (rank, boundary) order and writes
 * split[i (nb + 1) + k] = the number of rank i's keys that go to
 * destinations <= k (split[i (nb + 1) + nb] = n[i]): keys below the
 * boundary key in full, keys equal to it in rank order, so destination k
 * receives exactly g[k] - g[k-1] keys.  Deterministic: every rank computes
 * the same matrix. */
int drhip_split_windows(int p, const uint64_t *n, const uint64_t *stride, const uint64_t *nsamples,
                        const uint64_t *samples, int nb, const uint64_t *g, uint64_t *lo, uint64_t *hi,
                        uint64_t *win);
int drhip_split_exact(int p, const uint64_t *n, int nb, const uint64_t *g, const uint64_t *lo,
                      const uint64_t *hi, const uint64_t *win, const uint64_t *wkeys, uint64_t *split);
/* Destination step of the distributed sort: keys[0, n) holds nruns sorted
 * runs [run_offsets[r], run_offsets[r+1]) (host array, 0 .. n); on return
 * keys is sorted (radix order, as drhip_sort).  Pairwise merge-path rounds,
 * ceil(log2 nruns) passes of one read + one write per key, instead of a
 * second full radix sort; nruns <= 128.  Replaces the per-destination local
 * sort of the sample sort (SURVEY.md 8e "sort": local merge or second radix). */
int drhip_merge_workspace(int seg, int dtype, size_t n, int nruns, size_t *bytes);
int drhip_merge_runs(int seg, int dtype, void *keys, size_t n, const size_t *run_offsets, int nruns, void *tmp,
                     size_t tmp_bytes);
/* The same merge from src (the runs, e.g. where the all_to_all landed) into
 * a separate dst (e.g. the segment itself): the rounds alternate so that the
 * last one writes dst -- no copy of the keys before or after (the
 * distributed sort's destination step moves 8 B/key per round and nothing
 * else).  src, dst key-aligned and not overlapping; same workspace as
 * drhip_merge_runs. */
int drhip_merge_runs_to(int seg, int dtype, const void *src, void *dst, size_t n, const size_t *run_offsets,
                        int nruns, void *tmp, size_t tmp_bytes);
/* Sort by key (shp::sort_by_key): keys[0, n) of kdtype (the six key types of
 * drhip_sort) ascending, vals[i] carried with keys[i].  STABLE: pairs with
 * equal keys keep their input order (std::stable_sort of the pairs by key).
 * Key order as drhip_sort: std::less on the key values, -0.0 before +0.0,
 * NaN keys not supported.  Values are val_bytes = 4 or 8 bytes each and move
 * as bits (anything else: DRHIP_ERR_BAD_ARG).  The classic three-kernel pass
 * per 8-bit digit at every n (the persistent passes of drhip_sort carry no
 * payload), so DRHIP_SORT_ALGO has no effect and sorts from separate
 * processes may share a device.  Asynchronous on the segment's stream;
 * n < 2^32; keys key-aligned, vals aligned to val_bytes, tmp 256-byte
 * aligned with at least drhip_sort_pairs_workspace bytes (less:
 * DRHIP_ERR_BAD_ARG); n <= 1 returns DRHIP_OK and touches no memory.  The
 * workspace query needs no initialised device and is never below
 * drhip_sort_workspace(n) + n * val_bytes. */
int drhip_sort_pairs_workspace(int seg, int kdtype, size_t val_bytes, size_t n, size_t *bytes);
int drhip_sort_pairs(int seg, int kdtype, void *keys, void *vals, size_t val_bytes, size_t n, void *tmp,
                     size_t tmp_bytes);
/* drhip_merge_runs_to with a payload: src_keys[0, n) holds nruns sorted runs
 * [run_offsets[r], run_offsets[r+1]) and src_vals the value of every key;
 * dst_keys / dst_vals receive the merged pairs.  STABLE: on equal keys the
 * earlier run goes first and a run keeps its own order, so runs that are
 * stably sorted pieces in source order merge to the stable sort of the whole.
 * Rounds alternate between tmp and dst so that the last one writes dst; a
 * single run, or a run left unpaired in a round, is copied, keys and values
 * alike.  src and dst key- / value-aligned and not overlapping, src
 * unchanged; nruns <= 128; val_bytes 4 or 8; tmp 256-byte aligned with
 * drhip_merge_pairs_workspace bytes (no initialised device needed for the
 * query). */
int drhip_merge_pairs_workspace(int seg, int kdtype, size_t val_bytes, size_t n, int nruns, size_t *bytes);
int drhip_merge_pairs_runs_to(int seg, int kdtype, size_t val_bytes, const void *src_keys, const void *src_vals,
                              void *dst_keys, void *dst_vals, size_t n, const size_t *run_offsets, int nruns,
                              void *tmp, size_t tmp_bytes);

/* ----------------------------------------------------------- select ----
 * copy_if / count_if are absent from the reference (its shp algorithms stop
 * at for_each / reduce / inclusive_scan / gemv); defined with the semantics
 * of std::count_if / std::copy_if: the elements that satisfy the predicate,
 * in input order (stable).  What they replace is a copy of the segment to
 * the host and a host loop.  One single-pass kernel per call (tile ranks by
 * ballots, the tiles' offsets by a decoupled look-back over one 8-byte
 * {status, count} word per tile; include/dr/details/select_kernel.hpp): the
 * input is read once and only the survivors are written.
 * The predicate is `x[i] cmp *scalar_host` with the C++ operator of the
 * element type (the six dtypes), so IEEE rules hold for floats: a NaN passes
 * only DRHIP_NE, and -0.0 == +0.0.  scalar_host (element type) is read
 * during the call.
 * Asynchronous on the segment's stream.  *count (uint64, device-visible:
 * device or pinned host memory, not null) is written by the kernel; with
 * n == 0 it still receives 0 in stream order and nothing else is touched.
 * `out` needs room for the number selected -- a caller who does not know it
 * passes room for n -- and elements of out at or past *count are never
 * written.  out must not overlap in (or flags): DRHIP_ERR_BAD_ARG.  An
 * unknown dtype or cmp, elem_bytes outside {4, 8}, a null pointer with n > 0,
 * a null count and n >= 2^32 (counts are 32-bit inside the kernel) are
 * DRHIP_ERR_BAD_ARG too; the arguments are checked before the segment, so a
 * refusal leaves *count untouched.  The status words live in the segment's
 * workspace, which grows on demand -- not while a graph of the segment is
 * alive or being captured (DRHIP_ERR_UNSUPPORTED, see drhip_graph_begin:
 * warm up with one eager call at the largest n); they are re-zeroed by a
 * memset node before every launch, so a graph replay recomputes everything. */
typedef enum { DRHIP_LT = 0, DRHIP_LE = 1, DRHIP_GT = 2, DRHIP_GE = 3, DRHIP_EQ = 4, DRHIP_NE = 5 } drhip_cmp;
/* *count = |{ i < n : x[i] cmp *scalar_host }| (4 B/elem read, nothing written but *count) */
int drhip_count_if(int seg, int dtype, int cmp, const void *x, size_t n, const void *scalar_host, uint64_t *count);
/* out[0..*count) = the elements of in[0..n) with in[i] cmp *scalar_host, in input order */
int drhip_copy_if(int seg, int dtype, int cmp, const void *in, void *out, size_t n, const void *scalar_host,
                  uint64_t *count);
/* The same with flags[i] != 0 as the predicate (one byte per element, e.g.
 * the mask another kernel left); elements move as bits, elem_bytes = 4 or 8,
 * in and out aligned to elem_bytes. */
int drhip_copy_flagged(int seg, size_t elem_bytes, const void *in, const uint8_t *flags, void *out, size_t n,
                       uint64_t *count);

/* ---------------------------------------------------- reduce by key ----
 * The second half of a sort_by_key pipeline (group-by, combining duplicate
 * COO entries, row counts for a CSR rowptr); absent from the reference,
 * defined with the semantics of thrust::reduce_by_key / std::unique_copy.
 * A run is a maximal stretch of consecutive elements whose neighbouring keys
 * compare equal; element 0 starts a run.  Run r gives keys_out[r] = the bits
 * of the run's FIRST key and vals_out[r] = the fold of the run's values in
 * input order; the outputs are contiguous from the start and nothing at or
 * past index *num_runs is written.  Keys compare with the C++ == of the key
 * type (the six dtypes; IEEE for floats: -0.0 and +0.0 share a run, whose
 * key is the first one's bits, and every NaN key is a run of its own).
 * Values (the six dtypes) fold under DRHIP_PLUS / MUL / MIN / MAX as in
 * drhip_reduce: integers wrap; floats are folded in double, in the tile and
 * between tiles, and the output element is the value dtype, rounded once.
 * The fold may associate differently from a sequential loop but never
 * reorders: it is bit-exact whenever every partial result is representable.
 * One single-pass kernel (include/dr/details/segreduce_kernel.hpp: heads
 * ranked by ballots, only the 32-bit head count crosses workgroups through
 * select's look-back word, a segmented fold inside the tile) and one small
 * fix-up kernel that folds the runs left open at tile boundaries.
 * drhip_run_length_encode is the same kernel with a constant value 1 under
 * PLUS (no value stream is read; n < 2^32, so the counts are 4 bytes inside
 * the kernel and widened at the stores; counts_out is uint64, so a run of
 * any length fits once calls are joined); drhip_unique_copy writes the keys only.
 * Asynchronous on the segment's stream.  *num_runs (uint64, device-visible,
 * not null) is written by the kernel; with n == 0 it still receives 0 in
 * stream order and nothing else is touched.  The outputs need room for the
 * number of runs -- a caller who does not know it passes room for n.
 * DRHIP_ERR_BAD_ARG: an unknown dtype or op, a null pointer with n > 0, a
 * null num_runs, n >= 2^32 (counts are 32-bit inside the kernel), any output
 * overlapping any input (taken over n elements).  The arguments are checked
 * before the segment, so a refusal leaves *num_runs untouched.  The state
 * (tile counter, status words, tile records) lives in the segment's
 * workspace, which grows on demand -- not while a graph of the segment is
 * alive or being captured (DRHIP_ERR_UNSUPPORTED: warm up with one eager call
 * at the largest n, as for drhip_copy_if); it is re-zeroed by a memset node
 * before every launch, so a graph replay recomputes everything. */
int drhip_reduce_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                        void *keys_out, void *vals_out, uint64_t *num_runs);
/* keys_out[r], counts_out[r] = the first key and the length of run r */
int drhip_run_length_encode(int seg, int kdtype, const void *keys_in, size_t n, void *keys_out, uint64_t *counts_out,
                            uint64_t *num_runs);
/* keys_out[r] = the first key of run r */
int drhip_unique_copy(int seg, int kdtype, const void *keys_in, size_t n, void *keys_out, uint64_t *num_runs);

/* ------------------------------------------------------ scan by key -----
 * Absent from the reference; defined as thrust::inclusive_scan_by_key /
 * thrust::exclusive_scan_by_key: every element is kept and receives the
 * running fold of its own run.  A run is what drhip_reduce_by_key calls a
 * run: a maximal stretch of consecutive elements whose neighbouring keys
 * compare equal; element 0 starts one.  For element i of a run starting at s
 *   inclusive: vals_out[i] = v[s] op v[s+1] op ... op v[i]
 *   exclusive: vals_out[i] = init op v[s] op ... op v[i-1], so the first
 *              element of every run receives init.
 * Per-group running totals and running min / max, the rank of an element
 * inside its group (exclusive, PLUS, values all 1), the offset of a COO entry
 * inside its row.  Keys compare with the C++ == of the key type (the six
 * dtypes; IEEE for floats: -0.0 and +0.0 share a run, every NaN key is a run
 * of its own).  Values (the six dtypes) fold under DRHIP_PLUS / MUL / MIN /
 * MAX as in drhip_reduce_by_key: integers wrap; floats are folded in double,
 * in the tile and between tiles, and every output element is the value
 * dtype, rounded once.  The folds run in input order: they may associate
 * differently from a sequential loop but never reorder, and they are
 * bit-exact whenever every partial result is representable.
 * init_host (exclusive only; host memory, one element of the value dtype,
 * read during the call) may be null: the identity of op, as drhip_reduce
 * defines it (0, 1, +inf / the type's maximum, -inf / the type's lowest).
 * One single-pass kernel (include/dr/details/segscan_kernel.hpp): the loads,
 * head flags and in-tile segmented fold of the reduce, and a decoupled
 * look-back over the tiles' {has_head, fold of the open run} summaries in
 * 8-byte self-validating words.  A tile with a head publishes at once, only a
 * tile whose first element continues a run looks back, and the look-back ends
 * at the nearest tile with a head.  sizeof key + 2 sizeof value bytes move per
 * element.  vals_out may be vals_in itself (in place).
 * Asynchronous on the segment's stream.  n == 0 returns DRHIP_OK and touches
 * nothing.  DRHIP_ERR_BAD_ARG: an unknown dtype or op, a null keys_in,
 * vals_in or vals_out with n > 0, n >= 2^32, vals_out overlapping keys_in,
 * vals_out overlapping vals_in in any way other than vals_out == vals_in
 * (ranges taken over n elements).  The arguments are checked before the
 * segment.  The state (tile counter, one status granule per tile) lives in
 * the segment's workspace, which grows on demand -- not while a graph of the
 * segment is alive or being captured (DRHIP_ERR_UNSUPPORTED: warm up with one
 * eager call at the largest n, as for drhip_copy_if); it is re-zeroed by a
 * memset node before every launch, so a graph replay recomputes everything.
 * A look-back that waits past the spin bound sets the segment's error word
 * (DRHIP_ERR_TIMEOUT at drhip_sync). */
int drhip_inclusive_scan_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                                void *vals_out);
int drhip_exclusive_scan_by_key(int seg, int kdtype, int vdtype, int op, const void *keys_in, const void *vals_in, size_t n,
                                const void *init_host, void *vals_out);

/* ----------------------------------------------------------- search ----
 * The algorithms that answer a question about a range with a position:
 * std::find_if, std::is_sorted_until, std::mismatch, std::min_element,
 * std::max_element, std::minmax_element.  Absent from the reference; what
 * they replace is a copy of the segment to the host and a host loop.
 * Kernels: include/dr/details/search_kernel.hpp.
 * First match (find_if, is_sorted_until, mismatch): the answer is the least
 * matching index, exactly, whatever order the workgroups run in; a workgroup
 * stops reading once a match below its next tile is recorded, so a match at
 * position p costs about p / n of a full pass.  drhip_find_if's predicate is
 * `x[i] cmp *scalar_host` as in drhip_count_if (IEEE for floats: a NaN passes
 * only DRHIP_NE, -0.0 == +0.0); scalar_host (element type) is read during the
 * call.
 * Extrema compare with the C++ < of the element type; among equal elements
 * the FIRST wins, except the maximum of drhip_minmax_element, where the LAST
 * wins (std::minmax_element).  -0.0 and +0.0 are equal.  A NaN in an extremum
 * or sortedness input gives an unspecified index.
 * Asynchronous on the segment's stream.  index / idx2 (uint64, device-visible:
 * device or pinned host memory, not null) are written by a kernel in stream
 * order; with n == 0 they still receive 0 and nothing else is touched.
 * DRHIP_ERR_BAD_ARG: an unknown dtype or cmp, a null pointer with n > 0, a
 * null index and n >= 2^32 (positions are 32-bit inside the kernels); the
 * arguments are checked before the segment, so a refusal leaves *index
 * untouched.  The state (the result word; the workgroups' candidates) lives
 * in the segment's workspace, which grows on demand -- not while a graph of
 * the segment is alive or being captured (DRHIP_ERR_UNSUPPORTED: warm up with
 * one eager call, as for drhip_copy_if); the result word is reset by a memset
 * node before every launch, so a graph replay recomputes everything. */
/* least i with x[i] cmp *scalar_host (drhip_cmp, IEEE rules as drhip_count_if); n if none */
int drhip_find_if(int seg, int dtype, int cmp, const void *x, size_t n, const void *scalar_host, uint64_t *index);
/* least i >= 1 with x[i] < x[i-1] (std::is_sorted_until under std::less); n if sorted or n < 2 */
int drhip_is_sorted_until(int seg, int dtype, const void *x, size_t n, uint64_t *index);
/* least i with a[i] != b[i]; n if none */
int drhip_mismatch(int seg, int dtype, const void *a, const void *b, size_t n, uint64_t *index);
/* first least / first greatest element under operator<; n (= 0) when n == 0 */
int drhip_min_element(int seg, int dtype, const void *x, size_t n, uint64_t *index);
int drhip_max_element(int seg, int dtype, const void *x, size_t n, uint64_t *index);
/* idx2[0] = first least, idx2[1] = LAST greatest (std::minmax_element), one read of x */
int drhip_minmax_element(int seg, int dtype, const void *x, size_t n, uint64_t *idx2);

/* ---------------------------------------------------- sorted search ----
 * std::lower_bound, std::upper_bound and std::binary_search of a batch of m
 * needles in a haystack of n elements sorted under the C++ < of the element
 * type (what drhip_sort leaves behind; -0.0 and +0.0 are equal, +-inf are
 * ordinary values).  Absent from the reference; what they replace is a copy
 * of the segment to the host and a host loop.
 * Kernel: include/dr/details/bsearch_kernel.hpp.
 *   pos[i]   = the least p in [0, n] with !(hay[p] < needles[i])  (lower)
 *            = the least p in [0, n] with needles[i] < hay[p]     (upper)
 *   found[i] = 1 if some hay[p] is neither below nor above needles[i], else 0
 * A NaN in the haystack or the needles, or a haystack that is not sorted,
 * gives unspecified results; every pos[i] is still in [0, n], every found[i]
 * in {0, 1} and no read leaves hay[0, n): a search is a loop of fixed trip
 * count over clamped indices, never a data-dependent walk.
 * Every workgroup first copies DRHIP_SORTED_SEARCH_STAGE(element bytes) evenly
 * spaced haystack elements to LDS and resolves the top levels of every search
 * there; with m below that number the staging is skipped.
 * Asynchronous on the segment's stream.  hay and needles: n and m elements of
 * dtype; pos: m uint64, found: m uint8; all device-visible.  m == 0 returns
 * DRHIP_OK and touches nothing; n == 0 with m > 0 writes m zeros.
 * DRHIP_ERR_BAD_ARG: an unknown dtype, a null hay with n > 0, null needles or
 * output with m > 0, n >= 2^32 or m >= 2^32, and an output that overlaps hay
 * or needles (their full extents); the arguments are checked before the
 * segment, so a refusal leaves the output untouched.
 * The kernel keeps NO state in the segment's workspace: it reads hay and
 * needles and writes the output, nothing else.  A call can therefore be
 * captured between drhip_graph_begin and drhip_graph_end without an eager
 * warm-up call, and a replay recomputes everything from the buffers'
 * contents at that time. */
#define DRHIP_SORTED_SEARCH_STAGE(elem_bytes) ((elem_bytes) <= 4 ? 8192 : 8192)
int drhip_lower_bound(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint64_t *pos);
int drhip_upper_bound(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint64_t *pos);
int drhip_binary_search(int seg, int dtype, const void *hay, size_t n, const void *needles, size_t m, uint8_t *found);

/* ------------------------------------------------------------ merge ----
 * std::merge of two ranges sorted under the C++ < of the element type (what
 * drhip_sort leaves behind; NOT radix order: -0.0 and +0.0 are a tie, +-inf
 * are ordinary values), optionally carrying one value per key
 * (thrust::merge_by_key).  Absent from the reference; what it replaces is a
 * concatenation and another drhip_sort.
 * Kernel: include/dr/details/merge_kernel.hpp.
 *   out[d] = element d of the stable merge of a[0, na) and b[0, nb): on ties
 *   a's element comes first (so a's zero precedes b's whatever their signs)
 *   and each input keeps its own order.  drhip_merge_pairs moves the value
 *   of every key with it, as val_bytes (4 or 8) opaque bytes.
 * The output is cut into tiles of DRHIP_MERGE_TILE(element bytes) elements;
 * persistent workgroups take contiguous runs of tiles, find each tile's split
 * on the merge path themselves (a wave-wide search of global memory), stage
 * the two pieces in LDS and merge them there.
 * A NaN, or an input that is not sorted, gives unspecified output values; the
 * searches are bounded loops over indices that cannot leave their interval,
 * so no read leaves a[0, na) or b[0, nb) and exactly out[0, na + nb) is
 * written, each element once.
 * Asynchronous on the segment's stream.  All buffers device-visible.
 * na + nb == 0 returns DRHIP_OK and touches nothing; with one input empty
 * the call is a copy of the other.
 * DRHIP_ERR_BAD_ARG: an unknown dtype, val_bytes outside {4, 8}, a null
 * pointer with a non-zero length, na + nb >= 2^32, and any output that
 * overlaps any input or the other output (their full extents); the arguments
 * are checked before the segment, so a refusal leaves the outputs untouched.
 * The kernel keeps NO state in the segment's workspace: no partition array,
 * no counters.  A call can therefore be captured between drhip_graph_begin
 * and drhip_graph_end without an eager warm-up call, and a replay recomputes
 * everything from the buffers' contents at that time. */
#define DRHIP_MERGE_TILE(elem_bytes) ((elem_bytes) <= 4 ? 2048 : 2048)
int drhip_merge(int seg, int dtype, const void *a, size_t na, const void *b, size_t nb, void *out);
int drhip_merge_pairs(int seg, int kdtype, const void *a_keys, const void *a_vals, size_t na,
                      const void *b_keys, const void *b_vals, size_t nb, size_t val_bytes,
                      void *out_keys, void *out_vals);

/* ---------------------------------------------------------- stencil ----
 * mhp::transform of a radius-r 1-D stencil over a halo'd segment
 * (mhp/algorithms/cpu_algorithms.hpp:147-161 with the ops of
 * examples/mhp/stencil-1d.cpp:16-19): buffers are [r halo | owned | r halo];
 * for lo <= i < hi:  out[r+i] = sum_{d=-r..r} in[r+i+d].  I32 (wrapping)
 * and F32. */
int drhip_stencil1d(int seg, int dtype, const void *in_buf, void *out_buf, size_t n_owned,
                    int radius, size_t lo, size_t hi);
/* 5-point 2-D stencil on a row block with one halo row above and below:
 * buffers are (rows+2) x nx, row-major; for owned rows r in [rlo, rhi) and
 * columns 1..nx-2:  out = c + n + s + e + w. */
int drhip_stencil2d(int seg, int dtype, const void *in_buf, void *out_buf, size_t nx,
                    size_t rows, size_t rlo, size_t rhi);

/* ------------------------------------------------- RCCL over xGMI -------
 * The reference's cross-rank layer is MPI (mhp communicator,
 * include/dr/details/communicator.hpp:51-56 gather, :97-149 isend/irecv;
 * halo exchange details/halo.hpp:55-137) and, inside shp, peer USM copies.
 * Here every segment may own ONE RCCL communicator; calls are enqueued on
 * the segment's stream (asynchronous, like every other drhip call).
 *   multi-process (one rank per GPU, the mhp model, bench.py at N > 1):
 *     rank 0 drhip_comm_unique_id -> broadcast the 128 bytes by any channel
 *     (MPI_Bcast, torch.distributed store) -> every rank
 *     drhip_comm_init_rank(seg, nranks, rank, id);
 *   single process, many devices (the shp model): drhip_comm_init_all()
 *     builds one communicator per segment (distinct devices only), and a
 *     collective over all segments is issued between
 *     drhip_comm_group_start() / drhip_comm_group_end(). */
#define DRHIP_COMM_ID_BYTES 128
int drhip_comm_unique_id(void *id /* DRHIP_COMM_ID_BYTES */);
int drhip_comm_init_rank(int seg, int nranks, int rank, const void *id);
int drhip_comm_init_all(void);
int drhip_comm_destroy(int seg);
int drhip_comm_rank(int seg, int *rank, int *nranks);
int drhip_comm_group_start(void);
int drhip_comm_group_end(void);
/* shp::reduce partial fold (reduce.hpp:81-83) / scan totals: elementwise
 * allreduce of n values of dtype with op (+, *, min, max). */
int drhip_allreduce(int seg, int dtype, int op, const void *send, void *recv, size_t n);
/* gemv.hpp:30-42 x replication, scan carries, sort samples: recv holds
 * nranks blocks of `bytes` in rank order. */
int drhip_allgather(int seg, const void *send, void *recv, size_t bytes);
/* mhp gather to root (communicator.hpp:51-56, mhp reduce cpu_algorithms.hpp:102-140). */
int drhip_gather(int seg, const void *send, void *recv, size_t bytes, int root);
/* sort exchange: byte counts and offsets per peer; grouped
 * point-to-point sends/receives, zero-byte pairs skipped. */
int drhip_alltoallv(int seg, const void *send, const size_t *send_bytes, const size_t *send_off, void *recv,
                    const size_t *recv_bytes, const size_t *recv_off);
/* lib::span_halo exchange (details/halo.hpp:336-387): buf is
 * [prev halo | owned | next halo] in cells of cell_bytes (a 2-D row block
 * passes one row as a cell).  Sends the first `prev` owned cells to rank-1
 * (tag halo_reverse) and the last `next` owned cells to rank+1 (halo_forward);
 * receives rank-1's into the prev halo and rank+1's into the next halo; ends
 * are skipped unless periodic.  The reference's message pattern only pairs
 * up when prev == next (a send of `prev` cells lands in the neighbour's
 * `next`-cell halo), so prev != next is rejected. */
int drhip_halo_exchange(int seg, void *buf, size_t n_owned, size_t cell_bytes, size_t prev, size_t next,
                        int periodic);

/* ---------------------------------------- flag exchange (no collective) ----
 * The combine of a strong-scaled reduce + inclusive_scan step -- every rank
 * needs the w segment results in segment order (reduce.hpp:81-83,
 * inclusive_scan.hpp:108-116) -- as stores into peers' slots plus a flag
 * instead of an RCCL all_gather.  A rank allocates its slot
 * array (fine-grained device memory, drhip_xchg_alloc), every rank maps
 * every other rank's array (the same pointers in one process with peer
 * access; drhip_ipc_handle / drhip_ipc_open across processes) and
 * drhip_xchg_allgather (one 1-block kernel on seg's stream) posts the
 * value_bytes (4 or 8) at *value (device memory, e.g. drhip_reduce_tiles'
 * ACC result) into slot `rank` of every array and waits until all w values
 * of this exchange have arrived in its own, writing them to gathered[0..w)
 * (value_bytes each) in rank order -- the partials argument of
 * drhip_inclusive_scan_tiles.  Exchanges are counted
 * on the device (graph replays included), so every rank must make the same
 * sequence of exchanges on the same arrays.  peer_slots is a host array of
 * w device pointers with peer_slots[rank] == local_slots.  The w exchange
 * kernels must be able to run at the same time: one participant per device
 * or per process.  Segments that share a device inside one process do not
 * qualify -- the HIP runtime multiplexes their streams onto a few hardware
 * queues, so one segment's waiting kernel can sit in front of another's post
 * (8 duplicated segments hit the spin bound, round 5).  A wait past the
 * spin bound (1-2 s) sets the segment's error word:
 * drhip_sync returns DRHIP_ERR_TIMEOUT. */
#define DRHIP_IPC_HANDLE_BYTES 64
int drhip_xchg_bytes(int w, size_t *bytes);
int drhip_xchg_alloc(int seg, int w, void **slots);
int drhip_xchg_free(int seg, void *slots);
int drhip_xchg_allgather(int seg, void *local_slots, void *const *peer_slots, int w, int rank, const void *value,
                         int value_bytes, void *gathered);
/* Cross-process mapping of device memory (hipIpcGetMemHandle /
 * hipIpcOpenMemHandle): handle is DRHIP_IPC_HANDLE_BYTES of opaque bytes. */
int drhip_ipc_handle(const void *dev_ptr, void *handle);
int drhip_ipc_open(int seg, const void *handle, void **dev_ptr);
int drhip_ipc_close(int seg, void *dev_ptr);

#ifdef __cplusplus
}
#endif
#endif /* DRHIP_H */

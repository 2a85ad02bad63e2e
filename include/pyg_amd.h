/*
 * pyg_amd.h — C ABI of the MI355X (gfx950) message-passing / aggregation backend.
 *
 * This header is the drop-in boundary.  The reference (PyG 2.9, pure Python) has no C ABI of its
 * own; its native seam is the set of `torch.ops.torch_sparse.*`, `torch_scatter.*` and
 * `pyg_lib.ops.*` symbols it *expects to exist* (SURVEY.md §2.3, §8(b) S2).  Every entry point
 * below names the reference call site (file:line under the reference root) it replaces.
 *
 * Conventions
 *   - plain pointers and sizes only; every pointer is a DEVICE pointer unless marked [host];
 *   - `stream` is a `hipStream_t` passed as `void*` (NULL = the null stream); every call is
 *     asynchronous on that stream unless marked [sync];
 *   - index tensors are int32 or int64, selected by `idx_dtype` (PYGAMD_IDX_I32 / _I64) — the
 *     reference accepts both (torch_geometric/typing.py:32-36);
 *   - features are fp32, row-major, with an explicit leading dimension in ELEMENTS
 *     (`ldx`, `ldo` ≥ F) so callers can aggregate in/out of wider buffers without copies;
 *   - every function returns a pygamd_status (0 = ok).  No function allocates device memory:
 *     workspaces are passed in, their size comes from the matching `*_workspace_bytes` query;
 *   - outputs never alias inputs.
 */
#ifndef PYG_AMD_H
#define PYG_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PYGAMD_API __attribute__((visibility("default")))

#define PYGAMD_ABI_VERSION 11

typedef enum {
  PYGAMD_OK = 0,
  PYGAMD_ERR_INVALID_ARG = 1,   /* bad size / dtype / NULL pointer                     */
  PYGAMD_ERR_UNSUPPORTED = 2,   /* valid in the reference but not implemented natively */
  PYGAMD_ERR_WORKSPACE = 3,     /* workspace too small                                 */
  PYGAMD_ERR_HIP = 4            /* a HIP runtime call failed (see pygamd_last_hip_error) */
} pygamd_status;

typedef enum { PYGAMD_IDX_I32 = 0, PYGAMD_IDX_I64 = 1 } pygamd_idx_dtype;

/* layout of the gathered block of an aggregation (pygamd_spmm_args.x_format) */
typedef enum { PYGAMD_X_DENSE = 0, PYGAMD_X_COMPRESSED = 1 } pygamd_x_format;

/* reduce ids follow torch_geometric/utils/_scatter.py:14-138 */
typedef enum {
  PYGAMD_SUM = 0,
  PYGAMD_MEAN = 1,
  PYGAMD_MIN = 2,
  PYGAMD_MAX = 3,
  PYGAMD_MUL = 4,
  PYGAMD_ANY = 5
} pygamd_reduce;

/* ---- library info ------------------------------------------------------------------------- */
PYGAMD_API int pygamd_abi_version(void);
PYGAMD_API const char* pygamd_status_string(int status);
PYGAMD_API int pygamd_last_hip_error(void);          /* hipError_t of the last failing call */
PYGAMD_API const char* pygamd_build_arch(void);      /* "gfx950" */

/* ---- a12: index_sort ------------------------------------------------------------------------
 * Replaces `pyg_lib.ops.index_sort(inputs, max_value)` / `inputs.sort(stable=True)`
 * (torch_geometric/utils/_index_sort.py:10-32).  Stable LSD radix sort of non-negative integer
 * keys; `perm_out` (always int64, like torch.sort's indices) satisfies
 * keys_out[i] == keys_in[perm_out[i]] and is bit-identical to a stable sort.
 * `max_value` (>= every key, or <0 = unknown) bounds the radix passes (8 bits each; own kernels,
 * csrc/graph.hip).  Out of place (keys_in != keys_out), n < 2^32.                              */
PYGAMD_API int pygamd_index_sort_workspace_bytes(int idx_dtype, int64_t n, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_index_sort(const void* keys_in, int idx_dtype, int64_t n, int64_t max_value,
                                 void* keys_out, int64_t* perm_out, void* workspace,
                                 size_t workspace_bytes, void* stream);

/* ---- a11: index2ptr / ptr2index -------------------------------------------------------------
 * `torch._convert_indices_from_coo_to_csr(index, size)` and
 * `arange(n).repeat_interleave(ptr.diff())` (torch_geometric/index.py:27-37).
 * `index` must be sorted ascending with values in [0, size).  ptr has size+1 entries.          */
PYGAMD_API int pygamd_index2ptr(const void* index, int idx_dtype, int64_t n, int64_t size,
                                void* ptr_out, void* stream);
PYGAMD_API int pygamd_ptr2index(const void* ptr, int idx_dtype, int64_t size, int64_t n,
                                void* index_out, void* stream);

/* Range check used by maybe_num_nodes / _index_select_safe
 * (torch_geometric/utils/num_nodes.py, nn/conv/message_passing.py:269-290).
 * Writes {min, max} (int64) to `minmax_out` (device, 2 entries); n == 0 gives {INT64_MAX, -1}. */
PYGAMD_API int pygamd_index_minmax(const void* index, int idx_dtype, int64_t n,
                                   int64_t* minmax_out, void* stream);

/* out[i] = src[perm[i]] for integer payloads (COO -> CSR column permutation,
 * torch_geometric/edge_index.py:605-623).  perm is int64.                                      */
PYGAMD_API int pygamd_permute_index(const void* src, int idx_dtype, const int64_t* perm,
                                    int64_t n, void* out, void* stream);
/* out[i] = (idx_dtype) perm[i]; narrows an int64 permutation to the graph's index dtype.      */
PYGAMD_API int pygamd_cast_index(const int64_t* src, int64_t n, int idx_dtype, void* out,
                                 void* stream);

/* out[i] = index[i] if 0 <= index[i] < size, else `size` (a sentinel group behind the last real
 * one); *err (device int32, may be NULL) is set to 1 when any entry was replaced.  The sorted route
 * of a large unsorted `scatter` (torch_geometric/utils/_scatter.py:68-100) sorts these keys, so an
 * out-of-range index can neither corrupt the plan nor cost a blocking min / max read: such rows
 * fall behind the last group and are skipped — as the atomic kernels skip them — and the flag
 * travels to the host as theirs does (ABI 9).  `out` has `out_dtype` (int32 needs
 * size < 2^31: narrower keys sort in fewer bytes), out != index.                               */
PYGAMD_API int pygamd_index_guard(const void* index, int idx_dtype, int64_t n, int64_t size,
                                  void* out, int out_dtype, int32_t* err, void* stream);

/* out[i] = in[0] + ... + in[i] over int32 / int64 counts: `torch.cumsum(x, 0)` where the
 * reference builds offsets from counts (torch_geometric/utils/functions.py:5-26 `cumsum`,
 * utils/_coalesce.py:186, the samplers' per-hop offsets).  `out` may be `in`.  One launch up to
 * 32 k elements, three above.  The sum must fit the dtype.                                    */
PYGAMD_API int pygamd_cumsum_workspace_bytes(int idx_dtype, int64_t n, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_cumsum(const void* in, int idx_dtype, int64_t n, void* out, void* workspace,
                             size_t workspace_bytes, void* stream);

/* ---- (f)-4: sort_edge_index / coalesce (torch_geometric/utils/_sort_edge_index.py:105-113,
 * utils/_coalesce.py:131-176).  Like the reference, both sort the compound key
 * major * num_nodes + minor (major = row when by_row) with index_sort; these entry points build
 * the keys, flag the first entry of every run of equal sorted keys, and decode sorted keys back
 * into (row, col) — compacted to one entry per run when `scan` (the inclusive scan of the run
 * flags) is given, in which case gid_orig[perm[i]] (perm == NULL: gid_orig[i]) receives the run
 * slot of every original edge so that edge attributes can be merged with one scatter.
 * num_nodes^2 must fit int64 (the reference raises the same condition, _coalesce.py:134-135).   */
PYGAMD_API int pygamd_edge_key(const void* row, const void* col, int idx_dtype, int64_t E,
                               int64_t num_nodes, int by_row, int64_t* key_out, void* stream);
PYGAMD_API int pygamd_run_flags(const int64_t* key_sorted, int64_t E, int64_t* flag_out,
                                void* stream);
PYGAMD_API int pygamd_edge_unkey(const int64_t* key_sorted, const int64_t* scan,
                                 const int64_t* perm, int64_t E, int64_t num_nodes, int by_row,
                                 int idx_dtype, void* out_row, void* out_col, int64_t* gid_orig,
                                 void* stream);

/* ---- a10: hub plan for a CSR handle ---------------------------------------------------------
 * Rows with more than `threshold` stored entries ("hubs", power-law graphs) are split into
 * chunks of `chunk` entries so no single wavefront walks an unbounded row.  Produces, in
 * ascending row order, hub_rows[n_hub] and hub_chunk_ptr[n_hub+1] (exclusive scan of the chunk
 * counts).  Capacity of both outputs is `cap` (+1).  [sync]: n_hub / n_chunks are returned to
 * the host.  No reference equivalent (the reference never splits rows); internal to a10's cache
 * (torch_geometric/edge_index.py:677-696).                                                     */
PYGAMD_API int pygamd_hub_plan_workspace_bytes(int idx_dtype, int64_t n_rows, size_t* bytes);
PYGAMD_API int pygamd_hub_plan(const void* rowptr, int idx_dtype, int64_t n_rows,
                               int64_t threshold, int64_t chunk, void* hub_rows,
                               void* hub_chunk_ptr, int64_t cap, int64_t* n_hub_out /*[host]*/,
                               int64_t* n_chunks_out /*[host]*/, void* workspace,
                               size_t workspace_bytes, void* stream);

/* A CSR handle with its hub plan: what the one-pass kernels (pygamd_gatv2_*, pygamd_transformer_*,
 * pygamd_gine_*, pygamd_pna_*, pygamd_gen_*, pygamd_resgated_*) walk, one wave per row.  Row r
 * owns the slots [rowptr[r], rowptr[r + 1]) and col[k] is the row of the OTHER side that slot k
 * reads; a by-destination handle has the destinations as rows, a by-source handle (the `_src` /
 * GINE, PNA, GEN backward passes) the sources.
 * Rows of more than hub_threshold slots are walked as the plan's chunks of hub_chunk slots and
 * their partial results merged in chunk order; n_hub == 0 means that no row is split (the hub
 * pointers are then ignored and n_chunks must be 0).  The plan must come from pygamd_hub_plan on
 * this rowptr with the same threshold and chunk.  All index arrays share idx_dtype.            */
typedef struct pygamd_csr {
  const void* rowptr;        /* [n_rows + 1]                         */
  const void* col;           /* [nnz]                                */
  int32_t idx_dtype;         /* PYGAMD_IDX_I32 | PYGAMD_IDX_I64      */
  int32_t reserved0;         /* 0 */
  int64_t n_rows;
  const void* hub_rows;      /* [n_hub] or NULL                      */
  const void* hub_chunk_ptr; /* [n_hub + 1] or NULL                  */
  int64_t n_hub;
  int64_t n_chunks;
  int64_t hub_threshold;
  int64_t hub_chunk;
} pygamd_csr;

/* ---- a9/a13/a14: CSR SpMM (fused gather -> message -> segmented reduce) ---------------------
 * Replaces torch.ops.torch_sparse.spmm_{sum,mean,min,max}
 * (torch_geometric/edge_index.py:1798-1810) and the unfused
 * index_select -> message -> scatter chain of MessagePassing.propagate
 * (nn/conv/message_passing.py:421-563, utils/_scatter.py:68-80):
 *
 *   out[i, f] = post(i) * REDUCE_{k in [rowptr[i], rowptr[i+1])}
 *                   m(k, f) * x[col[k], f]
 *   m(k, f)  = (w ? w[e(k) * w_heads + f / head_dim] : 1) * (src_scale ? src_scale[col[k]] : 1)
 *   e(k)     = eid ? eid[k] : k
 *   post(i)  = reduce == MEAN ? 1 / max(deg(i), 1) : 1
 *
 * `col == NULL` means col[k] = k (segment reduce over contiguous rows: torch_scatter.segment_csr,
 * torch_geometric/utils/_segment.py:11-50).  Empty rows give 0 for every reduce.
 * For MIN/MAX `arg_out` (optional, same idx dtype, [n_rows, ldo]) receives the winning slot k
 * (first on ties) or -1 for an empty row; w/src_scale must be NULL.
 * The hub_* arrays come from pygamd_hub_plan (n_hub == 0: no splitting); `workspace` must hold
 * n_chunks * F floats (pygamd_spmm_csr_workspace_bytes).  Per-row accumulation order is the
 * slot order (deterministic; no atomics).                                                      */
typedef struct {
  const void* rowptr;        /* [n_rows + 1]                         */
  const void* col;           /* [nnz] or NULL                        */
  const void* eid;           /* [nnz] or NULL                        */
  const float* w;            /* [n_edges, w_heads] or NULL           */
  const float* src_scale;    /* [n_src] or NULL                      */
  const float* x;            /* [n_src, ldx]                         */
  float* out;                /* [n_rows, ldo]                        */
  void* arg_out;             /* [n_rows, ldo] or NULL (MIN/MAX only) */
  int64_t n_rows;
  int64_t n_src;
  int64_t F;
  int64_t ldx;
  int64_t ldo;
  int32_t idx_dtype;
  int32_t reduce;            /* PYGAMD_SUM | MEAN | MIN | MAX        */
  int32_t w_heads;           /* >= 1                                 */
  int32_t head_dim;          /* F / w_heads when w_heads > 1         */
  const void* hub_rows;      /* [n_hub] or NULL                      */
  const void* hub_chunk_ptr; /* [n_hub + 1] or NULL                  */
  int64_t n_hub;
  int64_t n_chunks;
  int64_t hub_threshold;
  int64_t hub_chunk;
  int32_t accumulate;        /* SUM/MEAN only: out += result (fused "x_root + aggregate") */
  int32_t hub_phase;         /* 0: rows + hubs; 1: non-hub rows only; 2: hub rows only (lets a
                                caller run row ranges as separate launches and the hubs once)  */
  int32_t* arg32_out;        /* MIN/MAX only, [n_rows, F] contiguous or NULL: per output the slot
                                OFFSET inside its row of the attaining neighbour (>= 0) when it
                                is the unique extremum; -1 for an empty row; -2 when the
                                gradient must be split (ties, or an extremum of exactly 0, which
                                ties with the zero-initialised output of the reference's
                                scatter_reduce_).  What pygamd_spmm_csr_minmax_backward_arg
                                consumes.                                                       */
  const float* relu_mask;    /* SUM/MEAN only, [n_rows, ld_mask] or NULL: the final value of
                                out[i, f] (after `accumulate`) is replaced by 0 where
                                relu_mask[i, f] <= 0 — aten::threshold_backward of the ReLU whose
                                OUTPUT relu_mask is, applied as the epilogue of the transposed
                                aggregation that produces that activation's gradient
                                (nn/models/basic_gnn.py:262-263 backward)                        */
  int64_t ld_mask;
  const uint32_t* relu_bits; /* the same mask as one BIT per element (32 x less to read), in
                                tiles of 32 rows x 32 columns: bit (f & 31) of word
                                relu_bits[((i >> 5) * ld_bits + (f >> 5)) * 32 + (i & 31)] is set
                                where the activation [i, f] is positive (the 32 words of a tile are
                                one 128-byte line: the producer's wave writes it with one store).
                                What pygamd_sage_layer_forward writes next to its output.  At most
                                one of relu_mask / relu_bits.                                      */
  int64_t ld_bits;           /* column blocks per row tile, >= ceil(F / 32); the array holds
                                ceil(n_rows / 32) * ld_bits * 32 words                             */
  const uint32_t* src_bits;  /* SUM/MEAN without w / src_scale (ignored with col == NULL, where
                                every row is read once anyway); NULL or one bit per
                                SOURCE row (bit j & 31 of word j >> 5, ceil(n_src / 32) words):
                                a clear bit promises that x[j, :] is all zero, and the row is not
                                read.  What pygamd_rows_pack writes.  The case: the gradient of a
                                loss taken on a training split (`out[train_idx]`, 8 % of the rows
                                of ogbn-products) entering the transposed aggregation of the last
                                layer — the reference gathers every zero row
                                (index_select on the full [E] index, message_passing.py:283-292)   */
  const int64_t* src_bits_set; /* NULL or a DEVICE counter of the set bits: with more than half of
                                the n_src rows live the kernel ignores src_bits (the lookup then
                                costs more than it saves) — decided on the device, no host sync    */
  int32_t x_format;          /* PYGAMD_X_DENSE (0), or PYGAMD_X_COMPRESSED: `x` is the block written
                                by pygamd_rows_compress / pygamd_sage_layer_fused.compressed_out
                                ([n_src, ldx] 32-bit words, F <= 256, F % 4 == 0, F + 12 <= ldx
                                < 2^30, n_src < 2^32); SUM/MEAN without w / src_scale /
                                src_bits, with or without rowend; same sums, bit for bit, as the
                                dense rows.  pygamd_sage_layer_fused takes it on both schedules
                                (the split schedule for F > 128, the fp32 one otherwise)          */
  int32_t reserved0;         /* 0 */
  const void* rowend;        /* NULL, or [n_rows]: the slots of row r are [rowptr[r], rowend[r])
                                instead of [rowptr[r], rowptr[r + 1]) — rows that own fixed-stride,
                                partly filled slot blocks (a sampled batch at its static fan-out
                                capacity: pygamd_sample_slots), or the live-source lists of
                                pygamd_live_lists_build.  SUM / MEAN, dense or compressed rows;
                                also honoured by pygamd_sage_layer_fused.  With a hub plan or with src_bits: plain
                                SUM only (no w / src_scale), every hub row must carry rowend[r] ==
                                rowptr[r + 1] (the hub kernels read rowptr alone), and with
                                src_bits rowptr has n_rows + 1 entries and the lists hold live
                                sources only (hub rows excepted: their bits are still looked up).  */
  int64_t accumulate_rows;   /* with accumulate: only rows < accumulate_rows have an old value, the
                                others start from 0 (0 = every row) — the root gradient of a
                                sampled layer exists for its destination rows only.  No hubs.   */
} pygamd_spmm_args;

/* Lossless compression of a [n_rows, F <= 256] block with many exact zeros (the output of a ReLU)
 * for the row GATHER of the next aggregation, whose cost on this chip is proportional to the
 * 128-byte lines a row touches (scripts/gather_lines_probe.py): row i of `out` (32-bit words, row
 * pitch ld_out >= F + 12; 288 for F = 256) = [8 mask words | the kept values in column order],
 * bit (c & 31) of mask word (c >> 5) set where x[i, c] is kept = has a bit pattern other than
 * +0.0 (-0.0 and NaN are kept).  Words past the last kept value are unspecified.  A half-empty
 * 256-float row then occupies 4.4 lines instead of 8.  Consumed by pygamd_spmm_csr /
 * pygamd_sage_layer_fused with x_format = PYGAMD_X_COMPRESSED; pygamd_sage_layer_fused writes the
 * same format from its epilogue (compressed_out).  The reference keeps activations dense
 * (nn/models/basic_gnn.py:262-263).                                                              */
PYGAMD_API int pygamd_rows_compress(const float* x, int64_t ldx, int64_t n_rows, int64_t F,
                                    uint32_t* out, int64_t ld_out, void* stream);
/* The same block of x[i, c] * row_scale[i] (row_scale: [n_rows] or NULL = pygamd_rows_compress):
 * one fp32 multiply per element, the value a dgrad epilogue writes into its row-scaled copy — the
 * 1/deg-scaled gradient rows that the one-launch input gradient of a mean layer gathers, without
 * the dense scaled copy in between.                                                              */
PYGAMD_API int pygamd_rows_compress_scaled(const float* x, int64_t ldx, int64_t n_rows, int64_t F,
                                           const float* row_scale, uint32_t* out, int64_t ld_out,
                                           void* stream);

/* Row-sparsity of a gradient block, found in the pass that lays it out for the backward of a
 * transform-then-aggregate layer: for every row i < n_rows of g ([n_rows, ldg], F columns)
 *   row_bits bit i   = [g[i, :] has an entry != 0]  (NaN counts; ceil(n_rows / 32) words, the
 *                      bits past n_rows are clear);
 *   scaled[i, f]     = g[i, f] * row_scale[i] (row_scale NULL: 1) for f < F, 0 for F <= f <
 *                      F_scaled (scaled NULL: skipped);
 *   copy[i, f]       = g[i, f] for f < F, 0 for F <= f < F_copy (copy NULL: skipped);
 *   *n_set           = the number of set bits (device int64, NULL: skipped; zeroed here).
 * `scaled` / `copy` may not alias g.  One read of g; replaces aten::mul + aten::copy_ + two fills
 * in the backward of the 256 -> 47 output layer and feeds pygamd_spmm_args.src_bits.             */
PYGAMD_API int pygamd_rows_pack(const float* g, int64_t ldg, int64_t n_rows, int64_t F,
                                const float* row_scale, float* scaled, int64_t ld_scaled,
                                int64_t F_scaled, float* copy, int64_t ld_copy, int64_t F_copy,
                                uint32_t* row_bits, int64_t* n_set, void* stream);

/* Live-source lists of a CSR handle: the stored lists with the entries that point at a dead source
 * row moved out of the way, for the sums whose source is known to be zero in those rows (the
 * backward of a loss taken on a training split: the same rows every step).  Kept by the caller in
 * persistent buffers and walked through pygamd_spmm_args.col / .rowend; built and revalidated on
 * the device, with no read-back:
 *
 *   pygamd_live_lists_flag   *flag = [bits differs from stored] (n_src bits, the layout of
 *       pygamd_rows_pack.row_bits; the bits past n_src are ignored), or 1 when `force`; `stored`
 *       then receives `bits`.
 *   pygamd_live_lists_build  returns at once, in every workgroup, when *flag == 0.  Otherwise, with
 *       live(c) = bit c of `live` | bit c of `live2` (live2 NULL: no second bitmap):
 *         - a row of at most hub_threshold entries (every row when hub_threshold == 0):
 *           col_live[rowptr[r] .. rowend_live[r]) = the entries of col[rowptr[r] .. rowptr[r + 1])
 *           with live(col[k]), in stored order; the slots behind them hold the row's other
 *           entries (valid column ids, order unspecified);
 *         - a longer row (a hub of the handle's plan) is copied whole, rowend_live[r] =
 *           rowptr[r + 1]: the plan, its chunk offsets and the `deg > hub_threshold` test of the
 *           row kernels classify every row as they do on the stored lists;
 *         - with n_set given and 2 * *n_set >= n_src (a dense bitmap: the test pygamd_spmm_csr
 *           makes on src_bits_set) every row is copied whole;
 *         - row_has_live (NULL: skipped; ceil(n_rows / 32) words, same layout) bit r = [some
 *           entry of row r is live], hub rows included.
 *       col_live / rowend_live may both be NULL (only row_has_live is wanted).  Plain stores, one
 *       wave per 8 rows, 64 entries at a time (ballot / mbcnt compaction).
 *   pygamd_live_lists_builds [sync] the number of pygamd_live_lists_build launches that ran for
 *       real on this device since the library was loaded (tests).
 * A sum that walks the live lists adds the same values in the same order as one that skips the
 * dead rows of the stored lists; a dead row that is NOT zero (non-finite weights upstream) is
 * skipped all the same.  No reference equivalent.                                                 */
PYGAMD_API int pygamd_live_lists_flag(const uint32_t* bits, uint32_t* stored, int64_t n_src,
                                      int force, int32_t* flag, void* stream);
PYGAMD_API int pygamd_live_lists_build(const void* rowptr, const void* col, int idx_dtype,
                                       int64_t n_rows, int64_t n_src, int64_t hub_threshold,
                                       const uint32_t* live, const uint32_t* live2,
                                       const int64_t* n_set, const int32_t* flag, void* col_live,
                                       void* rowend_live, uint32_t* row_has_live, void* stream);
PYGAMD_API int pygamd_live_lists_builds(int64_t* count /*[host]*/);

PYGAMD_API int pygamd_spmm_csr_workspace_bytes(const pygamd_spmm_args* args, size_t* bytes);
PYGAMD_API int pygamd_spmm_csr(const pygamd_spmm_args* args, void* workspace,
                               size_t workspace_bytes, void* stream);

/* Tie statistics for the backward of MIN/MAX, following the reference's CPU path
 * (zeros.scatter_reduce_(amax/amin, include_self=False), utils/_scatter.py:84-100): the
 * incoming gradient of out[i,f] is split evenly over all k with x[col[k],f] == out[i,f], and the
 * zero-initialised self entry counts as one more tie when out[i,f] == 0.
 * ntie_out[i,f] = (count_self ? [out[i,f] == 0] : 0) + #{k in row i : x[col[k],f] == out[i,f]}.
 * count_self = 0 gives the rule of torch._segment_reduce's backward (utils/_segment.py:37-50),
 * which has no self entry.                                                                      */
PYGAMD_API int pygamd_spmm_csr_tie_count(const void* rowptr, const void* col, int idx_dtype,
                                         const float* x, int64_t ldx, const float* out,
                                         int64_t ldo, int64_t n_rows, int64_t F, int count_self,
                                         float* ntie_out, void* stream);
/* grad_x[j,f] = sum over slots k of the TRANSPOSED handle (rowptr_t over sources, col_t = dst)
 *   [x[j,f] == out[col_t[k],f]] * grad_out[col_t[k],f] / ntie[col_t[k],f]                       */
PYGAMD_API int pygamd_spmm_csr_minmax_backward(const void* rowptr_t, const void* col_t,
                                               int idx_dtype, const float* x, int64_t ldx,
                                               const float* out, const float* grad_out,
                                               const float* ntie, int64_t ldo, int64_t n_src,
                                               int64_t F, float* grad_x, int64_t ldg,
                                               void* stream);
/* The same gradient, destination-driven and in ONE launch (no tie tensor, no by-source sort):
 * (rowptr, col) is the FORWARD's handle (rows = destinations, col = sources; col == NULL: slot k
 * is source k, i.e. segment reduce).  Per destination row the neighbours attaining out[i, f] are
 * counted (+1 for the zero-initialised self when count_self and out == 0), then every attaining
 * source receives grad_out[i, f] / ties through one fp32 atomic.  grad_x ([n_src, F], ld ldg) is
 * zeroed internally; sources reached from several destinations are summed in arbitrary order.  */
PYGAMD_API int pygamd_spmm_csr_minmax_backward_dst(const void* rowptr, const void* col,
                                                   int idx_dtype, const float* x, int64_t ldx,
                                                   const float* out, int64_t ldo,
                                                   const float* grad_out, int64_t ldgo,
                                                   int64_t n_rows, int64_t n_src, int64_t F,
                                                   int count_self, float* grad_x, int64_t ldg,
                                                   void* stream);
/* The fast path of the same gradient with the forward's saved `arg32` (pygamd_spmm_args.arg32_out):
 * every output whose extremum is unique sends its whole gradient to ONE source row with one fp32
 * atomic (no edge pass at all: arg32 and grad_out are read once, col is looked up inside the
 * row's slot range); outputs marked -2 are left to the two-pass kernel, which then only visits
 * rows that contain such an output.  grad_x is zeroed internally.  x / out are only read for the
 * marked outputs.                                                                                */
PYGAMD_API int pygamd_spmm_csr_minmax_backward_arg(const void* rowptr, const void* col,
                                                   int idx_dtype, const int32_t* arg32,
                                                   const float* x, int64_t ldx, const float* out,
                                                   int64_t ldo, const float* grad_out,
                                                   int64_t ldgo, int64_t n_rows, int64_t n_src,
                                                   int64_t F, int count_self, float* grad_x,
                                                   int64_t ldg, void* stream);
/* The same gradient WITHOUT the N x F scattered atomics (round 3).  Every output with a unique
 * extremum has exactly one winning edge: a destination-driven pass regroups the (feature, value)
 * pairs of grad_out by edge (`workspace`: n_rows x F pairs + one 32-bit (offset, count) word per
 * edge, pygamd_minmax_backward_src_workspace_bytes), then a source-driven pass over the TRANSPOSED
 * CSR (rowptr_t / col_t over the n_src sources; slot_map[e] = the by-destination slot of by-source
 * slot e, cf. EdgeIndex.src_slot_to_dst_slot) reads each out-edge's pairs — contiguous — and
 * sums them into the source's row in LDS, in slot order (deterministic for the unique extrema);
 * grad_x is written once, no memset.  Outputs marked -2 are then added by the two-pass tie kernel
 * like in pygamd_spmm_csr_minmax_backward_arg.  Needs F % 4 == 0, F <= 8192 and 16-byte aligned
 * rows (PYGAMD_ERR_UNSUPPORTED otherwise: use _arg).  Reference semantics: utils/_scatter.py:84-100
 * + ATen's amax / amin backward (ties share the gradient evenly).                               */
PYGAMD_API size_t pygamd_minmax_backward_src_workspace_bytes(int64_t n_rows, int64_t nnz,
                                                             int64_t F);
PYGAMD_API int pygamd_spmm_csr_minmax_backward_src(
    const void* rowptr, const void* col, const void* rowptr_t, const void* col_t,
    const void* slot_map, int idx_dtype, const int32_t* arg32, const float* x, int64_t ldx,
    const float* out, int64_t ldo, const float* grad_out, int64_t ldgo, int64_t n_rows,
    int64_t n_src, int64_t nnz, int64_t F, int count_self, void* workspace,
    size_t workspace_bytes, float* grad_x, int64_t ldg, void* stream);


/* ---- SDDMM: gradient w.r.t. edge weights ----------------------------------------------------
 * grad_w[e(k), h] = sum_{f in head h} grad_out[i, f] * x[col[k], f] * (src_scale? ...)  for k in
 * row i — the `value.requires_grad` branch of EdgeIndex._spmm (edge_index.py:1950-1953,
 * 1903-1922) and GATConv.message's alpha gradient (nn/conv/gat_conv.py:408-409).              */
PYGAMD_API int pygamd_sddmm_csr(const void* rowptr, const void* col, const void* eid,
                                int idx_dtype, const float* grad_out, int64_t ldg,
                                const float* x, int64_t ldx, int64_t n_rows, int64_t F,
                                int32_t w_heads, int32_t head_dim, float* grad_w, void* stream);
/* The two halves of a weighted aggregation's backward from ONE gather (ABI 9): over a CSR whose
 * row r holds `rows[r, :]` in registers and gathers x[col[k], :] for its slots k (e(k) = eid[k],
 * or k when eid is NULL),
 *   grad_w[e(k), h] = <rows[r, head h], x[col[k], head h]>          (the SDDMM above) and
 *   agg[r, f]       = sum_k w[e(k), head(f)] * x[col[k], f]          (pygamd_spmm_csr, per-head w).
 * GATConv's backward over the by-source form (nn/conv/gat_conv.py:387-409: rows = the projected
 * source features, x = the destinations' gradient rows, w = the attention coefficients) gets the
 * coefficient gradients and the aggregation's input gradient at the cost of one of them.  grad_w
 * must be zeroed by the caller when F > 256 (a head may span two lane groups: atomic adds).     */
PYGAMD_API int pygamd_sddmm_spmm_csr(const void* rowptr, const void* col, const void* eid,
                                     int idx_dtype, const float* rows, int64_t ldr,
                                     const float* x, int64_t ldx, int64_t n_rows, int64_t F,
                                     int32_t w_heads, int32_t head_dim, const float* w,
                                     float* grad_w, float* agg, int64_t lda, void* stream);

/* ---- a17: bias gradient of Linear --------------------------------------------------------------
 * out[f] = sum_r x[r, f]  (grad_bias = grad_out.sum(0), nn/dense/linear.py:121-127 backward).
 * `out` is zeroed internally; partial sums are combined with fp32 atomics.                     */
PYGAMD_API int pygamd_colsum(const float* x, int64_t ldx, int64_t n_rows, int64_t F, float* out,
                             void* stream);
/* ReLU backward fused with the bias gradient of the layer below (nn/models/basic_gnn.py:262-263
 * `self.act(x)` followed by a conv with bias):  grad_in[r,f] = act[r,f] <= 0 ? 0 : grad[r,f]
 * (aten::threshold_backward with threshold 0; `act` is the ReLU OUTPUT), and, when colsum_out is
 * not NULL, colsum_out[f] = sum_r grad_in[r,f] (zeroed internally, fp32 atomics).  grad_in may
 * alias grad.                                                                                   */
/* out = act(x + bias) in one pass (bias NULL: none; relu != 0: ReLU, NaN propagating) — the tail
 * of a conv layer: `out + self.bias` (gat_conv.py:378-385, gcn_conv.py:278-281) and the model's
 * activation (basic_gnn.py:262-263).  Its backward is pygamd_relu_backward_colsum on the OUTPUT. */
PYGAMD_API int pygamd_bias_act(const float* x, int64_t ldx, const float* bias, int64_t n_rows,
                               int64_t F, int relu, float* out, int64_t ldo, void* stream);
PYGAMD_API int pygamd_relu_backward_colsum(const float* grad, int64_t ldg, const float* act,
                                           int64_t lda, int64_t n_rows, int64_t F, float* grad_in,
                                           int64_t ldo, float* colsum_out, void* stream);

/* ---- a16/a17: segment_matmul (grouped GEMM over row segments, fp32 MFMA) ---------------------
 * Replaces pyg_lib.ops.segment_matmul(x, ptr, weight) (nn/conv/rgcn_conv.py:288,
 * nn/dense/linear.py:255):  out[ptr[g]:ptr[g+1]] = x[ptr[g]:ptr[g+1]] @ W[g].
 * `tiles` is a device array of int32 triples (segment, first row, rows <= tile_rows) covering
 * every non-empty segment in chunks of pygamd_segment_matmul_tile_rows() rows; W[g] is addressed
 * as w[g * w_seg_stride + k * w_stride_k + n * w_stride_n] so the same entry point computes the
 * input gradient (W^T: swap the two strides).  _wgrad: grad_w[g] = x[seg]^T @ g[seg] ([K, N]
 * row-major per segment; empty segments give 0); `chunks` uses the same triple format with any
 * chunk length (long segments are split so no wave walks a whole relation; fp32 atomics).
 * `blocks` > 1 (block-diagonal weights, RGCNConv(num_blocks=), rgcn_conv.py:222-244): group
 * g = segment * blocks + b multiplies the column block [b*K, (b+1)*K) of its rows of x by W[g]
 * into the column block [b*N, (b+1)*N) of out (ldx >= blocks*K, ldo >= blocks*N); no transposed
 * copies of the activations or the weights are needed.  blocks = 1: plain segment_matmul.      */
PYGAMD_API int pygamd_segment_matmul_tile_rows(void);
/* `n_groups` = number of weight matrices (segments * blocks).  `workspace` (device, 16-byte
 * aligned, pygamd_segment_matmul_workspace_bytes(n_groups, K, N); may be NULL): with it, in
 * PYGAMD_GEMM_SPLIT_BF16 mode, for K <= 128, K % 4 == 0 and 16-byte-aligned rows of x (weights
 * in any strides: W^T is read where it lies), the product runs on the convert-once split kernel
 * (csrc/segmm.hip: the weights' bf16 term planes are written there by a pre-pass, every call);
 * otherwise on the exact fp32 kernel (ABI 9).                                                  */
PYGAMD_API int pygamd_segment_matmul_workspace_bytes(int64_t n_groups, int64_t K, int64_t N,
                                                     size_t* bytes /*[host]*/);
/* `x_rows` / `g_rows` (device int64, or NULL): operand row r is x[x_rows[r]] (g[g_rows[r]]) — the
 * rows of a smaller tensor gathered on the fly.  RGCNConv sums its transformed (relation,
 * destination) rows per destination (rgcn_conv.py:284-290 + aggregate); the backward of that sum
 * hands every pair row the gradient row of its destination, and with the index the input- and
 * weight-gradient launches read those rows where they are instead of from a gathered [pairs, F]
 * copy (ABI 9).                                                                                */
PYGAMD_API int pygamd_segment_matmul(const float* x, int64_t ldx, const int64_t* x_rows,
                                     const float* w, int64_t w_seg_stride, int64_t w_stride_k,
                                     int64_t w_stride_n, int64_t n_groups, const int32_t* tiles,
                                     int64_t n_tiles, int64_t K, int64_t N, int64_t blocks,
                                     float* out, int64_t ldo, void* workspace,
                                     size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_segment_matmul_wgrad(const float* x, int64_t ldx, const float* g,
                                           int64_t ldg, const int64_t* g_rows,
                                           const int32_t* chunks, int64_t n_chunks,
                                           int64_t n_seg, int64_t K, int64_t N, int64_t blocks,
                                           float* grad_w, void* stream);

/* ---- a2: gather (index_select along dim 0) --------------------------------------------------
 * out[e, :] = x[index[e], :]  (nn/conv/message_passing.py:263-290, collect.jinja:118-127).
 * Out-of-range indices set *err_flag (device int32, optional) to 1 and read row 0.             */
PYGAMD_API int pygamd_gather_rows(const float* x, int64_t ldx, int64_t n_src, const void* index,
                                  int idx_dtype, int64_t n, int64_t F, float* out, int64_t ldo,
                                  int32_t* err_flag, void* stream);

/* Fused gather -> scale -> scatter-add on an unsorted edge list (the COO
 * fallback of the SpMM for graphs used once, e.g. the backward of a sampled mini-batch):
 *   out[scatter_idx[e], :] += (scale ? scale[gather_idx[e]] : 1) * (w ? w[e] : 1) * x[gather_idx[e], :]
 * `out` must be initialised by the caller (usually zeros); fp32 atomics.  `n_valid` (device int64,
 * may be NULL): only the first min(*n_valid, n_edges) entries of the fixed-capacity edge list are
 * real (a sampled hop at its static capacity: no host read, hipGraph-capturable).               */
PYGAMD_API int pygamd_gather_scatter_add(const float* x, int64_t ldx, const void* gather_idx,
                                         const void* scatter_idx, int idx_dtype,
                                         const float* scale, const float* w, int64_t n_edges,
                                         const int64_t* n_valid, int64_t F, float* out,
                                         int64_t ldo, void* stream);

/* ---- a5: scatter (unsorted COO, atomics) ----------------------------------------------------
 * out[index[e], :] (reduce)= src[e, :]   (utils/_scatter.py:14-138).  `out` must be
 * pre-initialised by pygamd_scatter_init; MEAN/MIN/MAX need `count` ([dim_size] float, zeroed)
 * and a pygamd_scatter_finalize call (mean: divide by clamp(count,1); min/max: untouched -> 0). */
PYGAMD_API int pygamd_scatter_init(float* out, int64_t ldo, int64_t dim_size, int64_t F,
                                   int reduce, float* count, void* stream);
PYGAMD_API int pygamd_scatter_rows(const float* src, int64_t lds, const void* index,
                                   int idx_dtype, int64_t n, int64_t F, float* out, int64_t ldo,
                                   int64_t dim_size, int reduce, float* count,
                                   int32_t* err_flag, void* stream);
PYGAMD_API int pygamd_scatter_finalize(float* out, int64_t ldo, int64_t dim_size, int64_t F,
                                       int reduce, const float* count, void* stream);
/* backward of MIN/MAX/MUL-free scatter: see utils/_scatter.py:84-100 (same tie rule as above).
 * ntie[g,f] = [out[g,f]==0] + #{e: index[e]==g, src[e,f]==out[g,f]}  (initialised internally);
 * grad_src[e,f] = [src[e,f]==out[g,f]] * grad_out[g,f] / ntie[g,f].                             */
PYGAMD_API int pygamd_scatter_minmax_tie_count(const float* src, int64_t lds, const void* index,
                                               int idx_dtype, int64_t n, int64_t F,
                                               const float* out, int64_t ldo, int64_t dim_size,
                                               float* ntie, void* stream);
PYGAMD_API int pygamd_scatter_minmax_backward(const float* src, int64_t lds, const void* index,
                                              int idx_dtype, int64_t n, int64_t F,
                                              const float* out, const float* grad_out,
                                              const float* ntie, int64_t ldo, int64_t dim_size,
                                              float* grad_src, int64_t ldg, void* stream);

/* Backward of scatter(reduce='mul'), i.e. of ones.scatter_reduce_('prod', include_self=True)
 * (utils/_scatter.py:119-133; ATen scatter_reduce_backward): with z zeros scattered into
 * (group, f):  z == 0: g * out / src_e;  z == 1: the zero element gets g * prod(others), all
 * other elements 0;  z >= 2: 0.  Rows with an out-of-range index get 0.  Workspace =
 * dim_size * F * 8 bytes.                                                                      */
PYGAMD_API int pygamd_scatter_mul_backward_workspace_bytes(int64_t dim_size, int64_t F,
                                                           size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_scatter_mul_backward(const float* src, int64_t lds, const void* index,
                                           int idx_dtype, int64_t n, int64_t F, const float* out,
                                           const float* grad_out, int64_t ldo, int64_t dim_size,
                                           float* grad_src, int64_t ldg, void* workspace,
                                           size_t workspace_bytes, void* stream);

/* ---- a6: scatter_argmax (1-D) ---------------------------------------------------------------
 * utils/_scatter.py:147-184: out[g] = the LAST e (largest e) with src[e] == max of group g,
 * dim_size-1 for empty groups.  `gmax` is a [dim_size] float scratch.                          */
PYGAMD_API int pygamd_scatter_argmax(const float* src, const void* index, int idx_dtype,
                                     int64_t n, int64_t dim_size, float* gmax, void* arg_out,
                                     void* stream);

/* ---- a8: segment softmax (edge softmax) -----------------------------------------------------
 * utils/_softmax.py:12-92, ptr branch :60-81 (also pyg_lib.ops.softmax_csr): for each segment
 * s and column h:  out[k,h] = exp(src[k,h] - max_s) / (sum_s exp(src - max_s) + 1e-16).
 * src/out are [n, H] contiguous.  Backward: grad_src = out * (grad_out - sum_s(out*grad_out)).  */
PYGAMD_API int pygamd_segment_softmax_forward(const float* src, const void* ptr, int idx_dtype,
                                              int64_t n_seg, int64_t H, float* out,
                                              void* stream);
PYGAMD_API int pygamd_segment_softmax_backward(const float* out, const float* grad_out,
                                               const void* ptr, int idx_dtype, int64_t n_seg,
                                               int64_t H, float* grad_src, void* stream);

/* The same softmax over an UNSORTED `index` ([n], values in [0, N)) — the index branch of
 * utils/_softmax.py:82-88 (scatter-max, gather, exp, scatter-sum, gather, div) as four launches:
 * group maxima (atomic float max), exp + group sums (fp32 atomics), normalisation.  `workspace`:
 * 2 x N x H floats (forward), N x H floats (backward).  Rows whose index is out of range are
 * skipped (their output is left untouched by the forward, their gradient is 0) and, like in the
 * scatter kernels, reported: `*err` ([dev] int32, may be NULL, zeroed by the caller) becomes
 * non-zero — the reference's scatter / index_select path raises there (ABI 8).               */
PYGAMD_API int pygamd_softmax_index_forward(const float* src, const void* index, int idx_dtype,
                                            int64_t n, int64_t H, int64_t N, float* workspace,
                                            float* out, int32_t* err, void* stream);
PYGAMD_API int pygamd_softmax_index_backward(const float* out, const float* grad_out,
                                             const void* index, int idx_dtype, int64_t n,
                                             int64_t H, int64_t N, float* workspace,
                                             float* grad_src, void* stream);

/* segment_logsumexp (utils/_segment.py:53-80): out[s,h] = log(sum_{k in s} exp(src[k,h])),
 * evaluated with the segment maximum subtracted; an empty segment gives 0.  src is [n, H]
 * contiguous, out [n_seg, H].  Backward: grad_src[k,h] = exp(src[k,h] - out[s,h]) * grad_out[s,h]. */
PYGAMD_API int pygamd_segment_logsumexp_forward(const float* src, const void* ptr, int idx_dtype,
                                                int64_t n_seg, int64_t H, float* out,
                                                void* stream);
PYGAMD_API int pygamd_segment_logsumexp_backward(const float* src, const float* out,
                                                 const float* grad_out, const void* ptr,
                                                 int idx_dtype, int64_t n_seg, int64_t H,
                                                 float* grad_src, void* stream);

/* ---- a15: GAT node terms ----------------------------------------------------------------------
 * out_a[n,h] = sum_c x[n, h*C + c] * att_a[h*C + c]  (and out_b with att_b when given) — the
 * `(x * att).sum(-1)` pair of nn/conv/gat_conv.py:330-332 in one pass over x.  Backward:
 * grad_x[n,f] (+)= grad_a[n,h(f)] att_a[f] + grad_b[n,h(f)] att_b[f]  (grad_x may be NULL;
 * `accumulate` != 0 adds to what grad_x holds — the gradient of the same x through the
 * aggregation, so that the two do not meet in a separate add pass; ABI 8),
 * grad_att_a[f] = sum_n grad_a[n,h(f)] x[n,f]  (zeroed internally, atomics).                     */
PYGAMD_API int pygamd_head_dot_forward(const float* x, int64_t ldx, const float* att_a,
                                       const float* att_b, int64_t n_rows, int64_t H, int64_t C,
                                       float* out_a, float* out_b, void* stream);
PYGAMD_API int pygamd_head_dot_backward(const float* x, int64_t ldx, const float* att_a,
                                        const float* att_b, const float* grad_a,
                                        const float* grad_b, int64_t n_rows, int64_t H,
                                        int64_t C, float* grad_x, int64_t ldg, int accumulate,
                                        float* grad_att_a, float* grad_att_b, void* stream);

/* ---- a15: fused GAT edge logits ------------------------------------------------------------
 * nn/conv/gat_conv.py:387-406 on a dst-sorted handle: for slot k in row i,
 *   logit = leaky_relu(alpha_src[col[k],h] + alpha_dst[i,h], slope); softmax over the row.
 * alpha_out is [nnz, H] in SLOT order.  Backward returns grad_alpha_src / grad_alpha_dst
 * accumulated with atomics (grad buffers must be zeroed).                                      */
PYGAMD_API int pygamd_gat_edge_softmax_forward(const void* rowptr, const void* col,
                                               int idx_dtype, const float* alpha_src,
                                               const float* alpha_dst, int64_t n_rows,
                                               int64_t H, float slope, float* alpha_out,
                                               void* stream);
PYGAMD_API int pygamd_gat_edge_softmax_backward(const void* rowptr, const void* col,
                                                int idx_dtype, const float* alpha_src,
                                                const float* alpha_dst, const float* alpha_out,
                                                const float* grad_alpha, int64_t n_rows,
                                                int64_t H, float slope, float* grad_alpha_src,
                                                float* grad_alpha_dst, void* stream);

/* ---- a16: GATv2 attention in one pass ---------------------------------------------------------
 * nn/conv/gatv2_conv.py:358-378 (edge_update + message + the 'add' aggregation) on a dst-sorted
 * handle.  For slot k of row i with j = col[k]:
 *   s[k,h]   = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[i,h,c], slope)
 *   alpha    = softmax over the row (maximum subtracted, 1e-16 on the denominator)
 *   out[i,h] = sum_k alpha[k,h] * x_l[j,h,:]
 * x_l [n_src, H*C], x_r [>= n_rows, H*C], att [H*C], all contiguous fp32.  alpha is [nnz, H] in
 * SLOT order and always written; out [n_rows, H*C] may be NULL ("score mode": alpha only).
 * Supported: H*C <= 512 and H <= 64 (pygamd_gatv2_supported), otherwise status 2.  `g` is the
 * handle (pygamd_csr; NULL: status 1) and n_src the row count of x_l; the workspace
 * (pygamd_gatv2_workspace_bytes of g's n_chunks) holds the chunks' partial results and, for
 * backward_dst, the per-workgroup partials of the att gradient.  No float atomics: all results are
 * bitwise reproducible.
 *
 * backward_dst: grad_s[k,h] = alpha * (d alpha - D), grad_x_r [n_rows, H*C], grad_att [H*C].
 *   d alpha = <grad_out[i,h,:], x_l[j,h,:]> and D = <grad_out[i,h,:], out[i,h,:]> when grad_out /
 *   out are given and grad_alpha is NULL; score mode passes grad_alpha [nnz, H] (slot order) and
 *   NULL for grad_out / out.
 * backward_src: g is the src-sorted handle (n_dst the row count of the by-destination one), with
 *   slot_map = by-source slot -> by-destination slot,
 *   grad_x_l[j] = sum_i alpha * grad_out[i] + grad_s * att * leaky_relu'(x_l[j] + x_r[i]); the
 *   first term is left out when grad_out is NULL (score mode).                                  */
PYGAMD_API int pygamd_gatv2_supported(int64_t H, int64_t C);
PYGAMD_API int pygamd_gatv2_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C,
                                            size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_gatv2_forward(const pygamd_csr* g, const float* x_l, const float* x_r,
                                    const float* att, int64_t n_src, int64_t H, int64_t C,
                                    float slope, float* alpha, float* out, void* workspace,
                                    size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_gatv2_backward_dst(const pygamd_csr* g, const float* x_l, const float* x_r,
                                         const float* att, const float* alpha,
                                         const float* grad_out, const float* out,
                                         const float* grad_alpha, int64_t n_src, int64_t H,
                                         int64_t C, float slope, float* grad_s, float* grad_x_r,
                                         float* grad_att, void* workspace, size_t workspace_bytes,
                                         void* stream);
PYGAMD_API int pygamd_gatv2_backward_src(const pygamd_csr* g, const void* slot_map,
                                         const float* x_l, const float* x_r, const float* att,
                                         const float* alpha, const float* grad_s,
                                         const float* grad_out, int64_t n_dst, int64_t H, int64_t C,
                                         float slope, float* grad_x_l, void* workspace,
                                         size_t workspace_bytes, void* stream);

/* ---- a16h: HAN's typed additive attention, every edge type in one pass ------------------------
 * nn/conv/han_conv.py:170-179 (message: GAT's additive score, the softmax per destination, the
 * weighting of x_j) + the 'add' aggregation and the ReLU of han_conv.py:155, for all edge types of
 * a layer call on ONE stacked dst-sorted handle.  Row r = row_begin[e] + i is destination i of edge
 * type e (an empty neighbourhood is an empty row), column c is a stacked (edge type, source).
 * For slot k of row r of edge type e with c = col[k]:
 *   s[k,h]   = leaky_relu(a_src[c,h] + a_dst[r,h], slope)
 *   alpha    = softmax over the row (maximum subtracted, 1e-16 on the denominator)
 *   out[r,h] = sum_k alpha[k,h] * x_all[c + val_shift[e], h, :]        (ReLU on top if relu != 0)
 * x_all [., H*C] holds every node type's projected rows once; a_src [n_cols, H], a_dst [n_rows, H],
 * out [n_rows, H*C] and alpha [nnz, H] (SLOT order), all contiguous fp32.  row_begin [n_et + 1] and
 * val_shift [n_et] are HOST arrays (n_et <= 64, otherwise status 2; row_begin[0] = 0,
 * row_begin[n_et] = g->n_rows) and travel by value in the kernel arguments.  Every column must read
 * a row of x_all: the caller checks the ids when it stacks the graph.  A -inf score has weight 0, a
 * row of -inf scores is NaN, NaN / +inf poison their own (row, head), an empty row is 0, and the
 * ReLU lets NaN through.  Supported: H*C <= 512 and H <= 64 (pygamd_han_supported), otherwise
 * status 2.  The workspace (pygamd_han_workspace_bytes of g's n_chunks) holds the chunks' partial
 * results.  No float atomics: all results are bitwise reproducible.
 *
 * backward_dst: with g = grad_out * [out > 0] (relu) or grad_out,
 *   grad_s[k,h] = alpha * (<g[r,h,:], x[c,h,:]> - <g[r,h,:], out[r,h,:]>) * leaky_relu'(.) (slope
 *   where the argument is <= 0), in slot order, and grad_a_dst[r] = sum_k grad_s[k].
 * backward_src: g is the src-sorted handle (rows = the forward's columns; n_dst the row count of
 *   the by-destination one), slot_map = by-source slot -> by-destination slot:
 *   grad_a_src[c] = sum grad_s, grad_xv[c] = sum alpha * g[r]  ([n_cols, H*C]: the caller adds the
 *   blocks of the edge types into the node types' rows).                                        */
PYGAMD_API int pygamd_han_supported(int64_t H, int64_t C);
PYGAMD_API int pygamd_han_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C,
                                          size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_han_forward(const pygamd_csr* g, const int64_t* row_begin /*[host]*/,
                                  const int64_t* val_shift /*[host]*/, int64_t n_et,
                                  const float* x_all, const float* a_src, const float* a_dst,
                                  int64_t n_cols, int64_t H, int64_t C, float slope, int relu,
                                  float* alpha, float* out, void* workspace,
                                  size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_han_backward_dst(const pygamd_csr* g, const int64_t* row_begin /*[host]*/,
                                       const int64_t* val_shift /*[host]*/, int64_t n_et,
                                       const float* x_all, const float* a_src, const float* a_dst,
                                       const float* alpha, const float* grad_out, const float* out,
                                       int64_t n_cols, int64_t H, int64_t C, float slope, int relu,
                                       float* grad_s, float* grad_a_dst, void* workspace,
                                       size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_han_backward_src(const pygamd_csr* g, const void* slot_map,
                                       const float* alpha, const float* grad_s,
                                       const float* grad_out, const float* out, int64_t n_dst,
                                       int64_t H, int64_t C, int relu, float* grad_a_src,
                                       float* grad_xv, void* workspace, size_t workspace_bytes,
                                       void* stream);

/* ---- a16b: TransformerConv's dot-product attention in one pass --------------------------------
 * nn/conv/transformer_conv.py:263-283 (message: the scaled dot product, the softmax and the
 * weighting of value_j) + the 'add' aggregation of propagate (transformer_conv.py:234-235) on a
 * dst-sorted handle, without edge features.  For slot k of row i with j = col[k]:
 *   s[k,h]   = scale * sum_c query[i,h,c] * key[j,h,c]          (scale = 1 / sqrt(C))
 *   alpha    = softmax over the row (maximum subtracted, 1e-16 on the denominator; utils/_softmax.py)
 *   out[i,h] = sum_k alpha[k,h] * value[j,h,:]
 * query [>= n_rows, H*C] contiguous fp32; key and value are two pointers to rows of H*C floats with
 * ONE row stride ld >= H*C (floats): separate contiguous tensors (ld = H*C) or the two halves of a
 * [n_src, 2*H*C] projection (ld = 2*H*C, value = key + H*C).  alpha is [nnz, H] in SLOT order and
 * always written; out [n_rows, H*C] may be NULL ("score mode": alpha only, value is not read).
 * Supported head layouts, the handle g and reproducibility as for pygamd_gatv2_*
 * (pygamd_transformer_supported; workspace of pygamd_transformer_workspace_bytes for g's
 * n_chunks, 0 bytes without hub rows).  Status 1 / 2 / 3 before any device work.
 *
 * backward_dst (transformer_conv.py:273-282 differentiated): grad_s[k,h] = alpha * (d alpha - D),
 *   grad_query[i] = scale * sum_k grad_s * key[j].  d alpha = <grad_out[i,h,:], value[j,h,:]> and
 *   D = <grad_out[i,h,:], out[i,h,:]> when grad_out / out are given and grad_alpha is NULL; score
 *   mode passes grad_alpha [nnz, H] (slot order), NULL for grad_out / out, and does not read value.
 * backward_src: g is the src-sorted handle, slot_map = by-source slot -> by-destination slot,
 *   grad_key[j] = scale * sum_i grad_s * query[i] and grad_value[j] = sum_i alpha * grad_out[i],
 *   both written at row stride ld (one [n_src, 2*H*C] gradient buffer feeds one dgrad GEMM);
 *   grad_out NULL = score mode: grad_key only, grad_value may be NULL.                          */
PYGAMD_API int pygamd_transformer_supported(int64_t H, int64_t C);
PYGAMD_API int pygamd_transformer_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C,
                                                  size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_transformer_forward(const pygamd_csr* g, const float* query, const float* key,
                                          const float* value, int64_t ld, int64_t n_src, int64_t H,
                                          int64_t C, float scale, float* alpha, float* out,
                                          void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_transformer_backward_dst(const pygamd_csr* g, const float* key,
                                               const float* value, int64_t ld, const float* alpha,
                                               const float* grad_out, const float* out,
                                               const float* grad_alpha, int64_t n_src, int64_t H,
                                               int64_t C, float scale, float* grad_s,
                                               float* grad_query, void* workspace,
                                               size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_transformer_backward_src(const pygamd_csr* g, const void* slot_map,
                                               const float* query, const float* alpha,
                                               const float* grad_s, const float* grad_out,
                                               int64_t n_dst, int64_t H, int64_t C, float scale,
                                               float* grad_key, float* grad_value, int64_t ld,
                                               void* workspace, size_t workspace_bytes,
                                               void* stream);

/* ---- a16c: TransformerConv's edge features (edge_dim) inside the one-pass kernels ---------------
 * nn/conv/transformer_conv.py:263-283 with lin_edge: key_j + e and value_j + e, e = W_e a_k.  The
 * edge term is linear, so the kernels never see it at width H*C.  With a_k [De] the raw features of
 * slot k and, per destination, bias[i,h,:] = scale * (W_e^h)^T query[i,h,:]  ([>= n_rows, H*De]):
 *   s[k,h]   = scale * <query[i,h,:], key[j,h,:]> + <bias[i,h,:], a_k>
 *   alpha    = softmax over the row, as pygamd_transformer_forward
 *   out[i,h] = sum_k alpha[k,h] * value[j,h,:]          (WITHOUT the edge term)
 *   z[i,h]   = sum_k alpha[k,h] * a_k                   ([n_rows, H*De])
 * and the caller adds W_e^h z[i,h] to out (transformer_conv.py:263-283: `out = value_j + edge_attr`).
 * edge_attr is [nnz, De] contiguous fp32 in SLOT order.  out and z are both given, or both NULL
 * ("score mode": alpha only).  Every other argument, the handle g and the
 * reproducibility are those of pygamd_transformer_forward; the workspace is that of
 * pygamd_transformer_edge_workspace_bytes.  pygamd_transformer_edge_supported (transformer_conv.py:
 * 263-283): the head layout of pygamd_transformer_supported and De <= 4 * lph_max, lph_max the
 * largest power of two with H * lph_max <= 64 (De <= 32 at H <= 8, De <= 4 at H = 64); otherwise
 * status 2.  Status 1 / 2 / 3 before any device work; n_rows == 0 returns 0.
 *
 * edge_backward_dst (transformer_conv.py:263-283 differentiated), with g = grad_out, gz = grad_z:
 *   d alpha[k,h] = <g[i,h,:], value[j,h,:]> + <gz[i,h,:], a_k>,  D = <g, out> + <gz, z> per (i, h)
 *   grad_s = alpha * (d alpha - D);  grad_query[i] = scale * sum_k grad_s * key[j]
 *   grad_bias[i,h,:] = sum_k grad_s[k,h] * a_k
 *   grad_edge_attr[k,:] = sum_h (grad_s[k,h] * bias[i,h,:] + alpha[k,h] * gz[i,h,:])   (slot order;
 *     NULL: not wanted, the work is skipped)
 *   score mode passes grad_alpha [nnz, H] and NULL for grad_out / out / grad_z / z: d alpha is
 *   given, D = sum_row alpha * d alpha, and grad_edge_attr holds the grad_s * bias part only.
 * The by-source pass is pygamd_transformer_backward_src, unchanged.                              */
PYGAMD_API int pygamd_transformer_edge_supported(int64_t H, int64_t C, int64_t De);
PYGAMD_API int pygamd_transformer_edge_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C,
                                                       int64_t De, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_transformer_edge_forward(const pygamd_csr* g, const float* query,
                                               const float* key, const float* value, int64_t ld,
                                               const float* edge_attr, const float* bias,
                                               int64_t n_src, int64_t H, int64_t C, int64_t De,
                                               float scale, float* alpha, float* out, float* z,
                                               void* workspace, size_t workspace_bytes,
                                               void* stream);
PYGAMD_API int pygamd_transformer_edge_backward_dst(
    const pygamd_csr* g, const float* key, const float* value, int64_t ld,
    const float* edge_attr, const float* bias, const float* alpha, const float* grad_out,
    const float* out, const float* grad_z, const float* z, const float* grad_alpha,
    int64_t n_src, int64_t H, int64_t C, int64_t De, float scale, float* grad_s,
    float* grad_query, float* grad_bias, float* grad_edge_attr, void* workspace,
    size_t workspace_bytes, void* stream);

/* ---- GINEConv's edge message (gin_conv.py:19-207) -------------------------------------------------
 * One destination row i of the by-destination handle g (pygamd_csr; NULL: status 1), slot k with
 * source j = col[k] and original edge edge_id[k] (NULL: slot order):
 *   out[i,:] = (x_root ? (1 + *eps) * x_root[i,:] : 0) + sum_k max(x_src[j,:] + e_k, 0)
 *   wide   (De == 0): e_k = edge_attr[edge_id[k], :],   edge_attr [E, F]
 *   linear (De >= 1): e_k = W a_k + b, a_k = edge_attr[edge_id[k], :De], weight W [F, De] in
 *                     torch.nn.Linear's layout, bias b [F] or NULL
 * (gin_conv.py:185-207: message = (x_j + lin(edge_attr)).relu(), out = nn((1 + eps) * x_r + sum)).
 * ONE launch, one 64-lane wave per row, lanes over the F columns; edge features are read in place
 * through edge_id and, in linear mode, every lane keeps its columns' rows of W in registers: no
 * [E, F] value is formed.  eps is a DEVICE pointer (it may be a parameter; no host read); x_root
 * and eps may be NULL (the bipartite (x_src, None) case).  x_src and x_root have row strides
 * ld_src / ld_root (floats), everything else is contiguous; fp32 data, int32 / int64 indices.
 * A split row's partial sums are added in chunk order.  No float atomics: bitwise reproducible.
 *
 * backward: ONE launch over the by-source handle g (col = the destination of every out-slot,
 * edge_id_t = that form's own slot -> original edge map, NULL: slot order), every
 * edge visited once, m = (x_src[j,:] + e_k > 0) (strict, as relu's backward), g = grad_out[i,:]:
 *   grad_x_src[j,:] = sum_t m * g                      (zeros for rows without out-slots)
 *   wide:   grad_edge_attr[k,:] = m * g                (original edge order; NULL: not wanted)
 *   linear: grad_edge_attr[k,d] = sum_f m_f g_f W[f,d] (NULL: not wanted, the wave sums are skipped)
 *           grad_weight[f,d] = sum_k m_f g_f a_k[d],  grad_bias[f] = sum_k m_f g_f (NULL iff bias is)
 * grad_weight / grad_bias accumulate in registers, leave one partial per workgroup in the
 * workspace and are reduced in workgroup order by a second small kernel inside the call; the grid
 * is a function of (n_src, n_chunks) only.  The self term (grad_x_root, grad_eps) is the caller's.
 *
 * pygamd_gine_supported(F, De) (De = 0: wide mode): F <= 512 and, in linear mode, De <= 32 and
 * F * De <= 4096; otherwise status 2.  The workspace (pygamd_gine_workspace_bytes) holds the
 * chunks' partial rows and, in linear mode, the backward's per-workgroup partials.  Status 1 / 2 /
 * 3 before any device work; n_rows == 0 returns 0.                                               */
PYGAMD_API int pygamd_gine_supported(int64_t F, int64_t De);
PYGAMD_API int pygamd_gine_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De,
                                           size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_gine_forward(const pygamd_csr* g, const void* edge_id, const float* x_src,
                                   int64_t ld_src, const float* x_root, int64_t ld_root,
                                   const float* eps, const float* edge_attr, const float* weight,
                                   const float* bias, int64_t n_src, int64_t F, int64_t De,
                                   float* out, void* workspace, size_t workspace_bytes,
                                   void* stream);
PYGAMD_API int pygamd_gine_backward(const pygamd_csr* g, const void* edge_id_t, const float* x_src,
                                    int64_t ld_src, const float* edge_attr, const float* weight,
                                    const float* bias, const float* grad_out, int64_t n_dst,
                                    int64_t F, int64_t De, float* grad_x_src, float* grad_edge_attr,
                                    float* grad_weight, float* grad_bias, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ---- PNAConv's multi-statistic aggregation (pna_conv.py:175-188, aggr/scaler.py:82) --------------
 * For a linear message (pre_layers = 1) the message of slot k of destination i with source
 * j = col[k] is m_k = p_dst[i,:] + u_k with u_k = p_src[j,:] + Wc a_k, a_k = edge_attr[edge_id[k],
 * :De], Wc [W, De] (De == 0: u_k = p_src[j,:]; edge_attr and wc are NULL).  forward
 * (pna_conv.py:175-188 is the message, aggr/scaler.py:82 the aggregation it feeds): ONE launch
 * over the by-destination handle g, one 64-lane wave per row, lanes over the W columns, one
 * gathered row per slot.  `stats` is a non-empty bit set (1 mean, 2 min, 4 max, 8 std); `out`
 * holds the selected statistics as consecutive [n_rows, W] planes in that order:
 *   mean = p_dst[i] + sum u / d,  min = p_dst[i] + min u,  max = p_dst[i] + max u,
 *   std = sqrt(max(var u, 1e-5)), 0 where that is <= sqrt(1e-5)
 * and exactly 0 for a row without slots.  The second moment is accumulated about the first u of
 * the row (or chunk).  `saved` [6, n_rows, W] takes what the backward needs: mean u, min u, max u,
 * std and the number of slots attaining the minimum / the maximum (as floats; 0, 0, 0, 0, 1, 1 for
 * a row without slots).  A split row's partials (seven rows per chunk) are merged in chunk order:
 * equal extrema add their counts, moments combine by the parallel-variance formula.
 *
 * backward (the gradient of pna_conv.py:175-188 under aggr/scaler.py:82): ONE launch over the
 * by-source handle g (col = the destination of every out-slot, edge_id_t = that form's slot ->
 * original edge map).  `coef` [n_dst, 6, W] is a packed row per destination: A, B, Gmin, Gmax,
 * min u, max u.  The launch rebuilds u_k bit for bit and forms
 *   grad_u = A + B u_k + Gmin [u_k == min u] + Gmax [u_k == max u]
 * (rows of a statistic outside `stats` are not read), then
 *   grad_p_src[j,:] = sum_t grad_u   (zeros for rows without out-slots)
 *   grad_edge_attr[k,d] = sum_c grad_u[c] Wc[c,d]   (original edge order; NULL: not wanted)
 *   grad_wc[c,d] = sum_k grad_u[c] a_k[d]   (per-workgroup partials reduced in workgroup order)
 * The gradient of p_dst is elementwise and the caller's.
 *
 * pygamd_pna_supported(W, De): W <= 512 and, with edge features, De <= 32 and W * De <= 4096;
 * otherwise status 2.  p_src / p_dst have row strides ld_src / ld_dst (floats); fp32 data, int32 /
 * int64 indices.  No float atomics: bitwise reproducible.  Status 1 / 2 / 3 before any device
 * work; n_rows == 0 returns 0.                                                                    */
PYGAMD_API int pygamd_pna_supported(int64_t W, int64_t De);
PYGAMD_API int pygamd_pna_workspace_bytes(int64_t n_chunks, int64_t W, int64_t De,
                                          size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_pna_forward(const pygamd_csr* g, const void* edge_id, const float* p_src,
                                  int64_t ld_src, const float* p_dst, int64_t ld_dst,
                                  const float* edge_attr, const float* wc, int64_t n_src,
                                  int64_t W, int64_t De, int stats, float* out, float* saved,
                                  void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_pna_backward(const pygamd_csr* g, const void* edge_id_t, const float* p_src,
                                   int64_t ld_src, const float* edge_attr, const float* wc,
                                   const float* coef, int64_t n_dst, int64_t W, int64_t De,
                                   int stats, float* grad_p_src, float* grad_edge_attr,
                                   float* grad_wc, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- GENConv's softmax aggregation (gen_conv.py:203-239, aggr/basic.py:142-215) ------------------
 * For slot k of destination i with source j = col[k] and original edge edge_id[k] (NULL: slot
 * order), column c:
 *   e_k = 0                                        (PYGAMD_GEN_EDGE_NONE:   edge_attr NULL, De = 0)
 *       = edge_attr[edge_id[k], :]                 (PYGAMD_GEN_EDGE_WIDE:   edge_attr [E, F], De = 0)
 *       = W a_k + b, a_k = edge_attr[edge_id[k], :De]  (PYGAMD_GEN_EDGE_LINEAR: W [F, De] in
 *                                                  torch.nn.Linear's layout, b [F] or NULL)
 *   m_k = max(x_src[j,:] + e_k, 0) + eps_msg                       (gen_conv.py:231-239, message)
 *   out[i,c] = sum_k alpha_kc m_kc,  alpha_kc = exp(t_c m_kc - M_ic) / (sum_k exp(t_c m_kc - M_ic)
 *              + 1e-16),  M_ic = max_k t_c m_kc                    (aggr/basic.py:205-215)
 * t is a DEVICE pointer to t_len = 1 or F values of any sign (it may be a parameter; no host
 * read).  forward (replaces gen_conv.py:213, propagate): ONE launch over the by-destination
 * handle g, one 64-lane wave per row, lanes over the F columns; every lane keeps a running
 * (M, L, acc) per column and takes a slot in with one expf per element.  No [E, F] value is formed.
 * out is exactly 0 for a row without slots.  `saved` takes the planes M and 1 / (L + 1e-16) of
 * [n_rows, F] each and, if want_s2, a third plane S2 = sum_k alpha m^2 (the gradient of t is
 * sum_i g (S2 - out^2), the caller's reduction).  A split row's chunks leave (M, L, acc, S2) in
 * the workspace and are merged per column in chunk order.  Logits of +inf or NaN poison their own
 * (row, column), as the reference's softmax does.
 *
 * backward (the gradient of gen_conv.py:213): ONE launch over the by-source handle g (col = the
 * destination of every out-slot, edge_id_t = that form's slot -> original edge map, NULL: slot
 * order).  `coef` [n_dst, 3, F] is a packed row per destination: M, G = grad_out[i,:] / (L +
 * 1e-16) and out[i,:]; with semi_grad [n_dst, 2, F]: M and G (the softmax weights are constants,
 * aggr/basic.py:209).  The launch rebuilds m_k and
 *   gm = (x_src[j,:] + e_k > 0) exp(t m_k - M) G (1 + t (m_k - out))   (semi_grad: without the
 *                                                                       last factor)
 *   grad_x_src[j,:] = sum_s gm                         (zeros for rows without out-slots)
 *   wide:   grad_edge_attr[k,:] = gm                   (original edge order)
 *   linear: grad_edge_attr[k,d] = sum_f gm_f W[f,d],  grad_weight[f,d] = sum_k gm_f a_k[d],
 *           grad_bias[f] = sum_k gm_f (NULL iff bias is)
 * grad_edge_attr is written iff want_grad_edge_attr (NULL otherwise); grad_weight / grad_bias
 * leave one partial per workgroup and are reduced in workgroup order inside the call; the grid is
 * a function of (n_src, n_chunks) only.
 *
 * pygamd_gen_supported(F, De) (De = 0 without lin_edge): F <= 512 and, in linear mode, De <= 32
 * and F * De <= 4096; otherwise status 2.  x_src has row stride ld_src (floats), everything else is
 * contiguous; fp32 data, int32 / int64 indices.  No float atomics: bitwise reproducible.  Status
 * 1 / 2 / 3 before any device work; n_rows == 0 returns 0.                                        */
#define PYGAMD_GEN_EDGE_NONE 0
#define PYGAMD_GEN_EDGE_WIDE 1
#define PYGAMD_GEN_EDGE_LINEAR 2
PYGAMD_API int pygamd_gen_supported(int64_t F, int64_t De);
PYGAMD_API int pygamd_gen_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De,
                                          size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_gen_forward(const pygamd_csr* g, const void* edge_id, const float* x_src,
                                  int64_t ld_src, int edge_mode, const float* edge_attr,
                                  const float* weight, const float* bias, const float* t,
                                  int64_t t_len, float eps_msg, int64_t n_src, int64_t F,
                                  int64_t De, int want_s2, float* out, float* saved,
                                  void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_gen_backward(const pygamd_csr* g, const void* edge_id_t, const float* x_src,
                                   int64_t ld_src, int edge_mode, const float* edge_attr,
                                   const float* weight, const float* bias, const float* t,
                                   int64_t t_len, float eps_msg, int semi_grad, const float* coef,
                                   int64_t n_dst, int64_t F, int64_t De, int want_grad_edge_attr,
                                   float* grad_x_src, float* grad_edge_attr, float* grad_weight,
                                   float* grad_bias, void* workspace, size_t workspace_bytes,
                                   void* stream);

/* ---- ResGatedGraphConv's gated sum (res_gated_graph_conv.py:107-148) ----------------------------
 * out_i = sum_{j->i} sigmoid(k_i + q_j) * v_j, F = out_channels.  The algebra the kernels rest on:
 *
 * Without edge_dim (res_gated_graph_conv.py:119-122, 148) key, query and value are node-level:
 *   K = lin_key(x_dst) [N_dst, F];  QV = [lin_query(x_src) | lin_value(x_src)] [N_src, 2F], ONE
 *   dense transform with stacked weights.
 * With edge_dim = De the reference runs three Linear(F_in + De, F) on cat([x, edge_attr]) PER EDGE
 * (res_gated_graph_conv.py:143-146).  Each splits into its node and its edge columns,
 *   lin_key(cat[x_i, a]) = Wk_x x_i + bk + Wk_e a       (query, value alike),
 * so for slot k of destination i with source j = col[k], raw features a_k = edge_attr[edge_id[k]]
 *   z_k = K_i + Q_j + Wg a_k,  Wg = Wk_e + Wq_e  [F, De]     (formed by the caller, differentiable)
 *   u_k = V_j + Wv a_k,        Wv = Wv_e         [F, De]
 *   out_i = sum_k sigmoid(z_k) * u_k                          (replaces :128, propagate, and :148)
 * with all three biases folded into K, Q, V.  `weight` is the two bias-free matrices stacked,
 * [2, F, De]: Wg, then Wv (torch.nn.Linear's layout each); NULL with edge_attr NULL and De = 0.
 *
 * forward: ONE launch over the by-destination handle g, one 64-lane wave per row, lanes over the F
 * columns, K_i in registers, per slot ONE gathered 2F row of QV read in place at ld_qv; the edge
 * terms are rebuilt per slot from the raw features with the lane's rows of Wg and Wv in registers.
 * sigmoid is 1 / (1 + expf(-z)): exactly 0.5 at 0, exactly 0 or 1 beyond expf's range.  A split
 * row's chunk partials are summed in chunk order.  out is exactly 0 for a row without slots.
 * Nothing is saved: the backward recomputes the sigmoid from the inputs.
 *
 * backward, with s = sigmoid(z_k), gz = g_i u_k s (1 - s), gu = g_i s, g = grad_out:
 *   pygamd_resgated_backward_dst (the forward's handle): grad_k[i,:] = sum_k gz; with De > 0 also
 *     grad_edge_attr[edge_id[k],:] = Wg^T gz + Wv^T gu (NULL: not wanted), grad_weight [2, F, De]
 *     = (sum gz a_k^T, sum gu a_k^T) from per-workgroup partials reduced in workgroup order; the
 *     grid is a function of (n_rows, n_chunks) only.
 *   pygamd_resgated_backward_src (the transposed handle: col = the destination of every out-slot,
 *     edge_id_t = that form's slot -> original edge map): Q_j, V_j in registers, K_i and g_i
 *     gathered per slot at ld_k and ld_g (two tensors in place, or the halves of one packed
 *     [N_dst, 2F] plane), grad_qv [N_src, 2F] = [sum gz | sum gu], zeros for rows without slots.
 *
 * pygamd_resgated_supported(F, De): F <= 512 and, with De > 0, De <= 32 and F * De <= 2048 (two
 * matrices share the registers gine.hip gives one; no instantiation uses scratch,
 * profiles/resgated_conv.md); otherwise status 2.  k, qv and grad_out have row strides (floats),
 * everything else is contiguous; fp32 data, int32 / int64 indices.  The workspace
 * (pygamd_resgated_workspace_bytes) holds the chunks' partial rows and, with De > 0, the
 * by-destination backward's per-workgroup partials.  No float atomics: bitwise reproducible.
 * Status 1 / 2 / 3 before any device work; n_rows == 0 returns 0.                                */
PYGAMD_API int pygamd_resgated_supported(int64_t F, int64_t De);
PYGAMD_API int pygamd_resgated_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De,
                                               size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_resgated_forward(const pygamd_csr* g, const void* edge_id, const float* k,
                                       int64_t ld_k, const float* qv, int64_t ld_qv,
                                       const float* edge_attr, const float* weight, int64_t n_src,
                                       int64_t F, int64_t De, float* out, void* workspace,
                                       size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_resgated_backward_dst(const pygamd_csr* g, const void* edge_id,
                                            const float* k, int64_t ld_k, const float* qv,
                                            int64_t ld_qv, const float* edge_attr,
                                            const float* weight, const float* grad_out,
                                            int64_t ld_g, int64_t n_src, int64_t F, int64_t De,
                                            float* grad_k, float* grad_edge_attr,
                                            float* grad_weight, void* workspace,
                                            size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_resgated_backward_src(const pygamd_csr* g, const void* edge_id_t,
                                            const float* k, int64_t ld_k, const float* qv,
                                            int64_t ld_qv, const float* edge_attr,
                                            const float* weight, const float* grad_out,
                                            int64_t ld_g, int64_t n_dst, int64_t F, int64_t De,
                                            float* grad_qv, void* workspace,
                                            size_t workspace_bytes, void* stream);

/* ---- CGConv's gated softplus sum (cg_conv.py:81-98) ---------------------------------------------
 * out_i = x_i + aggr_{j->i} sigmoid(lin_f(z_ij)) * softplus(lin_s(z_ij)), z_ij = cat[x_i, x_j, e_ij],
 * F = channels[1].  The reference forms z [E, F_dst + F_src + D], runs the two Linear over its E
 * rows and keeps both results, both activations and the product (cg_conv.py:93-98).  Each Linear
 * splits into its destination, source and edge columns,
 *   lin_f(cat[x_i, x_j, a]) = Wf_i x_i + bf + Wf_j x_j + Wf_e a            (lin_s alike),
 * so with the node-level products
 *   P = [Pf | Ps] = x_dst @ [Wf_i ; Ws_i]^T + [bf ; bs]   [N_dst, 2F]
 *   Q = [Qf | Qs] = x_src @ [Wf_j ; Ws_j]^T               [N_src, 2F]
 * slot k of destination i with source j = col[k] and edge id = edge_id[k] has
 *   zf_k = Pf_i + Qf_j + ef_k,  zs_k = Ps_i + Qs_j + es_k
 *   out_i = epilogue( sum_k sigmoid(zf_k) * softplus(zs_k) )     (replaces :88, propagate, and :90)
 * sigmoid(z) = 1 / (1 + expf(-z)); softplus(z) = z > 20 ? z : log1pf(expf(z)), the rule of
 * torch.nn.functional.softplus.  The edge terms by edge_mode (PYGAMD_GEN_EDGE_*), De = 0 unless
 * LINEAR:
 *   NONE    no edge term: edge_attr = weight = NULL;
 *   LINEAR  ef_k = Wf_e a_k, es_k = Ws_e a_k from the raw features a_k = edge_attr[id, :De];
 *           weight [2, F, De] = Wf_e, then Ws_e (torch.nn.Linear's layout each) sits in registers;
 *   WIDE    [ef_k | es_k] = edge_attr[id, :2F], where edge_attr is the caller's dense product
 *           edge_terms [E, 2F] = a @ [Wf_e ; Ws_e]^T; weight = NULL.
 * The epilogue, once per row (for a split row after its chunk partials were summed in chunk
 * order): scale = 1 (mean) divides by the row's slot count, an empty row stays 0; residual !=
 * NULL adds residual[i, :F] (row stride ld_r).  scale is 0 or 1.
 *
 * forward: ONE launch over the by-destination handle g, one 64-lane wave per row, lanes over the F
 * columns, Pf_i and Ps_i in registers, per slot ONE gathered 2F row of Q read in place at ld_q.
 * Nothing is saved: the backward recomputes both activations from the inputs.
 *
 * backward, with s = sigmoid(zf), p = softplus(zs), g = grad_out[i] (scale = 1: / slot count of i),
 *   gzf = g p s (1 - s),  gzs = g s (zs > 20 ? 1 : sigmoid(zs)):
 *   pygamd_cg_backward_dst (the forward's handle): grad_p[i, :2F] = [sum_k gzf | sum_k gzs] at row
 *     stride ld_gp.  grad_edge (NULL: not wanted) is, LINEAR, grad_edge_attr [E, De] with row id =
 *     Wf_e^T gzf + Ws_e^T gzs and, WIDE, grad_edge_terms [E, 2F] with row id = [gzf | gzs].
 *     grad_weight [2, F, De] (LINEAR; NULL otherwise) = (sum gzf a_k^T, sum gzs a_k^T) from
 *     per-workgroup partials reduced in workgroup order.
 *   pygamd_cg_backward_src (the transposed handle: col = the destination of every out-slot,
 *     edge_id_t = that form's slot -> original edge map): Qf_j, Qs_j in registers, the 2F row P_i
 *     and g_i gathered per slot, grad_q [N_src, 2F] = [sum gzf | sum gzs] at row stride ld_gq,
 *     zeros for rows without slots.  dst_rowptr: the by-destination rowptr at g's index type, for
 *     the slot counts, with scale = 1; NULL with scale = 0.
 * p, q, grad_out, residual, grad_p and grad_q have row strides (floats): with one x for both
 * roles the caller makes ONE [N, 4F] projection [P | Q] and the two backward launches write the
 * halves of ONE [N, 4F] gradient plane.  Everything else is contiguous; fp32 data, int32 / int64
 * indices.
 *
 * pygamd_cg_supported(F, De): F <= 512 and, for LINEAR (De > 0), De <= 32 and F * De <= 2048: no
 * instantiation uses scratch (profiles/cg_conv.md); otherwise status 2, and the caller uses WIDE.
 * There is no workspace query of its own: the entry points take a workspace of
 * pygamd_resgated_workspace_bytes(n_chunks, F, De) bytes (two F-wide partial rows per chunk and,
 * by destination with De > 0, two [F, De] partial matrices per workgroup; forward and by source:
 * De = 0 there) and return status 3 on a smaller one.  No float atomics, every grid a function of
 * (n_rows, n_chunks) only: bitwise reproducible.  Status 1 / 2 / 3 before any device work;
 * n_rows == 0 returns 0.                                                                         */
PYGAMD_API int pygamd_cg_supported(int64_t F, int64_t De);
PYGAMD_API int pygamd_cg_forward(const pygamd_csr* g, const void* edge_id, const float* p,
                                 int64_t ld_p, const float* q, int64_t ld_q, int edge_mode,
                                 const float* edge_attr, const float* weight,
                                 const float* residual, int64_t ld_r, int scale, int64_t n_src,
                                 int64_t F, int64_t De, float* out, void* workspace,
                                 size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_cg_backward_dst(const pygamd_csr* g, const void* edge_id, const float* p,
                                      int64_t ld_p, const float* q, int64_t ld_q, int edge_mode,
                                      const float* edge_attr, const float* weight,
                                      const float* grad_out, int64_t ld_g, int scale,
                                      int64_t n_src, int64_t F, int64_t De, float* grad_p,
                                      int64_t ld_gp, float* grad_edge, float* grad_weight,
                                      void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_cg_backward_src(const pygamd_csr* g, const void* edge_id_t, const float* p,
                                      int64_t ld_p, const float* q, int64_t ld_q, int edge_mode,
                                      const float* edge_attr, const float* weight,
                                      const float* grad_out, int64_t ld_g, int scale,
                                      const void* dst_rowptr, int64_t n_dst, int64_t F,
                                      int64_t De, float* grad_q, int64_t ld_gq, void* workspace,
                                      size_t workspace_bytes, void* stream);

/* ---- FiLMConv's typed feature modulation (film_conv.py:128-161) ----------------------------------
 * x'_i = act(gs_i * W_skip x_i + bs_i) + sum_r aggr_{j in N_r(i)} act(gamma_{r,i} * W_r x_j + beta_{r,i}),
 * [beta_{r,i} | gamma_{r,i}] = film_r(x_i), F = out_channels, R relations.  The reference runs one
 * masked propagate per relation (film_conv.py:139-153), each with a mask, edge_index[:, mask], two
 * [E_r, F] gathers of beta and gamma, one of x_j, the [E_r, F] message and its activation, and
 * 2R + 2 dense transforms.  The activation sits inside the sum and depends on both ends, but every
 * operand is node-level:
 *   H = x_src @ [W_0 ; ... ; W_{R-1}]^T                  [N_src, R F], relation r = columns [rF, (r+1)F)
 *   G = [film_0(x_dst) | ... | film_{R-1}(x_dst)]        [N_dst, R 2F], block r = [beta_r | gamma_r]:
 *       beta first, gamma second, as split(out_channels) gives them (film_conv.py:135, 140).
 * With the default Linear film nets both are one dense product with stacked weights, and with one
 * x in both roles ONE [N, 3RF] plane [H | G] that the kernels read in place through row strides;
 * the two backward launches then write ONE gradient plane of that shape, which feeds ONE
 * input-gradient product.  With a caller's nn, G is the cat of the R module outputs: the module
 * runs on nodes, never on edges.  The skip term act(gs * lin_skip(x_dst) + bs) is node-level too:
 * the caller computes it from a second stacked product x_dst @ [lin_skip ; film_skip]^T [N_dst, 3F]
 * and passes it as residual (row stride ld_r); its gradient is grad_out itself.
 *
 * Per slot k of destination i, with source j = col[k], edge e = edge_id[k] (NULL: e = k) and
 * r = rel[e] (int32 [E], in [0, R): the caller drops other edges when it builds the handle, the
 * kernels check no index, as the other one-pass kernels):
 *   pre = fmaf(gamma_{r,i}, H[j, rF:(r+1)F], beta_{r,i}),   m = act(pre)
 *   out_i = residual_i + sum_k scale[e] * m_k
 * act_mode 0 is the identity (act=None), 1 is ReLU: pre > 0 ? pre : 0 with derivative pre > 0 (0 at
 * exactly 0, as torch).  scale is NULL for add / sum; for mean it is the per-edge float
 * 1 / |N_r(i)|.  The sum does not depend on the relation, so the hub plan and the in-order chunk
 * merge apply unchanged; the residual is added once in the epilogue, for a split row after the
 * merge.  A row without slots gives exactly residual_i (0 without one).
 *
 * pygamd_film_forward: ONE launch over the by-destination handle g of all edges, one 64-lane wave
 *   per row, lanes over the F columns.  A slot gathers ONE F-wide row of H; the lane's
 *   [beta | gamma] stay in registers and are loaded again only when a slot's relation differs from
 *   the one before.  Any in-row order is correct; in a row grouped by relation (a stable
 *   by-destination sort of edges pre-sorted by relation) a wave reloads once per relation present.
 *   Nothing is saved: the backward recomputes the activation from the inputs.
 * pygamd_film_backward_dst: ONE launch over the (relation, destination) pair rows: row p of g holds
 *   the slots of relation pair_rel[p] into destination pair_dst[p] (index arrays at g's index
 *   type, one entry per row; the rows are the non-empty pairs, col = the sources).  With
 *   gm = grad_out_i * act'(pre):  grad_gb[i, r 2F:(r+1) 2F] = [sum gm | sum gm * h], with mean = 1
 *   divided by the pair row's length (once, after the merge for a split row).
 * pygamd_film_backward_src: ONE launch over the (relation, source) pair rows of the flipped graph
 *   (pair_rel, pair_src; col = the destinations; edge_id_t = that handle's slot -> edge map, for
 *   scale): grad_h[j, rF:(r+1)F] = sum scale[e] * grad_out_i * act'(pre) * gamma_{r,i}.
 * Neither backward launch writes the block of a pair that does not occur: the caller zero-fills
 * grad_h and grad_gb once.  h, gb, residual, grad_out, grad_h and grad_gb have row strides
 * (floats); everything else is contiguous; fp32 data, int32 / int64 indices.
 *
 * pygamd_film_supported(F): F <= 512, the lane shapes of the resgated kernels without an edge term
 * (no instantiation uses scratch: profiles/film_conv.md); otherwise status 2.  There is no
 * workspace query of its own: the three entry points take a workspace of
 * pygamd_resgated_workspace_bytes(n_chunks, F, 0) bytes, whose two F-wide partial rows per chunk
 * cover all three launches (F forward and by source, 2F by destination), and return status 3 on a
 * smaller one.  No float atomics, every grid a function of (n_rows, n_chunks) only: bitwise
 * reproducible.  Status 1 / 2 / 3 before any device work; n_rows == 0 returns 0.                  */
PYGAMD_API int pygamd_film_supported(int64_t F);
PYGAMD_API int pygamd_film_forward(const pygamd_csr* g, const void* edge_id, const int32_t* rel,
                                   const float* h, int64_t ld_h, const float* gb, int64_t ld_gb,
                                   const float* scale, const float* residual, int64_t ld_r,
                                   int act_mode, int64_t n_src, int64_t F, int64_t R, float* out,
                                   void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_film_backward_dst(const pygamd_csr* g, const void* pair_rel,
                                        const void* pair_dst, const float* h, int64_t ld_h,
                                        const float* gb, int64_t ld_gb, const float* grad_out,
                                        int64_t ld_g, int act_mode, int mean, int64_t n_src,
                                        int64_t F, int64_t R, float* grad_gb, int64_t ld_ggb,
                                        void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_film_backward_src(const pygamd_csr* g, const void* edge_id_t,
                                        const void* pair_rel, const void* pair_src,
                                        const float* h, int64_t ld_h, const float* gb,
                                        int64_t ld_gb, const float* scale, const float* grad_out,
                                        int64_t ld_g, int act_mode, int64_t n_dst, int64_t F,
                                        int64_t R, float* grad_h, int64_t ld_gh, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* ---- RGATConv's additive relational attention (rgat_conv.py:373-505) ------------------------------
 * The reference's message gathers one weight matrix per edge (rgat_conv.py:397-399:
 * index_select(w, 0, edge_type) is [E, in, H C]), runs two bmm over it, materialises outi and outj
 * as [E, H C] and makes several [E, H] passes for the softmax (rgat_conv.py:401-437).  With dim = 1
 * (additive mode forces it, rgat_conv.py:226-229) every per-edge operand is node-level, W = H C:
 *   P  = x @ [W_0 | ... | W_{R-1}]           [N, R W]   outj[e] = P[j, rW:(r+1)W], outi[e] = P[i, ..]
 *   QI[:, r] = P[:, r] @ q,  KJ[:, r] = P[:, r] @ k   [N, R H]   (rgat_conv.py:401-402; q and k are
 *       full [W, H] matrices that mix heads)
 *   B  = edge_attr @ (W_e^T e)               [E, H]     alpha_edge of rgat_conv.py:405-416
 *   s[e,h] = leaky_relu(QI[i,r,h] + KJ[j,r,h] (+ B[e,h]))           (rgat_conv.py:418-423)
 *   alpha  = softmax of s over ALL edges into i ("across-relation", rgat_conv.py:436-437)
 *   out[i,h,:] = sum_e alpha[e,h] * P[j,r,h,:]                      (rgat_conv.py:500-502)
 * or over those of relation r only ("within-relation", rgat_conv.py:430-435).  The degree factors
 * of mod = 'scaled' / 'f-scaled' (rgat_conv.py:459-471, 488-492) depend on the destination only and
 * are the caller's node-level code on `out`.
 *
 * pygamd_rgat_forward: ONE launch over the by-destination handle g of all edges, one 64-lane wave
 *   per row or per chunk of a long row.  rel is int32 [nnz] in SLOT order, in [0, R): the caller's
 *   to guarantee, the kernels check no index.  The lane keeps QI[i, r, h] of the current relation
 *   in a register and loads it again only when a slot's relation differs from the one before: any
 *   in-row order is correct, a row grouped by relation (a stable by-destination sort of edges
 *   pre-sorted by relation) reloads once per relation present.  Per slot one scalar of KJ, the
 *   optional b [nnz, H] (slot order, NULL: none) and ONE gathered W row of P; online softmax,
 *   non-finite rules (a -inf score has weight 0; a row whose every score is -inf is NaN in its own
 *   (row, head); an empty row is 0), the 1e-16 and the in-order merge of a long row's chunks as
 *   pygamd_han_forward.  Writes out [n_rows, W] and alpha [nnz, H] in slot order.  p, qi and kj
 *   have row strides (floats): three tensors, or the column blocks of one packed [P | QI | KJ].
 * pygamd_rgat_backward_dst: ONE launch over the same rows: d alpha = <g[i,h], P[j,r,h]>,
 *   D = <g[i,h], out[i,h]>, grad_s [nnz, H] = alpha (d alpha - D) * leaky_relu'(pre), the slope
 *   where pre <= 0 — this is also the gradient of b.  No workspace.
 * pygamd_rgat_backward_src: ONE launch over the (relation, node) pair rows of a pair handle g: row
 *   p holds the slots of relation pair_rel[p] at node pair_node[p] (index arrays at g's index
 *   type), col = the other endpoint, slot_map = pair slot -> by-destination slot.  Writes
 *   grad_a[node, r H:(r+1) H] = sum grad_s and, unless grad_p is NULL,
 *   grad_p[node, r W:(r+1) W] = sum alpha * grad_out[col].  On the (relation, source) rows that is
 *   grad_KJ and grad_P; on the (relation, destination) rows with grad_p = NULL (alpha and grad_out
 *   are then not read) it is grad_QI.  Blocks of pairs that do not occur are not written: the
 *   caller zero-fills the planes once.  grad_a and grad_p have row strides, so the three launches
 *   of a backward write ONE gradient plane of the packed plane's shape.
 * pygamd_rgat_pair_scalar: the within-relation normaliser, ONE scalar launch over the (relation,
 *   destination) pair rows (pair_rel, pair_dst, slot_map as above, col = the sources), every pair
 *   row whole.  alpha == NULL (forward): writes pair_stats [n_dst, R, 2H] = the pair's (maximum [H],
 *   1 / (sum + 1e-16) [H]); pairs that do not occur are not written and never read.  Handed to
 *   pygamd_rgat_forward as pair_stats (NULL there: across-relation), a slot's weight is
 *   exp(s - m_pair) / (l_pair + 1e-16): no rescaling, chunk partials merge by addition.  alpha
 *   given (backward): grad_s holds the raw d alpha that pygamd_rgat_backward_dst writes with
 *   within = 1; it becomes alpha (d alpha - D_pair) * leaky_relu'(pre) in place, D_pair = sum alpha
 *   * d alpha over the pair (rgat_conv.py:430-435 differentiated), and grad_qi[i, r H:(r+1) H] =
 *   sum grad_s — this launch then stands in for pygamd_rgat_backward_src on those rows.
 * Launches: across-relation ONE forward, within-relation two; three backward in either mode.
 * Envelope: H C <= 512, H <= 64, otherwise status 2; no limit on R.  There is no workspace query
 * of its own: forward and backward_src take a workspace of pygamd_han_workspace_bytes(n_chunks, H,
 * C) bytes for the launch's handle (a chunk's partial row and its 2 H statistics, the same layout)
 * and return status 3 on a smaller one.
 * No float atomics, every grid a function of (n_rows, n_chunks) only: bitwise reproducible.
 * Status 1 / 2 / 3 before any device work; n_rows == 0 returns 0.                                   */
PYGAMD_API int pygamd_rgat_supported(int64_t H, int64_t C);
PYGAMD_API int pygamd_rgat_forward(const pygamd_csr* g, const int32_t* rel, const float* p,
                                   int64_t ld_p, const float* qi, int64_t ld_qi, const float* kj,
                                   int64_t ld_kj, const float* b, const float* pair_stats,
                                   int64_t n_src, int64_t H, int64_t C, int64_t R, float slope,
                                   float* alpha, float* out, void* workspace,
                                   size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_rgat_backward_dst(const pygamd_csr* g, const int32_t* rel, const float* p,
                                        int64_t ld_p, const float* qi, int64_t ld_qi,
                                        const float* kj, int64_t ld_kj, const float* b,
                                        const float* alpha, const float* grad_out,
                                        const float* out, int64_t n_src, int64_t H, int64_t C,
                                        int64_t R, float slope, int within, float* grad_s,
                                        void* stream);
PYGAMD_API int pygamd_rgat_pair_scalar(const pygamd_csr* g, const void* slot_map,
                                       const void* pair_rel, const void* pair_dst,
                                       const float* qi, int64_t ld_qi, const float* kj,
                                       int64_t ld_kj, const float* b, const float* alpha,
                                       int64_t n_src, int64_t H, int64_t R, float slope,
                                       float* grad_s, float* pair_stats, float* grad_qi,
                                       int64_t ld_gqi, void* stream);
PYGAMD_API int pygamd_rgat_backward_src(const pygamd_csr* g, const void* slot_map,
                                        const void* pair_rel, const void* pair_node,
                                        const float* alpha, const float* grad_s,
                                        const float* grad_out, int64_t n_other, int64_t H,
                                        int64_t C, int64_t R, float* grad_a, int64_t ld_ga,
                                        float* grad_p, int64_t ld_gp, void* workspace,
                                        size_t workspace_bytes, void* stream);

/* ---- mixture messages, aggregate first (gmm_conv.py:154-165, nn_conv.py:119-122) -----------------
 * GMMConv's message is m_e = sum_k w_k(e_attr) (x_j G_k) with Gaussian weights w_k, NNConv's is
 * m_e = x_j reshape(nn(e_attr)), an affine map of the hidden edge features.  Both are a per-edge
 * mixture of K linear maps, m_e = sum_k c[e, k] (x_j W_k), and the reference forms [E, K, M]
 * (GMM) or [E, F, M] (NNConv).  Summing over the slots of a destination BEFORE the maps gives
 *   Z[i, k, :] = sum_{slots s of i} c[edge_id[s], k] * x[col[s], :]     Z [n_rows, K * F]
 *   out[i, :]  = Z[i].reshape(K F) @ W                                 W [K * F, M], by the caller
 * so a slot gathers ONE row of F floats and everything wide is per node.  The gradients:
 *   grad_x = expand over the TRANSPOSED handle (rows = sources, x := grad_out [n_dst, M], edge_id_t)
 *            then a dense product with W's axes permuted;
 *   grad_W = Z^T grad_out (Z recomputed by one more expand);
 *   grad_c[edge_id[s], k] = <wide[i, k F : (k + 1) F], x[col[s], :]>,  wide = grad_out @ W^T.
 *
 * pygamd_mixture_expand: Z over the handle g, one 64-lane wave per row, lane l the columns l + 64 e.
 *   k runs in compile-time tiles (tile * columns per lane <= 32 accumulators in registers); a row's
 *   slots are walked once per tile, the repeated x rows being cache hits; the coefficients of a
 *   slot and tile are loaded once by the first lanes and broadcast.  x [n_cols, F] is read at its
 *   row stride ld_x, coef [E, K] is contiguous in the caller's edge order (edge_id NULL: the slots
 *   are the edges), Z is contiguous.  A split row's chunk partials are summed in chunk order (the
 *   workspace, pygamd_mixture_workspace_bytes = n_chunks * K * F floats).  Rows without slots: 0.
 * pygamd_mixture_coef_grad: over the by-destination handle; wide [n_rows, K * F] contiguous, held
 *   per tile in registers; per slot and tile one gather of x[col[s]], the tile's dot products
 *   reduced across the wave together (halving exchanges, then a butterfly).  Every (edge, k) is
 *   written exactly once; rows without slots load nothing.  No workspace.
 *
 * pygamd_mixture_supported(F, K): 1 <= F <= 512 and 1 <= K <= 256 (no instantiation uses scratch,
 * profiles/mixture_conv.md); otherwise status 2.  fp32 data, int32 / int64 indices.  No float
 * atomics: bitwise reproducible.  Status 1 / 2 / 3 before any device work; n_rows == 0 returns 0. */
PYGAMD_API int pygamd_mixture_supported(int64_t F, int64_t K);
PYGAMD_API int pygamd_mixture_workspace_bytes(int64_t n_chunks, int64_t F, int64_t K,
                                              size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_mixture_expand(const pygamd_csr* g, const void* edge_id, const float* x,
                                     int64_t ld_x, const float* coef, int64_t n_cols, int64_t F,
                                     int64_t K, float* z, void* workspace, size_t workspace_bytes,
                                     void* stream);
PYGAMD_API int pygamd_mixture_coef_grad(const pygamd_csr* g, const void* edge_id,
                                        const float* wide, const float* x, int64_t ld_x,
                                        int64_t n_cols, int64_t F, int64_t K, float* grad_coef,
                                        void* stream);

/* ---- per-graph normalisation: GraphNorm and LayerNorm(mode='graph') --------------------------------
 * (nn/norm/graph_norm.py:72-76, nn/norm/layer_norm.py:82-108).  The reference forms the statistics
 * with two scatters, broadcasts them back with two index selects and makes about eight elementwise
 * passes over [N, F], keeping several of those planes for the backward.  Here the handle g is the
 * BY-GRAPH pointer of a sorted batch vector: rowptr = ptr [B + 1] (pygamd_index2ptr), graph b owns
 * the rows [ptr[b], ptr[b + 1]) of x, col is not read (NULL), and the hub plan over ptr cuts a graph
 * of more than hub_threshold nodes into chunks of hub_chunk nodes.  n is the row count of x.
 *   PYGAMD_NORM_CHANNEL (GraphNorm), per (graph, column): m = mean(x), u = x - mean_scale m,
 *       v = mean(u^2), y = weight u / sqrt(v + eps) + bias;
 *   PYGAMD_NORM_GRAPH (LayerNorm), one mean and variance per graph over its n_g F elements (counts
 *       max(n_g, 1) F): y = (x - m) / sqrt(v + eps) weight + bias; std_eps = 1 divides by
 *       sqrt(v) + eps instead, the reference's formula without a batch vector (layer_norm.py:87-88).
 * weight, bias, mean_scale are [F] or NULL (1, 0, 1); mean_scale must be NULL in GRAPH mode and
 * std_eps 0 in CHANNEL mode.  x, y, grad_y and grad_x have row strides (floats): a column block of
 * a wider plane is read and written in place, all index arithmetic is 64-bit.
 * Statistics: ONE pass of sums shifted by the graph's first row, s1 = sum(x - k), s2 = sum((x -
 * k)^2); GraphNorm's v = sigma^2 + (1 - mean_scale)^2 m^2 needs no pass over u.
 * forward: ONE launch when no graph is a hub — a 64-lane wave per graph, lanes over the columns,
 *   statistics and then y from the same rows; with hub graphs three: the chunks' partial sums go to
 *   the workspace, a merge adds them in chunk order, an apply launch covers the chunks.  Saved for
 *   the backward: mean (m, not mean_scale m) and rstd = 1 / sqrt(v + eps), [B, F] in CHANNEL and
 *   [B] in GRAPH mode.  Empty graphs are legal anywhere and own no rows.
 * backward: the same launch shape over (x, grad_y): with g = grad_y weight, u^ = u rstd,
 *   grad_u = (g - u^ mean_graph(g u^)) rstd and, CHANNEL, grad_x = grad_u - mean_scale
 *   mean_graph(grad_u); GRAPH: both means over all elements of the graph.  grad_weight = sum grad_y
 *   u^, grad_bias = sum grad_y, grad_mean_scale = -sum_graphs m sum_i grad_u (each [F] or NULL: not
 *   wanted; grad_mean_scale NULL in GRAPH mode) come from per-workgroup partials summed by one more
 *   launch in an order that depends on their number only.
 * pygamd_graph_norm_supported(F): 1 <= F <= 512, otherwise status 2.  There is no workspace query:
 *   forward   8 F n_chunks bytes (none without hub graphs),
 *   backward  4 F (2 n_chunks + 3 n_hub + 3 PYGAMD_GRAPH_NORM_BLOCKS) bytes,
 * and a smaller workspace is status 3.  No float atomics, every grid a function of (B, n_chunks)
 * only: bitwise reproducible, and a graph's rows depend on that graph's rows only.  Status 1 / 2 / 3
 * before any device work; n_rows == 0 returns 0.  fp32 data, int32 / int64 ptr.                    */
typedef enum { PYGAMD_NORM_CHANNEL = 0, PYGAMD_NORM_GRAPH = 1 } pygamd_norm_mode;
#define PYGAMD_GRAPH_NORM_BLOCKS 1024
PYGAMD_API int pygamd_graph_norm_supported(int64_t F);
PYGAMD_API int pygamd_graph_norm_forward(const pygamd_csr* g, int mode, const float* x, int64_t ldx,
                                         int64_t n, int64_t F, const float* weight,
                                         const float* bias, const float* mean_scale, float eps,
                                         int std_eps, float* y, int64_t ldy, float* mean,
                                         float* rstd, void* workspace, size_t workspace_bytes,
                                         void* stream);
PYGAMD_API int pygamd_graph_norm_backward(const pygamd_csr* g, int mode, const float* x,
                                          int64_t ldx, const float* grad_y, int64_t ldg, int64_t n,
                                          int64_t F, const float* weight, const float* mean_scale,
                                          float eps, int std_eps, const float* mean,
                                          const float* rstd, float* grad_x, int64_t ldgx,
                                          float* grad_weight, float* grad_bias,
                                          float* grad_mean_scale, void* workspace,
                                          size_t workspace_bytes, void* stream);

/* ---- one step of a linear propagation with its combination as the row epilogue ---------------------
 * The body of the layers that iterate x <- A^ x and combine the iterates (nn/conv/appnp.py:111-133,
 * sg_conv.py:93-95, ssg_conv.py:102-106, tag_conv.py:87-91, lg_conv.py:50, gcn2_conv.py:138-153).
 * The reference runs a step as one propagate and two to three elementwise launches over [N, F];
 * here the combination is the epilogue of the row that was just summed.  Row i of the handle g
 * (pygamd_csr; NULL: status 1), slot k with e(k) = edge_id ? edge_id[k] : k:
 *   t[i,:]   = sum_{k in row i, slot order} (w ? w[e(k)] : 1) * x[col[k],:]
 *   out[i,:] = a * t[i,:]  (+ b * y[i,:] if y)  (+ c * z[i,:] if z)            (if out)
 *   sum[i,:] = (sum_init ? 0 : sum[i,:]) + d * (that value)                      (if sum)
 * Every product and sum is rounded on its own (no contraction), in the order written; a term with a
 * NULL pointer is left out, no coefficient value is special (0 * NaN is NaN) and a row without
 * slots has t = +0.0 and still gets its epilogue.  x is [n_src, ldx]; y, z, out and sum have
 * g->n_rows rows at their own pitches (floats, each >= F): column blocks of wider planes are read
 * and written in place; every row offset is 64-bit.  out may be y or z (the epilogue is row-local);
 * out == x, sum == x and out == sum are status 1.  One wave per row (per group of rows below 64
 * lanes' worth of columns), column tiles past 512 floats; rows of more than hub_threshold slots are
 * walked as the plan's chunks into the workspace (n_chunks * F floats,
 * pygamd_hop_workspace_size) and a second launch adds a row's chunks in chunk order and applies
 * the epilogue once.  The backward of a step is the same call on the by-source handle:
 * grad_x = a * A^T grad_out.  No float atomics: bitwise reproducible.
 * Every width F >= 1 is served.  Before any launch: NULL g / args / x, out and sum both NULL, F < 1,
 * a pitch below F, a negative size, a forbidden alias or a non-zero reserved field -> status 1; a
 * hub plan (n_hub > 0) with a workspace below n_chunks * F floats -> status 3.  n_rows == 0
 * returns 0.  fp32 data, int32 / int64 indices.                                                   */
typedef struct pygamd_hop_args {
  const float* w;     /* [n_edges] or NULL                         */
  const float* x;     /* [n_src, ldx]                              */
  int64_t ldx;
  int64_t n_src;
  int64_t F;
  float a;
  const float* y;     /* [n_rows, ldy] or NULL                     */
  int64_t ldy;
  float b;
  const float* z;     /* [n_rows, ldz] or NULL                     */
  int64_t ldz;
  float c;
  float* out;         /* [n_rows, ldo] or NULL (only sum is wanted) */
  int64_t ldo;
  float* sum;         /* [n_rows, lds] or NULL                     */
  int64_t lds;
  float d;
  int32_t sum_init;   /* 1: sum starts from 0 instead of its old value */
  int64_t reserved[4]; /* 0 */
} pygamd_hop_args;
PYGAMD_API int pygamd_hop_workspace_size(int64_t n_chunks, int64_t F, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_hop(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* a,
                          void* workspace, size_t workspace_bytes, void* stream);

/* ---- §8(f)-1 (next): one hop of uniform neighbour sampling ------------------------------------
 * Device-side counterpart of torch.ops.pyg.neighbor_sample (sampler/neighbor_sampler.py:550-577)
 * on a CSC graph (colptr over destinations, row = source of every slot).  For frontier node
 * frontier[f] the caller provides offsets[f] / offsets[f+1] with offsets[f+1]-offsets[f] =
 * min(deg, k) (or deg for k < 0); the kernel writes, for every sampled slot, the global source
 * id, f (the position of the destination in the frontier) and the CSC slot (-> edge id through
 * the handle's permutation).  deg <= count: all neighbours; else a uniform subset (Floyd's
 * algorithm, counter-based hash of (seed, node, draw): reproducible).  max_per_node = the largest
 * bounded count requested (<= pygamd_sample_max_fanout(); pass 0 when every node takes all).
 * flags bit 0 (the reference's `replace=True`, loader/neighbor_loader.py:209; needs a bounded
 * fan-out): every frontier node with at least one in-neighbour gets exactly k independent uniform
 * draws (offsets from pygamd_sample_counts with replace set).  flags bit 1: the draws of a node
 * depend on its position in the frontier as well (disjoint sampling: one tree per seed).
 * seed_dev (device uint64, may be NULL) is added to `seed` on the device: a captured graph draws a
 * fresh batch at every replay by bumping that word.                                            */
PYGAMD_API int pygamd_sample_max_fanout(void);
PYGAMD_API int pygamd_sample_neighbors(const void* colptr, const void* row, int idx_dtype,
                                       const void* frontier, int64_t n_frontier,
                                       const void* offsets, int64_t max_per_node, uint64_t seed,
                                       int flags, const uint64_t* seed_dev, void* src_out,
                                       void* dstpos_out, void* slot_out, void* stream);

/* Weighted variant: the reference's NeighborLoader(..., weight_attr=...) -> NeighborSampler.
 * edge_weight -> torch.ops.pyg.neighbor_sample(..., edge_weight, ...)
 * (sampler/neighbor_sampler.py:559-571: "neighbors are more likely to get sampled the higher
 * their edge weights").  Same arguments, flags and return codes as pygamd_sample_neighbors, plus
 * weight_csc [E] fp32 in CSC slot order (the caller's edge weights permuted like `row`; finite,
 * >= 0).  With in-degree d and count k:
 *   k < 0, or no replacement and d <= k: every in-neighbour, in slot order (weights unused);
 *   no replacement, d > k: successive sampling in proportion to weight (the first pick is slot j
 *     with probability w_j / W, later picks renormalised over the slots left), realised with
 *     Efraimidis-Spirakis keys log(-ln u_j) - log(w_j), u_j in (0, 1) the counter-based hash of
 *     (seed, node, slot): the k smallest keys, emitted in key order.  Zero-weight slots are
 *     taken only when fewer than k positive-weight slots exist, then uniformly among themselves;
 *   replacement, d > 0: k independent draws, slot j with probability w_j / W; a zero-weight slot
 *     is never drawn; W = 0 (outside the reference's domain) draws uniformly over the d slots.
 * Every node's weights are read, one wave per node; the per-node sum must stay finite in fp32
 * and the in-degree below 2^32.  Draws depend on (seed, node, slot or draw) only (plus the
 * frontier position under flags bit 1, plus seed_dev): reproducible whatever the scheduling.
 * NULL weight_csc returns PYGAMD_ERR_INVALID_ARG, max_per_node > pygamd_sample_max_fanout()
 * PYGAMD_ERR_UNSUPPORTED, both before any launch.                                               */
PYGAMD_API int pygamd_sample_neighbors_weighted(const void* colptr, const void* row,
                                                int idx_dtype, const float* weight_csc,
                                                const void* frontier, int64_t n_frontier,
                                                const void* offsets, int64_t max_per_node,
                                                uint64_t seed, int flags,
                                                const uint64_t* seed_dev, void* src_out,
                                                void* dstpos_out, void* slot_out, void* stream);

/* Temporal variant: the reference's NeighborLoader(..., time_attr=..., input_time=...,
 * temporal_strategy=...) -> torch.ops.pyg.neighbor_sample(..., node_time, edge_time, seed_time,
 * ..., temporal_strategy) (sampler/neighbor_sampler.py:550-571).  Two launches per hop, window
 * then draw.  The CSC must be sorted like the reference's sort_csc (sampler/utils.py:24-42):
 * inside every column the slots ascend in time, ties in edge_index order (a stable lexsort).
 * The time key of slot j is time[row[j]] (level 0: node-level time, `time` [N]) or time[j]
 * (level 1: edge-level time already in CSC slot order, `time` [E]); int64.
 * pygamd_sample_temporal_window: for frontier node v = frontier[f] with seed time
 * t = frontier_time[f] (int64 [n_frontier], the seed time of f's tree: every node of a tree is
 * bounded by its root's time, not its own), the in-edge in slot j is eligible iff key(j) <= t;
 * the eligible slots are the prefix [s, hi) of v's column [s, e), hi the upper bound of t (one
 * wave per node, ceil(log64(deg)) rounds of 64 probes and one ballot).  Then
 *   strategy 0 ('uniform'): lo = s;
 *   strategy 1 ('last'):    lo = max(s, hi - k) for k >= 0, lo = s for k < 0;
 * and cnt[f] is pygamd_sample_counts' rule on the window w = hi - lo: min(w, k) (k < 0: w;
 * replace != 0 and k >= 0: k wherever w > 0, else 0).  lo_out / hi_out / cnt_out are [n_frontier]
 * in idx_dtype.  `n_valid` (device int64, may be NULL): entries past *n_valid get lo = hi = cnt = 0.
 * pygamd_sample_neighbors_temporal: the uniform draws of pygamd_sample_neighbors (same flags,
 * seed, seed_dev, outputs) on the slot range [lo[f], hi[f]) in place of the whole column, offsets
 * being the exclusive scan of cnt: Floyd without replacement (every slot of the window if it
 * holds at most cnt), cnt independent draws with replacement, the whole window for k < 0.  The
 * hash stream is the plain kernel's, so a window equal to the column draws, bit for bit, what
 * pygamd_sample_neighbors draws for the same (seed, node, frontier position).  With 'last' and
 * no replacement the node takes its min(k, w) most recent eligible edges (deterministic); with
 * replacement k draws among them.
 * Rejected before any launch: NULL time / frontier_time / lo / hi (and, when n_frontier > 0, any
 * other NULL pointer) or n_frontier < 0 -> PYGAMD_ERR_INVALID_ARG; a level or strategy other than
 * 0 / 1 -> PYGAMD_ERR_INVALID_ARG; k (max_per_node) > pygamd_sample_max_fanout() ->
 * PYGAMD_ERR_UNSUPPORTED; replacement without a bounded fan-out (k < 0 for the window,
 * max_per_node <= 0 for the draw) -> PYGAMD_ERR_INVALID_ARG; an unknown idx_dtype ->
 * PYGAMD_ERR_INVALID_ARG.                                                                       */
PYGAMD_API int pygamd_sample_temporal_window(const void* colptr, const void* row, int idx_dtype,
                                             const int64_t* time, int level,
                                             const void* frontier, const int64_t* frontier_time,
                                             int64_t n_frontier, int64_t k, int replace,
                                             int strategy, const int64_t* n_valid, void* lo_out,
                                             void* hi_out, void* cnt_out, void* stream);
PYGAMD_API int pygamd_sample_neighbors_temporal(const void* row, int idx_dtype,
                                                const void* frontier, int64_t n_frontier,
                                                const void* lo, const void* hi,
                                                const void* offsets, int64_t max_per_node,
                                                uint64_t seed, int flags,
                                                const uint64_t* seed_dev, void* src_out,
                                                void* dstpos_out, void* slot_out, void* stream);

/* cnt[f] = min(deg(frontier[f]), k) (k < 0: deg; replace != 0 and k >= 0: k wherever deg > 0, else
 * 0) — the per-node sample counts of one hop.
 * `n_valid` (device int64, may be NULL): only the first *n_valid entries of the fixed-capacity
 * `frontier` are real; the rest (which must hold valid node ids, e.g. 0) get count 0.  With it a
 * hop can be sized by the static bound frontier x fan-out and run WITHOUT a host sync.           */
PYGAMD_API int pygamd_sample_counts(const void* colptr, int idx_dtype, const void* frontier,
                                    int64_t n, int64_t k, int replace, const int64_t* n_valid,
                                    void* cnt_out, void* stream);
/* Relabelling of the sampled sources (global -> local ids, new nodes in order of first
 * appearance, deterministic).  `local_map` has one entry per graph node; entries
 * not in the batch hold a value below -(m+1) (the host side uses the type's minimum).
 * phase 0 "claim":  local[src[e]] = max(local[src[e]], -(e+2));
 * phase 1 "flag":   flag_or_scan[e] = (local[src[e]] == -(e+2));        (caller scans inclusively)
 * phase 2 "assign": claimants write local[s] = base + rank and out[rank] = s (out = new nodes);
 * phase 3 "lookup": out[e] = local[src[e]].
 * `m_dev` / `base_dev` (device int64, may be NULL) override min(m, *m_dev) / *base_dev: the
 * number of sampled edges and of batch nodes so far stay on the device, `m` is then the static
 * capacity of the hop (entries past *m_dev flag 0 / look up 0).                                  */
PYGAMD_API int pygamd_relabel(int phase, const void* src, int idx_dtype, int64_t m,
                              const int64_t* m_dev, void* local_map, int64_t* flag_or_scan,
                              int64_t base, const int64_t* base_dev, void* out, void* stream);

/* ---- link-level sampling: negatives and the seed block -----------------------------------------
 * pygamd_sample_negatives replaces the reference's negative draws of LinkNeighborLoader /
 * NeighborSampler.sample_from_edges: `neg_sample` (sampler/neighbor_sampler.py:1051-1096) and
 * `NegativeSampling.sample` (sampler/base.py:906-929, `torch.randint(num_nodes, (n, ))` /
 * `torch.multinomial(weight, n, replacement=True)`).  Writes n node ids into `out` (out_dtype
 * PYGAMD_IDX_I32 / _I64), one thread per draw.  Round r of draw j uses the counter-based hash of
 * (seed, j, r), with seed_dev (device uint64, may be NULL) mixed in as in
 * pygamd_sample_neighbors, and a salt of its own (the hop draws never share the stream).
 *   cdf == NULL: the candidate is uniform over [0, num_nodes): the high word of h * num_nodes for
 *     64 hash bits h, so no id is off its share 1 / num_nodes by more than num_nodes / 2^64;
 *   cdf != NULL (fp64 [num_nodes], the inclusive prefix sums of non-negative weights, cdf[N-1] > 0
 *     and finite): the first i with cdf[i] > u, u uniform in [0, cdf[N-1]) from 53 hash bits
 *     (binary search): node i with probability w_i / W; a node whose weight leaves the fp64 CDF
 *     unchanged (w_i = 0) is never drawn.
 *   node_time != NULL (int64 [num_nodes], node-level time; the reference has none for edge-level
 *     time): draw j is bounded by t = bound[j % n_bound] (int64 [n_bound]) and a candidate c is
 *     accepted iff node_time[c] <= t.  Up to 6 candidates (the reference's first draw and its 5
 *     retries), then `fallback` (the caller's node_time.argmin(): the smallest id among the
 *     earliest nodes, neighbor_sampler.py:1094), which may itself be later than t when no node is
 *     eligible.  The reference's first round accepts `node_time <= seed_time` (its comment says
 *     the same), but its retry rounds mark `node_time >= seed_time` as still invalid
 *     (neighbor_sampler.py:1079, 1089), so a retry whose time equals the bound is rejected there;
 *     every round here uses `<=`.
 * Rejected before any launch (PYGAMD_ERR_INVALID_ARG): n < 0; an out_dtype other than I32 / I64,
 * or I32 with num_nodes > INT32_MAX; bound without node_time; node_time with a NULL bound,
 * n_bound <= 0 or fallback outside [0, num_nodes); and, when n > 0, num_nodes <= 0 or a NULL out.
 * n == 0 otherwise returns PYGAMD_OK.
 *
 * pygamd_unique_inverse replaces `seed.unique(return_inverse=True)` of edge_sample
 * (sampler/neighbor_sampler.py:1004-1008: the seed nodes of an edge batch, cat([src, dst])) on the
 * output of pygamd_index_sort: keys_sorted (idx_dtype, ascending) and perm (int64, keys_sorted[i] =
 * keys[perm[i]]).  Three steps: rank[i] = 1 at the head of every run of equal keys, the inclusive
 * scan of rank (pygamd_cumsum in place, `workspace` of pygamd_cumsum_workspace_bytes(
 * PYGAMD_IDX_I64, n) bytes), then uniq_out[rank[i] - 1] = keys_sorted[i] at the heads,
 * inverse_out[perm[i]] = rank[i] - 1 and *n_unique = rank[n - 1] (device int64).  uniq_out has
 * room for n keys; its first *n_unique are torch.unique's result bit for bit (sorted), and
 * inverse_out (int64 [n]) its inverse.  rank is int64 [n] scratch.  n < 0, an unknown idx_dtype
 * or (n > 0) a NULL pointer -> PYGAMD_ERR_INVALID_ARG, a short workspace -> PYGAMD_ERR_WORKSPACE,
 * before any launch; n == 0 writes nothing.                                                     */
PYGAMD_API int pygamd_sample_negatives(int64_t n, int64_t num_nodes, uint64_t seed,
                                       const uint64_t* seed_dev, const double* cdf,
                                       const int64_t* node_time, const int64_t* bound,
                                       int64_t n_bound, int64_t fallback, int out_dtype,
                                       void* out, void* stream);
PYGAMD_API int pygamd_unique_inverse(const void* keys_sorted, const int64_t* perm, int idx_dtype,
                                     int64_t n, int64_t* rank, void* workspace,
                                     size_t workspace_bytes, void* uniq_out, int64_t* inverse_out,
                                     int64_t* n_unique, void* stream);

/* ---- heterogeneous neighbour sampling: the typed layer -----------------------------------------
 * Device-side counterpart of torch.ops.pyg.hetero_neighbor_sample(..., csc=True, ...) as the
 * reference's NeighborSampler._sample calls it for a HeteroData (sampler/neighbor_sampler.py:
 * 438-548): pyg-lib's sequential loop, hop by hop and, inside a hop, edge type by edge type.
 * Every edge type shares ONE stacked CSC (colptr, row, perm in idx_dtype): node i of node type t
 * has the global id node_base[t] + i, edge type et owns the columns [col_base[et], col_base[et] +
 * N_dst(et)), row holds global source ids and perm each slot's position in its own type's
 * edge_index.  A hop's work list is the concatenation, in edge-type order, of the frontier block of
 * every edge type's destination type: item i belongs to the edge type et with item_begin[et] <= i
 * < item_begin[et + 1] (item_begin: host int64 [n_et + 1], item_begin[0] = 0) and sits at
 * p = i - item_begin[et] of its block.  et_table is host int64 [n_et][4]: frontier_off (where the
 * block starts in `frontier`, the type-major buffer of global ids), col_off (col_base[et] -
 * node_base[dst(et)]: the item's column is frontier[frontier_off + p] + col_off), dst_local (the
 * typed local id of the block's first node) and k (the hop's fan-out, -1 = all, at most
 * pygamd_sample_max_fanout()).  The tables travel in the kernel arguments (n_et <= 64), so ONE
 * launch of each entry point serves a hop whatever the number of edge types.
 * pygamd_hetero_sample_counts: cnt[i] = pygamd_sample_counts' rule on item i's column with its
 *   edge type's k (replace != 0: k wherever deg > 0, for bounded k only).
 * pygamd_hetero_sample_neighbors: offsets = the exclusive scan of cnt ([n + 1]); one wave per item
 *   draws like pygamd_sample_neighbors (same flags: bit 0 replacement, applied only where the
 *   item's k >= 0, bit 1 the item's position salts the draws), keyed by the stacked column id and
 *   the item position, so one node type and one edge type (col_base = 0) draw bit for bit what
 *   pygamd_sample_neighbors draws for the same seed.  Writes per sampled edge the global source
 *   (src_out), the typed local destination dst_local + p (col_out), perm[slot] (edge_out) and,
 *   when fpos_out is not NULL, the destination's position in `frontier`.
 * pygamd_hetero_split: the hop's new nodes (global ids, the first *n_new of new_nodes[m] in order
 *   of first appearance; n_new on the device) partitioned by node type (node_base: host int64
 *   [n_t + 1], the last entry the total, n_t <= 64), stably.  Phase 0 writes the one-hot
 *   flag_or_scan[t * m + j] = (type(new_nodes[j]) == t) (int64 [n_t * m]), which the caller scans
 *   inclusively (pygamd_cumsum) as one vector.  Phase 1 reads that scan: node j of type t gets the
 *   type-major position r = scan[t * m + j] - 1 and the typed local id count_prev[t] (host int64
 *   [n_t]: nodes of type t in the batch before this hop) + its rank among the hop's nodes of type t;
 *   it writes local_map[g] (may be NULL) and typed_out[j] (may be NULL) = that id,
 *   sorted_global[r] = g, sorted_local[r] = g - node_base[t], aux_out[r] = aux_in[j] (int64 payload,
 *   may be NULL), and stats (int64 [n_t + n_et + 1]): the new nodes per type, then
 *   offsets[item_begin[e]] for e = 0 .. n_et (the hop's edge boundaries per edge type, 0 when
 *   offsets is NULL and n_et = 0) — what the caller reads back, once per hop.
 * Rejected before any launch: a bad phase, m < 0, n_t outside [1, 64], n_et outside [0, 64] (1 ..
 * 64 for the sampling entry points), decreasing item_begin, k < -1, negative table entries or a
 * NULL pointer the call needs -> PYGAMD_ERR_INVALID_ARG; k > pygamd_sample_max_fanout() ->
 * PYGAMD_ERR_UNSUPPORTED; an unknown idx_dtype -> PYGAMD_ERR_INVALID_ARG.  An empty work list or
 * m == 0 launches nothing.                                                                      */
PYGAMD_API int pygamd_hetero_sample_counts(const void* colptr, int idx_dtype,
                                           const void* frontier, const int64_t* item_begin,
                                           const int64_t* et_table, int n_et, int replace,
                                           void* cnt_out, void* stream);
PYGAMD_API int pygamd_hetero_sample_neighbors(const void* colptr, const void* row,
                                              const void* perm, int idx_dtype,
                                              const void* frontier, const void* offsets,
                                              const int64_t* item_begin,
                                              const int64_t* et_table, int n_et, uint64_t seed,
                                              int flags, void* src_out, void* col_out,
                                              void* edge_out, void* fpos_out, void* stream);
PYGAMD_API int pygamd_hetero_split(int phase, const void* new_nodes, int idx_dtype, int64_t m,
                                   const int64_t* n_new, const int64_t* node_base,
                                   const int64_t* count_prev, int n_t, int64_t* flag_or_scan,
                                   const void* offsets, const int64_t* item_begin, int n_et,
                                   const int64_t* aux_in, void* local_map, void* typed_out,
                                   void* sorted_global, void* sorted_local, int64_t* aux_out,
                                   int64_t* stats, void* stream);

/* ---- heterogeneous link-level sampling: the typed seed block of an edge batch -------------------
 * pygamd_hetero_link_seeds replaces the head of the reference's edge_sample for a HeteroData
 * (sampler/neighbor_sampler.py:852-937, `input_type is not None`): the two neg_sample calls, the
 * `torch.cat([src, src_neg])` / `torch.cat([dst, dst_neg])`, the `edge_label_time.repeat(...)` of
 * the seed times, and the shift of both endpoints into the stacked global id space of the typed
 * layer above.  For n_pos seed links of edge type (S, rel, D) with typed local endpoints src / dst
 * (idx_dtype [n_pos]) it writes, one thread per slot and in ONE launch,
 *   seeds_out (idx_dtype [n_src + n_dst]): the source block, then the destination block, as global
 *     ids (local id + node_base of the endpoint's type).  Slot j < n_pos of a block is the positive
 *     j; slot n_pos + j is a negative.  n_src = n_pos + num_neg for PYGAMD_LINK_NEG_BINARY and
 *     n_pos otherwise; n_dst = n_pos + num_neg for _BINARY and _TRIPLET and n_pos for _NONE;
 *   seed_time_out (int64 [n_src + n_dst], only when link_time is given): slot j of an endpoint
 *     carries link_time[j % n_pos] (int64 [n_pos]): the reference's `repeat` rule.
 * The negative in slot n_pos + j of endpoint e (0 source, 1 destination) is exactly
 * pygamd_sample_negatives' draw j for the seed `seed * 2 + e` (no seed_dev), that endpoint's
 * num_nodes, cdf (src_cdf / dst_cdf, fp64 [num_nodes] or NULL), node_time (src_node_time /
 * dst_node_time, int64 [num_nodes]: the type's own slice of the node-level time vector, or NULL
 * when the type has no times or time is edge-level: the draw is then unbounded,
 * `node_time.get(type)` in the reference), fallback, and the bound link_time[j % n_pos].
 * ep_table is host int64 [2][3]: num_nodes, node_base and fallback of the source, then of the
 * destination endpoint; it travels in the kernel arguments.
 * Rejected before any launch (PYGAMD_ERR_INVALID_ARG): a mode outside the three below; n_pos < 0
 * or num_neg < 0; num_neg != 0 with _NONE or with n_pos == 0; a NULL ep_table; negative num_nodes
 * or node_base; an unknown idx_dtype, or I32 with node_base + num_nodes > INT32_MAX; a node_time
 * without link_time, or with a fallback outside [0, num_nodes); link_time without seed_time_out;
 * an endpoint that draws from a type without nodes; and, when n_pos > 0, a NULL src, dst or
 * seeds_out.  n_pos == 0 otherwise returns PYGAMD_OK and launches nothing.                      */
#define PYGAMD_LINK_NEG_NONE 0
#define PYGAMD_LINK_NEG_BINARY 1
#define PYGAMD_LINK_NEG_TRIPLET 2
PYGAMD_API int pygamd_hetero_link_seeds(const void* src, const void* dst, int idx_dtype,
                                        int64_t n_pos, int64_t num_neg, int mode,
                                        const int64_t* link_time,
                                        const int64_t* ep_table /*[host]*/,
                                        const double* src_cdf, const double* dst_cdf,
                                        const int64_t* src_node_time,
                                        const int64_t* dst_node_time, uint64_t seed,
                                        void* seeds_out, int64_t* seed_time_out, void* stream);

/* ---- temporal heterogeneous hops: the typed window and the typed draw on a window -------------
 * The reference's NeighborLoader(hetero_data, time_attr=..., temporal_strategy=...) ->
 * hetero_neighbor_sample(..., node_time, edge_time, seed_time, ..., temporal_strategy)
 * (sampler/neighbor_sampler.py:438-471).  Same stacked CSC, work list, item_begin and et_table as
 * above.  Bit et of timed_mask marks edge type et as TIMED: inside each of its columns the slots
 * ascend in time (ties in edge_index order, the reference's sort_csc); the other edge types keep
 * edge_index order.  time is int64: level 0 (node level) one entry per GLOBAL node id, read through
 * row[slot]; level 1 (edge level) one entry per slot.  frontier_time is int64 and aligned with
 * `frontier`: entry fp holds the seed time of the tree of the destination at position fp.
 * pygamd_hetero_sample_temporal_window: one wave per work item.  A timed item's window is the
 *   prefix [s, hi) of its column with time <= frontier_time[fp] (the 64-probe / one-ballot search
 *   of pygamd_sample_temporal_window); strategy 1 ('last') narrows it to its last k slots for
 *   k >= 0, strategy 0 ('uniform') keeps lo = s.  An untimed item's window is its whole column,
 *   whatever the strategy.  cnt is pygamd_hetero_sample_counts' rule on hi - lo.  It takes the
 *   place of the counts launch of a temporal hop.  lo_out, hi_out, cnt_out: [n] in idx_dtype.
 * pygamd_hetero_sample_neighbors_temporal: pygamd_hetero_sample_neighbors on [lo[i], hi[i]) in
 *   place of item i's column: the same key, flags and outputs, so a window that is the whole column
 *   gives the non-temporal draw, and one node type with one edge type gives
 *   pygamd_sample_neighbors_temporal's draw, bit for bit.
 * Rejected before any launch, like the entry points above, plus: level or strategy outside
 * {0, 1}, a timed_mask bit at or above n_et, NULL time / frontier_time / lo / hi ->
 * PYGAMD_ERR_INVALID_ARG.                                                                        */
PYGAMD_API int pygamd_hetero_sample_temporal_window(const void* colptr, const void* row,
                                                    int idx_dtype, const int64_t* time, int level,
                                                    const void* frontier,
                                                    const int64_t* frontier_time,
                                                    const int64_t* item_begin,
                                                    const int64_t* et_table, int n_et,
                                                    uint64_t timed_mask, int replace,
                                                    int strategy, void* lo_out, void* hi_out,
                                                    void* cnt_out, void* stream);
PYGAMD_API int pygamd_hetero_sample_neighbors_temporal(const void* row, const void* perm,
                                                       int idx_dtype, const void* frontier,
                                                       const void* lo, const void* hi,
                                                       const void* offsets,
                                                       const int64_t* item_begin,
                                                       const int64_t* et_table, int n_et,
                                                       uint64_t seed, int flags, void* src_out,
                                                       void* col_out, void* edge_out,
                                                       void* fpos_out, void* stream);

/* ---- heterogeneous layers: every edge type of a HeteroConv in one aggregation --------------------
 * Replaces the aggregation half of the reference's per-edge-type loop, nn/conv/hetero_conv.py:
 * 117-167 calling nn/conv/sage_conv.py:118-152 once per edge type (one propagate each, and one
 * more each in the backward): csrc/hetero_conv.hip.
 * All edge types share ONE stacked CSR in idx_dtype: row row_begin[et] + i is the neighbourhood of
 * destination i under edge type et (row_begin: host int64 [n_et + 1], row_begin[0] = 0; rows are
 * dense, an empty neighbourhood is an empty row), rowptr is [row_begin[n_et] + 1] and col holds the
 * typed local source id of every slot.  The per-edge-type operands travel in the kernel arguments
 * (n_et <= 64), so ONE launch serves a layer whatever the number of edge types.
 * pygamd_hetero_spmm: out[et][i, :F] = sum (or mean: the sum / max(deg, 1)) over the row's slots of
 *   x[et][col[slot], :F].  x / out: host arrays [n_et] of device pointers (the source matrix of the
 *   edge type's source node type; row 0 of the edge type's output block, which may be a column
 *   block of a wider matrix); et_table: host int64 [n_et][4] = ldx, n_src, mean (0 / 1), ldo.  The
 *   lane shape is the one pygamd_spmm_csr picks for (F, the least aligned operand of the table),
 *   slot order and mean epilogue are that kernel's: equal shapes give equal bits.  A source id
 *   outside [0, n_src) sets *err_flag (device int32, optional) to 1 and reads row 0 (nothing when
 *   n_src = 0).  Rows of any degree are walked by one wave (no two-stage hub path).
 * pygamd_hetero_spmm_backward: the gradient of every source matrix in one launch, one wave per
 *   stacked source node and no atomics.  Node j of source node type t is the stacked node
 *   src_begin[t] + j (src_begin: host int64 [n_nt + 1], n_nt <= 64); rowptr_t [src_begin[n_nt] + 1]
 *   / col_t are the transposed structure: the slots of a stacked node name stacked (et, i) rows, in
 *   the order their contributions are added.  grad_x[t][j, :F] = sum over the slots r of
 *   grad[et(r)][r - row_begin[et(r)], :F] (for a mean edge type divided by max(deg(r), 1), deg from
 *   the forward rowptr); nodes without slots get zeros.  grad / grad_x: host arrays of device
 *   pointers ([n_et] / [n_nt]); et_table: host int64 [n_et][2] = ldg, mean; ld_grad_x: host int64
 *   [n_nt].
 * Rejected before any launch: n_et or n_nt above 64 -> PYGAMD_ERR_UNSUPPORTED; n_et / n_nt <= 0, a
 * block table that does not start at 0 or decreases, F < 0, a leading dimension below F or above
 * INT32_MAX, n_src < 0, a mean flag other than 0 / 1, an unknown idx_dtype or a NULL pointer the
 * call needs -> PYGAMD_ERR_INVALID_ARG.  No rows or F = 0 launches nothing.                      */
PYGAMD_API int pygamd_hetero_spmm(const void* rowptr, const void* col, int idx_dtype,
                                  const int64_t* row_begin, const float* const* x,
                                  float* const* out, const int64_t* et_table, int n_et, int64_t F,
                                  int32_t* err_flag, void* stream);
PYGAMD_API int pygamd_hetero_spmm_backward(const void* rowptr_t, const void* col_t,
                                           const void* rowptr, int idx_dtype,
                                           const int64_t* row_begin, const float* const* grad,
                                           const int64_t* et_table, int n_et,
                                           const int64_t* src_begin, float* const* grad_x,
                                           const int64_t* ld_grad_x, int n_nt, int64_t F,
                                           void* stream);

/* ---- HGTConv: the typed relation transform of every edge type in one launch ----------------------
 * Replaces nn/conv/hgt_conv.py:118-154 (_construct_src_node_feat: for K and again for V a cat over
 * the edge types, a transpose copy to [H * sum N, D], an int64 type vector, a grouped GEMM over
 * H * T segments and a transpose back): csrc/hgt.hip.  For edge type e of the call with n_e source
 * rows at stacked offset src_off[e] = sum of the n of the edge types before it:
 *   kv[src_off[e] + j, 0, h, :] = k[e][j, h, :] @ wk[h * T + widx(e)]       (D x D)
 *   kv[src_off[e] + j, 1, h, :] = v[e][j, h, :] @ wv[h * T + widx(e)]
 * k / v: host arrays [n_et] of device pointers to rows of H * D floats with ONE row stride per edge
 * type (the k and v column blocks of the [N, 3 H D] projection, or contiguous tensors); wk / wv are
 * the parameters as they are, [H * T, D, D] with T the number of edge types of the metadata and
 * widx(e) the metadata position of e; kv is [S, 2 H D] contiguous, the packed key | value table
 * pygamd_transformer_* reads with ld = 2 H D.  et_table: host int64 [n_et][4] = ld, n_e, widx,
 * position of the source node type in nt_table (read by the backward only).  Exact fp32 on
 * v_mfma_f32_16x16x4_f32 (an fmaf chain per output, reduction order fixed), a D that is not a
 * multiple of 16 is padded inside.
 * pygamd_hgt_relation_backward (no floating-point atomics, bitwise reproducible):
 *   grad_k[t][j, h, :] = sum over the edge types e of the call with source node type t, in call
 *   order, of grad_kv[src_off[e] + j, 0, h, :] @ wk[h * T + widx(e)]^T, accumulated in registers
 *   and written once at row stride nt_table[t][1] (likewise grad_v): nt_table is host int64
 *   [n_nt][2] = rows, ld; a node type no edge type reads gets zeros.  n_nt = 0 skips these.
 *   grad_wk[h * T + widx(e)] = sum_j k[e][j, h, :]^T . grad_kv[src_off[e] + j, 0, h, :] (likewise
 *   grad_wv): per-workgroup partial matrices in the workspace (pygamd_hgt_workspace_bytes for the
 *   same et_table), summed in chunk order; EVERY matrix of both [H * T, D, D] gradients is written,
 *   zeros for edge types that are not in the call.  grad_wk = grad_wv = NULL skips these.
 * Supported (pygamd_hgt_supported): H * D <= 512, H <= 64, D <= 128; otherwise, and for n_et or
 * n_nt above 64, PYGAMD_ERR_UNSUPPORTED.  n_et <= 0, T < n_et, H * T > 65535, a widx outside
 * [0, T) or named twice, negative rows, rows of an edge type that differ from its node type's, a
 * row stride below H * D or above INT32_MAX, a NULL pointer the call needs ->
 * PYGAMD_ERR_INVALID_ARG; a short workspace -> PYGAMD_ERR_WORKSPACE; all before any launch.  An
 * edge type with n_e = 0 is legal; a call without rows launches nothing in the forward.         */
PYGAMD_API int pygamd_hgt_supported(int64_t H, int64_t D);
PYGAMD_API int pygamd_hgt_workspace_bytes(const int64_t* et_table, int n_et, int64_t H, int64_t D,
                                          size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_hgt_relation_forward(const float* const* k, const float* const* v,
                                           const int64_t* et_table, int n_et, const float* wk,
                                           const float* wv, int64_t T, int64_t H, int64_t D,
                                           float* kv, void* stream);
PYGAMD_API int pygamd_hgt_relation_backward(const float* const* k, const float* const* v,
                                            const int64_t* et_table, int n_et, const float* wk,
                                            const float* wv, int64_t T, int64_t H, int64_t D,
                                            const float* grad_kv, float* const* grad_k,
                                            float* const* grad_v, const int64_t* nt_table,
                                            int n_nt, float* grad_wk, float* grad_wv,
                                            void* workspace, size_t workspace_bytes,
                                            void* stream);

/* ---- a18: one-pass multi-reduce (FusedAggregation) ---------------------------------------------
 * nn/aggr/fused.py:191-336 shares the group count, the sum and the sum of squares between
 * sum / mean / var / std / min / max.  Here ONE read of the rows produces all requested statistics
 * of every group: rows of group g are x[perm[k]] for k in [rowptr[g], rowptr[g+1]) (`perm` =
 * the stable sort permutation of the aggregation index, or NULL when the rows are already
 * grouped, i.e. the `ptr` form).  Null outputs are skipped; empty groups give 0.  Outputs are
 * [n_rows, F] with leading dimension ldo.                                                      */
PYGAMD_API int pygamd_multi_reduce_csr(const void* rowptr, const void* perm, int idx_dtype,
                                       const float* x, int64_t ldx, int64_t n_rows, int64_t F,
                                       float* out_sum, float* out_sq, float* out_min,
                                       float* out_max, int64_t ldo, void* stream);

/* ---- a17 / f3: the dense feature transform on the fp32 matrix cores ---------------------------
 * `F.linear(x, weight, bias)` of nn/dense/linear.py:121-127 — what SAGEConv's `lin_l(agg) +
 * lin_r(x)` (sage_conv.py:134-139), GCNConv's `lin(x)` (gcn_conv.py:260) etc. end in — and its
 * two gradients, written for v_mfma_f32_32x32x2_f32 (exact fp32).  Row-major, explicit leading
 * dimensions in elements, so halves of wider `[agg | x]` buffers are read / written in place.
 *   forward : out[M, N] = act(x[M, K] @ w[N, K]^T + bias[N]);  relu != 0 fuses the activation
 *             (basic_gnn.py:258-266), accumulate != 0 adds onto `out`.
 *   dgrad   : out[M, K] = g[M, N] @ w[N, K], the weight handed over TRANSPOSED (w_t[K, N],
 *             contiguous rows); columns [0, n_scaled) are multiplied by row_scale[row] in the
 *             epilogue (the 1/deg of a mean aggregation that follows, utils/_scatter.py:72-80);
 *             relu_mask ([M, ld_mask] or NULL): out[r, c] = 0 where relu_mask[r, c] <= 0, applied
 *             last — the backward of the ReLU whose output relu_mask is (basic_gnn.py:262-263);
 *             relu_bits (or NULL) is the same mask as one bit per element in the tiled layout of
 *             pygamd_spmm_args.relu_bits (ld_bits >= ceil(K / 32)); at most one of the two.
 *   wgrad   : out[N, K] = g[M, N]^T @ x[M, K]; deterministic (split over M, slabs summed in
 *             order); workspace from the _workspace_bytes query.  bias_grad ([N] or NULL)
 *             receives the column sums of g (the bias gradient of the same Linear,
 *             nn/dense/linear.py:121-127 backward) from the same pass over g: per-split sums taken
 *             while the rows are staged, added in split order (deterministic).                 */
/* Arithmetic of the three entry points below and of pygamd_sage_layer_forward (process-wide):
 *   PYGAMD_GEMM_FP32       (default) v_mfma_f32_32x32x2_f32: IEEE fp32 products and sums, bitwise
 *                          an fmaf chain over k;
 *   PYGAMD_GEMM_SPLIT_BF16 every fp32 operand as the exact sum of three bf16 terms, the six
 *                          leading cross products on v_mfma_f32_32x32x16_bf16 with fp32
 *                          accumulation: the same fp32 inputs and outputs, error against fp64 at
 *                          or below the fmaf chain's (profiles/r02_split_bf16_accuracy_probe.txt),
 *                          not bitwise equal to it; an Inf operand yields NaN.               */
#define PYGAMD_GEMM_FP32 0
#define PYGAMD_GEMM_SPLIT_BF16 1
PYGAMD_API int pygamd_set_gemm_mode(int mode);
PYGAMD_API int pygamd_get_gemm_mode(void);
/* Workspace of the forward / dgrad2 entry points (both are one "NT" product out[M, N_out] over a
 * reduction of K_red columns): 0 when the output has enough row tiles to fill the chip (every
 * full-batch layer); for few rows (sampled blocks of 1 k .. 16 k rows, Cora-sized inputs) room for
 * the partial tiles of a split over the reduction, combined in slice order by a second pass
 * (deterministic).  Without it (NULL) the launch runs unsliced: same result, fewer workgroups.  */
PYGAMD_API int pygamd_linear_nt_workspace_bytes(int64_t M, int64_t N_out, int64_t K_red,
                                                size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_linear_forward(const float* x, int64_t ldx, const float* w, int64_t ldw,
                                     const float* bias, int64_t M, int64_t K, int64_t N, int relu,
                                     int accumulate, float* out, int64_t ldo, void* workspace,
                                     size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_linear_dgrad(const float* g, int64_t ldg, const float* w_t, int64_t ldwt,
                                   const float* row_scale, int64_t n_scaled, int64_t M, int64_t N,
                                   int64_t K, int accumulate, const float* relu_mask,
                                   int64_t ld_mask, const uint32_t* relu_bits, int64_t ld_bits,
                                   float* out, int64_t ldo, void* stream);
/* pygamd_linear_dgrad with a second output: out_scaled[M, K] (or NULL) = out * row_scale[row] in
 * every column (row_scale required then; not with accumulate).  The one-kernel layer backward
 * (pygamd_sage_layer_fused with mask_bits) gathers the 1/deg-scaled gradient rows and takes the
 * unscaled ones as its root operand: this writes both from one pass.                             */
PYGAMD_API int pygamd_linear_dgrad2(const float* g, int64_t ldg, const float* w_t, int64_t ldwt,
                                    const float* row_scale, int64_t n_scaled, int64_t M,
                                    int64_t N, int64_t K, int accumulate, const float* relu_mask,
                                    int64_t ld_mask, const uint32_t* relu_bits, int64_t ld_bits,
                                    float* out, int64_t ldo, float* out_scaled, int64_t ld_scaled,
                                    void* workspace, size_t workspace_bytes, void* stream);
PYGAMD_API int pygamd_linear_wgrad_workspace_bytes(int64_t M, int64_t N, int64_t K,
                                                   size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_linear_wgrad(const float* g, int64_t ldg, const float* x, int64_t ldx,
                                   int64_t M, int64_t N, int64_t K, int accumulate,
                                   int wgs_per_cu /* 0 / 2: fill the chip; 1: leave room for a
                                   bandwidth-bound kernel running on another stream */,
                                   float* out, int64_t ldo, float* bias_grad, void* workspace,
                                   size_t workspace_bytes, void* stream);
/* The same against two operands side by side: out[N, K1 + K2] = g^T @ [x | x2] (x2 NULL, K2 = 0:
 * identical to pygamd_linear_wgrad) — SAGEConv's `[grad W_l | grad W_r]` (sage_conv.py:134-139
 * backward) from the aggregated rows and the layer input where they are, without a concatenated
 * copy.  Workspace as for K = K1 + K2.                                                           */
PYGAMD_API int pygamd_linear_wgrad2(const float* g, int64_t ldg, const float* x, int64_t ldx,
                                    int64_t K1, const float* x2, int64_t ldx2, int64_t K2,
                                    int64_t M, int64_t N, int accumulate, int wgs_per_cu,
                                    float* out, int64_t ldo, float* bias_grad, void* workspace,
                                    size_t workspace_bytes, void* stream);

/* ---- f1b: static-shape ("slot") sampled batches — csrc/minibatch.hip ---------------------------------
 * The sampling contract of pygamd_sample_neighbors (sampler/neighbor_sampler.py:550-577: per
 * frontier node a uniform min(deg, k)-subset of its in-neighbours, no replacement) with an output
 * layout in which a whole training step has the same shapes and row ranges every batch and reads
 * nothing back to the host.  Batch-local node ids are BLOCK POSITIONS: block 0 = the B seeds,
 * block h + 1 = the fanout[h] slots of every position of block h; bases[b] = first id of block b
 * (bases[hops + 1] = all rows R); slot e (global slot index, hop by hop) is row B + e.
 *   node_g  [R]   int64  graph node held by row r, -1 = hole (a duplicate, or nothing sampled)
 *   src_g   [R-B] int64  graph node sampled into slot e, -1 = slot not filled
 *   src_id  [R-B] int32  row that holds the features of slot e's source (the earliest occurrence)
 *   row_end [bases[hops]] int32  row r's slots are [row_begin[r], row_end[r]) with the static
 *           row_begin[r] = (bases[b + 1] - B) + (r - bases[b]) * fanout[b] for r in block b:
 *           pass them as pygamd_spmm_args.rowptr / .rowend with col = src_id
 *   inv_cnt [bases[hops]] float  1 / max(row_end - row_begin, 1)
 *   local_map [num_nodes] int64, zero-initialised ONCE: duplicates resolve through atomicMax of
 *           epoch << 32 | (2^32 - 1 - row) — never reset; *epoch_dev (device int64, >= 1) must
 *           grow from batch to batch and also salts the draws.
 * Call order per batch: seed, then per hop sample + resolve (resolve also counts, per source row,
 * the entries of the transposed CSRs the hop belongs to: counts[c], c < n_counts), then transpose
 * (one scan launch + one fill launch for all n_csr transposed CSRs; CSR c covers the slots
 * [0, n_slots[c]) with sources in rows [0, n_src_rows[c]); counts / cursor zeroed by the caller),
 * then gather (x[node_g] -> out, holes = zero rows).                                               */
PYGAMD_API int pygamd_slots_max_fanout(void);
PYGAMD_API int pygamd_slots_max_hops(void);
PYGAMD_API int pygamd_slots_seed(const void* seeds, int idx_dtype, int64_t B,
                                 const int64_t* epoch_dev, int64_t* local_map, int64_t* node_g,
                                 void* stream);
PYGAMD_API int pygamd_slots_sample(const void* colptr, const void* row, int idx_dtype,
                                   const int64_t* node_g, int64_t frontier_base,
                                   int64_t n_frontier, int fanout, int64_t slot_base, int64_t B,
                                   uint64_t seed, int hop, const int64_t* epoch_dev,
                                   int64_t* local_map, int64_t* src_g, int32_t* row_end,
                                   float* inv_cnt, void* stream);
PYGAMD_API int pygamd_slots_resolve(const int64_t* src_g, int64_t slot_base, int64_t n_slots,
                                    int64_t B, const int64_t* epoch_dev,
                                    const int64_t* local_map, int32_t* src_id,
                                    int64_t* node_g, int32_t* const* counts /*[host]*/,
                                    int n_counts, void* stream);
PYGAMD_API int pygamd_slots_gather(const float* x, int64_t ldx, int64_t F, const int64_t* node_g,
                                   int64_t n_rows, float* out, int64_t ldo, void* stream);
PYGAMD_API int pygamd_slots_transpose(const int64_t* src_g, const int32_t* src_id, int hops,
                                      const int32_t* fanout /*[host]*/,
                                      const int64_t* bases /*[host, hops + 2]*/, int n_csr,
                                      const int64_t* n_slots /*[host]*/,
                                      const int64_t* n_src_rows /*[host]*/,
                                      int32_t* const* counts /*[host]*/,
                                      int32_t* const* cursor /*[host]*/,
                                      int32_t* const* ptr /*[host]*/,
                                      int32_t* const* col /*[host]*/, void* stream);

/* ---- f1c: the loss and optimizer ends of a captured batch step — csrc/train.hip ----------------------
 * The reference's mini-batch loop (examples/multi_gpu/distributed_sampling.py:104-117) ends every
 * batch with `loss = F.cross_entropy(out, batch.y[:batch.batch_size]); loss.backward();
 * optimizer.step()` (torch.optim.Adam).  Inside a hipGraph every launch costs ~5 us, so these two
 * ends are 2 + 1 launches here (before: 7 ATen launches for the loss of 1024 rows, 42 us of
 * multi-tensor Adam for 0.2 M parameters, a concatenation / transpose launch per weight use).
 *
 * pygamd_cross_entropy_step: loss[0] = mean_r (logsumexp(logits[r, :]) - logits[r, label_r]),
 * grad[r, c] = (softmax(logits[r, :])[c] - [c == label_r]) / B — F.cross_entropy (reduction
 * 'mean', no class weights, no label smoothing) and its backward for an upstream gradient of 1.
 * label_r = y[label_idx[r]] (label_idx NULL: y[r]) — the seeds' labels are read from the graph's
 * label vector, no gathered copy.  row_idx (optional): row r of the loss is logits[row_idx[r], :]
 * (n_logit_rows = the rows `logits` holds) — `F.cross_entropy(out[train_idx], y[train_idx])` of a
 * full-batch model without the gathered copy of the rows; grad stays compact ([B, C]).  A label outside [0, C) sets *err_flag (device int32, optional)
 * and contributes neither loss nor gradient (no ignore_index: the mean divides by B).  The row
 * losses are added up in row order by a second, one-workgroup launch (deterministic; a
 * last-workgroup-done ticket inside one launch cost 28 us in fences for 1,024 rows).  step_counter
 * (device int64, optional) is incremented by one per call — the optimizer's step count of a
 * captured step (pygamd_adam_step's step_dev), kept by a launch the step has anyway.
 * Workspace: ..._workspace_bytes(B) (the row losses).                                             */
PYGAMD_API int pygamd_cross_entropy_step_workspace_bytes(int64_t B, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_cross_entropy_step(const float* logits, int64_t ld, const int64_t* row_idx,
                                         int64_t n_logit_rows, int64_t B, int64_t C,
                                         const int64_t* y, const int64_t* label_idx, float* grad,
                                         int64_t ldg, float* loss, void* workspace,
                                         size_t workspace_bytes, int32_t* err_flag,
                                         int64_t* step_counter, void* stream);
/* pygamd_adam_step: torch.optim.Adam (amsgrad / maximize off; weight_decay = the L2 form) over ONE
 * flat float32 buffer of n parameters with gradients `grad * grad_scale` (grad_scale = 1 / world
 * size after a SUM all-reduce).  The step count is read from the device: step = *step_dev -
 * step_base >= 1 (a captured step bumps *step_dev itself; bias corrections in float32 as the
 * capturable optimizer evaluates them).  `transposed` (optional): for each of n_segments (<=
 * PYGAMD_ADAM_MAX_SEGMENTS) row-major blocks param[seg_off .. + rows * cols) the updated values
 * are also stored transposed at transposed[seg_t_off + c * rows + r] — the W^T operand of
 * pygamd_linear_dgrad, kept current without a transpose launch per use.                          */
#define PYGAMD_ADAM_MAX_SEGMENTS 8
PYGAMD_API int pygamd_adam_step(float* param, const float* grad, float* exp_avg,
                                float* exp_avg_sq, int64_t n, const int64_t* step_dev,
                                int64_t step_base, double lr, double beta1, double beta2,
                                double eps, double weight_decay, double grad_scale,
                                float* transposed, int n_segments,
                                const int64_t* seg_off /*[host]*/,
                                const int32_t* seg_rows /*[host]*/,
                                const int32_t* seg_cols /*[host]*/,
                                const int64_t* seg_t_off /*[host]*/, void* stream);

/* ---- f3: SAGEConv layer forward in one kernel ----------------------------------------------------
 * y[i, :] = act([aggr_{j->i} x[j] | x_root[i]] @ w[Fo, 2F]^T + bias) — `propagate` + `lin_l(agg)
 * + lin_r(x)` of nn/conv/sage_conv.py:134-139 with the aggregated 32-row tile handed from the
 * gather phase to the MFMA loop through LDS.  `graph` describes the aggregation exactly as for
 * pygamd_spmm_csr (reduce SUM or MEAN, no edge weights; x / ldx = the rows that are gathered;
 * out / ldo = the global agg buffer, always required: hub rows are aggregated there first by the
 * two-stage hub kernels, and with save_agg != 0 every row is stored there once for the weight
 * gradient).
 * save_agg = PYGAMD_AGG_GIVEN ("rows given"): out / ldo ALREADY holds the aggregated row of every
 * destination row, in the final (mean-scaled) form a save_agg = 1 launch on the same graph and
 * gather source leaves there — the kernel reads those rows as a coalesced stream and does not
 * gather: rowptr, col, x and the hub plan are not read (rowptr / col / x may be NULL), the hub
 * pre-pass does not run and nothing is stored back.  y, relu_bits_out, y_scaled and
 * compressed_out are bit for bit those of the save_agg = 1 launch that wrote the rows.  Needs
 * out != NULL and ldo >= F (PYGAMD_ERR_INVALID_ARG); not with x_format = PYGAMD_X_COMPRESSED
 * (PYGAMD_ERR_UNSUPPORTED).  The workspace query leaves the hub partials out in this mode.
 * Supported: F % 4 == 0, F <= 256, Fo <= 256, 16-byte aligned operands (query below);
 * otherwise PYGAMD_ERR_UNSUPPORTED and the caller runs pygamd_spmm_csr + pygamd_linear_forward.
 * relu_bits_out (ceil(n_rows / 32) * ld_bits * 32 words or NULL; needs relu != 0): [y > 0] as
 * one bit per element in the tiled layout of pygamd_spmm_args.relu_bits — the form of the ReLU mask
 * that the backward's pygamd_spmm_csr / pygamd_linear_dgrad epilogues take
 * (ld_bits >= ceil(Fo / 32)).
 * Workspace: pygamd_sage_layer_fused_workspace_bytes (pygamd_spmm_csr_workspace_bytes(graph)
 * suffices in PYGAMD_GEMM_FP32 mode).                                                              */
#define PYGAMD_AGG_GIVEN 2 /* save_agg: read the aggregated rows from out / ldo, do not gather */
PYGAMD_API int pygamd_sage_layer_forward_supported(int64_t F, int64_t Fo, int reduce);
PYGAMD_API int pygamd_sage_layer_forward(const pygamd_spmm_args* graph, const float* x_root,
                                         int64_t ld_root, const float* w, int64_t ldw,
                                         const float* bias, int64_t Fo, int relu, int save_agg,
                                         float* y, int64_t ldy, uint32_t* relu_bits_out,
                                         int64_t ld_bits, void* workspace,
                                         size_t workspace_bytes, void* stream);

/* The same kernel with every epilogue it has, as one argument block (zero-initialise, fill what is
 * needed; save_agg as for pygamd_sage_layer_forward, PYGAMD_AGG_GIVEN included).  Beyond it:
 *  - mask_bits: y = bit ? y : 0 from a one-bit-per-element ReLU mask in the tiled layout of
 *    pygamd_spmm_args.relu_bits.  With the transposed graph, x = the (degree-scaled) gradient rows
 *    and w = [W_l^T | W_r^T] this launch IS a SAGEConv layer's input gradient,
 *      grad_x = [relu'(x)] * ((A^T D^-1 g) W_l + g W_r)
 *    (sage_conv.py:134-139 differentiated; the aggregation commutes with the right-multiplication
 *    by W_l), i.e. pygamd_linear_dgrad + the transposed pygamd_spmm_csr in one pass over the graph.
 *  - y_scaled / row_scale: a second copy y * row_scale[row] of the output (the next such launch
 *    gathers the 1/deg-scaled rows and takes the unscaled ones as its root operand).
 *  - arithmetic: the transform phase follows pygamd_set_gemm_mode.  PYGAMD_GEMM_SPLIT_BF16 runs
 *    the split schedule (csrc/sage_fused.hip (B): every operand element converted to three bf16
 *    terms ONCE where it is produced, the weight by a pre-pass into the workspace) for dense rows
 *    in and out; it needs the workspace of pygamd_sage_layer_fused_workspace_bytes
 *    (PYGAMD_ERR_WORKSPACE otherwise).
 * (The schedules that were measured and not adopted, and the kernels' timing probes, are reachable
 * through include/pyg_amd_lab.h only — not part of this boundary.)                                */
typedef struct pygamd_sage_fused_args {
  const float* x_root;       /* [n_rows, F] root rows                   */
  int64_t ld_root;
  const float* w;            /* [Fo, 2F] = [W_l | W_r]                  */
  int64_t ldw;
  const float* bias;         /* [Fo] or NULL                            */
  int64_t Fo;
  int32_t relu;
  int32_t save_agg;          /* 0, 1 (store the rows) or PYGAMD_AGG_GIVEN (read them back)     */
  float* y;                  /* [n_rows, Fo]                            */
  int64_t ldy;
  uint32_t* relu_bits_out;   /* NULL or [y > 0] as bits (needs relu)    */
  int64_t ld_bits_out;
  const uint32_t* mask_bits; /* NULL or the mask applied to y           */
  int64_t ld_mask_bits;
  const float* row_scale;    /* [n_rows], with y_scaled                 */
  float* y_scaled;           /* NULL or [n_rows, Fo]                    */
  int64_t ldy_scaled;
  uint32_t* compressed_out;  /* NULL or [n_rows, ld_compressed] words: y once more, in the format
                                of pygamd_rows_compress (the next layer's gather source).  Needs
                                Fo % 32 == 0.  With graph->x_format = PYGAMD_X_COMPRESSED the
                                gather source itself is such a block (F % 4 == 0, F <= 256).
                                Both run the fp32-instruction schedule whatever the mode.      */
  int64_t ld_compressed;
} pygamd_sage_fused_args;
/* hub partials (pygamd_spmm_csr_workspace_bytes) + the weight's bf16 term planes of the split
 * schedule (6 bytes per padded weight element; 768 KiB at F = Fo = 256)                          */
PYGAMD_API int pygamd_sage_layer_fused_workspace_bytes(const pygamd_spmm_args* graph,
                                                       const pygamd_sage_fused_args* f,
                                                       size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_sage_layer_fused(const pygamd_spmm_args* graph,
                                       const pygamd_sage_fused_args* f, void* workspace,
                                       size_t workspace_bytes, void* stream);

/* ---- geometric searches: knn, radius, fps — csrc/cluster.hip ---------------------------------------
 * The reference's fps / knn / knn_graph / radius / radius_graph / nearest only forward to
 * torch.ops.pyg.fps / knn / radius / nearest (nn/pool/__init__.py:85, 140, 199, 265, 331, 375) and
 * DynamicEdgeConv calls torch.ops.pyg.knn in every forward (nn/conv/edge_conv.py:138): pyg-lib,
 * which has no ROCm build.  These three entry points are those operators.
 * Examples are contiguous row ranges: example e owns the rows [ptr_x[e], ptr_x[e + 1]) of x and the
 * rows [ptr_y[e], ptr_y[e + 1]) of y (pointer vectors of B + 1 entries, pygamd_index2ptr of a
 * non-decreasing batch vector; int32 / int64 by idx_dtype).  A search never crosses an example.
 * x [N, ldx] and y [M, ldy] are read in place at their pitches (floats, >= F; 64-bit row offsets):
 * a column block of a wider plane needs no copy.  float32, no float atomics, bitwise reproducible.
 * Distance: sum_c (x_c - y_c)^2 accumulated in float32 in column order, in the DIFFERENCE form — a
 * point is at distance exactly 0 from itself, and the value is within (F + 4) 2^-23 (relative) of
 * the exact one.  knn's cosine distance is 1 - x.y / (|x| |y|), its three sums taken in one pass.
 *
 * pygamd_knn: for every row q of y the k rows of x of q's example with the smallest distance,
 *   ascending by (distance, index of x) — ties go to the smaller index.  out_index [M, k] holds
 *   global row indices of x in that order, padded with -1, out_count [M] the number found
 *   (min(k, candidates)).  exclude_same_index != 0 skips the candidate whose global row index
 *   equals q (knn_graph(loop=False)).  One query per wave at a time, four queries register-blocked
 *   per wave over candidate tiles of 64 staged in LDS; the running best k sits one slot per lane.
 *   Envelope: 1 <= k <= 64, 1 <= F <= 512; example sizes below 2^31.
 * pygamd_radius: for every row q of y the rows of x of q's example with distance < r * r (STRICT;
 *   r * r formed in float32), in ascending index; at most max_num_neighbors (>= 1), the FIRST ones
 *   in index order.  out_index [M, max_num_neighbors] padded with -1, out_count [M].  r >= 0.
 * pygamd_fps: farthest point sampling, one workgroup per example.  Example e yields the
 *   out_ptr[e + 1] - out_ptr[e] picks out[out_ptr[e] ...) (global row indices, selection order;
 *   the host computes the counts, ceil(ratio n_e), at most n_e), starting from the global row
 *   start[e].  Each step picks the not yet picked point with the largest minimum distance to the
 *   picked set, ties to the lowest index, so duplicates are picked at distance 0 rather than an
 *   index twice.  total = out_ptr[B].  Workspace: pygamd_fps_workspace_size(N) (the running minima
 *   of examples too large for LDS).  Envelope: 1 <= F <= 512.
 * Before any device work: k outside 1..64, max_num_neighbors < 1, r < 0 or NaN, F outside 1..512,
 * a pitch below F, a negative size, an unknown idx_dtype, or a NULL pointer with a non-empty size
 * -> status 1; a short fps workspace -> status 3.  M == 0 (fps: no pick wanted) returns 0.        */
PYGAMD_API int pygamd_knn(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy,
                          int64_t M, int64_t F, const void* ptr_x, const void* ptr_y,
                          int idx_dtype, int64_t B, int k, int cosine, int exclude_same_index,
                          int64_t* out_index, int32_t* out_count, void* stream);
PYGAMD_API int pygamd_radius(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy,
                             int64_t M, int64_t F, const void* ptr_x, const void* ptr_y,
                             int idx_dtype, int64_t B, float r, int64_t max_num_neighbors,
                             int exclude_same_index, int64_t* out_index, int32_t* out_count,
                             void* stream);
PYGAMD_API int pygamd_fps_workspace_size(int64_t N, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_fps(const float* x, int64_t ldx, int64_t N, int64_t F, const void* ptr,
                          const void* out_ptr, const void* start, int idx_dtype, int64_t B,
                          int64_t total, int64_t* out, void* workspace, size_t workspace_bytes,
                          void* stream);

/* ---- hierarchical pooling: top-k select, gather-scale, edge filter — csrc/pool.hip ----------------
 * The three steps TopKPooling and SAGPooling run after every conv block.  float32 values, int64
 * node ids, 64-bit row offsets at each plane's own pitch, no float atomics: every output element
 * has exactly one writer and every result is a function of the inputs only.
 *
 * pygamd_topk_select: the reference's topk(x, ratio, batch) (nn/pool/select/topk.py:28-45: a global
 *   sort of the scores, a stable sort of the gathered batch vector, four [N] temporaries and a
 *   mask) in ONE launch that never leaves the graph.  Graph g owns the nodes [ptr[g], ptr[g + 1])
 *   (pygamd_index2ptr of a non-decreasing batch vector; int32 / int64 by idx_dtype) and the output
 *   slots [out_ptr[g], out_ptr[g + 1]), out_ptr [B + 1] (int64) the exclusive prefix of
 *   min(k[g], n_g), M = out_ptr[B].  perm [M] (int64) receives the graph's nodes ordered by
 *   SCORE DESCENDING, THEN NODE INDEX ASCENDING, the first min(k[g], n_g) of them; weight [M] =
 *   score[perm] (may be NULL).  Any NaN ranks above every number (torch.sort(descending=True)
 *   does the same); -0.0 and +0.0 are equal.  A score maps to a monotone uint32 with -0 and NaN
 *   canonicalised and pairs with the local index into a unique 64-bit key; node i goes to slot
 *   out_ptr[g] + #{j : key_j > key_i} when that rank is below its graph's count.  Ranks are a
 *   permutation, so every slot has one writer.  A graph of at most PYGAMD_TOPK_WAVE_NODES nodes is
 *   one wave's (keys in registers, PYGAMD_TOPK_GROUP graphs per workgroup); a longer one is its
 *   workgroup's (keys in LDS, rank by counting), up to PYGAMD_TOPK_MAX_NODES nodes.  max_nodes is
 *   the caller's bound on the largest graph: above the envelope -> status 2 before any launch (the
 *   caller takes its generic route for the whole batch); a graph that is larger than the envelope
 *   all the same (a max_nodes below the true maximum) is skipped by the kernel: its slots of perm
 *   and weight are LEFT UNWRITTEN although the call returns 0, so max_nodes must be the true
 *   bound.  Pointer values are clamped to [0, N] and [0, M].
 * pygamd_gather_scale_forward: out[i, :] = multiplier * (score[perm[i]] * x[perm[i], :]), the two
 *   products in that order — bit for bit x[perm] * score.view(-1, 1) followed by multiplier * x
 *   (nn/pool/topk_pool.py:121-122, sag_pool.py:135-136: two or three [M, F] passes); weight [M] =
 *   score[perm] (may be NULL).  perm [M] int64 without duplicates; a perm[i] outside [0, N) yields
 *   a zero row.  Any F >= 1 (a column loop; several rows per wave for F < 64).
 * pygamd_gather_scale_backward: the reference's index_put + broadcast multiply + row sum:
 *   grad_x[perm[i], :] = multiplier * weight[i] * grad_out[i, :] with weight[i] = score[perm[i]],
 *   grad_score[perm[i]] = multiplier * dot(grad_out[i], x[perm[i]]) + grad_weight[i] (grad_weight
 *   may be NULL: 0).  Only the rows in perm are written: the caller zero-fills grad_x and
 *   grad_score, and the rows outside perm stay exactly zero.  Either output may be NULL.
 * pygamd_filter_edges: the reference's filter_adj (nn/pool/connect/filter_edges.py:25-36: four [E]
 *   gathers, a mask and three boolean-mask compactions, each with its own scan and host read).
 *   row / col are the two rows of edge_index (int32 / int64 by idx_dtype), element e of each at
 *   e * its stride (in elements: a transposed [E, 2] tensor or a column slice is read in place);
 *   node_map [N] (int64) holds a node's new id or -1.  An edge survives when both endpoints map to
 *   a non-negative id (an endpoint outside [0, N) counts as dropped).  out_row / out_col [E]
 *   (int64) receive the relabelled endpoints of the survivors IN THE ORIGINAL EDGE ORDER, kept [E]
 *   (int64) their edge ids; total [1] (int64, device) their number.  Three launches over chunks of
 *   4,096 edges: the chunks' counts, one workgroup's scan of them, the write (ballot + prefix
 *   popcount inside a wave).  Workspace: pygamd_filter_edges_workspace_size(E).
 * Before any device work: an unknown idx_dtype, a negative size, F < 1, a pitch below F, a stride
 * below 1 or a NULL pointer with a non-empty size -> status 1; a short workspace -> status 3.
 * Empty inputs (M == 0, E == 0) return 0 without a launch (total is then not written: the caller
 * knows the count).                                                                               */
#define PYGAMD_TOPK_WAVE_NODES 64
#define PYGAMD_TOPK_MAX_NODES 1024
#define PYGAMD_TOPK_GROUP 4
PYGAMD_API int pygamd_topk_select(const float* score, int64_t N, const void* ptr, int idx_dtype,
                                  int64_t B, const int64_t* k, const int64_t* out_ptr, int64_t M,
                                  int64_t max_nodes, int64_t* perm, float* weight, void* stream);
PYGAMD_API int pygamd_gather_scale_forward(const float* x, int64_t ldx, int64_t N, int64_t F,
                                           const float* score, const int64_t* perm, int64_t M,
                                           float multiplier, float* out, int64_t ldo,
                                           float* weight, void* stream);
PYGAMD_API int pygamd_gather_scale_backward(const float* x, int64_t ldx, int64_t N, int64_t F,
                                            const float* score, const int64_t* perm, int64_t M,
                                            float multiplier, const float* grad_out, int64_t ldg,
                                            const float* grad_weight, float* grad_x, int64_t ldgx,
                                            float* grad_score, void* stream);
PYGAMD_API int pygamd_filter_edges_workspace_size(int64_t E, size_t* bytes /*[host]*/);
PYGAMD_API int pygamd_filter_edges(const void* row, int64_t row_stride, const void* col,
                                   int64_t col_stride, int idx_dtype, int64_t E,
                                   const int64_t* node_map, int64_t N, int64_t* out_row,
                                   int64_t* out_col, int64_t* kept, int64_t* total,
                                   void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* PYG_AMD_H */

// pool.hip — the three steps of hierarchical pooling (TopKPooling, SAGPooling): the per-graph top-k
// select (torch_geometric/nn/pool/select/topk.py:28-45 of the reference), the gather of the kept
// rows scaled by their scores with its backward (nn/pool/topk_pool.py:121-122, sag_pool.py:135-136)
// and the edge filter (nn/pool/connect/filter_edges.py:25-36).  The graphs of a sorted batch vector
// are contiguous node ranges (the fact graph_norm.hip is built on), so a selection never leaves its
// graph: its keys sit in one wave's registers or one workgroup's LDS.  No float atomics; every
// output element has exactly one writer, every result is a function of the inputs only.
#include "common.h"
#include "scan_device.h"

namespace pygamd {
namespace {

constexpr int kTopkMax = PYGAMD_TOPK_MAX_NODES;        // the longest graph of the select kernel
constexpr int kTopkPerThread = kTopkMax / kBlock;      // its keys per thread
static_assert(PYGAMD_TOPK_WAVE_NODES == kWave, "a short graph is one key per lane");
static_assert(PYGAMD_TOPK_GROUP == kWavesPerBlock, "a workgroup owns one short graph per wave");
static_assert(kTopkMax % kBlock == 0, "whole keys per thread");

__device__ __forceinline__ int64_t clamp_to(int64_t v, int64_t hi) {
  return v < 0 ? 0 : (v > hi ? hi : v);
}

// The order "score descending, then local index ascending" as ONE unsigned comparison: the score
// as a monotone uint32 (any NaN above every number, -0 = +0) over the complemented local index.
// Keys of one graph are distinct, so #{j : key_j > key_i} is a permutation of 0 .. n - 1.
__device__ __forceinline__ uint64_t topk_key(float s, int local) {
  uint32_t m;
  if (s != s) {
    m = 0xFFFFFFFFu;
  } else {
    const uint32_t b = s == 0.f ? 0u : __float_as_uint(s);
    m = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  return (static_cast<uint64_t>(m) << 32) | static_cast<uint32_t>(~static_cast<uint32_t>(local));
}

struct TopkGraph {
  int64_t base;  // first node
  int64_t ob;    // first output slot
  int n;         // nodes (0: nothing to do, also for a graph past the envelope)
  int cnt;       // nodes kept
};

template <typename IdxT>
__device__ __forceinline__ TopkGraph topk_graph(const IdxT* __restrict__ ptr,
                                                const int64_t* __restrict__ k,
                                                const int64_t* __restrict__ out_ptr, int64_t g,
                                                int64_t N, int64_t M) {
  TopkGraph t;
  t.base = clamp_to(static_cast<int64_t>(ptr[g]), N);
  const int64_t end = clamp_to(static_cast<int64_t>(ptr[g + 1]), N);
  t.ob = clamp_to(out_ptr[g], M);
  const int64_t oe = clamp_to(out_ptr[g + 1], M);
  int64_t n = end - t.base;
  if (n < 0 || n > kTopkMax) n = 0;
  int64_t cnt = k[g];
  if (cnt > n) cnt = n;
  if (cnt > oe - t.ob) cnt = oe - t.ob;
  if (cnt < 0) cnt = 0;
  t.n = static_cast<int>(n);
  t.cnt = static_cast<int>(cnt);
  return t;
}

// A workgroup owns kWavesPerBlock consecutive graphs.  First every wave ranks its own graph if that
// has at most 64 nodes (one key per lane, the others' keys by v_readlane); then the workgroup walks
// the longer ones of its graphs one after the other: the keys go to LDS, a thread keeps its own
// (up to kTopkPerThread) in registers and counts the larger ones in one pass over LDS — every lane
// reads the same address, a broadcast.
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void topk_select_kernel(
    const float* __restrict__ score, int64_t N, const IdxT* __restrict__ ptr, int64_t B,
    const int64_t* __restrict__ k, const int64_t* __restrict__ out_ptr, int64_t M,
    int64_t* __restrict__ perm, float* __restrict__ weight) {
  __shared__ uint64_t keys[kTopkMax];
  const int wave = wave_in_block();
  const int lane = lane_id();
  const int64_t g0 = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock;
  if (g0 + wave < B) {
    const TopkGraph t = topk_graph(ptr, k, out_ptr, g0 + wave, N, M);
    if (t.n <= kWave && t.cnt > 0) {
      const int n = __builtin_amdgcn_readfirstlane(t.n);  // (the wave's graph: uniform)
      const bool mine = lane < n;
      const float s = mine ? score[t.base + lane] : 0.f;
      const int64_t key = static_cast<int64_t>(mine ? topk_key(s, lane) : 0ull);
      int rank = 0;
      for (int j = 0; j < n; ++j) {
        rank += static_cast<uint64_t>(bcast_uniform(key, j)) > static_cast<uint64_t>(key) ? 1 : 0;
      }
      if (mine && rank < t.cnt) {
        perm[t.ob + rank] = t.base + lane;
        if (weight) weight[t.ob + rank] = s;
      }
    }
  }
  for (int w = 0; w < kWavesPerBlock; ++w) {
    if (g0 + w >= B) break;
    const TopkGraph t = topk_graph(ptr, k, out_ptr, g0 + w, N, M);  // (the same in every thread)
    if (t.n <= kWave || t.cnt == 0) continue;
    __syncthreads();  // the previous long graph's keys have been read
    float s[kTopkPerThread];
    uint64_t key[kTopkPerThread];
    int rank[kTopkPerThread];
#pragma unroll
    for (int q = 0; q < kTopkPerThread; ++q) {
      const int i = q * kBlock + static_cast<int>(threadIdx.x);
      s[q] = i < t.n ? score[t.base + i] : 0.f;
      key[q] = i < t.n ? topk_key(s[q], i) : ~0ull;  // (past the end: ranks 0, never written)
      rank[q] = 0;
      if (i < t.n) keys[i] = key[q];
    }
    __syncthreads();
    for (int j = 0; j < t.n; ++j) {
      const uint64_t kj = keys[j];
#pragma unroll
      for (int q = 0; q < kTopkPerThread; ++q) rank[q] += kj > key[q] ? 1 : 0;
    }
#pragma unroll
    for (int q = 0; q < kTopkPerThread; ++q) {
      const int i = q * kBlock + static_cast<int>(threadIdx.x);
      if (i < t.n && rank[q] < t.cnt) {
        perm[t.ob + rank[q]] = t.base + i;
        if (weight) weight[t.ob + rank[q]] = s[q];
      }
    }
  }
}

// ---- gather-scale ------------------------------------------------------------------------------
// 2^lg lanes share a row and stride over its columns; a wave holds 64 >> lg rows.
constexpr unsigned kRowGrid = 1u << 20;  // cap of the row kernels' grids (they stride beyond it)

inline int lanes_log2(int64_t F) {
  int lg = 0;
  while (lg < 6 && (int64_t{1} << lg) < F) ++lg;
  return lg;
}

inline unsigned row_grid(int64_t M, int lg) {
  const int64_t rows_per_block = static_cast<int64_t>(kWavesPerBlock) * (kWave >> lg);
  const int64_t blocks = ceil_div(M, rows_per_block);
  return static_cast<unsigned>(blocks > kRowGrid ? kRowGrid : blocks);
}

__global__ __launch_bounds__(kBlock) void gather_scale_fwd_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int F, const float* __restrict__ score,
    const int64_t* __restrict__ perm, int64_t M, float multiplier, float* __restrict__ out,
    int64_t ldo, float* __restrict__ weight, int lg) {
  const int lane = lane_id();
  const int lpr = 1 << lg, rpw = kWave >> lg;
  const int sub = lane & (lpr - 1), rin = lane >> lg;
  const int64_t first = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block()) * rpw;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWavesPerBlock * rpw;
  for (int64_t i0 = first; i0 < M; i0 += step) {
    const int64_t i = i0 + rin;
    if (i >= M) continue;
    const int64_t p = perm[i];
    const bool ok = p >= 0 && p < N;
    const float w = ok ? score[p] : 0.f;
    if (sub == 0 && weight) weight[i] = w;
    const float* xr = x + (ok ? p : 0) * ldx;
    float* o = out + i * ldo;
    for (int c = sub; c < F; c += lpr) o[c] = ok ? multiplier * (w * xr[c]) : 0.f;
  }
}

__global__ __launch_bounds__(kBlock) void gather_scale_bwd_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int F, const float* __restrict__ score,
    const int64_t* __restrict__ perm, int64_t M, float multiplier,
    const float* __restrict__ grad_out, int64_t ldg, const float* __restrict__ grad_weight,
    float* __restrict__ grad_x, int64_t ldgx, float* __restrict__ grad_score, int lg) {
  const int lane = lane_id();
  const int lpr = 1 << lg, rpw = kWave >> lg;
  const int sub = lane & (lpr - 1), rin = lane >> lg;
  const int64_t first = (static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block()) * rpw;
  const int64_t step = static_cast<int64_t>(gridDim.x) * kWavesPerBlock * rpw;
  for (int64_t i0 = first; i0 < M; i0 += step) {   // (wave-uniform: every lane takes the shuffles)
    const int64_t i = i0 + rin;
    const int64_t p = i < M ? perm[i] : -1;
    const bool ok = p >= 0 && p < N;
    float dot = 0.f;
    if (ok) {
      const float w = score[p];
      const float* xr = x + p * ldx;
      const float* g = grad_out + i * ldg;
      for (int c = sub; c < F; c += lpr) {
        const float gc = g[c];
        if (grad_x) grad_x[p * ldgx + c] = (multiplier * gc) * w;
        dot = fmaf(gc, xr[c], dot);
      }
    }
    for (int off = lpr >> 1; off > 0; off >>= 1) dot += __shfl_xor(dot, off, kWave);
    if (ok && sub == 0 && grad_score) {
      grad_score[p] = multiplier * dot + (grad_weight ? grad_weight[i] : 0.f);
    }
  }
}

// ---- edge filter -------------------------------------------------------------------------------
// A workgroup owns a chunk of kScanChunk edges, wave w of it the w-th run of kEdgeRounds * 64
// consecutive edges: lane l looks at edge j * 64 + l of the run in round j, so a ballot's bit order
// is the edge order.
constexpr int kEdgeRounds = kScanChunk / kBlock;

template <typename IdxT>
__device__ __forceinline__ bool map_edge(const IdxT* __restrict__ row, int64_t rs,
                                         const IdxT* __restrict__ col, int64_t cs, int64_t e,
                                         int64_t E, const int64_t* __restrict__ node_map,
                                         int64_t N, int64_t& nr, int64_t& nc) {
  nr = nc = -1;
  if (e >= E) return false;
  const int64_t r = static_cast<int64_t>(row[e * rs]), c = static_cast<int64_t>(col[e * cs]);
  if (r >= 0 && r < N) nr = node_map[r];
  if (c >= 0 && c < N) nc = node_map[c];
  return nr >= 0 && nc >= 0;
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void filter_count_kernel(
    const IdxT* __restrict__ row, int64_t rs, const IdxT* __restrict__ col, int64_t cs, int64_t E,
    const int64_t* __restrict__ node_map, int64_t N, int64_t* __restrict__ sums) {
  __shared__ int wave_tot[kWavesPerBlock];
  const int wave = wave_in_block(), lane = lane_id();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kScanChunk +
                       static_cast<int64_t>(wave) * (kEdgeRounds * kWave);
  int cnt = 0;
  for (int j = 0; j < kEdgeRounds; ++j) {
    int64_t nr, nc;
    const bool ok = map_edge(row, rs, col, cs, base + j * kWave + lane, E, node_map, N, nr, nc);
    cnt += __popcll(__ballot(ok));
  }
  if (lane == 0) wave_tot[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
    int64_t t = 0;
    for (int w = 0; w < kWavesPerBlock; ++w) t += wave_tot[w];
    sums[blockIdx.x] = t;
  }
}

template <typename IdxT>
__global__ __launch_bounds__(kBlock) void filter_write_kernel(
    const IdxT* __restrict__ row, int64_t rs, const IdxT* __restrict__ col, int64_t cs, int64_t E,
    const int64_t* __restrict__ node_map, int64_t N, const int64_t* __restrict__ sums,
    int64_t n_chunks, int64_t* __restrict__ out_row, int64_t* __restrict__ out_col,
    int64_t* __restrict__ kept, int64_t* __restrict__ total) {
  __shared__ int wave_tot[kWavesPerBlock];
  const int wave = wave_in_block(), lane = lane_id();
  const int64_t base = static_cast<int64_t>(blockIdx.x) * kScanChunk +
                       static_cast<int64_t>(wave) * (kEdgeRounds * kWave);
  int64_t nr[kEdgeRounds], nc[kEdgeRounds];
  uint64_t mask[kEdgeRounds];
  int cnt = 0;
#pragma unroll
  for (int j = 0; j < kEdgeRounds; ++j) {
    const bool ok = map_edge(row, rs, col, cs, base + j * kWave + lane, E, node_map, N, nr[j], nc[j]);
    mask[j] = __ballot(ok);
    cnt += __popcll(mask[j]);
  }
  if (lane == 0) wave_tot[wave] = cnt;
  __syncthreads();
  int64_t off = sums[blockIdx.x];
  for (int w = 0; w < wave; ++w) off += wave_tot[w];
  const uint64_t below = (1ull << lane) - 1ull;
#pragma unroll
  for (int j = 0; j < kEdgeRounds; ++j) {
    if ((mask[j] >> lane) & 1ull) {
      const int64_t slot = off + __popcll(mask[j] & below);
      if (slot < E) {  // (always: the slots are a prefix count of the edges)
        out_row[slot] = nr[j];
        out_col[slot] = nc[j];
        kept[slot] = base + j * kWave + lane;
      }
    }
    off += __popcll(mask[j]);
  }
  if (blockIdx.x == 0 && threadIdx.x == 0 && total) total[0] = sums[n_chunks];
}

bool bad_idx(int idx_dtype) { return idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64; }

// what the gather-scale forward and backward share; 0 or the status
int check_rows(const float* x, int64_t ldx, int64_t N, int64_t F, const float* score,
               const int64_t* perm, int64_t M) {
  if (N < 0 || M < 0 || F < 1 || F > INT32_MAX || ldx < F) return PYGAMD_ERR_INVALID_ARG;
  if (M > 0 && (!x || !score || !perm || N < 1)) return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_topk_select(const float* score, int64_t N, const void* ptr, int idx_dtype, int64_t B,
                       const int64_t* k, const int64_t* out_ptr, int64_t M, int64_t max_nodes,
                       int64_t* perm, float* weight, void* stream) {
  if (bad_idx(idx_dtype) || N < 0 || B < 0 || M < 0 || max_nodes < 0 || M > N)
    return PYGAMD_ERR_INVALID_ARG;
  if (B > 0 && (!ptr || !k || !out_ptr)) return PYGAMD_ERR_INVALID_ARG;
  if (N > 0 && !score) return PYGAMD_ERR_INVALID_ARG;
  if (M > 0 && (!perm || B < 1)) return PYGAMD_ERR_INVALID_ARG;
  if (max_nodes > kTopkMax) return PYGAMD_ERR_UNSUPPORTED;
  if (B == 0 || M == 0) return PYGAMD_OK;
  if (ceil_div(B, kWavesPerBlock) > INT32_MAX) return PYGAMD_ERR_UNSUPPORTED;
  const dim3 grid(static_cast<unsigned>(ceil_div(B, kWavesPerBlock)));
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((topk_select_kernel<IdxT>), grid, dim3(kBlock), 0, st, score, N,
                       static_cast<const IdxT*>(ptr), B, k, out_ptr, M, perm, weight);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_gather_scale_forward(const float* x, int64_t ldx, int64_t N, int64_t F,
                                const float* score, const int64_t* perm, int64_t M,
                                float multiplier, float* out, int64_t ldo, float* weight,
                                void* stream) {
  const int rc = check_rows(x, ldx, N, F, score, perm, M);
  if (rc != PYGAMD_OK) return rc;
  if (ldo < F || (M > 0 && !out)) return PYGAMD_ERR_INVALID_ARG;
  if (M == 0) return PYGAMD_OK;
  const int lg = lanes_log2(F);
  hipLaunchKernelGGL(gather_scale_fwd_kernel, dim3(row_grid(M, lg)), dim3(kBlock), 0,
                     as_stream(stream), x, ldx, N, static_cast<int>(F), score, perm, M, multiplier,
                     out, ldo, weight, lg);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

int pygamd_gather_scale_backward(const float* x, int64_t ldx, int64_t N, int64_t F,
                                 const float* score, const int64_t* perm, int64_t M,
                                 float multiplier, const float* grad_out, int64_t ldg,
                                 const float* grad_weight, float* grad_x, int64_t ldgx,
                                 float* grad_score, void* stream) {
  const int rc = check_rows(x, ldx, N, F, score, perm, M);
  if (rc != PYGAMD_OK) return rc;
  if (ldg < F || (grad_x && ldgx < F) || (M > 0 && !grad_out)) return PYGAMD_ERR_INVALID_ARG;
  if (M == 0 || (!grad_x && !grad_score)) return PYGAMD_OK;
  const int lg = lanes_log2(F);
  hipLaunchKernelGGL(gather_scale_bwd_kernel, dim3(row_grid(M, lg)), dim3(kBlock), 0,
                     as_stream(stream), x, ldx, N, static_cast<int>(F), score, perm, M, multiplier,
                     grad_out, ldg, grad_weight, grad_x, ldgx, grad_score, lg);
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

int pygamd_filter_edges_workspace_size(int64_t E, size_t* bytes) {
  if (!bytes || E < 0) return PYGAMD_ERR_INVALID_ARG;
  *bytes = E == 0 ? 0 : scan_scratch_bytes(E, sizeof(int64_t));
  return PYGAMD_OK;
}

int pygamd_filter_edges(const void* row, int64_t row_stride, const void* col, int64_t col_stride,
                        int idx_dtype, int64_t E, const int64_t* node_map, int64_t N,
                        int64_t* out_row, int64_t* out_col, int64_t* kept, int64_t* total,
                        void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_idx(idx_dtype) || E < 0 || N < 0 || row_stride < 1 || col_stride < 1)
    return PYGAMD_ERR_INVALID_ARG;
  if (E > 0 && (!row || !col || !out_row || !out_col || !kept || !total))
    return PYGAMD_ERR_INVALID_ARG;
  if (N > 0 && !node_map) return PYGAMD_ERR_INVALID_ARG;
  if (E == 0) return PYGAMD_OK;
  if (!workspace || workspace_bytes < scan_scratch_bytes(E, sizeof(int64_t)))
    return PYGAMD_ERR_WORKSPACE;
  const int64_t n_chunks = scan_chunks_of(E);
  if (n_chunks > INT32_MAX) return PYGAMD_ERR_UNSUPPORTED;
  int64_t* sums = static_cast<int64_t*>(workspace);
  const dim3 grid(static_cast<unsigned>(n_chunks)), block(kBlock);
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const IdxT* r = static_cast<const IdxT*>(row);
    const IdxT* c = static_cast<const IdxT*>(col);
    hipLaunchKernelGGL((filter_count_kernel<IdxT>), grid, block, 0, st, r, row_stride, c,
                       col_stride, E, node_map, N, sums);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((scan_sums_kernel<int64_t>), dim3(1), block, 0, st, sums, n_chunks);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((filter_write_kernel<IdxT>), grid, block, 0, st, r, row_stride, c,
                       col_stride, E, node_map, N, sums, n_chunks, out_row, out_col, kept, total);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"

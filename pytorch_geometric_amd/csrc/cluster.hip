// cluster.hip — the geometric searches of point-cloud models: k nearest neighbours, fixed-radius
// neighbours and farthest point sampling (torch_geometric/nn/pool/__init__.py:41-375, which only
// forwards to torch.ops.pyg.*).  Examples are contiguous row ranges given by pointer vectors; a
// search never leaves its example.  Distances are float32 sums of squared DIFFERENCES in column
// order (never |x|^2 + |y|^2 - 2 x.y): a point is at distance exactly 0 from itself and there is no
// cancellation.  No float atomics, every result a function of the inputs only.
#include <math.h>

#include "common.h"

namespace pygamd {
namespace {

constexpr int kTile = 64;                         // candidates per tile: one per lane
constexpr int kChunk = 64;                        // columns staged per pass: one per lane
constexpr int kPitch = kChunk + 1;                // odd pitch: lane l reads bank (l + c) % 64
constexpr int kQ = 4;                             // queries register-blocked per wave
constexpr int kQBlock = kQ * kWavesPerBlock;      // queries per workgroup
constexpr int kFpsBlock = 1024;                   // one workgroup per example
constexpr int kFpsWaves = kFpsBlock / kWave;
constexpr int kFpsLdsFloats = 15360;              // 60 KiB: coordinates + running minima

__device__ __forceinline__ int64_t clamp_row(int64_t v, int64_t n) {
  return v < 0 ? 0 : (v > n ? n : v);
}

// The candidate rows [xb, xe) of query row q: the example e with ptr_y[e] <= q < ptr_y[e + 1]
// (empty examples repeat a pointer value: the LAST e with ptr_y[e] <= q is the one that owns q).
// Everything is clamped to [0, N], so a malformed pointer vector cannot send a read out of x.
template <typename IdxT>
__device__ __forceinline__ void candidate_range(const IdxT* __restrict__ ptr_y,
                                                const IdxT* __restrict__ ptr_x, int64_t B,
                                                int64_t q, int64_t N, int64_t& xb, int64_t& xe) {
  int64_t lo = 0, hi = B;
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(ptr_y[mid]) <= q) lo = mid; else hi = mid;
  }
  xb = xe = 0;
  if (q >= static_cast<int64_t>(ptr_y[lo]) && q < static_cast<int64_t>(ptr_y[lo + 1])) {
    xb = clamp_row(static_cast<int64_t>(ptr_x[lo]), N);
    xe = clamp_row(static_cast<int64_t>(ptr_x[lo + 1]), N);
    if (xe < xb) xe = xb;
  }
}

// The running best k of one query, ONE slot per lane: lane s < cnt holds the rank-s (distance,
// index) pair, ascending by (distance, index).  Candidates arrive in ascending index, so a
// candidate goes BEHIND every kept pair of equal distance, and one that ties with the k-th is not
// taken.  `dist` / `ok` are this lane's candidate of the tile whose first candidate is `base`.
__device__ __forceinline__ void knn_insert_tile(float dist, bool ok, int base, int k, float& bd,
                                                int& bi, int& cnt) {
  const int lane = lane_id();
  float thr = bcast_uniform(bd, k - 1);
  uint64_t m = __ballot(ok && (cnt < k || dist < thr));
  while (m) {
    const int j = __builtin_ctzll(m);
    m &= m - 1;
    const float d = bcast_uniform(dist, j);
    if (cnt == k && !(d < thr)) continue;   // an insertion of this tile lowered the k-th since
    const int pos = __popcll(__ballot(lane < cnt && bd <= d));
    const float up_d = __shfl_up(bd, 1, kWave);
    const int up_i = __shfl_up(bi, 1, kWave);
    if (lane > pos) { bd = up_d; bi = up_i; }
    if (lane == pos) { bd = d; bi = base + j; }
    if (cnt < k) ++cnt;
    thr = bcast_uniform(bd, k - 1);
  }
}

// knn: a workgroup owns kQBlock consecutive query rows, a wave kQ of them.  The workgroup walks
// the candidate rows from the first query's example to the last one's in tiles of 64, staging 64
// columns of a tile in LDS at a time; a lane owns one candidate, reads its element once from LDS
// and uses it for all kQ queries, whose elements come out of a register by v_readlane.  A query
// masks the candidates outside its own example.
template <typename IdxT, bool COSINE>
__global__ __launch_bounds__(kBlock) void knn_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, const float* __restrict__ y, int64_t ldy,
    int64_t M, int F, const IdxT* __restrict__ ptr_x, const IdxT* __restrict__ ptr_y, int64_t B,
    int k, int exclude_same, int64_t* __restrict__ out_index, int32_t* __restrict__ out_count) {
  __shared__ float tile[kTile * kPitch];
  const int wave = wave_in_block();
  const int lane = lane_id();
  const int64_t q0 = static_cast<int64_t>(blockIdx.x) * kQBlock;
  const int64_t q_last = (q0 + kQBlock < M ? q0 + kQBlock : M) - 1;
  int64_t lo, hi;
  {
    int64_t b0, e0, b1, e1;
    candidate_range(ptr_y, ptr_x, B, q0, N, b0, e0);
    candidate_range(ptr_y, ptr_x, B, q_last, N, b1, e1);
    lo = b0 < b1 ? b0 : b1;
    hi = e0 > e1 ? e0 : e1;
  }
  int64_t qxb[kQ], qxe[kQ], qrow[kQ];
  float bd[kQ];
  int bi[kQ], cnt[kQ];
#pragma unroll
  for (int qi = 0; qi < kQ; ++qi) {
    const int64_t q = q0 + wave * kQ + qi;
    qrow[qi] = q < M ? q : M - 1;               // a row that can be read; q >= M takes no part
    qxb[qi] = qxe[qi] = 0;
    if (q < M) candidate_range(ptr_y, ptr_x, B, q, N, qxb[qi], qxe[qi]);
    // (a query's own range lies inside [lo, hi) for a monotone pointer vector; clip for any other)
    if (qxb[qi] < lo) qxb[qi] = lo;
    if (qxe[qi] > hi) qxe[qi] = hi;
    bd[qi] = INFINITY;
    bi[qi] = -1;
    cnt[qi] = 0;
  }
  for (int64_t t = lo; t < hi; t += kTile) {
    float acc[kQ], ny[kQ];
    float nx = 0.f;
#pragma unroll
    for (int qi = 0; qi < kQ; ++qi) acc[qi] = ny[qi] = 0.f;
    for (int c0 = 0; c0 < F; c0 += kChunk) {
      const int fc = F - c0 < kChunk ? F - c0 : kChunk;
      __syncthreads();                            // the previous pass has read the tile
      for (int e = threadIdx.x; e < kTile * fc; e += kBlock) {
        const int r = e / fc, c = e - r * fc;
        const int64_t row = t + r;
        tile[r * kPitch + c] = row < hi ? x[row * ldx + c0 + c] : 0.f;
      }
      float yv[kQ];
#pragma unroll
      for (int qi = 0; qi < kQ; ++qi) yv[qi] = lane < fc ? y[qrow[qi] * ldy + c0 + lane] : 0.f;
      __syncthreads();
      const float* mine = tile + lane * kPitch;
      for (int c = 0; c < fc; ++c) {
        const float xv = mine[c];
        if (COSINE) nx = fmaf(xv, xv, nx);
#pragma unroll
        for (int qi = 0; qi < kQ; ++qi) {
          const float q = bcast_uniform(yv[qi], c);
          if (COSINE) {
            acc[qi] = fmaf(xv, q, acc[qi]);
            ny[qi] = fmaf(q, q, ny[qi]);
          } else {
            const float d = xv - q;
            acc[qi] = fmaf(d, d, acc[qi]);
          }
        }
      }
    }
    const int64_t cand = t + lane;
#pragma unroll
    for (int qi = 0; qi < kQ; ++qi) {
      const int64_t q = q0 + wave * kQ + qi;
      const bool ok = cand >= qxb[qi] && cand < qxe[qi] && !(exclude_same && cand == q);
      const float dist = COSINE ? 1.f - acc[qi] / (sqrtf(nx) * sqrtf(ny[qi])) : acc[qi];
      knn_insert_tile(dist, ok, static_cast<int>(t - lo), k, bd[qi], bi[qi], cnt[qi]);
    }
  }
#pragma unroll
  for (int qi = 0; qi < kQ; ++qi) {
    const int64_t q = q0 + wave * kQ + qi;
    if (q >= M) continue;
    if (lane < k) out_index[q * k + lane] = lane < cnt[qi] ? lo + bi[qi] : -1;
    if (lane == 0) out_count[q] = cnt[qi];
  }
}

// radius: one wave per query walks its example's rows in ascending order, 64 at a time; a ballot
// of `dist < r2` and its prefix popcount give the output slots, and the walk stops at the cap.
template <typename IdxT>
__global__ __launch_bounds__(kBlock) void radius_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, const float* __restrict__ y, int64_t ldy,
    int64_t M, int F, const IdxT* __restrict__ ptr_x, const IdxT* __restrict__ ptr_y, int64_t B,
    float r2, int64_t cap, int exclude_same, int64_t* __restrict__ out_index,
    int32_t* __restrict__ out_count) {
  const int lane = lane_id();
  const int64_t q = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (q >= M) return;
  int64_t xb, xe;
  candidate_range(ptr_y, ptr_x, B, q, N, xb, xe);
  const float* yq = y + q * ldy;
  int64_t* out = out_index + q * cap;
  int64_t cnt = 0;
  for (int64_t t = xb; t < xe && cnt < cap; t += kTile) {
    const int64_t cand = t + lane;
    const bool valid = cand < xe;
    const float* xr = x + (valid ? cand : xb) * ldx;
    float acc = 0.f;
    for (int c = 0; c < F; ++c) {
      const float d = xr[c] - yq[c];
      acc = fmaf(d, d, acc);
    }
    const bool ok = valid && acc < r2 && !(exclude_same && cand == q);
    const uint64_t m = __ballot(ok);
    const int64_t slot = cnt + __popcll(m & ((1ull << lane) - 1ull));
    if (ok && slot < cap) out[slot] = cand;
    cnt += __popcll(m);
  }
  if (cnt > cap) cnt = cap;
  for (int64_t s = cnt + lane; s < cap; s += kWave) out[s] = -1;
  if (lane == 0) out_count[q] = static_cast<int32_t>(cnt);
}

// fps: one workgroup per example.  Thread t owns the points t, t + 1024, ... and keeps their
// running minimum distance to the picked set (a picked point holds -1 and is never picked again,
// which is what lets a run go on through duplicate points at distance 0).  An iteration updates
// the minima with the distance to the last pick and takes the workgroup argmax, ties to the lowest
// index.  IN_LDS: coordinates (odd pitch) and minima live in LDS, otherwise in x / the workspace.
template <bool IN_LDS>
__device__ __forceinline__ void fps_run(const float* __restrict__ xg, int64_t ldx, int F,
                                        int64_t base, int n, int m, int start,
                                        int64_t* __restrict__ out, float* __restrict__ md_global,
                                        float* lds, float* red_v, int* red_i) {
  const int tid = threadIdx.x;
  const int lane = lane_id();
  const int wave = tid >> 6;
  const int pitch = F | 1;
  float* md = IN_LDS ? lds + static_cast<size_t>(n) * pitch : md_global + base;
  if (IN_LDS) {
    for (int e = tid; e < n * F; e += kFpsBlock) {
      const int r = e / F, c = e - r * F;
      lds[r * pitch + c] = xg[(base + r) * ldx + c];
    }
  }
  for (int i = tid; i < n; i += kFpsBlock) md[i] = INFINITY;
  __syncthreads();
  int last = start;
  for (int it = 0; it < m; ++it) {
    if (tid == 0) out[it] = base + last;
    if (it + 1 == m) break;
    float best_v = -2.f;
    int best_i = 0x7fffffff;
    for (int i = tid; i < n; i += kFpsBlock) {
      float v = md[i];
      if (i == last) {
        v = -1.f;
      } else if (v >= 0.f) {
        float acc = 0.f;
        if (IN_LDS) {
          const float* a = lds + i * pitch;
          const float* b = lds + last * pitch;
          for (int c = 0; c < F; ++c) {
            const float d = a[c] - b[c];
            acc = fmaf(d, d, acc);
          }
        } else {
          const float* a = xg + (base + i) * ldx;
          const float* b = xg + (base + last) * ldx;
          for (int c = 0; c < F; ++c) {
            const float d = a[c] - b[c];
            acc = fmaf(d, d, acc);
          }
        }
        v = fminf(v, acc);
      }
      md[i] = v;
      if (v > best_v) { best_v = v; best_i = i; }   // ascending i: the lowest index keeps a tie
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
      const float ov = __shfl_xor(best_v, off, kWave);
      const int oi = __shfl_xor(best_i, off, kWave);
      if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
    }
    float* rv = red_v + (it & 1) * kFpsWaves;     // two sets: one barrier per iteration
    int* ri = red_i + (it & 1) * kFpsWaves;
    if (lane == 0) { rv[wave] = best_v; ri[wave] = best_i; }
    __syncthreads();
    best_v = rv[0];
    best_i = ri[0];
#pragma unroll
    for (int w = 1; w < kFpsWaves; ++w) {
      const float ov = rv[w];
      const int oi = ri[w];
      if (ov > best_v || (ov == best_v && oi < best_i)) { best_v = ov; best_i = oi; }
    }
    // (no comparison holds against NaN minima: stay inside the example whatever the data)
    last = best_i < n ? best_i : 0;
  }
}

template <typename IdxT>
__global__ __launch_bounds__(kFpsBlock) void fps_kernel(
    const float* __restrict__ x, int64_t ldx, int64_t N, int F, const IdxT* __restrict__ ptr,
    const IdxT* __restrict__ out_ptr, const IdxT* __restrict__ start, int64_t total,
    int64_t* __restrict__ out, float* __restrict__ md_global) {
  extern __shared__ float lds[];
  __shared__ float red_v[2 * kFpsWaves];
  __shared__ int red_i[2 * kFpsWaves];
  const int64_t b = blockIdx.x;
  const int64_t base = clamp_row(static_cast<int64_t>(ptr[b]), N);
  const int64_t end = clamp_row(static_cast<int64_t>(ptr[b + 1]), N);
  const int64_t ob = clamp_row(static_cast<int64_t>(out_ptr[b]), total);
  const int64_t oe = clamp_row(static_cast<int64_t>(out_ptr[b + 1]), total);
  if (end <= base || oe <= ob) return;
  const int n = static_cast<int>(end - base);
  int m = static_cast<int>(oe - ob);
  if (m > n) m = n;                               // no index twice: at most every point once
  int64_t s = static_cast<int64_t>(start[b]) - base;
  if (s < 0 || s >= n) s = 0;
  const bool in_lds = static_cast<int64_t>(n) * ((F | 1) + 1) <= kFpsLdsFloats;
  if (in_lds) {
    fps_run<true>(x, ldx, F, base, n, m, static_cast<int>(s), out + ob, md_global, lds, red_v,
                  red_i);
  } else {
    fps_run<false>(x, ldx, F, base, n, m, static_cast<int>(s), out + ob, md_global, lds, red_v,
                   red_i);
  }
  // an example asked for more picks than it has points: pad (the host never asks, ratio <= 1)
  for (int64_t i = ob + m + threadIdx.x; i < oe; i += kFpsBlock) out[i] = -1;
}

bool bad_idx(int idx_dtype) { return idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64; }

// the arguments knn and radius share; 0 or the status
int check_search(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy, int64_t M,
                 int64_t F, const void* ptr_x, const void* ptr_y, int idx_dtype, int64_t B,
                 const void* out_index, const void* out_count) {
  if (bad_idx(idx_dtype) || N < 0 || M < 0 || B < 0) return PYGAMD_ERR_INVALID_ARG;
  if (F < 1 || F > 512 || ldx < F || ldy < F) return PYGAMD_ERR_INVALID_ARG;
  if (N > 0 && !x) return PYGAMD_ERR_INVALID_ARG;
  if (M > 0 && (!y || !ptr_x || !ptr_y || !out_index || !out_count || B < 1))
    return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_knn(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy, int64_t M,
               int64_t F, const void* ptr_x, const void* ptr_y, int idx_dtype, int64_t B, int k,
               int cosine, int exclude_same_index, int64_t* out_index, int32_t* out_count,
               void* stream) {
  if (k < 1 || k > 64) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_search(x, ldx, N, y, ldy, M, F, ptr_x, ptr_y, idx_dtype, B, out_index,
                              out_count);
  if (rc != PYGAMD_OK) return rc;
  if (M == 0) return PYGAMD_OK;
  const dim3 grid(static_cast<unsigned>(ceil_div(M, kQBlock)));
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const IdxT* px = static_cast<const IdxT*>(ptr_x);
    const IdxT* py = static_cast<const IdxT*>(ptr_y);
    if (cosine) {
      hipLaunchKernelGGL((knn_kernel<IdxT, true>), grid, dim3(kBlock), 0, st, x, ldx, N, y, ldy, M,
                         static_cast<int>(F), px, py, B, k, exclude_same_index, out_index,
                         out_count);
    } else {
      hipLaunchKernelGGL((knn_kernel<IdxT, false>), grid, dim3(kBlock), 0, st, x, ldx, N, y, ldy,
                         M, static_cast<int>(F), px, py, B, k, exclude_same_index, out_index,
                         out_count);
    }
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_radius(const float* x, int64_t ldx, int64_t N, const float* y, int64_t ldy, int64_t M,
                  int64_t F, const void* ptr_x, const void* ptr_y, int idx_dtype, int64_t B,
                  float r, int64_t max_num_neighbors, int exclude_same_index, int64_t* out_index,
                  int32_t* out_count, void* stream) {
  if (max_num_neighbors < 1 || !(r >= 0.f)) return PYGAMD_ERR_INVALID_ARG;
  const int rc = check_search(x, ldx, N, y, ldy, M, F, ptr_x, ptr_y, idx_dtype, B, out_index,
                              out_count);
  if (rc != PYGAMD_OK) return rc;
  if (M == 0) return PYGAMD_OK;
  const float r2 = r * r;                         // formed in float32: the device rule
  const dim3 grid(static_cast<unsigned>(ceil_div(M, kWavesPerBlock)));
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((radius_kernel<IdxT>), grid, dim3(kBlock), 0, st, x, ldx, N, y, ldy, M,
                       static_cast<int>(F), static_cast<const IdxT*>(ptr_x),
                       static_cast<const IdxT*>(ptr_y), B, r2, max_num_neighbors,
                       exclude_same_index, out_index, out_count);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_fps_workspace_size(int64_t N, size_t* bytes) {
  if (!bytes || N < 0) return PYGAMD_ERR_INVALID_ARG;
  *bytes = sizeof(float) * static_cast<size_t>(N);
  return PYGAMD_OK;
}

int pygamd_fps(const float* x, int64_t ldx, int64_t N, int64_t F, const void* ptr,
               const void* out_ptr, const void* start, int idx_dtype, int64_t B, int64_t total,
               int64_t* out, void* workspace, size_t workspace_bytes, void* stream) {
  if (bad_idx(idx_dtype) || N < 0 || B < 0 || total < 0) return PYGAMD_ERR_INVALID_ARG;
  if (F < 1 || F > 512 || ldx < F) return PYGAMD_ERR_INVALID_ARG;
  if (N > 0 && !x) return PYGAMD_ERR_INVALID_ARG;
  if (B > 0 && (!ptr || !out_ptr || !start)) return PYGAMD_ERR_INVALID_ARG;
  if (total > 0 && (!out || B < 1)) return PYGAMD_ERR_INVALID_ARG;
  if (B == 0 || total == 0 || N == 0) return PYGAMD_OK;
  if (!workspace || workspace_bytes < sizeof(float) * static_cast<size_t>(N))
    return PYGAMD_ERR_WORKSPACE;
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((fps_kernel<IdxT>), dim3(static_cast<unsigned>(B)), dim3(kFpsBlock),
                       sizeof(float) * kFpsLdsFloats, st, x, ldx, N, static_cast<int>(F),
                       static_cast<const IdxT*>(ptr), static_cast<const IdxT*>(out_ptr),
                       static_cast<const IdxT*>(start), total, out,
                       static_cast<float*>(workspace));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"

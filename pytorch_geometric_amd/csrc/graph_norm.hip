// graph_norm.hip — per-graph normalisation of node features: GraphNorm (nn/norm/graph_norm.py:72-76
// of the reference) and LayerNorm with mode = 'graph' (nn/norm/layer_norm.py:82-108).  The graphs of
// a sorted batch vector are contiguous row ranges of x, so this is one more row-walking kernel over
// a ptr: its "rows" are graphs, its "slots" are nodes, and the hub plan over ptr cuts a long graph
// into chunks of nodes.
//
//   CHANNEL (GraphNorm), per (graph, column):  m = mean(x), u = x - alpha m, v = mean(u^2),
//            y = w u / sqrt(v + eps) + b
//   GRAPH   (LayerNorm), per graph over all n_g F elements:  m = mean(x), v = mean((x - m)^2),
//            y = (x - m) / sqrt(v + eps) w + b          (std_eps: / (sqrt(v) + eps), the
//            reference's formula without a batch vector, layer_norm.py:87-88)
//
// Statistics: ONE pass of shifted sums about a pivot k, the graph's first row (CHANNEL: per column;
// GRAPH: its first element): s1 = sum(x - k), s2 = sum((x - k)^2), then d = s1 / n, m = k + d,
// sigma^2 = s2 / n - d^2 — the cancelling form only ever sees data shifted by one of its own
// samples.  GraphNorm needs no second pass over u: v = sigma^2 + (1 - alpha)^2 m^2.
//
// Lanes own columns (rowwalk_device.h's layout with one head), so CHANNEL needs no cross-lane step
// and GRAPH one xor-butterfly per graph.  A graph at or under the plan's threshold is one wave's:
// statistics, then its rows again (from L2) for y, in the same launch.  A longer graph is the
// plan's chunks: the chunks' partial sums (all about the graph's pivot) go to the workspace, a merge
// launch adds them in chunk order, an apply launch covers the chunks.  The backward has the same
// shape with the sums of g = grad_y w and g u^; grad_weight, grad_bias and grad_mean_scale
// accumulate in the lanes' registers, fold through LDS in wave order into one partial per workgroup
// and are summed in an order that depends on the number of workgroups only.  No float atomics, every grid a function of (B, n_chunks)
// only: bitwise reproducible, and a graph's rows depend on nothing but that graph.
#include <math.h>

#include "common.h"
#include "rowwalk_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;

constexpr int kNormMaxWidth = 512;
constexpr unsigned kNormBlocks = PYGAMD_GRAPH_NORM_BLOCKS;  // cap of the backward's main grid
constexpr int kMergeWaves = 16;                             // a merge workgroup: 1,024 threads
constexpr int kMergeBlock = kMergeWaves * kWave;

template <int EPL>
struct NormRows {  // rows in flight per wave
  static constexpr int n = EPL >= 8 ? 2 : 4;
};

struct NormParams {
  const float* weight;      // [F] or NULL: 1
  const float* bias;        // [F] or NULL: 0
  const float* mean_scale;  // [F] or NULL: 1 (CHANNEL only)
  float eps;
  int std_eps;              // GRAPH only: 1 / (sqrt(v) + eps)
};

template <int EPL, bool VEC>
__device__ __forceinline__ void lane_cols(const Lay& L, bool (&ok)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) ok[e] = L.head_ok && lane_col<VEC>(L, e) < L.C;
}

// entries of a [F] parameter at the lane's columns; `fill` where there is no parameter
template <int EPL, bool VEC>
__device__ __forceinline__ void load_param(const float* __restrict__ p, const Lay& L, float fill,
                                           const bool (&ok)[EPL], float (&v)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) v[e] = ok[e] ? (p ? p[lane_col<VEC>(L, e)] : fill) : 0.f;
}

__device__ __forceinline__ float wave_sum(float v) { return group_sum(v, kWave); }

template <int EPL>
__device__ __forceinline__ float lane_total(const float (&v)[EPL]) {
  float t = 0.f;
#pragma unroll
  for (int e = 0; e < EPL; ++e) t += v[e];
  return t;
}

// u = x - alpha m as ONE fused operation everywhere, so that u and its mean (1 - alpha) m =
// centred(m, alpha, m) round alike: a graph of one node with alpha near 1 — u^2 against eps — would
// otherwise see u^ and rstd disagree in the backward (1 - u^2 rstd^2 is a cancellation there).
// GRAPH mode passes alpha = 1.
__device__ __forceinline__ float centred(float x, float alpha, float m) {
  return fmaf(-alpha, m, x);
}

// ---- the statistics from the shifted sums ------------------------------------------------------
// CHANNEL, one (graph, column): the mean m and 1 / sqrt(v + eps) of u = x - alpha m
__device__ __forceinline__ void finish_channel(float s1, float s2, float k, int64_t n, float alpha,
                                               float eps, float& m, float& r) {
  const float cnt = static_cast<float>(n < 1 ? 1 : n);
  const float d = s1 / cnt;
  m = k + d;
  const float var = fmaxf(s2 / cnt - d * d, 0.f);
  const float q = centred(m, alpha, m);
  r = 1.f / sqrtf(var + q * q + eps);
}

// GRAPH, one graph: counts are max(n, 1) * F as in the reference (layer_norm.py:93-94)
__device__ __forceinline__ void finish_graph(float s1, float s2, float k, int64_t n, int F,
                                             float eps, int std_eps, float& m, float& r) {
  const float cnt = static_cast<float>(n < 1 ? 1 : n) * static_cast<float>(F);
  const float d = s1 / cnt;
  m = k + d;
  const float var = fmaxf(s2 / cnt - d * d, 0.f);
  r = std_eps ? 1.f / (sqrtf(var) + eps) : 1.f / sqrtf(var + eps);
}

// y[k, :] = (x[k, :] - al m) * a + b over the rows [k0, k1)
template <int EPL, bool VEC>
__device__ __forceinline__ void apply_rows(const float* __restrict__ x, int64_t ldx,
                                           float* __restrict__ y, int64_t ldy, int64_t k0,
                                           int64_t k1, const Lay& L, const float (&al)[EPL],
                                           const float (&m)[EPL], const float (&a)[EPL],
                                           const float (&b)[EPL]) {
  constexpr int U = NormRows<EPL>::n;
  for (int64_t k = k0; k < k1; k += U) {
    float xx[U][EPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < k1) load_row<EPL, VEC>(x + (k + u) * ldx, L, xx[u]);
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < k1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) xx[u][e] = fmaf(centred(xx[u][e], al[e], m[e]), a[e], b[e]);
        store_row<EPL, VEC>(y + (k + u) * ldy, L, xx[u]);
      }
    }
  }
}

// the scale of apply_rows from a graph's statistics
template <int EPL>
__device__ __forceinline__ void apply_coef(const float (&r)[EPL], const float (&w)[EPL],
                                           float (&a)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) a[e] = r[e] * w[e];
}

// a graph's saved statistics at the lane's columns
template <int EPL, bool VEC, bool GRAPH>
__device__ __forceinline__ void load_stats(const float* __restrict__ mean,
                                           const float* __restrict__ rstd, int64_t row,
                                           const Lay& L, float (&m)[EPL], float (&r)[EPL]) {
  if constexpr (GRAPH) {
    const float mg = mean[row], rg = rstd[row];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      m[e] = mg;
      r[e] = rg;
    }
  } else {
    load_row<EPL, VEC>(mean + row * L.C, L, m);
    load_row<EPL, VEC>(rstd + row * L.C, L, r);
  }
}

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, bool GRAPH>
__global__ void __launch_bounds__(kBlock)
    norm_fwd_kernel(Items<IdxT> it, const float* __restrict__ x, int64_t ldx, NormParams p, int F,
                    int lph, float* __restrict__ y, int64_t ldy, float* __restrict__ mean,
                    float* __restrict__ rstd, float* __restrict__ part) {
  constexpr int U = NormRows<EPL>::n;
  const Lay L = make_lay(1, F, lph);
  bool ok[EPL];
  lane_cols<EPL, VEC>(L, ok);
  float w[EPL], b[EPL], al[EPL];
  load_param<EPL, VEC>(p.weight, L, 1.f, ok, w);
  load_param<EPL, VEC>(p.bias, L, 0.f, ok, b);
  load_param<EPL, VEC>(GRAPH ? nullptr : p.mean_scale, L, 1.f, ok, al);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    const int64_t n = s.row_end - s.row_start;
    float kv[EPL], k0 = 0.f;
#pragma unroll
    for (int e = 0; e < EPL; ++e) kv[e] = 0.f;
    if (n > 0) {  // the pivot: the graph's first row, for every chunk of it
      if constexpr (GRAPH) {
        k0 = x[s.row_start * ldx];
#pragma unroll
        for (int e = 0; e < EPL; ++e) kv[e] = ok[e] ? k0 : 0.f;
      } else {
        load_row<EPL, VEC>(x + s.row_start * ldx, L, kv);
      }
    }
    float s1[EPL], s2[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) s1[e] = s2[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float xx[U][EPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) load_row<EPL, VEC>(x + (k + u) * ldx, L, xx[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float d = xx[u][e] - kv[e];
            s1[e] += d;
            s2[e] = fmaf(d, d, s2[e]);
          }
        }
      }
    }
    float t1 = 0.f, t2 = 0.f;
    if constexpr (GRAPH) {
      t1 = wave_sum(lane_total<EPL>(s1));
      t2 = wave_sum(lane_total<EPL>(s2));
    }
    if (s.chunk_id >= 0) {  // a chunk's partial sums about the graph's pivot
      float* dst = part + s.chunk_id * 2 * F;
      if constexpr (GRAPH) {
        if (lane == 0) {
          dst[0] = t1;
          dst[1] = t2;
        }
      } else {
        store_row<EPL, VEC>(dst, L, s1);
        store_row<EPL, VEC>(dst + F, L, s2);
      }
      continue;
    }
    float m[EPL], r[EPL];
    if constexpr (GRAPH) {
      float mg, rg;
      finish_graph(t1, t2, k0, n, F, p.eps, p.std_eps, mg, rg);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        m[e] = mg;
        r[e] = rg;
      }
      if (lane == 0) {
        mean[s.row] = mg;
        rstd[s.row] = rg;
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) finish_channel(s1[e], s2[e], kv[e], n, al[e], p.eps, m[e], r[e]);
      store_row<EPL, VEC>(mean + s.row * F, L, m);
      store_row<EPL, VEC>(rstd + s.row * F, L, r);
    }
    float a[EPL];
    apply_coef<EPL>(r, w, a);
    apply_rows<EPL, VEC>(x, ldx, y, ldy, s.k0, s.k1, L, al, m, a, b);
  }
}

// The two partial sums of hub graph `hr` in a fixed order that depends on its chunk count only:
// wave v of the workgroup takes the v-th contiguous share of the chunks and the shares are added
// in wave order.  CHANNEL: blockIdx.y is a block of 64 columns, a lane's column is its own and it
// adds its share's chunks in chunk order.  GRAPH: the 64 lanes stride over the share's chunks and an
// xor-butterfly follows — not chunk order, but the same order in every run and in every batch the
// graph is part of.  Returns true in the threads of wave 0 that own a result, with the totals of
// the first and second partial in t1 and t2.
template <typename IdxT, bool GRAPH>
__device__ __forceinline__ bool merge_partials(const IdxT* __restrict__ hub_cptr, int64_t hr,
                                               int F, const float* __restrict__ part, float& t1,
                                               float& t2) {
  __shared__ float red[kMergeWaves][kWave][2];
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int64_t per = (c1 - c0 + kMergeWaves - 1) / kMergeWaves;
  const int64_t a0 = c0 + wv * per, a1 = a0 + per < c1 ? a0 + per : c1;
  const int col = GRAPH ? 0 : static_cast<int>(blockIdx.y) * kWave + lane;
  const int64_t S = 2 * static_cast<int64_t>(F);
  t1 = t2 = 0.f;
  if constexpr (GRAPH) {
    for (int64_t c = a0 + lane; c < a1; c += kWave) {
      t1 += part[c * S];
      t2 += part[c * S + 1];
    }
    t1 = wave_sum(t1);
    t2 = wave_sum(t2);
  } else {
    if (col < F) {
      for (int64_t c = a0; c < a1; ++c) {
        t1 += part[c * S + col];
        t2 += part[c * S + F + col];
      }
    }
  }
  red[wv][lane][0] = t1;
  red[wv][lane][1] = t2;
  __syncthreads();
  if (wv != 0) return false;
  t1 = t2 = 0.f;
  for (int v = 0; v < kMergeWaves; ++v) {
    t1 += red[v][lane][0];
    t2 += red[v][lane][1];
  }
  return GRAPH ? lane == 0 : col < F;
}

template <typename IdxT, bool GRAPH>
__global__ void __launch_bounds__(kMergeBlock)
    norm_fwd_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                          const IdxT* __restrict__ hub_cptr, const float* __restrict__ x,
                          int64_t ldx, NormParams p, int F, const float* __restrict__ part,
                          float* __restrict__ mean, float* __restrict__ rstd) {
  const int64_t hr = blockIdx.x;
  float t1, t2;
  if (!merge_partials<IdxT, GRAPH>(hub_cptr, hr, F, part, t1, t2)) return;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t r0 = static_cast<int64_t>(rowptr[row]), r1 = static_cast<int64_t>(rowptr[row + 1]);
  float m, r;
  if constexpr (GRAPH) {
    finish_graph(t1, t2, x[r0 * ldx], r1 - r0, F, p.eps, p.std_eps, m, r);
    mean[row] = m;
    rstd[row] = r;
  } else {
    const int col = static_cast<int>(blockIdx.y) * kWave + (threadIdx.x & (kWave - 1));
    finish_channel(t1, t2, x[r0 * ldx + col], r1 - r0, p.mean_scale ? p.mean_scale[col] : 1.f,
                   p.eps, m, r);
    mean[row * F + col] = m;
    rstd[row * F + col] = r;
  }
}

// hub graphs, forward: y over the chunks from the merged statistics
template <typename IdxT, int EPL, bool VEC, bool GRAPH>
__global__ void __launch_bounds__(kBlock)
    norm_fwd_apply_kernel(Items<IdxT> it, const float* __restrict__ x, int64_t ldx, NormParams p,
                          int F, int lph, const float* __restrict__ mean,
                          const float* __restrict__ rstd, float* __restrict__ y, int64_t ldy) {
  const Lay L = make_lay(1, F, lph);
  bool ok[EPL];
  lane_cols<EPL, VEC>(L, ok);
  float w[EPL], b[EPL], al[EPL];
  load_param<EPL, VEC>(p.weight, L, 1.f, ok, w);
  load_param<EPL, VEC>(p.bias, L, 0.f, ok, b);
  load_param<EPL, VEC>(GRAPH ? nullptr : p.mean_scale, L, 1.f, ok, al);
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < it.n_chunks; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float m[EPL], r[EPL], a[EPL];
    load_stats<EPL, VEC, GRAPH>(mean, rstd, s.row, L, m, r);
    apply_coef<EPL>(r, w, a);
    apply_rows<EPL, VEC>(x, ldx, y, ldy, s.k0, s.k1, L, al, m, a, b);
  }
}

// ---- backward --------------------------------------------------------------------------------
// With g = grad_y w, u^ = (x - alpha m) rstd (GRAPH: alpha = 1), c1 = mean(g u^), and per graph
//   CHANNEL: t = alpha (mean(g) - mean(u^) c1), mean(u^) = (1 - alpha) m rstd (not 0 unless alpha = 1)
//   GRAPH:   t = mean(g); std_eps: c1 *= 1 / (1 - eps rstd), the derivative of 1 / (sigma + eps)
// grad_x = rstd ((g - u^ c1) - t).  A graph's share of grad_mean_scale is
// -m sum_i grad_u = -m rstd (sum(g) - c1 n mean(u^)).
template <bool GRAPH>
__device__ __forceinline__ void bwd_coef(float sg, float sgu, float m, float r, float alpha,
                                         int64_t n, int F, float eps, int std_eps, float& c1,
                                         float& t, float& ms) {
  if constexpr (GRAPH) {
    const float cnt = static_cast<float>(n < 1 ? 1 : n) * static_cast<float>(F);
    c1 = sgu / cnt;
    if (std_eps) c1 = c1 / (1.f - eps * r);
    t = sg / cnt;
    ms = 0.f;
  } else {
    const float cnt = static_cast<float>(n < 1 ? 1 : n);
    const float mh = centred(m, alpha, m) * r;
    c1 = sgu / cnt;
    t = alpha * (sg / cnt - mh * c1);
    ms = m * r * (sg - c1 * (static_cast<float>(n) * mh));
  }
}

// grad_x over the rows [k0, k1)
template <int EPL, bool VEC>
__device__ __forceinline__ void bwd_rows(const float* __restrict__ x, int64_t ldx,
                                         const float* __restrict__ gy, int64_t ldg,
                                         float* __restrict__ gx, int64_t ldgx, int64_t k0,
                                         int64_t k1, const Lay& L, const float (&al)[EPL],
                                         const float (&m)[EPL], const float (&r)[EPL], const float (&w)[EPL],
                                         const float (&c1)[EPL], const float (&t)[EPL]) {
  constexpr int U = NormRows<EPL>::n;
  for (int64_t k = k0; k < k1; k += U) {
    float xx[U][EPL], gg[U][EPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < k1) {
        load_row<EPL, VEC>(x + (k + u) * ldx, L, xx[u]);
        load_row<EPL, VEC>(gy + (k + u) * ldg, L, gg[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < k1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const float uh = centred(xx[u][e], al[e], m[e]) * r[e];
          const float g = gg[u][e] * w[e];
          xx[u][e] = r[e] * ((g - uh * c1[e]) - t[e]);
        }
        store_row<EPL, VEC>(gx + (k + u) * ldgx, L, xx[u]);
      }
    }
  }
}

template <typename IdxT, int EPL, bool VEC, bool GRAPH>
__global__ void __launch_bounds__(kBlock)
    norm_bwd_kernel(Items<IdxT> it, const float* __restrict__ x, int64_t ldx,
                    const float* __restrict__ gy, int64_t ldg, const float* __restrict__ mean,
                    const float* __restrict__ rstd, NormParams p, int F, int lph,
                    float* __restrict__ gx, int64_t ldgx, float* __restrict__ part,
                    float* __restrict__ wpart) {
  constexpr int U = NormRows<EPL>::n;
  const Lay L = make_lay(1, F, lph);
  bool ok[EPL];
  lane_cols<EPL, VEC>(L, ok);
  float w[EPL], al[EPL], gw[EPL], gb[EPL], gms[EPL];
  load_param<EPL, VEC>(p.weight, L, 1.f, ok, w);
  load_param<EPL, VEC>(GRAPH ? nullptr : p.mean_scale, L, 1.f, ok, al);
#pragma unroll
  for (int e = 0; e < EPL; ++e) gw[e] = gb[e] = gms[e] = 0.f;
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    const int64_t n = s.row_end - s.row_start;
    float m[EPL], r[EPL], sg[EPL], sgu[EPL];
    load_stats<EPL, VEC, GRAPH>(mean, rstd, s.row, L, m, r);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      sg[e] = sgu[e] = 0.f;
    }
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float xx[U][EPL], gg[U][EPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          load_row<EPL, VEC>(x + (k + u) * ldx, L, xx[u]);
          load_row<EPL, VEC>(gy + (k + u) * ldg, L, gg[u]);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float uh = centred(xx[u][e], al[e], m[e]) * r[e];
            const float g = gg[u][e] * w[e];
            sg[e] += g;
            sgu[e] = fmaf(g, uh, sgu[e]);
            gw[e] = fmaf(gg[u][e], uh, gw[e]);
            gb[e] += gg[u][e];
          }
        }
      }
    }
    if constexpr (GRAPH) {
      const float t1 = wave_sum(lane_total<EPL>(sg)), t2 = wave_sum(lane_total<EPL>(sgu));
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        sg[e] = t1;
        sgu[e] = t2;
      }
    }
    if (s.chunk_id >= 0) {
      float* dst = part + s.chunk_id * 2 * F;
      if constexpr (GRAPH) {
        if (lane == 0) {
          dst[0] = sg[0];
          dst[1] = sgu[0];
        }
      } else {
        store_row<EPL, VEC>(dst, L, sg);
        store_row<EPL, VEC>(dst + F, L, sgu);
      }
      continue;
    }
    float c1[EPL], t[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      float ms;
      bwd_coef<GRAPH>(sg[e], sgu[e], m[e], r[e], al[e], n, F, p.eps, p.std_eps, c1[e], t[e], ms);
      gms[e] += ms;
    }
    bwd_rows<EPL, VEC>(x, ldx, gy, ldg, gx, ldgx, s.k0, s.k1, L, al, m, r, w, c1, t);
  }
  if (!wpart) return;  // (wave-uniform: no parameter gradient is wanted)
  // the workgroup's partial [gw | gb | gms]: its waves add theirs in wave order
  __shared__ float red[3 * kNormMaxWidth];
  for (int wv = 0; wv < kWavesPerBlock; ++wv) {
    if (wave_in_block() == wv) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        const int c = lane_col<VEC>(L, e);
        if (ok[e]) {
          red[c] = (wv == 0 ? 0.f : red[c]) + gw[e];
          red[F + c] = (wv == 0 ? 0.f : red[F + c]) + gb[e];
          red[2 * F + c] = (wv == 0 ? 0.f : red[2 * F + c]) + gms[e];
        }
      }
    }
    __syncthreads();
  }
  float* dst = wpart + static_cast<int64_t>(blockIdx.x) * 3 * F;
  for (int t = threadIdx.x; t < 3 * F; t += kBlock) dst[t] = red[t];
}

// hub graphs, backward: the chunks' (sum g, sum g u^) in chunk order -> the graph's (c1, t) for the
// apply launch and its share of grad_mean_scale
template <typename IdxT, bool GRAPH>
__global__ void __launch_bounds__(kMergeBlock)
    norm_bwd_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                          const IdxT* __restrict__ hub_cptr, NormParams p, int F,
                          const float* __restrict__ part, const float* __restrict__ mean,
                          const float* __restrict__ rstd, float* __restrict__ coef,
                          float* __restrict__ hub_ms) {
  const int64_t hr = blockIdx.x;
  float sg, sgu;
  if (!merge_partials<IdxT, GRAPH>(hub_cptr, hr, F, part, sg, sgu)) return;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t n = static_cast<int64_t>(rowptr[row + 1]) - static_cast<int64_t>(rowptr[row]);
  const int col = GRAPH ? 0 : static_cast<int>(blockIdx.y) * kWave + (threadIdx.x & (kWave - 1));
  const int64_t at = GRAPH ? row : row * F + col;
  float c1, t, ms;
  bwd_coef<GRAPH>(sg, sgu, mean[at], rstd[at], (!GRAPH && p.mean_scale) ? p.mean_scale[col] : 1.f,
                  n, F, p.eps, p.std_eps, c1, t, ms);
  coef[hr * 2 * F + col] = c1;
  coef[hr * 2 * F + (GRAPH ? 1 : F + col)] = t;
  if constexpr (!GRAPH) hub_ms[hr * F + col] = ms;
}

template <typename IdxT, int EPL, bool VEC, bool GRAPH>
__global__ void __launch_bounds__(kBlock)
    norm_bwd_apply_kernel(Items<IdxT> it, const float* __restrict__ x, int64_t ldx,
                          const float* __restrict__ gy, int64_t ldg,
                          const float* __restrict__ mean, const float* __restrict__ rstd,
                          NormParams p, int F, int lph, const float* __restrict__ coef,
                          float* __restrict__ gx, int64_t ldgx) {
  const Lay L = make_lay(1, F, lph);
  bool ok[EPL];
  lane_cols<EPL, VEC>(L, ok);
  float w[EPL], al[EPL];
  load_param<EPL, VEC>(p.weight, L, 1.f, ok, w);
  load_param<EPL, VEC>(GRAPH ? nullptr : p.mean_scale, L, 1.f, ok, al);
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < it.n_chunks; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float m[EPL], r[EPL], c1[EPL], t[EPL];
    load_stats<EPL, VEC, GRAPH>(mean, rstd, s.row, L, m, r);
    const float* cf = coef + s.hub * 2 * F;
    if constexpr (GRAPH) {
      const float cg = cf[0], tg = cf[1];
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        c1[e] = cg;
        t[e] = tg;
      }
    } else {
      load_row<EPL, VEC>(cf, L, c1);
      load_row<EPL, VEC>(cf + F, L, t);
    }
    bwd_rows<EPL, VEC>(x, ldx, gy, ldg, gx, ldgx, s.k0, s.k1, L, al, m, r, w, c1, t);
  }
}

// The workgroups' partials [gw | gb | gms] in an order that depends on their number only, then the
// hub graphs' shares of grad_mean_scale in hub order.  A workgroup serves 64 of the 3 F columns;
// wave v adds the v-th contiguous share of the partials in workgroup order (64 coalesced floats per
// step) and the shares are added in wave order.  (One thread per column walking all 1,024 partials
// took 234 us at F = 128, four times the backward's main kernel: profiles/graph_norm.md.)
__global__ void __launch_bounds__(kMergeBlock)
    norm_param_reduce_kernel(const float* __restrict__ wpart, int n_blocks, int F,
                             const float* __restrict__ hub_ms, int64_t n_hub,
                             float* __restrict__ grad_weight, float* __restrict__ grad_bias,
                             float* __restrict__ grad_mean_scale) {
  __shared__ float red[kMergeWaves][kWave];
  const int wv = threadIdx.x >> 6, lane = threadIdx.x & (kWave - 1);
  const int t = blockIdx.x * kWave + lane;
  const int per = (n_blocks + kMergeWaves - 1) / kMergeWaves;
  const int g0 = wv * per, g1 = g0 + per < n_blocks ? g0 + per : n_blocks;
  float acc = 0.f;
  if (t < 3 * F) {
    for (int g = g0; g < g1; ++g) acc += wpart[static_cast<int64_t>(g) * 3 * F + t];
  }
  red[wv][lane] = acc;
  __syncthreads();
  if (wv != 0 || t >= 3 * F) return;
  acc = 0.f;
  for (int v = 0; v < kMergeWaves; ++v) acc += red[v][lane];
  if (t < F) {
    if (grad_weight) grad_weight[t] = acc;
  } else if (t < 2 * F) {
    if (grad_bias) grad_bias[t - F] = acc;
  } else if (grad_mean_scale) {
    for (int64_t h = 0; h < n_hub; ++h) acc += hub_ms[h * F + (t - 2 * F)];
    grad_mean_scale[t - 2 * F] = -acc;
  }
}

// ---- host side -------------------------------------------------------------------------------
// `...` sees the constants EPL and VEC of the shape.  ROWWALK_DISPATCH_SHAPE without its
// 16-register case: with one head and F <= 512 a lane has at most 8, and these kernels hold
// several rows of EPL registers at once — the case would be compiled for nothing.
#define NORM_DISPATCH_SHAPE(shape, ...)                                                         \
  do {                                                                                          \
    if ((shape).vec) {                                                                          \
      if ((shape).epl == 4) { constexpr int EPL = 4; constexpr bool VEC = true; __VA_ARGS__ }   \
      else { constexpr int EPL = 8; constexpr bool VEC = true; __VA_ARGS__ }                    \
    } else {                                                                                    \
      switch ((shape).epl) {                                                                    \
        case 1: { constexpr int EPL = 1; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 2: { constexpr int EPL = 2; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 4: { constexpr int EPL = 4; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        case 8: { constexpr int EPL = 8; constexpr bool VEC = false; __VA_ARGS__ } break;       \
        default: return PYGAMD_ERR_UNSUPPORTED;                                                 \
      }                                                                                         \
    }                                                                                           \
  } while (0)

#define NORM_DISPATCH_MODE(mode, ...)                                  \
  do {                                                                 \
    if ((mode) == PYGAMD_NORM_GRAPH) { constexpr bool GRAPH = true; __VA_ARGS__ }  \
    else { constexpr bool GRAPH = false; __VA_ARGS__ }                 \
  } while (0)

inline int64_t fwd_ws_floats(int64_t n_chunks, int64_t F) { return 2 * F * n_chunks; }
inline int64_t bwd_ws_floats(int64_t n_chunks, int64_t n_hub, int64_t F) {
  return F * (2 * n_chunks + 3 * n_hub + 3 * static_cast<int64_t>(kNormBlocks));
}

// what forward and backward share: 0 = go on
inline int norm_check(const pygamd_csr* g, int mode, int64_t n, int64_t F) {
  const int rc = check_handle(g, n);
  if (rc != PYGAMD_OK) return rc;
  if (F < 1 || (mode != PYGAMD_NORM_CHANNEL && mode != PYGAMD_NORM_GRAPH))
    return PYGAMD_ERR_INVALID_ARG;
  return F > kNormMaxWidth ? PYGAMD_ERR_UNSUPPORTED : PYGAMD_OK;
}

inline dim3 merge_grid(int64_t n_hub, int mode, int64_t F) {
  return dim3(static_cast<unsigned>(n_hub),
              mode == PYGAMD_NORM_GRAPH ? 1u : static_cast<unsigned>(ceil_div(F, kWave)));
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_graph_norm_supported(int64_t F) { return (F >= 1 && F <= kNormMaxWidth) ? 1 : 0; }

int pygamd_graph_norm_forward(const pygamd_csr* g, int mode, const float* x, int64_t ldx, int64_t n,
                              int64_t F, const float* weight, const float* bias,
                              const float* mean_scale, float eps, int std_eps, float* y,
                              int64_t ldy, float* mean, float* rstd, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int rc = norm_check(g, mode, n, F);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ldx < F || ldy < F || (mode == PYGAMD_NORM_GRAPH && mean_scale) ||
      (mode == PYGAMD_NORM_CHANNEL && std_eps))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !x || !y || !mean || !rstd) return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 &&
      (!workspace || workspace_bytes < sizeof(float) * static_cast<size_t>(fwd_ws_floats(n_chunks, F))))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(x) && ldx % 4 == 0 && aligned16(y) && ldy % 4 == 0 &&
                  aligned16(mean) && aligned16(rstd) && (n_chunks == 0 || aligned16(workspace));
  Shape sh;
  if (!choose_shape(1, F, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  const NormParams p{weight, bias, mean_scale, eps, std_eps};
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const int Fi = static_cast<int>(F);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    NORM_DISPATCH_MODE(mode, NORM_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((norm_fwd_kernel<IdxT, EPL, VEC, GRAPH>), grid, block, 0, st, it, x, ldx,
                         p, Fi, sh.lph, y, ldy, mean, rstd, part);
    }););
    PYGAMD_LAUNCH_CHECK();
    if (n_hub == 0) return PYGAMD_OK;
    NORM_DISPATCH_MODE(mode, {
      hipLaunchKernelGGL((norm_fwd_merge_kernel<IdxT, GRAPH>), merge_grid(n_hub, mode, F),
                         dim3(kMergeBlock), 0, st, it.rowptr, it.hub_rows, it.hub_cptr, x, ldx, p,
                         Fi, part, mean, rstd);
    });
    PYGAMD_LAUNCH_CHECK();
    const dim3 cgrid(wave_grid(n_chunks));
    NORM_DISPATCH_MODE(mode, NORM_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((norm_fwd_apply_kernel<IdxT, EPL, VEC, GRAPH>), cgrid, block, 0, st, it,
                         x, ldx, p, Fi, sh.lph, mean, rstd, y, ldy);
    }););
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_graph_norm_backward(const pygamd_csr* g, int mode, const float* x, int64_t ldx,
                               const float* grad_y, int64_t ldg, int64_t n, int64_t F,
                               const float* weight, const float* mean_scale, float eps,
                               int std_eps, const float* mean, const float* rstd, float* grad_x,
                               int64_t ldgx, float* grad_weight, float* grad_bias,
                               float* grad_mean_scale, void* workspace, size_t workspace_bytes,
                               void* stream) {
  const int rc = norm_check(g, mode, n, F);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ldx < F || ldg < F || ldgx < F ||
      (mode == PYGAMD_NORM_GRAPH && (mean_scale || grad_mean_scale)) ||
      (mode == PYGAMD_NORM_CHANNEL && std_eps))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !x || !grad_y || !mean || !rstd || !grad_x) return PYGAMD_ERR_INVALID_ARG;
  if (!workspace ||
      workspace_bytes < sizeof(float) * static_cast<size_t>(bwd_ws_floats(n_chunks, n_hub, F)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(x) && ldx % 4 == 0 && aligned16(grad_y) && ldg % 4 == 0 &&
                  aligned16(grad_x) && ldgx % 4 == 0 && aligned16(mean) && aligned16(rstd) &&
                  aligned16(workspace);
  Shape sh;
  if (!choose_shape(1, F, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  const NormParams p{weight, nullptr, mean_scale, eps, std_eps};
  hipStream_t st = as_stream(stream);
  const bool params = grad_weight || grad_bias || grad_mean_scale;
  float* part = static_cast<float*>(workspace);
  float* coef = part + 2 * F * n_chunks;
  float* hub_ms = coef + 2 * F * n_hub;
  float* wpart = hub_ms + F * n_hub;
  const int Fi = static_cast<int>(F);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    unsigned n_blocks = wave_grid(n_rows + n_chunks);
    if (n_blocks > kNormBlocks) n_blocks = kNormBlocks;
    const dim3 grid(n_blocks), block(kBlock);
    NORM_DISPATCH_MODE(mode, NORM_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((norm_bwd_kernel<IdxT, EPL, VEC, GRAPH>), grid, block, 0, st, it, x, ldx,
                         grad_y, ldg, mean, rstd, p, Fi, sh.lph, grad_x, ldgx, part,
                         params ? wpart : nullptr);
    }););
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      NORM_DISPATCH_MODE(mode, {
        hipLaunchKernelGGL((norm_bwd_merge_kernel<IdxT, GRAPH>), merge_grid(n_hub, mode, F),
                           dim3(kMergeBlock), 0, st, it.rowptr, it.hub_rows, it.hub_cptr, p, Fi,
                           part, mean, rstd, coef, hub_ms);
      });
      PYGAMD_LAUNCH_CHECK();
      const dim3 cgrid(wave_grid(n_chunks));
      NORM_DISPATCH_MODE(mode, NORM_DISPATCH_SHAPE(sh, {
        hipLaunchKernelGGL((norm_bwd_apply_kernel<IdxT, EPL, VEC, GRAPH>), cgrid, block, 0, st, it,
                           x, ldx, grad_y, ldg, mean, rstd, p, Fi, sh.lph, coef, grad_x, ldgx);
      }););
      PYGAMD_LAUNCH_CHECK();
    }
    if (params) {
      hipLaunchKernelGGL(norm_param_reduce_kernel, dim3(static_cast<unsigned>(ceil_div(3 * F, kWave))),
                         dim3(kMergeBlock), 0, st, wpart, static_cast<int>(n_blocks), Fi, hub_ms,
                         mode == PYGAMD_NORM_GRAPH ? int64_t{0} : n_hub, grad_weight, grad_bias,
                         grad_mean_scale);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

}  // extern "C"

// pna.hip — the aggregation of PNAConv (nn/conv/pna_conv.py:175-188 and nn/aggr/scaler.py:82 of the
// reference) for a LINEAR message (pre_layers = 1) as a pair of row-gather kernels on a sorted
// handle.  The message of slot k of destination i with source j splits into a per-node and a
// per-edge part,
//     m_k = P_dst[i] + u_k,    u_k = P_src[j] + Wc a_k     (Wc [W, De], a_k = edge_attr[k, :De];
//                                                            u_k = P_src[j] without edge features)
// so the four statistics of a destination with d > 0 slots are
//     mean = P_dst[i] + sum u / d,  min = P_dst[i] + min u,  max = P_dst[i] + max u,
//     std  = sqrt(max(var u, 1e-5)), set to 0 where that is <= sqrt(1e-5)   (var is shift invariant)
// and exactly 0 for d = 0.  The forward walks the CSR by destination once and gathers ONE row per
// slot; per column it keeps the sum and the second moment of u ABOUT THE FIRST u OF THE SPAN (so
// that a large common offset does not cancel), the extrema and the number of slots that attain
// each.  The backward walks the CSR by source, rebuilds u_k with the same operations in the same
// order (u_k == min u is then a bitwise test) and needs one packed coefficient row per destination:
//     grad_u = A + B u + Gmin [u == min u] + Gmax [u == max u]
// Lane layout, weights in registers, schedule and dispatch: rowwalk_device.h / gine_device.h.  No
// float atomics anywhere: every result is bitwise reproducible.
#include <math.h>

#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using namespace gine;

enum { kPnaMean = 1, kPnaMin = 2, kPnaMax = 4, kPnaStd = 8 };
constexpr int kPnaParts = 7;  // a chunk's partial rows: shift, s1, s2, min, max, cnt_min, cnt_max
constexpr int kPnaCoef = 6;   // a destination's coefficient row: A, B, Gmin, Gmax, min u, max u
constexpr float kPnaVarFloor = 1e-5f;
constexpr float kPnaStdFloor = 0.0031622776601683794f;  // sqrt(1e-5)

template <int EPL, int DE>
struct PnaFwdSlots {  // slots in flight per wave
  static constexpr int n = (EPL >= 8 || DE > 0) ? 2 : 4;
};
template <int EPL, int DE>
struct PnaBwdSlots {  // (a slot holds up to six gathered rows here)
  static constexpr int n = (EPL * DE >= 64 || EPL >= 8) ? 1 : 2;
};

struct PnaOut {
  float* stat[4];  // mean, min, max, std [n_rows, W]; NULL: not selected
  float* saved;    // [6, n_rows, W]: mean u, min u, max u, std, cnt_min, cnt_max (for the backward)
  int64_t plane;   // n_rows * W
};

// (count n, mean, sum of squares about the mean) of one more group of slots, Chan et al.
__device__ __forceinline__ void moments_merge(float& n, float& mean, float& m2, float nb,
                                              float mean_b, float m2_b) {
  const float nn = n + nb, delta = mean_b - mean;
  mean = fmaf(delta, nb / nn, mean);
  m2 = m2 + m2_b + delta * delta * (n * nb / nn);
  n = nn;
}

__device__ __forceinline__ void extremum_merge(float& v, float& cnt, float vb, float cb, bool less) {
  if (vb == v) {
    cnt += cb;
  } else if (less ? vb < v : vb > v) {
    v = vb;
    cnt = cb;
  }
}

__device__ __forceinline__ float pna_std(float m2, float n) {
  const float s = sqrtf(fmaxf(m2 / n, kPnaVarFloor));
  return s <= kPnaStdFloor ? 0.f : s;
}

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    pna_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const IdxT* __restrict__ edge_id,
                   const float* __restrict__ p_src, int64_t ld, const float* __restrict__ p_dst,
                   int64_t ld_dst, EdgeArgs ed, int W, int lph, PnaOut o,
                   float* __restrict__ part) {
  constexpr int U = PnaFwdSlots<EPL, DE>::n;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, W, lph);
  float w[LIN ? EPL : 1][LIN ? DE : 1], unused[EPL];
  if constexpr (LIN) load_weight<EPL, VEC, DE>(ed.weight, nullptr, L, ed.De, w, unused);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;  // (a row without slots is an item: it gets its zeros)
    float sh[EPL], s1[EPL], s2[EPL], mn[EPL], mx[EPL], cmn[EPL], cmx[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      sh[e] = s1[e] = s2[e] = cmn[e] = cmx[e] = 0.f;
      mn[e] = INFINITY;
      mx[e] = -INFINITY;
    }
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float xx[U][EPL], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const int64_t j = static_cast<int64_t>(col[k + u]);
          load_row<EPL, VEC>(p_src + j * ld, L, xx[u]);
          if constexpr (LIN) av[u] = edge_lane(ed, slot_edge(edge_id, k + u), lane);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          float uu[EPL];
          if constexpr (LIN) {
            edge_term<EPL, DE>(w, xx[u], av[u], uu);
          } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) uu[e] = xx[u][e];
          }
          const bool first = k + u == s.k0;
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            if (first) sh[e] = uu[e];
            const float t = uu[e] - sh[e];
            s1[e] += t;
            s2[e] = fmaf(t, t, s2[e]);
            extremum_merge(mn[e], cmn[e], uu[e], 1.f, true);
            extremum_merge(mx[e], cmx[e], uu[e], 1.f, false);
          }
        }
      }
    }
    if (s.chunk_id >= 0) {  // the partials of one chunk of a long row
      float* dst = part + s.chunk_id * kPnaParts * W;
      store_row<EPL, VEC>(dst, L, sh);
      store_row<EPL, VEC>(dst + W, L, s1);
      store_row<EPL, VEC>(dst + 2 * W, L, s2);
      store_row<EPL, VEC>(dst + 3 * W, L, mn);
      store_row<EPL, VEC>(dst + 4 * W, L, mx);
      store_row<EPL, VEC>(dst + 5 * W, L, cmn);
      store_row<EPL, VEC>(dst + 6 * W, L, cmx);
      continue;
    }
    const float n = static_cast<float>(s.k1 - s.k0);
    float mean[EPL], sd[EPL], pd[EPL], r[EPL];
    if (n > 0.f) {
      load_row<EPL, VEC>(p_dst + s.row * ld_dst, L, pd);
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        mean[e] = sh[e] + s1[e] / n;
        sd[e] = pna_std(s2[e] - s1[e] * s1[e] / n, n);
      }
    } else {
#pragma unroll
      for (int e = 0; e < EPL; ++e) {
        mean[e] = sd[e] = pd[e] = mn[e] = mx[e] = 0.f;
        cmn[e] = cmx[e] = 1.f;
      }
    }
    const int64_t at = s.row * W;
    if (o.stat[0]) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = pd[e] + mean[e];
      store_row<EPL, VEC>(o.stat[0] + at, L, r);
    }
    if (o.stat[1]) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = pd[e] + mn[e];
      store_row<EPL, VEC>(o.stat[1] + at, L, r);
    }
    if (o.stat[2]) {
#pragma unroll
      for (int e = 0; e < EPL; ++e) r[e] = pd[e] + mx[e];
      store_row<EPL, VEC>(o.stat[2] + at, L, r);
    }
    if (o.stat[3]) store_row<EPL, VEC>(o.stat[3] + at, L, sd);
    store_row<EPL, VEC>(o.saved + at, L, mean);
    store_row<EPL, VEC>(o.saved + o.plane + at, L, mn);
    store_row<EPL, VEC>(o.saved + 2 * o.plane + at, L, mx);
    store_row<EPL, VEC>(o.saved + 3 * o.plane + at, L, sd);
    store_row<EPL, VEC>(o.saved + 4 * o.plane + at, L, cmn);
    store_row<EPL, VEC>(o.saved + 5 * o.plane + at, L, cmx);
  }
}

// hub rows, forward: the chunks' partials IN CHUNK ORDER — equal extrema add their counts, the
// moments combine by the parallel-variance formula — then the same finish as a short row
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    pna_fwd_merge_kernel(Items<IdxT> it, int64_t W, const float* __restrict__ part,
                         const float* __restrict__ p_dst, int64_t ld_dst, PnaOut o) {
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(it.hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(it.hub_cptr[hr]);
  const int64_t c1 = static_cast<int64_t>(it.hub_cptr[hr + 1]);
  const int64_t k0 = static_cast<int64_t>(it.rowptr[row]);
  const int64_t k1 = static_cast<int64_t>(it.rowptr[row + 1]);
  for (int64_t t = threadIdx.x; t < W; t += kWave) {
    float n = 0.f, mean = 0.f, m2 = 0.f, mn = INFINITY, mx = -INFINITY, cmn = 0.f, cmx = 0.f;
    for (int64_t c = c0; c < c1; ++c) {
      const int64_t b0 = k0 + (c - c0) * it.chunk;
      const int64_t b1 = b0 + it.chunk < k1 ? b0 + it.chunk : k1;
      if (b1 <= b0) continue;
      const float nb = static_cast<float>(b1 - b0);
      const float* p = part + c * kPnaParts * W + t;
      const float s1 = p[W], s2 = p[2 * W];
      const float mean_b = p[0] + s1 / nb, m2_b = s2 - s1 * s1 / nb;
      if (n == 0.f) {
        n = nb;
        mean = mean_b;
        m2 = m2_b;
      } else {
        moments_merge(n, mean, m2, nb, mean_b, m2_b);
      }
      extremum_merge(mn, cmn, p[3 * W], p[5 * W], true);
      extremum_merge(mx, cmx, p[4 * W], p[6 * W], false);
    }
    const float sd = pna_std(m2, n);  // (a hub row has slots)
    const float pd = p_dst[row * ld_dst + t];
    const int64_t at = row * W + t;
    if (o.stat[0]) o.stat[0][at] = pd + mean;
    if (o.stat[1]) o.stat[1][at] = pd + mn;
    if (o.stat[2]) o.stat[2][at] = pd + mx;
    if (o.stat[3]) o.stat[3][at] = sd;
    o.saved[at] = mean;
    o.saved[o.plane + at] = mn;
    o.saved[2 * o.plane + at] = mx;
    o.saved[3 * o.plane + at] = sd;
    o.saved[4 * o.plane + at] = cmn;
    o.saved[5 * o.plane + at] = cmx;
  }
}

// ---- backward, by source ------------------------------------------------------------------------
// A wave owns source row j (or a chunk of its out-slots) and keeps P_src[j] in registers; slot t
// has destination i = col_t[t] and edge k = edge_id_t[t].  With the coefficient row of i,
//     grad_u = A + B u + Gmin [u == min u] + Gmax [u == max u]
// (a statistic that was not selected has zero coefficients and its rows are not read), and
// grad_P_src[j] = sum_t grad_u, grad_edge_attr[k, d] = sum_c grad_u[c] Wc[c, d] (a wave sum per d),
// grad_Wc[c, d] = sum_k grad_u[c] a_k[d] in the lane's registers over all items of the wave; the
// waves of a workgroup add theirs in wave order in LDS and the workgroup leaves ONE partial.
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    pna_bwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                   const IdxT* __restrict__ edge_id_t, const float* __restrict__ p_src, int64_t ld,
                   EdgeArgs ed, const float* __restrict__ coef, int stats, int W, int lph,
                   float* __restrict__ grad_p, float* __restrict__ grad_edge,
                   float* __restrict__ part, float* __restrict__ wpart) {
  constexpr int U = PnaBwdSlots<EPL, DE>::n;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, W, lph);
  float w[LIN ? EPL : 1][LIN ? DE : 1], gw[LIN ? EPL : 1][LIN ? DE : 1], unused[EPL];
  if constexpr (LIN) {
    load_weight<EPL, VEC, DE>(ed.weight, nullptr, L, ed.De, w, unused);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
#pragma unroll
      for (int d = 0; d < DE; ++d) gw[e][d] = 0.f;
    }
  }
  const bool has_a = (stats & (kPnaMean | kPnaStd)) != 0, has_b = (stats & kPnaStd) != 0;
  const bool has_min = (stats & kPnaMin) != 0, has_max = (stats & kPnaMax) != 0;
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float x[EPL], gx[EPL];
    load_row<EPL, VEC>(p_src + s.row * ld, L, x);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gx[e] = 0.f;
    for (int64_t t = s.k0; t < s.k1; t += U) {
      float ca[U][EPL], cb[U][EPL], gn[U][EPL], gm[U][EPL], vn[U][EPL], vm[U][EPL], av[U];
      int64_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) ca[u][e] = cb[u][e] = gn[u][e] = gm[u][e] = vn[u][e] = vm[u][e] = 0.f;
        if (t + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[t + u]);
          id[u] = slot_edge(edge_id_t, t + u);
          const float* c = coef + i * kPnaCoef * W;
          if (has_a) load_row<EPL, VEC>(c, L, ca[u]);
          if (has_b) load_row<EPL, VEC>(c + W, L, cb[u]);
          if (has_min) {
            load_row<EPL, VEC>(c + 2 * W, L, gn[u]);
            load_row<EPL, VEC>(c + 4 * W, L, vn[u]);
          }
          if (has_max) {
            load_row<EPL, VEC>(c + 3 * W, L, gm[u]);
            load_row<EPL, VEC>(c + 5 * W, L, vm[u]);
          }
          if constexpr (LIN) av[u] = edge_lane(ed, id[u], lane);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          float uu[EPL], gu[EPL];
          if constexpr (LIN) {
            edge_term<EPL, DE>(w, x, av[u], uu);
          } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) uu[e] = x[e];
          }
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            float g = fmaf(cb[u][e], uu[e], ca[u][e]);
            g += (has_min && uu[e] == vn[u][e]) ? gn[u][e] : 0.f;
            g += (has_max && uu[e] == vm[u][e]) ? gm[u][e] : 0.f;
            gu[e] = g;
            gx[e] += g;
          }
          if constexpr (LIN) {  // (no bias: `unused` stays untouched)
            edge_grad_take<false, EPL, DE>(gu, av[u], w, ed.De, lane, grad_edge, id[u], gw, unused);
          }
        }
      }
    }
    if (s.chunk_id >= 0) {
      store_row<EPL, VEC>(part + s.chunk_id * W, L, gx);
    } else {
      store_row<EPL, VEC>(grad_p + s.row * W, L, gx);
    }
  }
  if constexpr (LIN) {
    __shared__ float red[kGineMaxWeight];
    const int De = ed.De;
    const int WD = W * De;
    for (int wv = 0; wv < kWavesPerBlock; ++wv) {
      if (wave_in_block() == wv) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int c = lane_col<VEC>(L, e);
          if (L.head_ok && c < W) {
#pragma unroll
            for (int d = 0; d < DE; ++d) {
              if (d < De) red[c * De + d] = (wv == 0 ? 0.f : red[c * De + d]) + gw[e][d];
            }
          }
        }
      }
      __syncthreads();
    }
    float* dst = wpart + static_cast<int64_t>(blockIdx.x) * WD;
    for (int t = threadIdx.x; t < WD; t += kBlock) dst[t] = red[t];
  }
}

// ---- host side -------------------------------------------------------------------------------
// the chunks' partials of the forward (the backward's single row per chunk fits inside them), then
// the backward's per-workgroup partials of grad_Wc
int64_t pna_chunk_floats(int64_t n_chunks, int64_t W) { return n_chunks * kPnaParts * W; }

size_t pna_ws_bytes(int64_t n_chunks, int64_t W, int64_t De) {
  return sizeof(float) *
         static_cast<size_t>(pna_chunk_floats(n_chunks, W) + wpart_floats(W, De, false));
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_pna_supported(int64_t W, int64_t De) { return gine_envelope(W, De) ? 1 : 0; }

int pygamd_pna_workspace_bytes(int64_t n_chunks, int64_t W, int64_t De, size_t* bytes) {
  if (!bytes || n_chunks < 0 || W < 1 || De < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!gine_envelope(W, De)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = pna_ws_bytes(n_chunks, W, De);
  return PYGAMD_OK;
}

int pygamd_pna_forward(const pygamd_csr* g, const void* edge_id, const float* p_src,
                       int64_t ld_src, const float* p_dst, int64_t ld_dst,
                       const float* edge_attr, const float* wc, int64_t n_src, int64_t W,
                       int64_t De, int stats, float* out, float* saved, void* workspace,
                       size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, W, De);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld_src < W || ld_dst < W || stats < 1 || stats > 15) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  const EdgeArgs ed{edge_attr, wc, nullptr, static_cast<int>(De)};
  if (!g->rowptr || !g->col || !p_src || !p_dst || !out || !saved) return PYGAMD_ERR_INVALID_ARG;
  // (the mode constants are the public ones of GEN; PNA has no edge term or the linear one)
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_NONE, ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < pna_ws_bytes(n_chunks, W, 0)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(p_src) && ld_src % 4 == 0 && aligned16(p_dst) && ld_dst % 4 == 0 &&
                  aligned16(out) && aligned16(saved) && (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(W, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  PnaOut o;
  o.plane = n_rows * W;
  o.saved = saved;
  float* next = out;  // the selected statistics follow each other in the order mean, min, max, std
  for (int q = 0; q < 4; ++q) {
    o.stat[q] = (stats >> q) & 1 ? next : nullptr;
    if (o.stat[q]) next += o.plane;
  }
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(gine_grid(n_rows + n_chunks, De > 0, kGineFwdBlocks)), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((pna_fwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), p_src, ld_src,
                         p_dst, ld_dst, ed, static_cast<int>(W), sh.lph, o, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((pna_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it, W, part, p_dst, ld_dst, o);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_pna_backward(const pygamd_csr* g, const void* edge_id_t, const float* p_src,
                        int64_t ld_src, const float* edge_attr, const float* wc,
                        const float* coef, int64_t n_dst, int64_t W, int64_t De, int stats,
                        float* grad_p_src, float* grad_edge_attr, float* grad_wc, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_dst, W, De);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (ld_src < W || stats < 1 || stats > 15) return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  const EdgeArgs ed{edge_attr, wc, nullptr, static_cast<int>(De)};
  if (!g->rowptr || !g->col || !p_src || !coef || !grad_p_src ||
      (De > 0) != (grad_wc != nullptr) || (De == 0 && grad_edge_attr))
    return PYGAMD_ERR_INVALID_ARG;
  // (the mode constants are the public ones of GEN; PNA has no edge term or the linear one)
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_NONE, ed);
  if (rce != PYGAMD_OK) return rce;
  if ((n_chunks > 0 || De > 0) && (!workspace || workspace_bytes < pna_ws_bytes(n_chunks, W, De)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(p_src) && ld_src % 4 == 0 && aligned16(coef) &&
                  aligned16(grad_p_src) && (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(W, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* wpart = part + pna_chunk_floats(n_chunks, W);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const unsigned n_blocks = gine_grid(n_src + n_chunks, De > 0, kGineBwdBlocks);
    const dim3 grid(n_blocks), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((pna_bwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t), p_src, ld_src,
                         ed, coef, stats, static_cast<int>(W), sh.lph, grad_p_src, grad_edge_attr,
                         part, wpart);
    });
    PYGAMD_LAUNCH_CHECK();
    return launch_backward_tail<IdxT>(it, W, De, false, n_blocks, part, grad_p_src, wpart, grad_wc,
                                      nullptr, st);
  });
}

}  // extern "C"

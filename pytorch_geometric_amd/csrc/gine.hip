// gine.hip — the edge message of GINEConv (nn/conv/gin_conv.py:19-207 of the reference) as a pair
// of row-gather kernels on a sorted handle.  For destination i and the source j of slot k:
//     e_k      = edge_attr[k, :]                      (wide,   edge_dim = None)
//              = W a_k + b,  a_k = edge_attr[k, :De]   (linear, edge_dim = De; W [F, De], b [F])
//     out[i,:] = (1 + eps) * x_root[i,:] + sum_k max(x_src[j,:] + e_k, 0)
// The ReLU sits between the edge term and the sum, so nothing factors out per destination (as the
// linear edge term of transformer.hip does): the kernels rebuild e_k per slot, in registers.  In
// linear mode every lane keeps the rows of W of ITS columns in registers for the whole launch and
// a slot's raw features reach the lanes by v_readlane: no [E, F] value exists anywhere.
//
// Lanes run over the F columns (rowwalk_device.h's layout with one head): scalar registers for any
// F, float4 units where F % 4 == 0 and every row is 16-byte aligned.  Work items, the hub plan's
// chunks and the in-order merge of a long row's partials: rowwalk_device.h.  The forward walks the
// CSR by destination, the backward the CSR by source and visits every edge exactly once.  No float
// atomics anywhere: every result is bitwise reproducible.
#include <math.h>

#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using namespace gine;

template <int EPL, int DE>
struct GineSlots {  // slots in flight per wave
  static constexpr int n = (EPL >= 8 || DE > 0) ? 2 : 4;
};

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    gine_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                    const IdxT* __restrict__ edge_id, const float* __restrict__ x_src, int64_t ld,
                    const float* __restrict__ x_root, int64_t ld_root,
                    const float* __restrict__ eps, EdgeArgs ed, int F, int lph,
                    float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = GineSlots<EPL, DE>::n;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float w[LIN ? EPL : 1][LIN ? DE : 1], b[EPL];
  if constexpr (LIN) load_weight<EPL, VEC, DE>(ed.weight, ed.bias, L, ed.De, w, b);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float acc[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float xx[U][EPL], ee[U][EPL], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const int64_t j = static_cast<int64_t>(col[k + u]);
          const int64_t id = slot_edge(edge_id, k + u);
          load_row<EPL, VEC>(x_src + j * ld, L, xx[u]);
          if constexpr (LIN) {
            av[u] = edge_lane(ed, id, lane);
          } else {
            load_row<EPL, VEC>(ed.edge_attr + id * F, L, ee[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          if constexpr (LIN) edge_term<EPL, DE>(w, b, av[u], ee[u]);
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] += fmaxf(xx[u][e] + ee[u][e], 0.f);
        }
      }
    }
    if (s.chunk_id >= 0) {  // partial sum of one chunk of a long row
      store_row<EPL, VEC>(part + s.chunk_id * F, L, acc);
      continue;
    }
    if (x_root) {
      const float sc = 1.f + (eps ? *eps : 0.f);
      float r[EPL];
      load_row<EPL, VEC>(x_root + s.row * ld_root, L, r);
#pragma unroll
      for (int e = 0; e < EPL; ++e) acc[e] = fmaf(sc, r[e], acc[e]);
    }
    store_row<EPL, VEC>(out + s.row * F, L, acc);
  }
}

// hub rows, forward: the chunks' partial sums in chunk order, then the self term
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    gine_fwd_merge_kernel(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_cptr,
                          int64_t F, const float* __restrict__ part,
                          const float* __restrict__ x_root, int64_t ld_root,
                          const float* __restrict__ eps, float* __restrict__ out) {
  const int64_t hr = blockIdx.x;
  merge_sum_row(hub_rows, hub_cptr, hr, F, part, F, out, F);
  if (!x_root) return;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const float sc = 1.f + (eps ? *eps : 0.f);
  // (thread t wrote the columns t, t + 64, ... above: it reads its own stores)
  for (int64_t t = threadIdx.x; t < F; t += kWave)
    out[row * F + t] = fmaf(sc, x_root[row * ld_root + t], out[row * F + t]);
}

// ---- backward, by source ------------------------------------------------------------------------
// A wave owns source row j (or a chunk of its out-slots) and keeps x_src[j] in registers; slot t
// has destination i = col_t[t] and edge k = edge_id_t[t].  m = (x_src[j] + e_k > 0), g =
// grad_out[i]:  grad_x_src[j] = sum_t m g;  wide: grad_edge_attr[k] = m g;  linear:
// grad_edge_attr[k,d] = sum_f m g W[f,d] (a wave sum per d), and grad_W[f,d] = sum_k m g a_k[d],
// grad_b[f] = sum_k m g accumulate in the lane's registers over all items of the wave; the waves
// of a workgroup add theirs in wave order in LDS and the workgroup leaves ONE partial.
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    gine_bwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                    const IdxT* __restrict__ edge_id_t, const float* __restrict__ x_src,
                    int64_t ld, EdgeArgs ed, const float* __restrict__ grad_out, int F, int lph,
                    float* __restrict__ grad_x, float* __restrict__ grad_edge,
                    float* __restrict__ part, float* __restrict__ wpart) {
  constexpr int U = GineSlots<EPL, DE>::n;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float w[LIN ? EPL : 1][LIN ? DE : 1], b[EPL];
  float gw[LIN ? EPL : 1][LIN ? DE : 1], gb[EPL];
  if constexpr (LIN) {
    load_weight<EPL, VEC, DE>(ed.weight, ed.bias, L, ed.De, w, b);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      gb[e] = 0.f;
#pragma unroll
      for (int d = 0; d < DE; ++d) gw[e][d] = 0.f;
    }
  }
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float x[EPL], gx[EPL];
    load_row<EPL, VEC>(x_src + s.row * ld, L, x);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gx[e] = 0.f;
    for (int64_t t = s.k0; t < s.k1; t += U) {
      float gg[U][EPL], ee[U][EPL], av[U];
      int64_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[t + u]);
          id[u] = slot_edge(edge_id_t, t + u);
          load_row<EPL, VEC>(grad_out + i * F, L, gg[u]);
          if constexpr (LIN) {
            av[u] = edge_lane(ed, id[u], lane);
          } else {
            load_row<EPL, VEC>(ed.edge_attr + id[u] * F, L, ee[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          if constexpr (LIN) edge_term<EPL, DE>(w, b, av[u], ee[u]);
          float mg[EPL];
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            mg[e] = (x[e] + ee[u][e] > 0.f) ? gg[u][e] : 0.f;
            gx[e] += mg[e];
          }
          if constexpr (LIN) {
            edge_grad_take<true, EPL, DE>(mg, av[u], w, ed.De, lane, grad_edge, id[u], gw, gb);
          } else {
            if (grad_edge) store_row<EPL, VEC>(grad_edge + id[u] * F, L, mg);
          }
        }
      }
    }
    if (s.chunk_id >= 0) {
      store_row<EPL, VEC>(part + s.chunk_id * F, L, gx);
    } else {
      store_row<EPL, VEC>(grad_x + s.row * F, L, gx);
    }
  }
  if constexpr (LIN) {
    __shared__ float red[kGineMaxWeight + kMaxWidth];
    const int De = ed.De;
    const int FD = F * De;
    for (int wv = 0; wv < kWavesPerBlock; ++wv) {
      if (wave_in_block() == wv) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int c = lane_col<VEC>(L, e);
          if (L.head_ok && c < F) {
#pragma unroll
            for (int d = 0; d < DE; ++d) {
              if (d < De) red[c * De + d] = (wv == 0 ? 0.f : red[c * De + d]) + gw[e][d];
            }
            red[FD + c] = (wv == 0 ? 0.f : red[FD + c]) + gb[e];
          }
        }
      }
      __syncthreads();
    }
    float* dst = wpart + static_cast<int64_t>(blockIdx.x) * (FD + F);
    for (int t = threadIdx.x; t < FD + F; t += kBlock) dst[t] = red[t];
  }
}

// ---- host side -------------------------------------------------------------------------------
size_t gine_ws_bytes(int64_t n_chunks, int64_t F, int64_t De) {
  // a chunk's partial row; in linear mode the backward's partials of (grad_W, grad_b) follow
  return sizeof(float) * static_cast<size_t>(n_chunks * F + wpart_floats(F, De, true));
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_gine_supported(int64_t F, int64_t De) { return gine_envelope(F, De) ? 1 : 0; }

int pygamd_gine_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F < 1 || De < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!gine_envelope(F, De)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = gine_ws_bytes(n_chunks, F, De);
  return PYGAMD_OK;
}

int pygamd_gine_forward(const pygamd_csr* g, const void* edge_id, const float* x_src,
                        int64_t ld_src, const float* x_root, int64_t ld_root, const float* eps,
                        const float* edge_attr, const float* weight, const float* bias,
                        int64_t n_src, int64_t F, int64_t De, float* out, void* workspace,
                        size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, De);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld_src < F || (x_root && ld_root < F)) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  const EdgeArgs ed{edge_attr, weight, bias, static_cast<int>(De)};
  if (!g->rowptr || !g->col || !x_src || !out) return PYGAMD_ERR_INVALID_ARG;
  // (the mode constants are the public ones of GEN; GINE has the wide and the linear mode)
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_WIDE, ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * F))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(x_src) && ld_src % 4 == 0 && aligned16(out) &&
                  (De > 0 || aligned16(edge_attr)) &&
                  (!x_root || (aligned16(x_root) && ld_root % 4 == 0)) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(gine_grid(n_rows + n_chunks, De > 0, kGineFwdBlocks)), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((gine_fwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), x_src,
                         ld_src, x_root, ld_root, eps, ed, static_cast<int>(F), sh.lph, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((gine_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, F, part, x_root, ld_root,
                         eps, out);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_gine_backward(const pygamd_csr* g, const void* edge_id_t, const float* x_src,
                         int64_t ld_src, const float* edge_attr, const float* weight,
                         const float* bias, const float* grad_out, int64_t n_dst, int64_t F,
                         int64_t De, float* grad_x_src, float* grad_edge_attr, float* grad_weight,
                         float* grad_bias, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_dst, F, De);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (ld_src < F) return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  const EdgeArgs ed{edge_attr, weight, bias, static_cast<int>(De)};
  if (!g->rowptr || !g->col || !x_src || !grad_out || !grad_x_src ||
      (De > 0) != (grad_weight != nullptr) || (grad_bias && !bias))
    return PYGAMD_ERR_INVALID_ARG;
  // (the mode constants are the public ones of GEN; GINE has the wide and the linear mode)
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_WIDE, ed);
  if (rce != PYGAMD_OK) return rce;
  if ((n_chunks > 0 || De > 0) &&
      (!workspace || workspace_bytes < gine_ws_bytes(n_chunks, F, De)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(x_src) && ld_src % 4 == 0 && aligned16(grad_out) &&
                  aligned16(grad_x_src) &&
                  (De > 0 || (aligned16(edge_attr) && aligned16(grad_edge_attr))) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* wpart = part + n_chunks * F;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const unsigned n_blocks = gine_grid(n_src + n_chunks, De > 0, kGineBwdBlocks);
    const dim3 grid(n_blocks), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((gine_bwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t),
                         x_src, ld_src, ed, grad_out, static_cast<int>(F), sh.lph, grad_x_src,
                         grad_edge_attr, part, wpart);
    });
    PYGAMD_LAUNCH_CHECK();
    return launch_backward_tail<IdxT>(it, F, De, true, n_blocks, part, grad_x_src, wpart,
                                      grad_weight, grad_bias, st);
  });
}

}  // extern "C"

// resgated.hip — the propagate step of ResGatedGraphConv (nn/conv/res_gated_graph_conv.py:128 and
// its message, 138-148, of the reference) as row-gather kernels on a sorted handle.  For
// destination i, slot k with source j = col[k], raw edge features a_k = edge_attr[edge_id[k], :De]:
//     z_k      = K[i,:] + Q[j,:] + Wg a_k          (Wg = Wk_e + Wq_e; without edge_dim: no a_k)
//     u_k      = V[j,:] + Wv a_k
//     out[i,:] = sum_k sigmoid(z_k) * u_k
// K [N_dst, F] and the packed QV = [Q | V] [N_src, 2F] are node-level projections with every bias
// folded in (the algebra: include/pyg_amd.h).  A slot gathers ONE 2F row; the edge terms are
// rebuilt per slot from the raw features with the rows of Wg and Wv of the lane's columns in
// registers, as gine.hip does for its one matrix.  Nothing of size E x F exists anywhere and the
// backward recomputes the sigmoid from the inputs.
//
// Backward, with s = sigmoid(z), gz = g u s (1 - s), gu = g s (g = grad_out[i,:]):
//   by destination (the forward's handle):  grad_K[i,:] = sum_k gz, and with De > 0 per slot
//     grad_edge_attr[k,:] = Wg^T gz + Wv^T gu and the per-workgroup partials of grad_Wg = sum gz
//     a^T, grad_Wv = sum gu a^T.  This pass carries ONE accumulator row, so it has the registers
//     for the two matrices and their two gradient accumulators (profiles/resgated_conv.md).
//   by source (the transposed handle):  Q[j], V[j] stay in registers, a slot gathers K[i] and g[i]
//     (each pointer-plus-stride: two rows in place, or the halves of one packed row), and the
//     packed grad_QV[j,:] = [sum gz | sum gu] is written once.
//
// Lane layout, work items, hub chunks, in-order merges and the reduce of the parameter partials:
// rowwalk_device.h.  Edge term, lane shape, capped grid and dispatch: gine_device.h.  No float
// atomics anywhere and every grid depends on the problem's sizes only: every result is bitwise
// reproducible.
#include <math.h>

#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using namespace gine;

// Two matrices share the registers gine.hip gives one: 2 * 2048 / 64 = 64 registers per lane for
// the weights, and as many for their gradients in the by-destination backward.
constexpr int kResMaxWeight = 2048;  // F * De
constexpr int kResMaxRegs = 64;      // EPL * DE of a reachable instantiation

template <int EPL, int DE>
struct ResSlots {  // slots in flight per wave (two rows per slot)
  static constexpr int fwd = DE > 0 ? (EPL * DE >= 64 ? 1 : 2) : (EPL >= 8 ? 2 : 4);
  static constexpr int dst = DE > 0 ? (EPL * DE >= 32 ? 1 : 2) : (EPL >= 8 ? 2 : 4);
  static constexpr int src = fwd;
};

// The edge arguments are gine_device.h's EdgeArgs without a bias: edge_attr [E, De] and weight
// [2, F, De] = Wg, then Wv; both NULL with De = 0.

// plain 1 / (1 + exp(-z)): exactly 0.5 at 0; expf overflows to +inf (s = 0) or underflows to 0
// (s = 1) without a NaN, and s (1 - s) is exactly 0 there
__device__ __forceinline__ float sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// the rows of Wg and Wv of the lane's columns
template <int EPL, bool VEC, int DE>
__device__ __forceinline__ void load_weights(const EdgeArgs& ed, const Lay& L, int F,
                                             float (&wg)[EPL][DE], float (&wv)[EPL][DE]) {
  float none[EPL];
  load_weight<EPL, VEC, DE>(ed.weight, nullptr, L, ed.De, wg, none);
  load_weight<EPL, VEC, DE>(ed.weight + static_cast<int64_t>(F) * ed.De, nullptr, L, ed.De, wv,
                            none);
}

// z = kk + q (+ Wg a), u = v (+ Wv a) of one slot; lane d holds a[d] in `av`
template <int EPL, int DE, int WE, int WD>
__device__ __forceinline__ void slot_terms(const float (&kk)[EPL], const float (&q)[EPL],
                                           const float (&v)[EPL], const float (&wg)[WE][WD],
                                           const float (&wv)[WE][WD], float av, float (&z)[EPL],
                                           float (&u)[EPL]) {
  if constexpr (DE > 0) {
    edge_term<EPL, DE>(wg, kk, av, z);
    edge_term<EPL, DE>(wv, v, av, u);
#pragma unroll
    for (int e = 0; e < EPL; ++e) z[e] += q[e];
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      z[e] = kk[e] + q[e];
      u[e] = v[e];
    }
  }
}

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    resgated_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                        const IdxT* __restrict__ edge_id, const float* __restrict__ K,
                        int64_t ld_k, const float* __restrict__ QV, int64_t ld_qv, EdgeArgs ed,
                        int F, int lph, float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = ResSlots<EPL, DE>::fwd;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wg[LIN ? EPL : 1][LIN ? DE : 1], wv[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) load_weights<EPL, VEC, DE>(ed, L, F, wg, wv);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float kk[EPL], acc[EPL];
    load_row<EPL, VEC>(K + s.row * ld_k, L, kk);
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float qq[U][EPL], vv[U][EPL], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const float* row = QV + static_cast<int64_t>(col[k + u]) * ld_qv;
          load_row<EPL, VEC>(row, L, qq[u]);
          load_row<EPL, VEC>(row + F, L, vv[u]);
          if constexpr (LIN) av[u] = edge_lane(ed, slot_edge(edge_id, k + u), lane);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          float z[EPL], uu[EPL];
          slot_terms<EPL, DE>(kk, qq[u], vv[u], wg, wv, LIN ? av[u] : 0.f, z, uu);
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(sigmoid(z[e]), uu[e], acc[e]);
        }
      }
    }
    if (s.chunk_id >= 0) {  // partial sum of one chunk of a long row
      store_row<EPL, VEC>(part + s.chunk_id * F, L, acc);
    } else {
      store_row<EPL, VEC>(out + s.row * F, L, acc);
    }
  }
}

// ---- backward, by destination ----------------------------------------------------------------
// A wave owns destination i (or a chunk of its slots) with K[i] and g = grad_out[i] in registers.
// wpart: one partial of (grad_Wg [F De], grad_Wv [F De]) per workgroup, its waves added in wave
// order.
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    resgated_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                            const IdxT* __restrict__ edge_id, const float* __restrict__ K,
                            int64_t ld_k, const float* __restrict__ QV, int64_t ld_qv, EdgeArgs ed,
                            const float* __restrict__ grad_out, int64_t ld_g, int F, int lph,
                            float* __restrict__ grad_k, float* __restrict__ grad_edge,
                            float* __restrict__ part, float* __restrict__ wpart) {
  constexpr int U = ResSlots<EPL, DE>::dst;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wg[LIN ? EPL : 1][LIN ? DE : 1], wv[LIN ? EPL : 1][LIN ? DE : 1];
  float gwg[LIN ? EPL : 1][LIN ? DE : 1], gwv[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) {
    load_weights<EPL, VEC, DE>(ed, L, F, wg, wv);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
#pragma unroll
      for (int d = 0; d < DE; ++d) gwg[e][d] = gwv[e][d] = 0.f;
    }
  }
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float kk[EPL], g[EPL], gk[EPL];
    load_row<EPL, VEC>(K + s.row * ld_k, L, kk);
    load_row<EPL, VEC>(grad_out + s.row * ld_g, L, g);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gk[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float qq[U][EPL], vv[U][EPL], av[U];
      int64_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const float* row = QV + static_cast<int64_t>(col[k + u]) * ld_qv;
          load_row<EPL, VEC>(row, L, qq[u]);
          load_row<EPL, VEC>(row + F, L, vv[u]);
          if constexpr (LIN) {
            id[u] = slot_edge(edge_id, k + u);
            av[u] = edge_lane(ed, id[u], lane);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          float z[EPL], uu[EPL], gz[EPL], gu[EPL];
          slot_terms<EPL, DE>(kk, qq[u], vv[u], wg, wv, LIN ? av[u] : 0.f, z, uu);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float sg = sigmoid(z[e]);
            gz[e] = (g[e] * uu[e]) * (sg * (1.f - sg));
            gu[e] = g[e] * sg;
            gk[e] += gz[e];
          }
          if constexpr (LIN) {
            // the parameter gradients of both matrices; the edge's own gradient takes both terms
            // in ONE wave sum per feature
            float none[EPL];  // (no bias: never touched)
            edge_grad_take<false, EPL, DE>(gz, av[u], wg, ed.De, lane, nullptr, id[u], gwg, none);
            edge_grad_take<false, EPL, DE>(gu, av[u], wv, ed.De, lane, nullptr, id[u], gwv, none);
            if (grad_edge) {
              float mine = 0.f;
#pragma unroll
              for (int d = 0; d < DE; ++d) {
                if (d < ed.De) {
                  float p = 0.f;
#pragma unroll
                  for (int e = 0; e < EPL; ++e) p = fmaf(gu[e], wv[e][d], fmaf(gz[e], wg[e][d], p));
                  p = group_sum(p, kWave);
                  if (lane == d) mine = p;
                }
              }
              if (lane < ed.De) grad_edge[id[u] * ed.De + lane] = mine;
            }
          }
        }
      }
    }
    if (s.chunk_id >= 0) {
      store_row<EPL, VEC>(part + s.chunk_id * F, L, gk);
    } else {
      store_row<EPL, VEC>(grad_k + s.row * F, L, gk);
    }
  }
  if constexpr (LIN) {
    __shared__ float red[2 * kResMaxWeight];
    const int De = ed.De;
    const int FD = F * De;
    for (int wave = 0; wave < kWavesPerBlock; ++wave) {
      if (wave_in_block() == wave) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const int c = lane_col<VEC>(L, e);
          if (L.head_ok && c < F) {
#pragma unroll
            for (int d = 0; d < DE; ++d) {
              if (d < De) {
                const int o = c * De + d;
                red[o] = (wave == 0 ? 0.f : red[o]) + gwg[e][d];
                red[FD + o] = (wave == 0 ? 0.f : red[FD + o]) + gwv[e][d];
              }
            }
          }
        }
      }
      __syncthreads();
    }
    float* dst = wpart + static_cast<int64_t>(blockIdx.x) * (2 * FD);
    for (int t = threadIdx.x; t < 2 * FD; t += kBlock) dst[t] = red[t];
  }
}

// ---- backward, by source ---------------------------------------------------------------------
// A wave owns source j (or a chunk of its out-slots) with Q[j], V[j] in registers; slot t has
// destination i = col_t[t] and edge edge_id_t[t].  part and grad_qv hold rows of 2F: [gq | gv].
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    resgated_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                            const IdxT* __restrict__ edge_id_t, const float* __restrict__ K,
                            int64_t ld_k, const float* __restrict__ QV, int64_t ld_qv, EdgeArgs ed,
                            const float* __restrict__ grad_out, int64_t ld_g, int F, int lph,
                            float* __restrict__ grad_qv, float* __restrict__ part) {
  constexpr int U = ResSlots<EPL, DE>::src;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wg[LIN ? EPL : 1][LIN ? DE : 1], wv[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) load_weights<EPL, VEC, DE>(ed, L, F, wg, wv);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float q[EPL], v[EPL], gq[EPL], gv[EPL];
    load_row<EPL, VEC>(QV + s.row * ld_qv, L, q);
    load_row<EPL, VEC>(QV + s.row * ld_qv + F, L, v);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gq[e] = gv[e] = 0.f;
    for (int64_t t = s.k0; t < s.k1; t += U) {
      float kk[U][EPL], gg[U][EPL], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[t + u]);
          load_row<EPL, VEC>(K + i * ld_k, L, kk[u]);
          load_row<EPL, VEC>(grad_out + i * ld_g, L, gg[u]);
          if constexpr (LIN) av[u] = edge_lane(ed, slot_edge(edge_id_t, t + u), lane);
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          float z[EPL], uu[EPL];
          slot_terms<EPL, DE>(kk[u], q, v, wg, wv, LIN ? av[u] : 0.f, z, uu);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float sg = sigmoid(z[e]);
            gq[e] += (gg[u][e] * uu[e]) * (sg * (1.f - sg));
            gv[e] += gg[u][e] * sg;
          }
        }
      }
    }
    float* row = s.chunk_id >= 0 ? part + s.chunk_id * 2 * F : grad_qv + s.row * 2 * F;
    store_row<EPL, VEC>(row, L, gq);
    store_row<EPL, VEC>(row + F, L, gv);
  }
}

// ---- host side -------------------------------------------------------------------------------
bool res_envelope(int64_t F, int64_t De) {
  if (F < 1 || F > kMaxWidth || De < 0) return false;
  return De == 0 || (De <= kGineMaxDe && F * De <= kResMaxWeight);
}

size_t res_ws_bytes(int64_t n_chunks, int64_t F, int64_t De) {
  // a chunk's partial row (2F: the by-source backward's); with De > 0 the by-destination
  // backward's per-workgroup partials of (grad_Wg, grad_Wv) follow
  return sizeof(float) * static_cast<size_t>(n_chunks * 2 * F + wpart_floats(F, 2 * De, false));
}

// gine_device.h's shape table, without the instantiations the narrower envelope never reaches
#define RES_DISPATCH(...)                                  \
  GINE_DISPATCH({                                          \
    if constexpr (EPL * DE <= kResMaxRegs) {               \
      __VA_ARGS__                                          \
    } else {                                               \
      return PYGAMD_ERR_UNSUPPORTED;                       \
    }                                                      \
  })

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_resgated_supported(int64_t F, int64_t De) { return res_envelope(F, De) ? 1 : 0; }

int pygamd_resgated_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F < 1 || De < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!res_envelope(F, De)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = res_ws_bytes(n_chunks, F, De);
  return PYGAMD_OK;
}

int pygamd_resgated_forward(const pygamd_csr* g, const void* edge_id, const float* k, int64_t ld_k,
                            const float* qv, int64_t ld_qv, const float* edge_attr,
                            const float* weight, int64_t n_src, int64_t F, int64_t De, float* out,
                            void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, De, res_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (ld_k < F || ld_qv < 2 * F) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !k || !qv || !out) return PYGAMD_ERR_INVALID_ARG;
  const EdgeArgs ed{edge_attr, weight, nullptr, static_cast<int>(De)};
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_NONE, ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * F))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(k) && ld_k % 4 == 0 && aligned16(qv) && ld_qv % 4 == 0 &&
                  aligned16(out) && (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(gine_grid(n_rows + n_chunks, De > 0, kGineFwdBlocks)), block(kBlock);
    RES_DISPATCH({
      hipLaunchKernelGGL((resgated_fwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), k, ld_k, qv,
                         ld_qv, ed, static_cast<int>(F), sh.lph, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' partial sums in chunk order)
    return launch_sum_merge(it, F, part, out, st);
  });
}

int pygamd_resgated_backward_dst(const pygamd_csr* g, const void* edge_id, const float* k,
                                 int64_t ld_k, const float* qv, int64_t ld_qv,
                                 const float* edge_attr, const float* weight,
                                 const float* grad_out, int64_t ld_g, int64_t n_src, int64_t F,
                                 int64_t De, float* grad_k, float* grad_edge_attr,
                                 float* grad_weight, void* workspace, size_t workspace_bytes,
                                 void* stream) {
  const int rc = gine_check(g, n_src, F, De, res_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (ld_k < F || ld_qv < 2 * F || ld_g < F) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !k || !qv || !grad_out || !grad_k ||
      (De > 0) != (grad_weight != nullptr) || (De == 0 && grad_edge_attr))
    return PYGAMD_ERR_INVALID_ARG;
  const EdgeArgs ed{edge_attr, weight, nullptr, static_cast<int>(De)};
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_NONE, ed);
  if (rce != PYGAMD_OK) return rce;
  if ((n_chunks > 0 || De > 0) &&
      (!workspace || workspace_bytes < res_ws_bytes(n_chunks, F, De)))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(k) && ld_k % 4 == 0 && aligned16(qv) && ld_qv % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_k) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* wpart = part + n_chunks * 2 * F;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const unsigned n_blocks = gine_grid(n_rows + n_chunks, De > 0, kGineBwdBlocks);
    const dim3 grid(n_blocks), block(kBlock);
    RES_DISPATCH({
      hipLaunchKernelGGL((resgated_bwd_dst_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), k, ld_k, qv,
                         ld_qv, ed, grad_out, ld_g, static_cast<int>(F), sh.lph, grad_k,
                         grad_edge_attr, part, wpart);
    });
    PYGAMD_LAUNCH_CHECK();
    // (the partials hold two matrices: 2 F De floats per workgroup, as one of [F, 2 De] would)
    return launch_backward_tail<IdxT>(it, F, 2 * De, false, n_blocks, part, grad_k, wpart,
                                      grad_weight, nullptr, st);
  });
}

int pygamd_resgated_backward_src(const pygamd_csr* g, const void* edge_id_t, const float* k,
                                 int64_t ld_k, const float* qv, int64_t ld_qv,
                                 const float* edge_attr, const float* weight,
                                 const float* grad_out, int64_t ld_g, int64_t n_dst, int64_t F,
                                 int64_t De, float* grad_qv, void* workspace,
                                 size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_dst, F, De, res_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (ld_k < F || ld_qv < 2 * F || ld_g < F) return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !k || !qv || !grad_out || !grad_qv) return PYGAMD_ERR_INVALID_ARG;
  const EdgeArgs ed{edge_attr, weight, nullptr, static_cast<int>(De)};
  const int rce = check_edge(De > 0 ? PYGAMD_GEN_EDGE_LINEAR : PYGAMD_GEN_EDGE_NONE, ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * 2 * F))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(k) && ld_k % 4 == 0 && aligned16(qv) && ld_qv % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_qv) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(gine_grid(n_src + n_chunks, De > 0, kGineBwdBlocks)), block(kBlock);
    RES_DISPATCH({
      hipLaunchKernelGGL((resgated_bwd_src_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t), k, ld_k, qv,
                         ld_qv, ed, grad_out, ld_g, static_cast<int>(F), sh.lph, grad_qv, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' packed partial rows of 2F in chunk order)
    return launch_sum_merge(it, 2 * F, part, grad_qv, st);
  });
}

}  // extern "C"

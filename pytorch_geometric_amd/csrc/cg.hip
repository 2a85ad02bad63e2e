// cg.hip — the propagate step of CGConv (nn/conv/cg_conv.py:88 and its message, 93-98, of the
// reference) as row-gather kernels on a sorted handle.  For destination i, slot k with source
// j = col[k] and edge id = edge_id[k]:
//     zf_k     = Pf[i,:] + Qf[j,:] + ef_k,    zs_k = Ps[i,:] + Qs[j,:] + es_k
//     out[i,:] = epilogue( sum_k sigmoid(zf_k) * softplus(zs_k) )
// P = [Pf | Ps] [N_dst, 2F] and Q = [Qf | Qs] [N_src, 2F] are node-level projections with both
// biases folded into P (the algebra: include/pyg_amd.h).  The edge terms (ef_k | es_k):
//     NONE    none;
//     LINEAR  Wf_e a_k | Ws_e a_k from the raw features a_k = edge_attr[id, :De], the rows of both
//             matrices of the lane's columns in registers, as resgated.hip holds its two;
//     WIDE    the row edge_terms[id, :2F] of a dense product the caller made.
// A slot gathers ONE 2F row of Q (and, WIDE, one of edge_terms).  The epilogue divides by the
// row's slot count (scale = 1: mean) and adds residual[i,:]; it runs once per row, after the merge
// for a split row.  Nothing is saved: the backward recomputes both activations from the inputs.
//
// Backward, with s = sigmoid(zf), p = softplus(zs), g = grad_out[i,:] (/ deg_i for mean):
//     gzf = g p s (1 - s),    gzs = g s (zs > 20 ? 1 : sigmoid(zs))
//   by destination (the forward's handle):  grad_P[i,:] = [sum_k gzf | sum_k gzs]; LINEAR: per slot
//     grad_edge_attr[id,:] = Wf_e^T gzf + Ws_e^T gzs and the per-workgroup partials of grad_Wf_e =
//     sum gzf a^T, grad_Ws_e = sum gzs a^T; WIDE: [gzf | gzs] goes to grad_edge_terms[id, :2F].
//   by source (the transposed handle):  Qf[j], Qs[j] stay in registers, a slot gathers the 2F row
//     P[i] and g[i], and grad_Q[j,:] = [sum gzf | sum gzs] is written once.
// grad_P and grad_Q carry row strides: the two launches may write the halves of one plane.
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

// Two matrices and, by destination, their two gradients in registers next to FIVE rows (Pf, Ps,
// g and two accumulators).  The envelope is ALL of resgated.hip's, the widest the shared workspace
// formula allows: no instantiation inside it uses scratch; at EPL * DE = 64 the by-destination
// backward holds 256 VGPRs plus 50 to 116 AGPRs, one wave per SIMD.  The choice rests on the
// compiler's report alone: those shapes were not timed against WIDE (profiles/cg_conv.md).
constexpr int kCgMaxDe = 32;
constexpr int kCgMaxWeight = 2048;  // F * De
constexpr int kCgMaxRegs = 64;      // EPL * DE of a reachable instantiation

template <int EPL, int DE, bool WIDE>
struct CgSlots {  // slots in flight per wave (a 2F row per slot; WIDE: two of them)
  static constexpr int fwd =
      DE > 0 ? (EPL * DE >= 64 ? 1 : 2) : WIDE ? (EPL >= 8 ? 1 : 2) : (EPL >= 8 ? 2 : 4);
  static constexpr int dst = DE > 0 ? (EPL * DE >= 32 ? 1 : 2) : fwd;
  static constexpr int src = DE > 0 ? fwd : (EPL >= 8 ? 1 : 2);  // (three rows per slot)
};

// resgated.hip's: exactly 0.5 at 0, exactly 0 or 1 beyond expf's range, never a NaN
__device__ __forceinline__ float sigmoid(float z) { return 1.f / (1.f + expf(-z)); }

// torch.nn.functional.softplus (beta 1, threshold 20)
__device__ __forceinline__ float softplus(float z) { return z > 20.f ? z : log1pf(expf(z)); }
__device__ __forceinline__ float softplus_grad(float z) { return z > 20.f ? 1.f : sigmoid(z); }

// the rows of Wf_e and Ws_e of the lane's columns
template <int EPL, bool VEC, int DE>
__device__ __forceinline__ void load_weights(const EdgeArgs& ed, const Lay& L, int F,
                                             float (&wf)[EPL][DE], float (&ws)[EPL][DE]) {
  float none[EPL];
  load_weight<EPL, VEC, DE>(ed.weight, nullptr, L, ed.De, wf, none);
  load_weight<EPL, VEC, DE>(ed.weight + static_cast<int64_t>(F) * ed.De, nullptr, L, ed.De, ws,
                            none);
}

// zf = pf + qf (+ Wf_e a), zs = ps + qs (+ Ws_e a) of one slot; lane d holds a[d] in `av`
template <int EPL, int DE, int WE, int WD>
__device__ __forceinline__ void slot_terms(const float (&pf)[EPL], const float (&ps)[EPL],
                                           const float (&qf)[EPL], const float (&qs)[EPL],
                                           const float (&wf)[WE][WD], const float (&ws)[WE][WD],
                                           float av, float (&zf)[EPL], float (&zs)[EPL]) {
  if constexpr (DE > 0) {
    edge_term<EPL, DE>(wf, pf, av, zf);
    edge_term<EPL, DE>(ws, ps, av, zs);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      zf[e] += qf[e];
      zs[e] += qs[e];
    }
  } else {
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      zf[e] = pf[e] + qf[e];
      zs[e] = ps[e] + qs[e];
    }
  }
}

// the gradients of the two pre-activations of one slot
template <int EPL>
__device__ __forceinline__ void slot_grads(const float (&g)[EPL], const float (&zf)[EPL],
                                           const float (&zs)[EPL], float (&gzf)[EPL],
                                           float (&gzs)[EPL]) {
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    const float sg = sigmoid(zf[e]);
    gzf[e] = (g[e] * softplus(zs[e])) * (sg * (1.f - sg));
    gzs[e] = (g[e] * sg) * softplus_grad(zs[e]);
  }
}

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, int DE, bool WIDE>
__global__ void __launch_bounds__(kBlock)
    cg_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const IdxT* __restrict__ edge_id,
                  const float* __restrict__ P, int64_t ld_p, const float* __restrict__ Q,
                  int64_t ld_q, EdgeArgs ed, const float* __restrict__ residual, int64_t ld_r,
                  int mean, int F, int lph, float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = CgSlots<EPL, DE, WIDE>::fwd;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wf[LIN ? EPL : 1][LIN ? DE : 1], ws[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) load_weights<EPL, VEC, DE>(ed, L, F, wf, ws);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float pf[EPL], ps[EPL], acc[EPL];
    load_row<EPL, VEC>(P + s.row * ld_p, L, pf);
    load_row<EPL, VEC>(P + s.row * ld_p + F, L, ps);
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float qf[U][EPL], qs[U][EPL], ef[WIDE ? U : 1][EPL], es[WIDE ? U : 1][EPL], av[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const float* row = Q + static_cast<int64_t>(col[k + u]) * ld_q;
          load_row<EPL, VEC>(row, L, qf[u]);
          load_row<EPL, VEC>(row + F, L, qs[u]);
          if constexpr (LIN) av[u] = edge_lane(ed, slot_edge(edge_id, k + u), lane);
          if constexpr (WIDE) {
            const float* er = ed.edge_attr + slot_edge(edge_id, k + u) * (2 * F);
            load_row<EPL, VEC>(er, L, ef[u]);
            load_row<EPL, VEC>(er + F, L, es[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          float zf[EPL], zs[EPL];
          slot_terms<EPL, DE>(pf, ps, qf[u], qs[u], wf, ws, LIN ? av[u] : 0.f, zf, zs);
          if constexpr (WIDE) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              zf[e] += ef[u][e];
              zs[e] += es[u][e];
            }
          }
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(sigmoid(zf[e]), softplus(zs[e]), acc[e]);
        }
      }
    }
    if (s.chunk_id >= 0) {  // partial sum of one chunk of a long row: the merge has the epilogue
      store_row<EPL, VEC>(part + s.chunk_id * F, L, acc);
    } else {
      const int64_t deg = s.row_end - s.row_start;
      if (mean && deg > 0) {
        const float d = static_cast<float>(deg);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] /= d;
      }
      if (residual) {
        float r[EPL];
        load_row<EPL, VEC>(residual + s.row * ld_r, L, r);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] += r[e];
      }
      store_row<EPL, VEC>(out + s.row * F, L, acc);
    }
  }
}

// ---- backward, by destination ----------------------------------------------------------------
// A wave owns destination i (or a chunk of its slots) with P[i] and g = grad_out[i] in registers.
// part and grad_p hold rows of 2F: [sum gzf | sum gzs].  wpart: one partial of (grad_Wf_e [F De],
// grad_Ws_e [F De]) per workgroup, its waves added in wave order.
template <typename IdxT, int EPL, bool VEC, int DE, bool WIDE>
__global__ void __launch_bounds__(kBlock)
    cg_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                      const IdxT* __restrict__ edge_id, const float* __restrict__ P, int64_t ld_p,
                      const float* __restrict__ Q, int64_t ld_q, EdgeArgs ed,
                      const float* __restrict__ grad_out, int64_t ld_g, int mean, int F, int lph,
                      float* __restrict__ grad_p, int64_t ld_gp, float* __restrict__ grad_edge,
                      float* __restrict__ part, float* __restrict__ wpart) {
  constexpr int U = CgSlots<EPL, DE, WIDE>::dst;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wf[LIN ? EPL : 1][LIN ? DE : 1], ws[LIN ? EPL : 1][LIN ? DE : 1];
  float gwf[LIN ? EPL : 1][LIN ? DE : 1], gws[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) {
    load_weights<EPL, VEC, DE>(ed, L, F, wf, ws);
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
#pragma unroll
      for (int d = 0; d < DE; ++d) gwf[e][d] = gws[e][d] = 0.f;
    }
  }
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float pf[EPL], ps[EPL], g[EPL], gpf[EPL], gps[EPL];
    load_row<EPL, VEC>(P + s.row * ld_p, L, pf);
    load_row<EPL, VEC>(P + s.row * ld_p + F, L, ps);
    load_row<EPL, VEC>(grad_out + s.row * ld_g, L, g);
    if (mean) {  // (a decoded span has slots only if its row has)
      const float d = static_cast<float>(s.row_end > s.row_start ? s.row_end - s.row_start : 1);
#pragma unroll
      for (int e = 0; e < EPL; ++e) g[e] /= d;
    }
#pragma unroll
    for (int e = 0; e < EPL; ++e) gpf[e] = gps[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float qf[U][EPL], qs[U][EPL], ef[WIDE ? U : 1][EPL], es[WIDE ? U : 1][EPL], av[U];
      int64_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const float* row = Q + static_cast<int64_t>(col[k + u]) * ld_q;
          load_row<EPL, VEC>(row, L, qf[u]);
          load_row<EPL, VEC>(row + F, L, qs[u]);
          if constexpr (LIN || WIDE) id[u] = slot_edge(edge_id, k + u);
          if constexpr (LIN) av[u] = edge_lane(ed, id[u], lane);
          if constexpr (WIDE) {
            const float* er = ed.edge_attr + id[u] * (2 * F);
            load_row<EPL, VEC>(er, L, ef[u]);
            load_row<EPL, VEC>(er + F, L, es[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          float zf[EPL], zs[EPL], gzf[EPL], gzs[EPL];
          slot_terms<EPL, DE>(pf, ps, qf[u], qs[u], wf, ws, LIN ? av[u] : 0.f, zf, zs);
          if constexpr (WIDE) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              zf[e] += ef[u][e];
              zs[e] += es[u][e];
            }
          }
          slot_grads<EPL>(g, zf, zs, gzf, gzs);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            gpf[e] += gzf[e];
            gps[e] += gzs[e];
          }
          if constexpr (WIDE) {
            if (grad_edge) {
              float* gr = grad_edge + id[u] * (2 * F);
              store_row<EPL, VEC>(gr, L, gzf);
              store_row<EPL, VEC>(gr + F, L, gzs);
            }
          }
          if constexpr (LIN) {
            // the parameter gradients of both matrices; the edge's own gradient takes both terms
            // in ONE wave sum per feature
            float none[EPL];  // (no bias: never touched)
            edge_grad_take<false, EPL, DE>(gzf, av[u], wf, ed.De, lane, nullptr, id[u], gwf, none);
            edge_grad_take<false, EPL, DE>(gzs, av[u], ws, ed.De, lane, nullptr, id[u], gws, none);
            if (grad_edge) {
              float mine = 0.f;
#pragma unroll
              for (int d = 0; d < DE; ++d) {
                if (d < ed.De) {
                  float p = 0.f;
#pragma unroll
                  for (int e = 0; e < EPL; ++e)
                    p = fmaf(gzs[e], ws[e][d], fmaf(gzf[e], wf[e][d], p));
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
    float* row = s.chunk_id >= 0 ? part + s.chunk_id * 2 * F : grad_p + s.row * ld_gp;
    store_row<EPL, VEC>(row, L, gpf);
    store_row<EPL, VEC>(row + F, L, gps);
  }
  if constexpr (LIN) {
    __shared__ float red[2 * kCgMaxWeight];
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
                red[o] = (wave == 0 ? 0.f : red[o]) + gwf[e][d];
                red[FD + o] = (wave == 0 ? 0.f : red[FD + o]) + gws[e][d];
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
// A wave owns source j (or a chunk of its out-slots) with Qf[j], Qs[j] in registers; slot t has
// destination i = col_t[t] and edge edge_id_t[t].  dst_ptr (mean only): the by-destination
// rowptr, for the slot count of i.  part and grad_q hold rows of 2F: [sum gzf | sum gzs].
template <typename IdxT, int EPL, bool VEC, int DE, bool WIDE>
__global__ void __launch_bounds__(kBlock)
    cg_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                      const IdxT* __restrict__ edge_id_t, const float* __restrict__ P,
                      int64_t ld_p, const float* __restrict__ Q, int64_t ld_q, EdgeArgs ed,
                      const float* __restrict__ grad_out, int64_t ld_g,
                      const IdxT* __restrict__ dst_ptr, int F, int lph,
                      float* __restrict__ grad_q, int64_t ld_gq, float* __restrict__ part) {
  constexpr int U = CgSlots<EPL, DE, WIDE>::src;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float wf[LIN ? EPL : 1][LIN ? DE : 1], ws[LIN ? EPL : 1][LIN ? DE : 1];
  if constexpr (LIN) load_weights<EPL, VEC, DE>(ed, L, F, wf, ws);
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float qf[EPL], qs[EPL], gqf[EPL], gqs[EPL];
    load_row<EPL, VEC>(Q + s.row * ld_q, L, qf);
    load_row<EPL, VEC>(Q + s.row * ld_q + F, L, qs);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gqf[e] = gqs[e] = 0.f;
    for (int64_t t = s.k0; t < s.k1; t += U) {
      float pf[U][EPL], ps[U][EPL], gg[U][EPL], ef[WIDE ? U : 1][EPL], es[WIDE ? U : 1][EPL];
      float av[U], deg[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[t + u]);
          load_row<EPL, VEC>(P + i * ld_p, L, pf[u]);
          load_row<EPL, VEC>(P + i * ld_p + F, L, ps[u]);
          load_row<EPL, VEC>(grad_out + i * ld_g, L, gg[u]);
          deg[u] = dst_ptr ? static_cast<float>(dst_ptr[i + 1] - dst_ptr[i]) : 1.f;
          if constexpr (LIN) av[u] = edge_lane(ed, slot_edge(edge_id_t, t + u), lane);
          if constexpr (WIDE) {
            const float* er = ed.edge_attr + slot_edge(edge_id_t, t + u) * (2 * F);
            load_row<EPL, VEC>(er, L, ef[u]);
            load_row<EPL, VEC>(er + F, L, es[u]);
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (t + u < s.k1) {
          float zf[EPL], zs[EPL], gzf[EPL], gzs[EPL];
          slot_terms<EPL, DE>(pf[u], ps[u], qf, qs, wf, ws, LIN ? av[u] : 0.f, zf, zs);
          if constexpr (WIDE) {
#pragma unroll
            for (int e = 0; e < EPL; ++e) {
              zf[e] += ef[u][e];
              zs[e] += es[u][e];
            }
          }
          if (dst_ptr) {  // (the same division as by destination)
#pragma unroll
            for (int e = 0; e < EPL; ++e) gg[u][e] /= deg[u];
          }
          slot_grads<EPL>(gg[u], zf, zs, gzf, gzs);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            gqf[e] += gzf[e];
            gqs[e] += gzs[e];
          }
        }
      }
    }
    float* row = s.chunk_id >= 0 ? part + s.chunk_id * 2 * F : grad_q + s.row * ld_gq;
    store_row<EPL, VEC>(row, L, gqf);
    store_row<EPL, VEC>(row + F, L, gqs);
  }
}

// hub rows: the chunks' partial rows (W floats each) summed in chunk order, then the forward's
// epilogue (mean: / the row's slot count; residual != NULL: + residual[row]) into dst at ld_dst
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    cg_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                    const IdxT* __restrict__ hub_cptr, int64_t W, const float* __restrict__ part,
                    int mean, const float* __restrict__ residual, int64_t ld_r,
                    float* __restrict__ dst, int64_t ld_dst) {
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const float d = static_cast<float>(rowptr[row + 1] - rowptr[row]);  // (a hub row has slots)
  for (int64_t t = threadIdx.x; t < W; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part[c * W + t];
    if (mean) acc /= d;
    if (residual) acc += residual[row * ld_r + t];
    dst[row * ld_dst + t] = acc;
  }
}

// ---- host side -------------------------------------------------------------------------------
// Every mode walks its items at the stride of a capped grid (gine_device.h caps the linear mode
// only, for its weights): consecutive rows go to different workgroups.  On a graph with skewed
// in-degrees the long rows have neighbouring ids, and one wave per row in row order would hand
// them all to the same few compute units (profiles/cg_conv.md).  Without weights to load the cap
// is the number of workgroups the device holds at once.
constexpr unsigned kCgBlocks = 2048;

unsigned cg_grid(int64_t n_items, bool linear, unsigned linear_cap) {
  return gine_grid(n_items, true, linear ? linear_cap : kCgBlocks);
}

bool cg_envelope(int64_t F, int64_t De) {
  if (F < 1 || F > kMaxWidth || De < 0) return false;
  return De == 0 || (De <= kCgMaxDe && F * De <= kCgMaxWeight);
}

// pygamd_resgated_workspace_bytes(n_chunks, F, De): a chunk's partial row of 2F and, with De > 0,
// the by-destination backward's per-workgroup partials of two [F, De] matrices
size_t cg_ws_bytes(int64_t n_chunks, int64_t F, int64_t De) {
  size_t bytes = 0;
  pygamd_resgated_workspace_bytes(n_chunks, F, De, &bytes);  // (inside resgated's envelope)
  return bytes;
}

// what every entry point checks on its edge arguments; De counts for LINEAR only
int cg_edge(int edge_mode, const float* edge_attr, const float* weight, int64_t De, EdgeArgs* ed) {
  *ed = EdgeArgs{edge_attr, weight, nullptr, static_cast<int>(De)};
  return check_edge(edge_mode, *ed);
}

template <typename IdxT>
int launch_merge(const Items<IdxT>& it, int64_t W, const float* part, int mean,
                 const float* residual, int64_t ld_r, float* dst, int64_t ld_dst, hipStream_t st) {
  if (it.n_hub > 0) {
    hipLaunchKernelGGL((cg_merge_kernel<IdxT>), dim3(static_cast<unsigned>(it.n_hub)), dim3(kWave),
                       0, st, it.rowptr, it.hub_rows, it.hub_cptr, W, part, mean, residual, ld_r,
                       dst, ld_dst);
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

// gine_device.h's shape table, without the instantiations the narrower envelope never reaches;
// `...` also sees WIDE (`wide`, a host bool, picks it where DE = 0)
#define CG_DISPATCH(...)                                     \
  GINE_DISPATCH({                                            \
    if constexpr (EPL * DE > kCgMaxRegs) {                   \
      return PYGAMD_ERR_UNSUPPORTED;                         \
    } else if constexpr (DE == 0) {                          \
      if (wide) {                                            \
        constexpr bool WIDE = true;                          \
        __VA_ARGS__                                          \
      } else {                                               \
        constexpr bool WIDE = false;                         \
        __VA_ARGS__                                          \
      }                                                      \
    } else {                                                 \
      constexpr bool WIDE = false;                           \
      __VA_ARGS__                                            \
    }                                                        \
  })

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_cg_supported(int64_t F, int64_t De) { return cg_envelope(F, De) ? 1 : 0; }

int pygamd_cg_forward(const pygamd_csr* g, const void* edge_id, const float* p, int64_t ld_p,
                      const float* q, int64_t ld_q, int edge_mode, const float* edge_attr,
                      const float* weight, const float* residual, int64_t ld_r, int scale,
                      int64_t n_src, int64_t F, int64_t De, float* out, void* workspace,
                      size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, De, cg_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (ld_p < 2 * F || ld_q < 2 * F || (residual && ld_r < F) || (scale != 0 && scale != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !p || !q || !out) return PYGAMD_ERR_INVALID_ARG;
  EdgeArgs ed;
  const int rce = cg_edge(edge_mode, edge_attr, weight, De, &ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < cg_ws_bytes(n_chunks, F, 0)))
    return PYGAMD_ERR_WORKSPACE;
  const bool wide = edge_mode == PYGAMD_GEN_EDGE_WIDE;
  const bool al = aligned16(p) && ld_p % 4 == 0 && aligned16(q) && ld_q % 4 == 0 &&
                  aligned16(out) && (!residual || (aligned16(residual) && ld_r % 4 == 0)) &&
                  (!wide || aligned16(edge_attr)) && (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(cg_grid(n_rows + n_chunks, De > 0, kGineFwdBlocks)), block(kBlock);
    CG_DISPATCH({
      hipLaunchKernelGGL((cg_fwd_kernel<IdxT, EPL, VEC, DE, WIDE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), p, ld_p, q, ld_q,
                         ed, residual, ld_r, scale, static_cast<int>(F), sh.lph, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' partial sums in chunk order, then the epilogue, once)
    return launch_merge<IdxT>(it, F, part, scale, residual, ld_r, out, F, st);
  });
}

int pygamd_cg_backward_dst(const pygamd_csr* g, const void* edge_id, const float* p, int64_t ld_p,
                           const float* q, int64_t ld_q, int edge_mode, const float* edge_attr,
                           const float* weight, const float* grad_out, int64_t ld_g, int scale,
                           int64_t n_src, int64_t F, int64_t De, float* grad_p, int64_t ld_gp,
                           float* grad_edge, float* grad_weight, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_src, F, De, cg_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (ld_p < 2 * F || ld_q < 2 * F || ld_g < F || ld_gp < 2 * F || (scale != 0 && scale != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !p || !q || !grad_out || !grad_p ||
      (De > 0) != (grad_weight != nullptr) || (edge_mode == PYGAMD_GEN_EDGE_NONE && grad_edge))
    return PYGAMD_ERR_INVALID_ARG;
  EdgeArgs ed;
  const int rce = cg_edge(edge_mode, edge_attr, weight, De, &ed);
  if (rce != PYGAMD_OK) return rce;
  if ((n_chunks > 0 || De > 0) &&
      (!workspace || workspace_bytes < cg_ws_bytes(n_chunks, F, De)))
    return PYGAMD_ERR_WORKSPACE;
  const bool wide = edge_mode == PYGAMD_GEN_EDGE_WIDE;
  const bool al = aligned16(p) && ld_p % 4 == 0 && aligned16(q) && ld_q % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_p) && ld_gp % 4 == 0 &&
                  (!wide || (aligned16(edge_attr) && aligned16(grad_edge))) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* wpart = part + n_chunks * 2 * F;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const unsigned n_blocks = cg_grid(n_rows + n_chunks, De > 0, kGineBwdBlocks);
    const dim3 grid(n_blocks), block(kBlock);
    CG_DISPATCH({
      hipLaunchKernelGGL((cg_bwd_dst_kernel<IdxT, EPL, VEC, DE, WIDE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), p, ld_p, q, ld_q,
                         ed, grad_out, ld_g, scale, static_cast<int>(F), sh.lph, grad_p, ld_gp,
                         grad_edge, part, wpart);
    });
    PYGAMD_LAUNCH_CHECK();
    const int rcm = launch_merge<IdxT>(it, 2 * F, part, 0, nullptr, 0, grad_p, ld_gp, st);
    if (rcm != PYGAMD_OK || De <= 0) return rcm;
    // the workgroups' partials of both matrices (2 F De floats) in workgroup order
    return launch_param_reduce(wpart, n_blocks, static_cast<int>(2 * F * De), 0, grad_weight,
                               nullptr, st);
  });
}

int pygamd_cg_backward_src(const pygamd_csr* g, const void* edge_id_t, const float* p,
                           int64_t ld_p, const float* q, int64_t ld_q, int edge_mode,
                           const float* edge_attr, const float* weight, const float* grad_out,
                           int64_t ld_g, int scale, const void* dst_rowptr, int64_t n_dst,
                           int64_t F, int64_t De, float* grad_q, int64_t ld_gq, void* workspace,
                           size_t workspace_bytes, void* stream) {
  const int rc = gine_check(g, n_dst, F, De, cg_envelope);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (ld_p < 2 * F || ld_q < 2 * F || ld_g < F || ld_gq < 2 * F || (scale != 0 && scale != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !p || !q || !grad_out || !grad_q ||
      (scale == 1) != (dst_rowptr != nullptr))
    return PYGAMD_ERR_INVALID_ARG;
  EdgeArgs ed;
  const int rce = cg_edge(edge_mode, edge_attr, weight, De, &ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < cg_ws_bytes(n_chunks, F, 0)))
    return PYGAMD_ERR_WORKSPACE;
  const bool wide = edge_mode == PYGAMD_GEN_EDGE_WIDE;
  const bool al = aligned16(p) && ld_p % 4 == 0 && aligned16(q) && ld_q % 4 == 0 &&
                  aligned16(grad_out) && ld_g % 4 == 0 && aligned16(grad_q) && ld_gq % 4 == 0 &&
                  (!wide || aligned16(edge_attr)) && (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(cg_grid(n_src + n_chunks, De > 0, kGineBwdBlocks)), block(kBlock);
    CG_DISPATCH({
      hipLaunchKernelGGL((cg_bwd_src_kernel<IdxT, EPL, VEC, DE, WIDE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t), p, ld_p, q,
                         ld_q, ed, grad_out, ld_g, static_cast<const IdxT*>(dst_rowptr),
                         static_cast<int>(F), sh.lph, grad_q, ld_gq, part);
    });
    PYGAMD_LAUNCH_CHECK();
    // (hub rows: the chunks' packed partial rows of 2F in chunk order)
    return launch_merge<IdxT>(it, 2 * F, part, 0, nullptr, 0, grad_q, ld_gq, st);
  });
}

}  // extern "C"

// gen.hip — the propagate step of GENConv (nn/conv/gen_conv.py:203-239 of the reference with the
// SoftmaxAggregation of nn/aggr/basic.py:142-215) as a pair of row-gather kernels on a sorted
// handle.  For destination i, slot k with source j = col[k] and column c:
//     e_k      = 0 | edge_attr[k, :] (wide) | W a_k + b, a_k = edge_attr[k, :De] (linear)
//     m_k      = max(x_src[j] + e_k, 0) + eps_msg
//     out[i,c] = sum_k alpha_kc m_kc,   alpha_kc = softmax over the slots of i of t_c m_kc
// The softmax runs PER COLUMN: a lane keeps a running (M, L, acc[, S2]) for each of its columns and
// takes a slot in with one expf per element (of the two factors of the online update one is always
// exp(0)).  The message is rebuilt per slot in registers as in gine.hip; nothing of size E x F
// exists anywhere.  The forward leaves M and 1 / (L + 1e-16) per (destination, column) — and, for
// a learned t, S2 = sum_k alpha m^2 — from which the backward rebuilds alpha per out-slot.
//
// Lane layout, work items, hub chunks and in-order merges: rowwalk_device.h.  Edge term, envelope,
// capped grid and dispatch: gine_device.h.  The softmax weight of a score: attn_device.h.  No float
// atomics anywhere and every grid depends on the problem's sizes only: every result is bitwise
// reproducible.
#include <math.h>

#include "attn_device.h"  // softmax_weight
#include "common.h"
#include "gine_device.h"

namespace pygamd {
namespace {

using namespace rowwalk;
using attn::softmax_weight;
using namespace gine;

template <int EPL, int DE>
struct GenSlots {  // slots in flight per wave
  static constexpr int fwd = (EPL >= 8 || DE > 0) ? 2 : 4;
  static constexpr int bwd = (EPL * DE >= 64) ? 1 : 2;
};

// the lane's entries of t: a row of F values, or one value for every column
template <int EPL, bool VEC>
__device__ __forceinline__ void load_t(const float* __restrict__ t, int t_len, const Lay& L,
                                       float (&tt)[EPL]) {
  if (t_len == 1) {
    const float v = t[0];
#pragma unroll
    for (int e = 0; e < EPL; ++e) tt[e] = v;
  } else {
    load_row<EPL, VEC>(t, L, tt);
  }
}

// max(v, 0) that keeps a NaN (fmaxf would drop it; torch's relu does not)
__device__ __forceinline__ float relu_nan(float v) { return v < 0.f ? 0.f : v; }

// The logit t m, rounded once and never contracted into its consumers (a plain product, or
// __fmul_rn, fuses with the subtraction that follows into one fma of the UNROUNDED product): the
// backward rebuilds the forward's logits bit for bit, so a slot that set the maximum has weight
// exp(0) there too.  An fma with +0 cannot be simplified to a product (-0 would come out as +0).
__device__ __forceinline__ float logit(float t, float m) { return fmaf(t, m, 0.f); }

// A running (M, L, acc, s2) of one column takes in the message m with logit p.  Of the old side's
// factor exp(M - mn) and the new one's exp(p - mn) one is exp(0) = 1: a single expf of minus the
// distance.  A side at -inf has weight exactly 0 (softmax_weight's guard: nothing seen yet); a
// logit of +inf or NaN poisons the column as the reference's exp(inf - inf) does.
__device__ __forceinline__ void online_take(float m, float p, float& M, float& L, float& acc,
                                            float& s2) {
  const bool up = p > M;
  const float e = (up && M == -INFINITY) ? 0.f : expf(up ? M - p : p - M);
  const float self = p == INFINITY ? NAN : 1.f;
  const float wo = up ? e : 1.f, wn = up ? self : e;
  const float wm = wn * m;
  L = fmaf(L, wo, wn);
  acc = fmaf(acc, wo, wm);
  s2 = fmaf(s2, wo, wm * m);
  M = up ? p : M;
}

// ---- forward ---------------------------------------------------------------------------------
// part: per chunk four rows of F (M, L, acc, S2).  saved: the planes M, 1 / (L + 1e-16) and, if
// want_s2, S2 of [n_rows, F] each.
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    gen_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const IdxT* __restrict__ edge_id,
                   const float* __restrict__ x_src, int64_t ld, EdgeArgs ed,
                   const float* __restrict__ t, int t_len, float eps_msg, int F, int lph,
                   float* __restrict__ out, float* __restrict__ saved, int want_s2,
                   float* __restrict__ part) {
  constexpr int U = GenSlots<EPL, DE>::fwd;
  constexpr bool LIN = DE > 0;
  const Lay L = make_lay(1, F, lph);
  float w[LIN ? EPL : 1][LIN ? DE : 1], b[EPL];
  if constexpr (LIN) load_weight<EPL, VEC, DE>(ed.weight, ed.bias, L, ed.De, w, b);
  float tt[EPL];
  load_t<EPL, VEC>(t, t_len, L, tt);
  const bool has_edge = ed.edge_attr != nullptr;  // (wave-uniform)
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  const int64_t plane = it.n_rows * static_cast<int64_t>(F);
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float M[EPL], Ls[EPL], acc[EPL], s2[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      M[e] = -INFINITY;
      Ls[e] = acc[e] = s2[e] = 0.f;
    }
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
            if (has_edge) {
              load_row<EPL, VEC>(ed.edge_attr + id * F, L, ee[u]);
            } else {
#pragma unroll
              for (int e = 0; e < EPL; ++e) ee[u][e] = 0.f;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          if constexpr (LIN) edge_term<EPL, DE>(w, b, av[u], ee[u]);
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float m = relu_nan(xx[u][e] + ee[u][e]) + eps_msg;
            online_take(m, logit(tt[e], m), M[e], Ls[e], acc[e], s2[e]);
          }
        }
      }
    }
    if (s.chunk_id >= 0) {  // the running state of one chunk of a long row
      float* p = part + s.chunk_id * 4 * F;
      store_row<EPL, VEC>(p, L, M);
      store_row<EPL, VEC>(p + F, L, Ls);
      store_row<EPL, VEC>(p + 2 * F, L, acc);
      store_row<EPL, VEC>(p + 3 * F, L, s2);
      continue;
    }
    const bool has = s.k1 > s.k0;
    float inv[EPL];
#pragma unroll
    for (int e = 0; e < EPL; ++e) {
      inv[e] = has ? 1.f / (Ls[e] + 1e-16f) : 0.f;
      acc[e] *= inv[e];
      s2[e] *= inv[e];
      if (!has) M[e] = 0.f;
    }
    store_row<EPL, VEC>(out + s.row * F, L, acc);
    store_row<EPL, VEC>(saved + s.row * F, L, M);
    store_row<EPL, VEC>(saved + plane + s.row * F, L, inv);
    if (want_s2) store_row<EPL, VEC>(saved + 2 * plane + s.row * F, L, s2);
  }
}

// hub rows, forward: the chunks' (M, L, acc, S2) of a column combined in chunk order
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    gen_fwd_merge_kernel(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_cptr,
                         int64_t F, int64_t n_rows, const float* __restrict__ part,
                         float* __restrict__ out, float* __restrict__ saved, int want_s2) {
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t plane = n_rows * F;
  for (int64_t c = threadIdx.x; c < F; c += kWave) {
    float M = -INFINITY, L = 0.f, acc = 0.f, s2 = 0.f;
    for (int64_t q = c0; q < c1; ++q) {
      const float* p = part + q * 4 * F + c;
      const float Mq = p[0];
      const float mn = fmaxf(M, Mq);
      const float wo = softmax_weight(M, mn), wq = softmax_weight(Mq, mn);
      L = L * wo + p[F] * wq;
      acc = acc * wo + p[2 * F] * wq;
      s2 = s2 * wo + p[3 * F] * wq;
      M = mn;
    }
    const float inv = 1.f / (L + 1e-16f);  // (a hub row has slots)
    out[row * F + c] = acc * inv;
    saved[row * F + c] = M;
    saved[plane + row * F + c] = inv;
    if (want_s2) saved[2 * plane + row * F + c] = s2 * inv;
  }
}

// ---- backward, by source ------------------------------------------------------------------------
// A wave owns source row j (or a chunk of its out-slots) and keeps x_src[j] in registers; slot s
// has destination i = col_t[s] and edge k = edge_id_t[s].  coef [n_dst, planes, F] is a packed
// row per destination: M, G = grad_out[i] / (L + 1e-16), out[i] (planes = 3) or M, G (planes = 2,
// semi_grad: the weights are constants), so that
//     grad_m = exp(t m - M) G (1 + t (m - out))      semi_grad: exp(t m - M) G
// with m - out formed first (no cancellation against t out for a large t).  Through the ReLU:
// gm = (x_src[j] + e_k > 0) grad_m;  grad_x_src[j] = sum_s gm;  grad_edge_attr, grad_W and grad_b
// from gm exactly as gine.hip's backward forms them from its masked grad_out.
template <typename IdxT, int EPL, bool VEC, int DE>
__global__ void __launch_bounds__(kBlock)
    gen_bwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                   const IdxT* __restrict__ edge_id_t, const float* __restrict__ x_src, int64_t ld,
                   EdgeArgs ed, const float* __restrict__ t, int t_len, float eps_msg,
                   const float* __restrict__ coef, int planes, int F, int lph,
                   float* __restrict__ grad_x, float* __restrict__ grad_edge,
                   float* __restrict__ part, float* __restrict__ wpart) {
  constexpr int U = GenSlots<EPL, DE>::bwd;
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
  float tt[EPL];
  load_t<EPL, VEC>(t, t_len, L, tt);
  const bool has_edge = ed.edge_attr != nullptr;  // (wave-uniform)
  const bool full = planes == 3;                  // (wave-uniform)
  const int lane = lane_id();
  const Walk wk = item_walk(it);
  const int64_t ldc = static_cast<int64_t>(planes) * F;
  for (int64_t item = wk.first; item < wk.n; item += wk.stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float x[EPL], gx[EPL];
    load_row<EPL, VEC>(x_src + s.row * ld, L, x);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gx[e] = 0.f;
    for (int64_t q = s.k0; q < s.k1; q += U) {
      float cm[U][EPL], cp[U][EPL], cq[U][EPL], ee[U][EPL], av[U];
      int64_t id[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (q + u < s.k1) {
          const int64_t i = static_cast<int64_t>(col_t[q + u]);
          id[u] = slot_edge(edge_id_t, q + u);
          const float* c = coef + i * ldc;
          load_row<EPL, VEC>(c, L, cm[u]);
          load_row<EPL, VEC>(c + F, L, cp[u]);
          if (full) {
            load_row<EPL, VEC>(c + 2 * F, L, cq[u]);
          } else {
#pragma unroll
            for (int e = 0; e < EPL; ++e) cq[u][e] = 0.f;
          }
          if constexpr (LIN) {
            av[u] = edge_lane(ed, id[u], lane);
          } else {
            if (has_edge) {
              load_row<EPL, VEC>(ed.edge_attr + id[u] * F, L, ee[u]);
            } else {
#pragma unroll
              for (int e = 0; e < EPL; ++e) ee[u][e] = 0.f;
            }
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (q + u < s.k1) {
          if constexpr (LIN) edge_term<EPL, DE>(w, b, av[u], ee[u]);
          float mg[EPL];
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float v = x[e] + ee[u][e];
            const float m = relu_nan(v) + eps_msg;
            const float a = expf(logit(tt[e], m) - cm[u][e]) * cp[u][e];
            mg[e] = v > 0.f ? (full ? a * fmaf(tt[e], m - cq[u][e], 1.f) : a) : 0.f;
            gx[e] += mg[e];
          }
          if constexpr (LIN) {
            // (gine_device.h's edge_grad_take, written out: as a call it cost this kernel 1 %)
#pragma unroll
            for (int d = 0; d < DE; ++d) {
              const float a = bcast_uniform(av[u], d);
#pragma unroll
              for (int e = 0; e < EPL; ++e) gw[e][d] = fmaf(mg[e], a, gw[e][d]);
            }
#pragma unroll
            for (int e = 0; e < EPL; ++e) gb[e] += mg[e];
            if (grad_edge) {  // (wave-uniform)
              float mine = 0.f;
#pragma unroll
              for (int d = 0; d < DE; ++d) {
                if (d < ed.De) {
                  float p = 0.f;
#pragma unroll
                  for (int e = 0; e < EPL; ++e) p = fmaf(mg[e], w[e][d], p);
                  p = group_sum(p, kWave);
                  if (lane == d) mine = p;
                }
              }
              if (lane < ed.De) grad_edge[id[u] * ed.De + lane] = mine;
            }
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
    for (int i = threadIdx.x; i < FD + F; i += kBlock) dst[i] = red[i];
  }
}

// ---- host side -------------------------------------------------------------------------------
size_t gen_ws_bytes(int64_t n_chunks, int64_t F, int64_t De) {
  // four rows per chunk (the forward's running state; the backward uses the first n_chunks rows
  // for its partial sums); in linear mode the backward's partials of (grad_W, grad_b) follow
  return sizeof(float) * static_cast<size_t>(n_chunks * 4 * F + wpart_floats(F, De, true));
}

int gen_check(const pygamd_csr* g, int64_t n_other, int64_t F, int64_t De, int edge_mode,
              int64_t t_len) {
  if (edge_mode < PYGAMD_GEN_EDGE_NONE || edge_mode > PYGAMD_GEN_EDGE_LINEAR)
    return PYGAMD_ERR_INVALID_ARG;
  if ((edge_mode == PYGAMD_GEN_EDGE_LINEAR) != (De > 0)) return PYGAMD_ERR_INVALID_ARG;
  const int rc = gine_check(g, n_other, F, De);
  if (rc != PYGAMD_OK) return rc;
  return (t_len == 1 || t_len == F) ? PYGAMD_OK : PYGAMD_ERR_INVALID_ARG;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_gen_supported(int64_t F, int64_t De) { return gine_envelope(F, De) ? 1 : 0; }

int pygamd_gen_workspace_bytes(int64_t n_chunks, int64_t F, int64_t De, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F < 1 || De < 0) return PYGAMD_ERR_INVALID_ARG;
  if (!gine_envelope(F, De)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = gen_ws_bytes(n_chunks, F, De);
  return PYGAMD_OK;
}

int pygamd_gen_forward(const pygamd_csr* g, const void* edge_id, const float* x_src,
                       int64_t ld_src, int edge_mode, const float* edge_attr, const float* weight,
                       const float* bias, const float* t, int64_t t_len, float eps_msg,
                       int64_t n_src, int64_t F, int64_t De, int want_s2, float* out, float* saved,
                       void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gen_check(g, n_src, F, De, edge_mode, t_len);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld_src < F) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !x_src || !t || !out || !saved) return PYGAMD_ERR_INVALID_ARG;
  const EdgeArgs ed{edge_attr, weight, bias, static_cast<int>(De)};
  const int rce = check_edge(edge_mode, ed);
  if (rce != PYGAMD_OK) return rce;
  if (n_chunks > 0 && (!workspace || workspace_bytes < sizeof(float) * n_chunks * 4 * F))
    return PYGAMD_ERR_WORKSPACE;
  const bool al = aligned16(x_src) && ld_src % 4 == 0 && aligned16(out) && aligned16(saved) &&
                  (t_len == 1 || aligned16(t)) &&
                  (edge_mode != PYGAMD_GEN_EDGE_WIDE || aligned16(edge_attr)) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(gine_grid(n_rows + n_chunks, De > 0, kGineFwdBlocks)), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((gen_fwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id), x_src, ld_src,
                         ed, t, static_cast<int>(t_len), eps_msg, static_cast<int>(F), sh.lph,
                         out, saved, want_s2, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((gen_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, F, n_rows, part, out, saved,
                         want_s2);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_gen_backward(const pygamd_csr* g, const void* edge_id_t, const float* x_src,
                        int64_t ld_src, int edge_mode, const float* edge_attr,
                        const float* weight, const float* bias, const float* t, int64_t t_len,
                        float eps_msg, int semi_grad, const float* coef, int64_t n_dst, int64_t F,
                        int64_t De, int want_grad_edge_attr, float* grad_x_src,
                        float* grad_edge_attr, float* grad_weight, float* grad_bias,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = gen_check(g, n_dst, F, De, edge_mode, t_len);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (ld_src < F) return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !x_src || !t || !coef || !grad_x_src)
    return PYGAMD_ERR_INVALID_ARG;
  const EdgeArgs ed{edge_attr, weight, bias, static_cast<int>(De)};
  const int rce = check_edge(edge_mode, ed);
  if (rce != PYGAMD_OK) return rce;
  const bool want_edge = want_grad_edge_attr != 0;
  if ((want_edge && edge_mode == PYGAMD_GEN_EDGE_NONE) || want_edge != (grad_edge_attr != nullptr))
    return PYGAMD_ERR_INVALID_ARG;
  if ((De > 0) != (grad_weight != nullptr) || (grad_bias && !bias)) return PYGAMD_ERR_INVALID_ARG;
  if ((n_chunks > 0 || De > 0) &&
      (!workspace || workspace_bytes < gen_ws_bytes(n_chunks, F, De)))
    return PYGAMD_ERR_WORKSPACE;
  const int planes = semi_grad ? 2 : 3;
  const bool al = aligned16(x_src) && ld_src % 4 == 0 && aligned16(coef) &&
                  aligned16(grad_x_src) && (t_len == 1 || aligned16(t)) &&
                  (edge_mode != PYGAMD_GEN_EDGE_WIDE ||
                   (aligned16(edge_attr) && aligned16(grad_edge_attr))) &&
                  (n_chunks == 0 || aligned16(workspace));
  GineShape sh;
  if (!gine_shape(F, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* wpart = part + n_chunks * 4 * F;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const unsigned n_blocks = gine_grid(n_src + n_chunks, De > 0, kGineBwdBlocks);
    const dim3 grid(n_blocks), block(kBlock);
    GINE_DISPATCH({
      hipLaunchKernelGGL((gen_bwd_kernel<IdxT, EPL, VEC, DE>), grid, block, 0, st, it,
                         typed_col<IdxT>(*g), static_cast<const IdxT*>(edge_id_t), x_src, ld_src,
                         ed, t, static_cast<int>(t_len), eps_msg, coef, planes,
                         static_cast<int>(F), sh.lph, grad_x_src, grad_edge_attr, part, wpart);
    });
    PYGAMD_LAUNCH_CHECK();
    return launch_backward_tail<IdxT>(it, F, De, true, n_blocks, part, grad_x_src, wpart,
                                      grad_weight, grad_bias, st);
  });
}

}  // extern "C"

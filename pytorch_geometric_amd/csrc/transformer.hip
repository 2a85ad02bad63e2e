// transformer.hip — dot-product attention of TransformerConv (nn/conv/transformer_conv.py:263-283
// of the reference) as row-gather kernels on a sorted handle.  For destination i and the source j
// of slot k:
//     s[k,h]     = scale * sum_c q[i,h,c] * key[j,h,c]
//     alpha[k,h] = softmax of s over the row (maximum subtracted, 1e-16 on the denominator)
//     out[i,h,:] = sum_k alpha[k,h] * value[j,h,:]
// ONE pass per destination keeps q[i] in registers, gathers every key[j] and value[j] once, runs an
// online softmax per head and (AGG) accumulates the weighted value row.  Nothing of size E x H*C is
// ever written.  key and value are two pointers with one row stride `ld` (floats): the two halves
// of one [N_src, 2*H*C] projection are read in place, a slot's gather being one contiguous span.
//
// Lane layout, work items, long rows and their in-order sum merge: rowwalk_device.h.  Online
// softmax, its merge and the edge registers: attn_device.h (shared with gatv2.hip).  No float
// atomics anywhere: every result is bitwise reproducible.
#include <math.h>

#include "attn_device.h"
#include "common.h"

namespace pygamd {
namespace {

using namespace rowwalk;  // layout, work items and the sum merge: rowwalk_device.h
using namespace attn;     // online softmax and its merge: attn_device.h

// slots in flight per wave: every slot gathers TWO rows (key and value, or query and grad_out), so
// half of what gatv2's one-row forward keeps
template <int EPL>
struct SlotsInFlight {
  static constexpr int n = EPL >= 8 ? 2 : 4;
};

// ---- edge features ------------------------------------------------------------------------------
// The edge term W_e a_k of key and value is linear, so it never exists per edge at width H*C:
//     s[k,h]     = scale * <q, key_j> + <b[i,h,:], a_k>        b = scale * W_e^T q      [n_dst, H, De]
//     out[i,h,:] = sum_k alpha value_j + W_e z[i,h,:]          z = sum_k alpha[k,h] a_k [n_dst, H, De]
// The kernels read the raw a_k [E, De] in SLOT order and b, and produce z (forward) and the
// gradients of b and a (backward); the two small per-node products with W_e are the caller's.
struct EdgeFwd {
  const float* ea;  // [E, De], slot order
  const float* b;   // [>= n_rows, H * De]
  float* z;         // [n_rows, H * De]; not written in score mode
  int De;
};

struct EdgeBwd {
  const float* ea;
  const float* b;
  const float* gz;  // grad z and z [n_rows, H * De]; not read in score mode
  const float* z;
  float* gb;        // [>= n_rows, H * De]
  float* ga;        // [E, De] in slot order, or NULL: not wanted (wave-uniform)
  int De;
};

// ---- forward ---------------------------------------------------------------------------------
// EDGE: the lane layout's edge registers (attn_device.h) add <b, a_k> to the lane's partial dot
// product BEFORE the group sum, and z is rescaled and accumulated exactly like acc.
template <typename IdxT, int EPL, bool VEC, bool AGG, bool EDGE>
__device__ __forceinline__ void
    transformer_fwd_body(const Items<IdxT>& it, const IdxT* __restrict__ col,
                         const float* __restrict__ query, const float* __restrict__ key,
                         const float* __restrict__ value, int64_t ld, int H, int C, int lph,
                         float scale, float* __restrict__ alpha, float* __restrict__ out,
                         float* __restrict__ part, const EdgeFwd& ed) {
  constexpr int U = SlotsInFlight<EPL>::n;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float q[EPL], acc[EPL];
  load_row<EPL, VEC>(query + s.row * W, L, q);
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float m = -INFINITY, l = 0.f;
  float bb[kEdgeRegs], zz[kEdgeRegs];
  if constexpr (EDGE) {
    load_edge(ed.b + (s.row * H + L.h) * ed.De, L, ed.De, bb);
#pragma unroll
    for (int r = 0; r < kEdgeRegs; ++r) zz[r] = 0.f;
  }
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float kk[U][EPL], vv[AGG ? U : 1][EPL], aa[EDGE ? U : 1][kEdgeRegs];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        load_row<EPL, VEC>(key + j * ld, L, kk[u]);
        if constexpr (AGG) load_row<EPL, VEC>(value + j * ld, L, vv[u]);
        if constexpr (EDGE) load_edge(ed.ea + (k + u) * ed.De, L, ed.De, aa[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) p = fmaf(q[e], kk[u][e], p);
        if constexpr (EDGE) {
          float pb = 0.f;
#pragma unroll
          for (int r = 0; r < kEdgeRegs; ++r) pb = fmaf(bb[r], aa[u][r], pb);
          p = group_sum(fmaf(p, scale, pb), lph);
        } else {
          p = group_sum(p, lph) * scale;
        }
        // the raw score; the lane that writes it is the lane that rescales it below
        if (L.head_ok && L.sub == static_cast<int>((k + u - s.row_start) & (lph - 1)))
          alpha[(k + u) * H + L.h] = p;
        const float mn = fmaxf(m, p);
        const float sc = softmax_weight(m, mn), pe = softmax_weight(p, mn);
        l = fmaf(l, sc, pe);
        if constexpr (AGG) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(acc[e], sc, pe * vv[u][e]);
          if constexpr (EDGE) {
#pragma unroll
            for (int r = 0; r < kEdgeRegs; ++r) zz[r] = fmaf(zz[r], sc, pe * aa[u][r]);
          }
        }
        m = mn;
      }
    }
  }
  if (s.chunk_id >= 0) {  // partial (acc, [z,] m, l) of one chunk of a long row
    const int64_t Z = EDGE ? static_cast<int64_t>(H) * ed.De : 0;
    float* p = part + s.chunk_id * (W + Z + 2 * H);
    if constexpr (AGG) store_row<EPL, VEC>(p, L, acc);
    if constexpr (AGG && EDGE) store_edge(p + W + L.h * ed.De, L, ed.De, zz);
    if (L.head_ok && L.sub == 0) {
      p[W + Z + L.h] = m;
      p[W + Z + H + L.h] = l;
    }
    return;
  }
  const float inv = softmax_inv(m, l, s.k1 > s.k0);
  if constexpr (AGG) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] *= inv;
    store_row<EPL, VEC>(out + s.row * W, L, acc);
    if constexpr (EDGE) {
#pragma unroll
      for (int r = 0; r < kEdgeRegs; ++r) zz[r] *= inv;
      store_edge(ed.z + (s.row * H + L.h) * ed.De, L, ed.De, zz);
    }
  }
  if (L.head_ok) {
    for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
      alpha[k * H + L.h] = expf(alpha[k * H + L.h] - m) * inv;
  }
}

template <typename IdxT, int EPL, bool VEC, bool AGG>
__global__ void __launch_bounds__(kBlock)
    transformer_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                           const float* __restrict__ query, const float* __restrict__ key,
                           const float* __restrict__ value, int64_t ld, int H, int C, int lph,
                           float scale, float* __restrict__ alpha, float* __restrict__ out,
                           float* __restrict__ part) {
  transformer_fwd_body<IdxT, EPL, VEC, AGG, false>(it, col, query, key, value, ld, H, C, lph,
                                                   scale, alpha, out, part, EdgeFwd{});
}

template <typename IdxT, int EPL, bool VEC, bool AGG>
__global__ void __launch_bounds__(kBlock)
    transformer_edge_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                                const float* __restrict__ query, const float* __restrict__ key,
                                const float* __restrict__ value, int64_t ld, int H, int C, int lph,
                                float scale, float* __restrict__ alpha, float* __restrict__ out,
                                float* __restrict__ part, EdgeFwd ed) {
  transformer_fwd_body<IdxT, EPL, VEC, AGG, true>(it, col, query, key, value, ld, H, C, lph,
                                                  scale, alpha, out, part, ed);
}

// Hub rows, forward: workgroup (hub row, block of 64 columns) merges the chunks' partials into the
// final (m, l) per head and its columns of the output row; the first column block also leaves
// (m, 1 / (l + 1e-16)) in `stats`.  The row's alpha (tens of thousands of slots on a power-law
// graph) is rescaled by the launch below, one wave per chunk, not by this workgroup.
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    transformer_fwd_merge_kernel(const IdxT* __restrict__ rowptr,
                                 const IdxT* __restrict__ hub_rows,
                                 const IdxT* __restrict__ hub_cptr, int H, int C,
                                 const float* __restrict__ part, float* __restrict__ alpha,
                                 float* __restrict__ out, float* __restrict__ stats) {
  __shared__ float sm[kAttnMaxHeads], sinv[kAttnMaxHeads];
  const int64_t W = static_cast<int64_t>(H) * C;
  const int64_t col0 = static_cast<int64_t>(blockIdx.y) * kWave;
  merge_softmax_row(rowptr, hub_rows, hub_cptr, static_cast<int64_t>(blockIdx.x), H, C, part,
                    alpha, out, sm, sinv, col0, col0 + kWave < W ? col0 + kWave : W, false,
                    blockIdx.y == 0 ? stats : nullptr);
}

// alpha = exp(s - m) / (l + 1e-16) over the slots of one chunk of a hub row (the expression of the
// plain rows and of merge_softmax_row)
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    transformer_alpha_rescale_kernel(Items<IdxT> it, int H, const float* __restrict__ stats,
                                     float* __restrict__ alpha) {
  const int64_t chunk = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  Span s;
  if (chunk >= it.n_chunks || !decode(it, chunk, s)) return;
  const float* st = stats + s.hub * 2 * H;
  const int64_t t1 = s.k1 * H;
  for (int64_t t = s.k0 * H + lane_id(); t < t1; t += kWave) {
    const int h = static_cast<int>(t % H);
    alpha[t] = expf(alpha[t] - st[h]) * st[H + h];
  }
}

// partial gradient rows of a hub row summed in chunk order: n_out (1 or 2) outputs of W floats,
// side by side in a chunk's partial, each to its own pointer at row stride ld
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    transformer_sum_merge_kernel(const IdxT* __restrict__ hub_rows,
                                 const IdxT* __restrict__ hub_cptr, int64_t W, int n_out,
                                 const float* __restrict__ part, float* __restrict__ dst0,
                                 float* __restrict__ dst1, int64_t ld) {
  const int64_t hr = blockIdx.x;
  merge_sum_row(hub_rows, hub_cptr, hr, W, part, n_out * W, dst0, ld);
  if (n_out > 1) merge_sum_row(hub_rows, hub_cptr, hr, W, part + W, n_out * W, dst1, ld);
}

// The forward merge of the edge variant: the chunks' partials (acc [W], z [H*De], m [H], l [H])
// combined in chunk order with the rescale of merge_softmax_row; workgroup (hub row, block of 64 of
// the W + H*De columns of out | z).  have_out false (score mode): the statistics only.
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    transformer_edge_fwd_merge_kernel(const IdxT* __restrict__ hub_rows,
                                      const IdxT* __restrict__ hub_cptr, int H, int C, int De,
                                      const float* __restrict__ part, float* __restrict__ out,
                                      float* __restrict__ z, float* __restrict__ stats) {
  __shared__ float sm[kAttnMaxHeads], sinv[kAttnMaxHeads];
  const int64_t hr = blockIdx.x;
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t W = static_cast<int64_t>(H) * C, Z = static_cast<int64_t>(H) * De;
  const int64_t S = W + Z + 2 * H;
  const int lane = threadIdx.x;
  if (lane < H) {
    float m = -INFINITY, l = 0.f;
    for (int64_t c = c0; c < c1; ++c) {
      const float mc = part[c * S + W + Z + lane], lc = part[c * S + W + Z + H + lane];
      const float mn = fmaxf(m, mc);
      l = l * softmax_weight(m, mn) + lc * softmax_weight(mc, mn);
      m = mn;
    }
    sm[lane] = m;
    sinv[lane] = softmax_inv(m, l, true);  // (a hub row has slots)
  }
  __syncthreads();
  const int64_t t = static_cast<int64_t>(blockIdx.y) * kWave + lane;
  if (out && t < W + Z) {
    const int h = static_cast<int>(t < W ? t / C : (t - W) / De);
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c)
      acc = fmaf(part[c * S + t], expf(part[c * S + W + Z + h] - sm[h]), acc);
    if (t < W) out[row * W + t] = acc * sinv[h]; else z[row * Z + t - W] = acc * sinv[h];
  }
  if (blockIdx.y == 0 && lane < H) {
    stats[hr * 2 * H + lane] = sm[lane];
    stats[hr * 2 * H + H + lane] = sinv[lane];
  }
}

// the by-destination partials of the edge variant, (grad_query [W], grad_b [H*De]) per chunk,
// summed in chunk order
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    transformer_edge_sum_merge_kernel(const IdxT* __restrict__ hub_rows,
                                      const IdxT* __restrict__ hub_cptr, int64_t W, int64_t Z,
                                      const float* __restrict__ part, float* __restrict__ gq,
                                      float* __restrict__ gb) {
  const int64_t hr = blockIdx.x;
  merge_sum_row(hub_rows, hub_cptr, hr, W, part, W + Z, gq, W);
  merge_sum_row(hub_rows, hub_cptr, hr, Z, part + W, W + Z, gb, Z);
}

// Score mode on long rows: D[i,h] = sum_row alpha * d alpha spans the whole row.  Were every chunk
// to walk its row for it, a row of d slots would cost d^2 / chunk reads; this pre-pass leaves one
// partial per (chunk, head) and each chunk adds its row's partials, in chunk order.
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    transformer_hub_d_kernel(Items<IdxT> it, const float* __restrict__ alpha,
                             const float* __restrict__ galpha, int H, float* __restrict__ dpart) {
  const int64_t t = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (t >= it.n_chunks * H) return;
  const int h = static_cast<int>(t % H);
  Span s;
  float D = 0.f;
  if (decode(it, t / H, s)) {
    for (int64_t k = s.k0; k < s.k1; ++k) D = fmaf(alpha[k * H + h], galpha[k * H + h], D);
  }
  dpart[t] = D;
}

// ---- backward, by destination -------------------------------------------------------------------
// d s[k,h] = alpha * (d alpha - D);  grad_q[i] = scale * sum_k d s * key[j].
// SCORE: d alpha is given (the layer consumed alpha itself) and D = sum_row alpha * d alpha;
// otherwise d alpha = <grad_out[i,h,:], value[j,h,:]> and D = <grad_out[i,h,:], out[i,h,:]>.
// EDGE: d alpha gains <gz[i,h,:], a_k> and D gains <gz[i,h,:], z[i,h,:]> (neither in score mode);
// grad_b[i,h,:] = sum_k d s * a_k is accumulated beside grad_q, and, when wanted,
// grad_a[k,:] = sum_h (d s * b[i,h,:] + alpha * gz[i,h,:]) is summed over the lane groups.
template <typename IdxT, int EPL, bool VEC, bool SCORE, bool EDGE>
__device__ __forceinline__ void
    transformer_bwd_dst_body(const Items<IdxT>& it, const IdxT* __restrict__ col,
                             const float* __restrict__ key, const float* __restrict__ value,
                             int64_t ld, const float* __restrict__ alpha,
                             const float* __restrict__ gout, const float* __restrict__ outp,
                             const float* __restrict__ galpha, int H, int C, int lph,
                             float scale, float* __restrict__ ds, float* __restrict__ gq,
                             float* __restrict__ part, const float* __restrict__ dpart,
                             const EdgeBwd& ed) {
  constexpr int U = SlotsInFlight<EPL>::n;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float g[SCORE ? 1 : EPL], acc[EPL];
  float D = 0.f;
  if constexpr (SCORE) {
    if (s.chunk_id >= 0) {  // the row's per-chunk partials (transformer_hub_d_kernel)
      if (L.head_ok && L.sub == 0) {
        const int64_t c1 = static_cast<int64_t>(it.hub_cptr[s.hub + 1]);
        for (int64_t c = static_cast<int64_t>(it.hub_cptr[s.hub]); c < c1; ++c)
          D += dpart[c * H + L.h];
      }
    } else if (L.head_ok) {
      for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
        D = fmaf(alpha[k * H + L.h], galpha[k * H + L.h], D);
    }
  } else {
    float o[EPL];
    load_row<EPL, VEC>(gout + s.row * W, L, g);
    load_row<EPL, VEC>(outp + s.row * W, L, o);
#pragma unroll
    for (int e = 0; e < EPL; ++e) D = fmaf(g[e], o[e], D);
  }
  float bb[kEdgeRegs], gzz[kEdgeRegs], gb[kEdgeRegs];
  if constexpr (EDGE) {
    const int64_t hz = (s.row * H + L.h) * ed.De;
    load_edge(ed.b + hz, L, ed.De, bb);
#pragma unroll
    for (int r = 0; r < kEdgeRegs; ++r) gb[r] = 0.f;
    if constexpr (!SCORE) {
      float zr[kEdgeRegs];
      load_edge(ed.gz + hz, L, ed.De, gzz);
      load_edge(ed.z + hz, L, ed.De, zr);
#pragma unroll
      for (int r = 0; r < kEdgeRegs; ++r) D = fmaf(gzz[r], zr[r], D);
    }
  }
  D = group_sum(D, lph);
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float kk[U][EPL], vv[SCORE ? 1 : U][EPL], aa[EDGE ? U : 1][kEdgeRegs];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        load_row<EPL, VEC>(key + j * ld, L, kk[u]);
        if constexpr (!SCORE) load_row<EPL, VEC>(value + j * ld, L, vv[u]);
        if constexpr (EDGE) load_edge(ed.ea + (k + u) * ed.De, L, ed.De, aa[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        float da = 0.f;
        if constexpr (SCORE) {
          da = L.head_ok ? galpha[(k + u) * H + L.h] : 0.f;
        } else {
#pragma unroll
          for (int e = 0; e < EPL; ++e) da = fmaf(g[e], vv[u][e], da);
          if constexpr (EDGE) {
#pragma unroll
            for (int r = 0; r < kEdgeRegs; ++r) da = fmaf(gzz[r], aa[u][r], da);
          }
          da = group_sum(da, lph);
        }
        const float al = L.head_ok ? alpha[(k + u) * H + L.h] : 0.f;
        const float d = al * (da - D);
        if (L.head_ok && L.sub == 0) ds[(k + u) * H + L.h] = d;
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = fmaf(d, kk[u][e], acc[e]);
        if constexpr (EDGE) {
#pragma unroll
          for (int r = 0; r < kEdgeRegs; ++r) gb[r] = fmaf(d, aa[u][r], gb[r]);
          if (ed.ga) {  // wave-uniform; lanes past the last head hold d = al = 0
            float t[kEdgeRegs];
#pragma unroll
            for (int r = 0; r < kEdgeRegs; ++r) {
              t[r] = d * bb[r];
              if constexpr (!SCORE) t[r] = fmaf(al, gzz[r], t[r]);
              t[r] = head_sum(t[r], lph);
            }
            if (L.h == 0) store_edge(ed.ga + (k + u) * ed.De, L, ed.De, t);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] *= scale;
  if constexpr (EDGE) {
    const int64_t Z = static_cast<int64_t>(H) * ed.De;
    if (s.chunk_id >= 0) {
      float* p = part + s.chunk_id * (W + Z);
      store_row<EPL, VEC>(p, L, acc);
      store_edge(p + W + L.h * ed.De, L, ed.De, gb);
    } else {
      store_row<EPL, VEC>(gq + s.row * W, L, acc);
      store_edge(ed.gb + (s.row * H + L.h) * ed.De, L, ed.De, gb);
    }
  } else {
    store_row<EPL, VEC>(s.chunk_id >= 0 ? part + s.chunk_id * W : gq + s.row * W, L, acc);
  }
}

template <typename IdxT, int EPL, bool VEC, bool SCORE>
__global__ void __launch_bounds__(kBlock)
    transformer_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                               const float* __restrict__ key, const float* __restrict__ value,
                               int64_t ld, const float* __restrict__ alpha,
                               const float* __restrict__ gout, const float* __restrict__ outp,
                               const float* __restrict__ galpha, int H, int C, int lph,
                               float scale, float* __restrict__ ds, float* __restrict__ gq,
                               float* __restrict__ part, const float* __restrict__ dpart) {
  transformer_bwd_dst_body<IdxT, EPL, VEC, SCORE, false>(it, col, key, value, ld, alpha, gout,
                                                         outp, galpha, H, C, lph, scale, ds, gq,
                                                         part, dpart, EdgeBwd{});
}

template <typename IdxT, int EPL, bool VEC, bool SCORE>
__global__ void __launch_bounds__(kBlock)
    transformer_edge_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                                    const float* __restrict__ key,
                                    const float* __restrict__ value, int64_t ld,
                                    const float* __restrict__ alpha,
                                    const float* __restrict__ gout,
                                    const float* __restrict__ outp,
                                    const float* __restrict__ galpha, int H, int C, int lph,
                                    float scale, float* __restrict__ ds, float* __restrict__ gq,
                                    float* __restrict__ part, const float* __restrict__ dpart,
                                    EdgeBwd ed) {
  transformer_bwd_dst_body<IdxT, EPL, VEC, SCORE, true>(it, col, key, value, ld, alpha, gout,
                                                        outp, galpha, H, C, lph, scale, ds, gq,
                                                        part, dpart, ed);
}

// ---- backward, by source ---------------------------------------------------------------------
// over the edges j -> i of source j: grad_key[j] = scale * sum d s * q[i] and (not in SCORE mode)
// grad_value[j] = sum alpha * grad_out[i]; alpha and d s are read at the mapped by-destination slot.
template <typename IdxT, int EPL, bool VEC, bool SCORE>
__global__ void __launch_bounds__(kBlock)
    transformer_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                               const IdxT* __restrict__ slot_map,
                               const float* __restrict__ query, const float* __restrict__ alpha,
                               const float* __restrict__ ds, const float* __restrict__ gout,
                               int H, int C, int lph, float scale, float* __restrict__ gkey,
                               float* __restrict__ gvalue, int64_t ld,
                               float* __restrict__ part) {
  constexpr int U = SlotsInFlight<EPL>::n;
  constexpr int NOUT = SCORE ? 1 : 2;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float gk[EPL], gv[SCORE ? 1 : EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) gk[e] = 0.f;
  if constexpr (!SCORE) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) gv[e] = 0.f;
  }
  for (int64_t t = s.k0; t < s.k1; t += U) {
    float qq[U][EPL], g[SCORE ? 1 : U][EPL];
    float al[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t + u < s.k1) {
        const int64_t i = static_cast<int64_t>(col_t[t + u]);
        const int64_t kd = static_cast<int64_t>(slot_map[t + u]);
        load_row<EPL, VEC>(query + i * W, L, qq[u]);
        if constexpr (!SCORE) load_row<EPL, VEC>(gout + i * W, L, g[u]);
        al[u] = (!SCORE && L.head_ok) ? alpha[kd * H + L.h] : 0.f;
        d[u] = L.head_ok ? ds[kd * H + L.h] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (t + u < s.k1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          gk[e] = fmaf(d[u], qq[u][e], gk[e]);
          if constexpr (!SCORE) gv[e] = fmaf(al[u], g[u][e], gv[e]);
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < EPL; ++e) gk[e] *= scale;
  if (s.chunk_id >= 0) {
    float* p = part + s.chunk_id * (NOUT * W);
    store_row<EPL, VEC>(p, L, gk);
    if constexpr (!SCORE) store_row<EPL, VEC>(p + W, L, gv);
    return;
  }
  store_row<EPL, VEC>(gkey + s.row * ld, L, gk);
  if constexpr (!SCORE) store_row<EPL, VEC>(gvalue + s.row * ld, L, gv);
}

// ---- host side -------------------------------------------------------------------------------
// the largest use decides: forward n_chunks * (W + 2H) partials + n_hub * 2H statistics
// (n_hub <= n_chunks), by destination n_chunks * (W + H) (the partial rows, then the score mode's partials of D), by
// source n_chunks * 2W floats
size_t tf_ws_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  return sizeof(float) * static_cast<size_t>(n_chunks * (2 * H * C + 4 * H));
}

// the edge variant: forward n_chunks * (W + H*De + 2H) partials + n_hub * 2H statistics, by
// destination n_chunks * (W + H*De + H)
size_t tf_edge_ws_bytes(int64_t n_chunks, int64_t H, int64_t C, int64_t De) {
  return sizeof(float) * static_cast<size_t>(n_chunks * (H * C + H * De + 4 * H));
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_transformer_supported(int64_t H, int64_t C) {
  Shape s;
  return choose_shape(H, C, false, &s) ? 1 : 0;
}

int pygamd_transformer_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C, size_t* bytes) {
  if (!bytes || n_chunks < 0 || H < 1 || C < 1) return PYGAMD_ERR_INVALID_ARG;
  if (H * C > kMaxWidth || H > kAttnMaxHeads) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = tf_ws_bytes(n_chunks, H, C);
  return PYGAMD_OK;
}

int pygamd_transformer_forward(const pygamd_csr* g, const float* query, const float* key,
                               const float* value, int64_t ld, int64_t n_src, int64_t H, int64_t C,
                               float scale, float* alpha, float* out, void* workspace,
                               size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld < H * C) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !query || !key || !alpha || (out && !value))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < tf_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(query) && aligned16(key) && ld % 4 == 0 && aligned16(workspace) &&
                  (!out || (aligned16(out) && aligned16(value))) &&
                  (H % 2 == 0 || n_chunks == 0);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (out) {
        hipLaunchKernelGGL((transformer_fwd_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st, it,
                           c, query, key, value, ld, static_cast<int>(H), static_cast<int>(C),
                           sh.lph, scale, alpha, out, part);
      } else {
        hipLaunchKernelGGL((transformer_fwd_kernel<IdxT, EPL, VEC, false>), grid, block, 0, st,
                           it, c, query, key, value, ld, static_cast<int>(H), static_cast<int>(C),
                           sh.lph, scale, alpha, out, part);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      float* stats = part + n_chunks * (H * C + 2 * H);
      hipLaunchKernelGGL((transformer_fwd_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(n_hub),
                              out ? static_cast<unsigned>(ceil_div(H * C, kWave)) : 1u),
                         dim3(kWave), 0, st, it.rowptr, it.hub_rows, it.hub_cptr,
                         static_cast<int>(H), static_cast<int>(C), part, alpha, out, stats);
      PYGAMD_LAUNCH_CHECK();
      hipLaunchKernelGGL((transformer_alpha_rescale_kernel<IdxT>), dim3(wave_grid(n_chunks)),
                         block, 0, st, it, static_cast<int>(H), stats, alpha);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_transformer_backward_dst(const pygamd_csr* g, const float* key, const float* value,
                                    int64_t ld, const float* alpha, const float* grad_out,
                                    const float* out, const float* grad_alpha, int64_t n_src,
                                    int64_t H, int64_t C, float scale, float* grad_s,
                                    float* grad_query, void* workspace, size_t workspace_bytes,
                                    void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld < H * C) return PYGAMD_ERR_INVALID_ARG;
  // exactly one of (grad_out, out) and grad_alpha says where d alpha comes from
  const bool score = grad_alpha != nullptr;
  if (score ? (grad_out || out) : (!grad_out || !out)) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !key || (!score && !value) || !alpha || !grad_s || !grad_query)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < tf_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(key) && ld % 4 == 0 && aligned16(workspace) &&
                  aligned16(grad_query) &&
                  (score || (aligned16(value) && aligned16(grad_out) && aligned16(out)));
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int64_t W = H * C;
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    float* dpart = part + n_chunks * W;
    if (score && n_chunks > 0) {
      hipLaunchKernelGGL((transformer_hub_d_kernel<IdxT>),
                         dim3(static_cast<unsigned>(ceil_div(n_chunks * H, kBlock))), block, 0, st,
                         it, alpha, grad_alpha, static_cast<int>(H), dpart);
      PYGAMD_LAUNCH_CHECK();
    }
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (score) {
        hipLaunchKernelGGL((transformer_bwd_dst_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st,
                           it, c, key, value, ld, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, scale, grad_s,
                           grad_query, part, dpart);
      } else {
        hipLaunchKernelGGL((transformer_bwd_dst_kernel<IdxT, EPL, VEC, false>), grid, block, 0,
                           st, it, c, key, value, ld, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, scale, grad_s,
                           grad_query, part, dpart);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((transformer_sum_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(n_hub)), dim3(kWave), 0, st, it.hub_rows,
                         it.hub_cptr, W, 1, part, grad_query, static_cast<float*>(nullptr), W);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_transformer_backward_src(const pygamd_csr* g, const void* slot_map, const float* query,
                                    const float* alpha, const float* grad_s, const float* grad_out,
                                    int64_t n_dst, int64_t H, int64_t C, float scale,
                                    float* grad_key, float* grad_value, int64_t ld, void* workspace,
                                    size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_dst, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld < H * C) return PYGAMD_ERR_INVALID_ARG;
  if (n_src == 0) return PYGAMD_OK;
  const bool score = grad_out == nullptr;
  if (!g->rowptr || !g->col || !slot_map || !query || !alpha || !grad_s || !grad_key ||
      (!score && !grad_value))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < tf_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(query) && aligned16(grad_key) && ld % 4 == 0 &&
                  aligned16(workspace) && (score || (aligned16(grad_out) && aligned16(grad_value)));
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int64_t W = H * C;
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_src + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    const IdxT* sm = static_cast<const IdxT*>(slot_map);
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (score) {
        hipLaunchKernelGGL((transformer_bwd_src_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st,
                           it, c, sm, query, alpha, grad_s, grad_out, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, scale, grad_key, grad_value, ld, part);
      } else {
        hipLaunchKernelGGL((transformer_bwd_src_kernel<IdxT, EPL, VEC, false>), grid, block, 0,
                           st, it, c, sm, query, alpha, grad_s, grad_out, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, scale, grad_key, grad_value, ld, part);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((transformer_sum_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(n_hub)), dim3(kWave), 0, st, it.hub_rows,
                         it.hub_cptr, W, score ? 1 : 2, part, grad_key, grad_value, ld);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

// ---- the edge variant (edge_dim) ------------------------------------------------------------------
int pygamd_transformer_edge_supported(int64_t H, int64_t C, int64_t De) {
  Shape s;
  return choose_shape_edge(H, C, De, false, &s) ? 1 : 0;
}

int pygamd_transformer_edge_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C, int64_t De,
                                            size_t* bytes) {
  if (!bytes || n_chunks < 0 || H < 1 || C < 1 || De < 1) return PYGAMD_ERR_INVALID_ARG;
  if (!pygamd_transformer_edge_supported(H, C, De)) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = tf_edge_ws_bytes(n_chunks, H, C, De);
  return PYGAMD_OK;
}

int pygamd_transformer_edge_forward(const pygamd_csr* g, const float* query, const float* key,
                                    const float* value, int64_t ld, const float* edge_attr,
                                    const float* bias, int64_t n_src, int64_t H, int64_t C,
                                    int64_t De, float scale, float* alpha, float* out, float* z,
                                    void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld < H * C || De < 1) return PYGAMD_ERR_INVALID_ARG;
  if (!pygamd_transformer_edge_supported(H, C, De)) return PYGAMD_ERR_UNSUPPORTED;
  if (n_rows == 0) return PYGAMD_OK;
  // out and z come together (aggregation) or not at all (score mode)
  if (!g->rowptr || !g->col || !query || !key || !edge_attr || !bias || !alpha || (out && !value) ||
      (out != nullptr) != (z != nullptr))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < tf_edge_ws_bytes(n_chunks, H, C, De)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  // (a chunk's partial is W + H*De + 2H floats: float4 stores of its row need that a multiple of 4)
  const bool al = aligned16(query) && aligned16(key) && ld % 4 == 0 && aligned16(workspace) &&
                  (!out || (aligned16(out) && aligned16(value))) &&
                  ((H * De + 2 * H) % 4 == 0 || n_chunks == 0);
  if (!choose_shape_edge(H, C, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  const EdgeFwd ed{edge_attr, bias, z, static_cast<int>(De)};
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (out) {
        hipLaunchKernelGGL((transformer_edge_fwd_kernel<IdxT, EPL, VEC, true>), grid, block, 0,
                           st, it, c, query, key, value, ld, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, scale, alpha, out, part, ed);
      } else {
        hipLaunchKernelGGL((transformer_edge_fwd_kernel<IdxT, EPL, VEC, false>), grid, block, 0,
                           st, it, c, query, key, value, ld, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, scale, alpha, out, part, ed);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      float* stats = part + n_chunks * (H * C + H * De + 2 * H);
      hipLaunchKernelGGL((transformer_edge_fwd_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(n_hub),
                              out ? static_cast<unsigned>(ceil_div(H * C + H * De, kWave)) : 1u),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, static_cast<int>(H),
                         static_cast<int>(C), static_cast<int>(De), part, out, z, stats);
      PYGAMD_LAUNCH_CHECK();
      hipLaunchKernelGGL((transformer_alpha_rescale_kernel<IdxT>), dim3(wave_grid(n_chunks)),
                         block, 0, st, it, static_cast<int>(H), stats, alpha);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_transformer_edge_backward_dst(
    const pygamd_csr* g, const float* key, const float* value, int64_t ld, const float* edge_attr,
    const float* bias, const float* alpha, const float* grad_out, const float* out,
    const float* grad_z, const float* z, const float* grad_alpha, int64_t n_src, int64_t H,
    int64_t C, int64_t De, float scale, float* grad_s, float* grad_query, float* grad_bias,
    float* grad_edge_attr, void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (ld < H * C || De < 1) return PYGAMD_ERR_INVALID_ARG;
  if (!pygamd_transformer_edge_supported(H, C, De)) return PYGAMD_ERR_UNSUPPORTED;
  // exactly one of (grad_out, out, grad_z, z) and grad_alpha says where d alpha comes from
  const bool score = grad_alpha != nullptr;
  if (score ? (grad_out || out || grad_z || z) : (!grad_out || !out || !grad_z || !z))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !key || (!score && !value) || !edge_attr || !bias || !alpha ||
      !grad_s || !grad_query || !grad_bias)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < tf_edge_ws_bytes(n_chunks, H, C, De)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(key) && ld % 4 == 0 && aligned16(workspace) &&
                  aligned16(grad_query) && ((H * De) % 4 == 0 || n_chunks == 0) &&
                  (score || (aligned16(value) && aligned16(grad_out) && aligned16(out)));
  if (!choose_shape_edge(H, C, De, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int64_t W = H * C, Z = H * De;
  float* part = static_cast<float*>(workspace);
  const EdgeBwd ed{edge_attr, bias, grad_z, z, grad_bias, grad_edge_attr, static_cast<int>(De)};
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    float* dpart = part + n_chunks * (W + Z);
    if (score && n_chunks > 0) {
      hipLaunchKernelGGL((transformer_hub_d_kernel<IdxT>),
                         dim3(static_cast<unsigned>(ceil_div(n_chunks * H, kBlock))), block, 0, st,
                         it, alpha, grad_alpha, static_cast<int>(H), dpart);
      PYGAMD_LAUNCH_CHECK();
    }
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (score) {
        hipLaunchKernelGGL((transformer_edge_bwd_dst_kernel<IdxT, EPL, VEC, true>), grid, block,
                           0, st, it, c, key, value, ld, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, scale, grad_s,
                           grad_query, part, dpart, ed);
      } else {
        hipLaunchKernelGGL((transformer_edge_bwd_dst_kernel<IdxT, EPL, VEC, false>), grid, block,
                           0, st, it, c, key, value, ld, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, scale, grad_s,
                           grad_query, part, dpart, ed);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((transformer_edge_sum_merge_kernel<IdxT>),
                         dim3(static_cast<unsigned>(n_hub)), dim3(kWave), 0, st, it.hub_rows,
                         it.hub_cptr, W, Z, part, grad_query, grad_bias);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

}  // extern "C"

// rgat.hip — RGATConv's additive relational attention (nn/conv/rgat_conv.py:373-505 of the reference:
// a weight matrix gathered per edge, two bmm over it, the [E, H*C] outi / outj and several [E, H]
// softmax passes) in ONE pass per destination over the by-destination handle of ALL edges, the
// softmax running across every relation of the destination ("across-relation", the default).
//
// With dim = 1 every per-edge operand is node-level (the algebra: include/pyg_amd.h):
//   P  [N, R, H*C]  the R source transforms as one dense product, relation r = columns [rW, (r+1)W)
//   QI [N, R, H]    P[:, r] @ q         KJ [N, R, H]    P[:, r] @ k
//   B  [E, H]       the optional per-edge score bias of edge_dim, in slot order
// For destination i, slot k with source j = col[k] and relation r = rel[k] (int32, slot order):
//   s[k,h]   = leaky_relu(QI[i,r,h] + KJ[j,r,h] (+ B[k,h]))
//   alpha    = softmax of s over the row (online: maximum subtracted, 1e-16 on the denominator)
//   out[i,h] = sum_k alpha[k,h] * P[j,r,h,:]
// The lane keeps QI[i,r,h] of the current relation in a register and loads it again only when a
// slot's relation differs from the slot before it: any in-row order is correct, a row grouped by
// relation reloads once per relation present.  A slot gathers one scalar of KJ and ONE H*C row of
// P; nothing of size E x H*C exists.  P, QI and KJ have row strides: three tensors, or the column
// blocks of one packed plane [P | QI | KJ] read in place.
//
// Backward, with g = grad_out[i]:
//   by destination (the same rows): d alpha[k,h] = <g[h], P[j,r,h]>, D[h] = <g[h], out[i,h]>,
//     grad_s[k,h] = alpha (d alpha - D) * leaky_relu'(pre)   (the slope where pre <= 0), which is
//     grad_B as it stands;
//   by pair (the (relation, node) pair rows of _onepass's pair forms, with the map from a pair
//     slot to its by-destination slot): grad_a[node, r, h] = sum grad_s — grad_QI on the
//     (relation, destination) rows, grad_KJ on the (relation, source) rows — and, on the latter,
//     grad_P[j, r] = sum alpha * g[i] from ONE gathered row of grad_out per slot.
// Pairs that do not occur are not written: the caller zero-fills the gradient planes once.
//
// Within-relation (the softmax over the edges of relation r into i): one scalar launch over the
// (relation, destination) pair rows first writes the pair's (maximum, 1 / (sum + 1e-16)) [N, R, 2H];
// the same row kernel then weighs a slot with exp(s - m_pair) / (l_pair + 1e-16), rescales nothing
// and merges the chunks of a long row by addition.  Backward: the by-destination launch writes the
// raw d alpha, and the scalar launch over the pair rows subtracts the PAIR's sum alpha * d alpha,
// applies the slope and sums grad_QI (it stands in for the pair launch over those rows).
//
// Lane layout, work items, hub chunks and their in-order sum merge: rowwalk_device.h.  Online
// softmax, non-finite rules and its merge: attn_device.h.  No float atomics and every grid depends
// on the problem's sizes only: every result is bitwise reproducible.
#include <math.h>

#include "attn_device.h"
#include "common.h"

namespace pygamd {
namespace {

using namespace rowwalk;  // layout, work items and the sum merge: rowwalk_device.h
using namespace attn;     // online softmax and its merge: attn_device.h

template <int EPL>
struct RgatInFlight {
  static constexpr int rows = EPL >= 16 ? 2 : 4;  // gathered rows in flight per wave
};

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    rgat_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const int* __restrict__ rel,
                    const float* __restrict__ P, int64_t ld_p, const float* __restrict__ QI,
                    int64_t ld_qi, const float* __restrict__ KJ, int64_t ld_kj,
                    const float* __restrict__ B, const float* __restrict__ stats, int64_t R,
                    int H, int C, int lph, float slope, float* __restrict__ alpha,
                    float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = RgatInFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  const float* qrow = QI + s.row * ld_qi;
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float m = -INFINITY, l = 0.f, qi = 0.f;
  float pm = 0.f, pinv = 0.f;  // within-relation: the pair's (maximum, 1 / (sum + 1e-16))
  int cur = -1;                // the relation whose QI (and pair statistics) the registers hold
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float v[U][EPL], kj[U], b[U];
    int r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        r[u] = rel[k + u];
        kj[u] = L.head_ok ? KJ[j * ld_kj + static_cast<int64_t>(r[u]) * H + L.h] : 0.f;
        b[u] = (B && L.head_ok) ? B[(k + u) * H + L.h] : 0.f;
        load_row<EPL, VEC>(P + j * ld_p + static_cast<int64_t>(r[u]) * W, L, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        if (r[u] != cur) {
          cur = r[u];
          qi = L.head_ok ? qrow[static_cast<int64_t>(cur) * H + L.h] : 0.f;
          if (stats && L.head_ok) {
            const float* st = stats + (s.row * R + cur) * 2 * H;
            pm = st[L.h];
            pinv = st[H + L.h];
          }
        }
        const float t = B ? (qi + kj[u]) + b[u] : qi + kj[u];
        const float p = t > 0.f ? t : t * slope;  // (every lane of a head holds the same score)
        if (stats) {  // within-relation: the finished coefficient, no rescaling
          const float w = softmax_weight(p, pm) * pinv;
          if (L.head_ok && L.sub == 0) alpha[(k + u) * H + L.h] = w;
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(w, v[u][e], acc[e]);
          continue;
        }
        // the raw score; the lane that writes it is the lane that rescales it below
        if (L.head_ok && L.sub == static_cast<int>((k + u - s.row_start) & (lph - 1)))
          alpha[(k + u) * H + L.h] = p;
        const float mn = fmaxf(m, p);
        const float sc = softmax_weight(m, mn), pe = softmax_weight(p, mn);
        l = fmaf(l, sc, pe);
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = fmaf(acc[e], sc, pe * v[u][e]);
        m = mn;
      }
    }
  }
  if (s.chunk_id >= 0) {  // partial (acc, m, l) of one chunk of a long row
    float* p = part + s.chunk_id * (W + 2 * H);
    store_row<EPL, VEC>(p, L, acc);
    if (L.head_ok && L.sub == 0) {
      p[W + L.h] = m;
      p[W + H + L.h] = l;
    }
    return;
  }
  if (stats) {
    store_row<EPL, VEC>(out + s.row * W, L, acc);
    return;
  }
  const float inv = softmax_inv(m, l, s.k1 > s.k0);
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] *= inv;
  store_row<EPL, VEC>(out + s.row * W, L, acc);
  if (L.head_ok) {
    for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
      alpha[k * H + L.h] = expf(alpha[k * H + L.h] - m) * inv;
  }
}

// one 64-lane workgroup per hub row: final (m, l) per head, the output row, the row's alpha
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    rgat_fwd_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                          const IdxT* __restrict__ hub_cptr, int H, int C, int within,
                          const float* __restrict__ part, float* __restrict__ alpha,
                          float* __restrict__ out) {
  __shared__ float sm[kAttnMaxHeads], sinv[kAttnMaxHeads];
  if (within) {  // finished coefficients: the chunks' partial rows add up, in chunk order
    const int64_t W = static_cast<int64_t>(H) * C;
    merge_sum_row(hub_rows, hub_cptr, static_cast<int64_t>(blockIdx.x), W, part, W + 2 * H, out, W);
    return;
  }
  merge_softmax_row(rowptr, hub_rows, hub_cptr, static_cast<int64_t>(blockIdx.x), H, C, part,
                    alpha, out, sm, sinv, 0, static_cast<int64_t>(H) * C, true, nullptr);
}

// ---- backward, by destination -------------------------------------------------------------------
// Every slot's grad_s depends on its own row's g and D only, so a chunk of a long row is a row
// like any other here: no partials, no merge.
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    rgat_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const int* __restrict__ rel,
                        const float* __restrict__ P, int64_t ld_p, const float* __restrict__ QI,
                        int64_t ld_qi, const float* __restrict__ KJ, int64_t ld_kj,
                        const float* __restrict__ B, const float* __restrict__ alpha,
                        const float* __restrict__ gout, const float* __restrict__ outp, int H,
                        int C, int lph, float slope, int within, float* __restrict__ ds) {
  constexpr int U = RgatInFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  const float* qrow = QI + s.row * ld_qi;
  float g[EPL];
  load_row<EPL, VEC>(gout + s.row * W, L, g);
  float D = 0.f;
  if (!within) {  // (within-relation: the pair launch sums the PAIR's D, the row's is not used)
    float o[EPL];
    load_row<EPL, VEC>(outp + s.row * W, L, o);
#pragma unroll
    for (int e = 0; e < EPL; ++e) D = fmaf(g[e], o[e], D);
    D = group_sum(D, lph);
  }
  float qi = 0.f;
  int cur = -1;
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float v[U][EPL], kj[U], b[U], al[U];
    int r[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        r[u] = rel[k + u];
        kj[u] = L.head_ok ? KJ[j * ld_kj + static_cast<int64_t>(r[u]) * H + L.h] : 0.f;
        b[u] = (B && L.head_ok) ? B[(k + u) * H + L.h] : 0.f;
        al[u] = L.head_ok ? alpha[(k + u) * H + L.h] : 0.f;
        load_row<EPL, VEC>(P + j * ld_p + static_cast<int64_t>(r[u]) * W, L, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        if (r[u] != cur) {
          cur = r[u];
          qi = L.head_ok ? qrow[static_cast<int64_t>(cur) * H + L.h] : 0.f;
        }
        float da = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) da = fmaf(g[e], v[u][e], da);
        da = group_sum(da, lph);
        const float t = B ? (qi + kj[u]) + b[u] : qi + kj[u];  // (the forward's own sum)
        // (within-relation: the raw d alpha; the pair launch subtracts the PAIR's sum)
        const float d = within ? da : al[u] * (da - D) * (t > 0.f ? 1.f : slope);
        if (L.head_ok && L.sub == 0) ds[(k + u) * H + L.h] = d;
      }
    }
  }
}

// ---- backward, by pair --------------------------------------------------------------------------
// A wave owns pair row p = (r, node) (or a chunk of its slots); slot q of it is the by-destination
// slot slot_map[q] and has the other endpoint col[q].  ga[node, r, :] = sum grad_s; with gp
// (the (relation, source) rows: col = the destinations) gp[node, r] = sum alpha * g[col].
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    rgat_bwd_pair_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                         const IdxT* __restrict__ slot_map, const IdxT* __restrict__ pair_rel,
                         const IdxT* __restrict__ pair_node, const float* __restrict__ alpha,
                         const float* __restrict__ ds, const float* __restrict__ gout, int H, int C,
                         int lph, float* __restrict__ ga, int64_t ld_ga, float* __restrict__ gp,
                         int64_t ld_gp, float* __restrict__ part, float* __restrict__ part_h) {
  constexpr int U = RgatInFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  const int64_t r = static_cast<int64_t>(pair_rel[s.row]);
  const int64_t node = static_cast<int64_t>(pair_node[s.row]);
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float gs = 0.f;
  for (int64_t q = s.k0; q < s.k1; q += U) {
    float g[U][EPL], al[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
        const int64_t kd = static_cast<int64_t>(slot_map[q + u]);
        d[u] = L.head_ok ? ds[kd * H + L.h] : 0.f;
        if (gp) {
          al[u] = L.head_ok ? alpha[kd * H + L.h] : 0.f;
          load_row<EPL, VEC>(gout + static_cast<int64_t>(col[q + u]) * W, L, g[u]);
        }
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
        gs += d[u];
        if (gp) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(al[u], g[u][e], acc[e]);
        }
      }
    }
  }
  if (gp) store_row<EPL, VEC>(s.chunk_id >= 0 ? part + s.chunk_id * W : gp + node * ld_gp + r * W,
                              L, acc);
  if (L.head_ok && L.sub == 0)
    (s.chunk_id >= 0 ? part_h + s.chunk_id * H : ga + node * ld_ga + r * H)[L.h] = gs;
}

// long pair rows: the chunks' partial rows summed in chunk order into block pair_rel[row] of row
// pair_node[row]: the [H] sums and, with gp, the [W] row
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    rgat_pair_merge_kernel(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_cptr,
                           const IdxT* __restrict__ pair_rel, const IdxT* __restrict__ pair_node,
                           int64_t W, int64_t H, const float* __restrict__ part,
                           const float* __restrict__ part_h, float* __restrict__ ga, int64_t ld_ga,
                           float* __restrict__ gp, int64_t ld_gp) {
  const int64_t hr = static_cast<int64_t>(blockIdx.x);
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t r = static_cast<int64_t>(pair_rel[row]);
  const int64_t node = static_cast<int64_t>(pair_node[row]);
  for (int64_t t = threadIdx.x; t < H; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part_h[c * H + t];
    ga[node * ld_ga + r * H + t] = acc;
  }
  if (!gp) return;
  for (int64_t t = threadIdx.x; t < W; t += kWave) {
    float acc = 0.f;
    for (int64_t c = c0; c < c1; ++c) acc += part[c * W + t];
    gp[node * ld_gp + r * W + t] = acc;
  }
}

// ---- within-relation: the pair rows' scalars --------------------------------------------------------
// A wave owns pair row p = (r, i) of the (relation, destination) form WHOLE (scalars only: a long
// pair row is a longer loop, not a chunked one).  lps lanes per head take the row's slots in turn;
// slot q is the by-destination slot f = slot_map[q] with source col[q].
//   forward  (alpha == NULL): stats[i, r] = (m [H], 1 / (l + 1e-16) [H]) of the pair's scores;
//   backward (alpha given; ds holds the raw d alpha of rgat_bwd_dst_kernel): D = sum alpha * d alpha
//     over the pair, ds[f] = alpha (d alpha - D) * leaky_relu'(pre) in place, gqi[i, r] = sum ds.
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    rgat_pair_scalar_kernel(Items<IdxT> it, const IdxT* __restrict__ col,
                            const IdxT* __restrict__ slot_map, const IdxT* __restrict__ pair_rel,
                            const IdxT* __restrict__ pair_node, const float* __restrict__ QI,
                            int64_t ld_qi, const float* __restrict__ KJ, int64_t ld_kj,
                            const float* __restrict__ B, int64_t R, int H, int lps, float slope,
                            const float* __restrict__ alpha, float* __restrict__ ds,
                            float* __restrict__ stats, float* __restrict__ gqi, int64_t ld_gqi) {
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const int h = lane_id() / lps, sub = lane_id() % lps;
  const bool ok = h < H;
  const int64_t r = static_cast<int64_t>(pair_rel[s.row]);
  const int64_t node = static_cast<int64_t>(pair_node[s.row]);
  const float qi = ok ? QI[node * ld_qi + r * H + h] : 0.f;
  if (!alpha) {
    float m = -INFINITY, l = 0.f;
    for (int64_t q = s.k0 + sub; q < s.k1; q += lps) {
      const int64_t j = static_cast<int64_t>(col[q]);
      const int64_t f = static_cast<int64_t>(slot_map[q]);
      const float kj = ok ? KJ[j * ld_kj + r * H + h] : 0.f;
      const float t = B ? (qi + kj) + (ok ? B[f * H + h] : 0.f) : qi + kj;
      const float p = t > 0.f ? t : t * slope;
      const float mn = fmaxf(m, p);
      l = l * softmax_weight(m, mn) + softmax_weight(p, mn);
      m = mn;
    }
    for (int o = lps >> 1; o > 0; o >>= 1) {
      const float mo = __shfl_xor(m, o, kWave), lo = __shfl_xor(l, o, kWave);
      const float mn = fmaxf(m, mo);
      l = l * softmax_weight(m, mn) + lo * softmax_weight(mo, mn);
      m = mn;
    }
    if (ok && sub == 0) {
      float* st = stats + (node * R + r) * 2 * H;
      st[h] = m;
      st[H + h] = softmax_inv(m, l, true);  // (a pair row has slots)
    }
    return;
  }
  float D = 0.f;
  for (int64_t q = s.k0 + sub; q < s.k1; q += lps) {
    const int64_t f = static_cast<int64_t>(slot_map[q]);
    if (ok) D = fmaf(alpha[f * H + h], ds[f * H + h], D);
  }
  D = group_sum(D, lps);
  float gs = 0.f;
  for (int64_t q = s.k0 + sub; q < s.k1; q += lps) {  // (every lane rewrites the slots it read)
    const int64_t j = static_cast<int64_t>(col[q]);
    const int64_t f = static_cast<int64_t>(slot_map[q]);
    if (ok) {
      const float kj = KJ[j * ld_kj + r * H + h];
      const float t = B ? (qi + kj) + B[f * H + h] : qi + kj;
      const float d = alpha[f * H + h] * (ds[f * H + h] - D) * (t > 0.f ? 1.f : slope);
      ds[f * H + h] = d;
      gs += d;
    }
  }
  gs = group_sum(gs, lps);
  if (ok && sub == 0) gqi[node * ld_gqi + r * H + h] = gs;
}

// ---- host side -------------------------------------------------------------------------------
// pygamd_han_workspace_bytes(n_chunks, H, C): a chunk's partial is the forward's (acc [W], m [H],
// l [H]), by pair (acc [W], sums [H])
size_t rgat_ws_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  size_t bytes = 0;
  pygamd_han_workspace_bytes(n_chunks, H, C, &bytes);  // (inside the shared envelope)
  return bytes;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_rgat_supported(int64_t H, int64_t C) {
  Shape s;
  return choose_shape(H, C, false, &s) ? 1 : 0;
}

int pygamd_rgat_forward(const pygamd_csr* g, const int32_t* rel, const float* p, int64_t ld_p,
                        const float* qi, int64_t ld_qi, const float* kj, int64_t ld_kj,
                        const float* b, const float* pair_stats, int64_t n_src, int64_t H,
                        int64_t C, int64_t R, float slope, float* alpha, float* out,
                        void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks, W = H * C;
  if (R < 1 || ld_p < R * W || ld_qi < R * H || ld_kj < R * H) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !rel || !p || !qi || !kj || !alpha || !out)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < rgat_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(p) && ld_p % 4 == 0 && aligned16(out) && aligned16(workspace) &&
                  (H % 2 == 0 || n_chunks == 0);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((rgat_fwd_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, rel, p,
                         ld_p, qi, ld_qi, kj, ld_kj, b, pair_stats, R, static_cast<int>(H),
                         static_cast<int>(C), sh.lph, slope, alpha, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((rgat_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.rowptr, it.hub_rows, it.hub_cptr,
                         static_cast<int>(H), static_cast<int>(C), pair_stats ? 1 : 0, part,
                         alpha, out);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_rgat_backward_dst(const pygamd_csr* g, const int32_t* rel, const float* p,
                             int64_t ld_p, const float* qi, int64_t ld_qi, const float* kj,
                             int64_t ld_kj, const float* b, const float* alpha,
                             const float* grad_out, const float* out, int64_t n_src, int64_t H,
                             int64_t C, int64_t R, float slope, int within, float* grad_s,
                             void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks, W = H * C;
  if (R < 1 || ld_p < R * W || ld_qi < R * H || ld_kj < R * H || (within != 0 && within != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !rel || !p || !qi || !kj || !alpha || !grad_out || !out || !grad_s)
    return PYGAMD_ERR_INVALID_ARG;
  Shape sh;
  const bool al = aligned16(p) && ld_p % 4 == 0 && aligned16(grad_out) && aligned16(out);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((rgat_bwd_dst_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, rel, p,
                         ld_p, qi, ld_qi, kj, ld_kj, b, alpha, grad_out, out,
                         static_cast<int>(H), static_cast<int>(C), sh.lph, slope, within, grad_s);
    });
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_rgat_pair_scalar(const pygamd_csr* g, const void* slot_map, const void* pair_rel,
                            const void* pair_dst, const float* qi, int64_t ld_qi, const float* kj,
                            int64_t ld_kj, const float* b, const float* alpha, int64_t n_src,
                            int64_t H, int64_t R, float slope, float* grad_s, float* pair_stats,
                            float* grad_qi, int64_t ld_gqi, void* stream) {
  const int rc = check_args(g, n_src, H, 1);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows;
  if (R < 1 || ld_qi < R * H || ld_kj < R * H || (alpha && ld_gqi < R * H))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !slot_map || !pair_rel || !pair_dst || !qi || !kj ||
      (alpha ? (!grad_s || !grad_qi) : !pair_stats))
    return PYGAMD_ERR_INVALID_ARG;
  int lps = 1;
  while (lps * 2 * H <= kWave) lps *= 2;
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    // (every pair row whole: the handle's hub plan is not used)
    const Items<IdxT> it{static_cast<const IdxT*>(g->rowptr), nullptr, nullptr, n_rows, 0, 0, 0, 0};
    hipLaunchKernelGGL((rgat_pair_scalar_kernel<IdxT>), dim3(wave_grid(n_rows)), dim3(kBlock), 0,
                       st, it, typed_col<IdxT>(*g), static_cast<const IdxT*>(slot_map),
                       static_cast<const IdxT*>(pair_rel), static_cast<const IdxT*>(pair_dst), qi,
                       ld_qi, kj, ld_kj, b, R, static_cast<int>(H), lps, slope, alpha, grad_s,
                       pair_stats, grad_qi, ld_gqi);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_rgat_backward_src(const pygamd_csr* g, const void* slot_map, const void* pair_rel,
                             const void* pair_node, const float* alpha, const float* grad_s,
                             const float* grad_out, int64_t n_other, int64_t H, int64_t C,
                             int64_t R, float* grad_a, int64_t ld_ga, float* grad_p,
                             int64_t ld_gp, void* workspace, size_t workspace_bytes,
                             void* stream) {
  const int rc = check_args(g, n_other, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks, W = H * C;
  if (R < 1 || ld_ga < R * H || (grad_p && ld_gp < R * W)) return PYGAMD_ERR_INVALID_ARG;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !slot_map || !pair_rel || !pair_node || !grad_s || !grad_a ||
      (grad_p && (!alpha || !grad_out)))
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < rgat_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = grad_p && aligned16(grad_out) && aligned16(grad_p) && ld_gp % 4 == 0 &&
                  aligned16(workspace);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  float* part_h = part + n_chunks * W;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    const IdxT* sm = static_cast<const IdxT*>(slot_map);
    const IdxT* prel = static_cast<const IdxT*>(pair_rel);
    const IdxT* pnode = static_cast<const IdxT*>(pair_node);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((rgat_bwd_pair_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, sm,
                         prel, pnode, alpha, grad_s, grad_out, static_cast<int>(H),
                         static_cast<int>(C), sh.lph, grad_a, ld_ga, grad_p, ld_gp, part, part_h);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((rgat_pair_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, prel, pnode, W, H, part,
                         part_h, grad_a, ld_ga, grad_p, ld_gp);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

}  // extern "C"

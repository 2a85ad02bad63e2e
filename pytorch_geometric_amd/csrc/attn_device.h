// attn_device.h — what the one-pass attention kernels add to the row walk of rowwalk_device.h: the
// online softmax of a row's scores and the in-order merge of the (m, l, acc) partials of a long
// row's chunks, the per-head edge registers of transformer.hip's edge variant with its lane shape,
// and the entry points' check of a head layout.
// Included by gatv2.hip, transformer.hip, han.hip and rgat.hip, and by gen.hip for softmax_weight.
#pragma once
#include <math.h>

#include "common.h"
#include "rowwalk_device.h"

namespace pygamd {
namespace attn {

using namespace rowwalk;

constexpr int kAttnMaxHeads = 64;

// ---- the online softmax -------------------------------------------------------------------------
// A running (maximum m, sum l, weighted sum acc) takes in a score p, or a chunk's (m_c, l_c, acc_c),
// as   mn = fmaxf(m, p);  l = l * exp(m - mn) + exp(p - mn)   (acc like l).
// Both factors are exp(-inf - -inf) = NaN while nothing finite has been seen: a masked score
// (p = -inf) ahead of the first finite one, or a fully masked first chunk, would poison the row.
// A side that is -inf has weight exactly 0 — which is also what expf gives whenever the other side
// is finite, so for finite scores nothing changes, bit for bit.  NaN and +inf scores still reach l
// through the other factor and poison their own (row, head), as the reference's softmax does.
__device__ __forceinline__ float softmax_weight(float x, float mn) {
  return x == -INFINITY ? 0.f : expf(x - mn);
}

// 1 / (l + 1e-16) of a finished row; NaN for a row with slots whose every score is -inf (m is still
// -inf: l and acc are 0), the reference's exp(-inf - -inf).  A row without slots keeps out = 0.
__device__ __forceinline__ float softmax_inv(float m, float l, bool has_slots) {
  return (has_slots && m == -INFINITY) ? NAN : 1.f / (l + 1e-16f);
}

// ---- edge features (transformer.hip's edge variant) -----------------------------------------------
// The lane that serves head h, sub-lane `sub` additionally owns the edge features d = sub + lph * r,
// r < kEdgeRegs, of that head: a fixed register capacity with predication, so De <= kEdgeRegs * lph.
constexpr int kEdgeRegs = 4;

// `row` holds De floats: a slot's raw features (every head reads the same line) or one head's block
// of a per-destination [H, De] row
__device__ __forceinline__ void load_edge(const float* __restrict__ row, const Lay& L, int De,
                                          float (&v)[kEdgeRegs]) {
#pragma unroll
  for (int r = 0; r < kEdgeRegs; ++r) {
    const int d = L.sub + L.lph * r;
    v[r] = (L.head_ok && d < De) ? row[d] : 0.f;
  }
}

__device__ __forceinline__ void store_edge(float* __restrict__ row, const Lay& L, int De,
                                           const float (&v)[kEdgeRegs]) {
#pragma unroll
  for (int r = 0; r < kEdgeRegs; ++r) {
    const int d = L.sub + L.lph * r;
    if (L.head_ok && d < De) row[d] = v[r];
  }
}

// sum over the heads, i.e. across the lane groups of a wave: lanes with equal `sub` are combined by
// an xor-butterfly over the lane offsets lph, 2 * lph, ...; every lane gets the total
__device__ __forceinline__ float head_sum(float v, int lph) {
  for (int o = lph; o < kWave; o <<= 1) v += __shfl_xor(v, o, kWave);
  return v;
}

// The forward merge of hub row `hr`, for one 64-lane workgroup: the chunks' partials
// (acc [W], m [H], l [H]) at stride W + 2H combined IN CHUNK ORDER into the final (m, l) per head,
// the columns [col0, col1) of the output row (out may be NULL) and the row's alpha (raw scores in,
// coefficients out; left alone unless rescale_alpha).  stats != NULL: (m [H], 1 / (l + 1e-16) [H])
// go to stats + hr * 2H, for a launch that rescales the alpha of all chunks in parallel.
template <typename IdxT>
__device__ __forceinline__ void merge_softmax_row(const IdxT* __restrict__ rowptr,
                                                  const IdxT* __restrict__ hub_rows,
                                                  const IdxT* __restrict__ hub_cptr, int64_t hr,
                                                  int H, int C, const float* __restrict__ part,
                                                  float* __restrict__ alpha,
                                                  float* __restrict__ out, float* sm,
                                                  float* sinv, int64_t col0, int64_t col1,
                                                  bool rescale_alpha,
                                                  float* __restrict__ stats) {
  const int64_t row = static_cast<int64_t>(hub_rows[hr]);
  const int64_t c0 = static_cast<int64_t>(hub_cptr[hr]), c1 = static_cast<int64_t>(hub_cptr[hr + 1]);
  const int64_t W = static_cast<int64_t>(H) * C, S = W + 2 * H;
  const int lane = threadIdx.x;
  if (lane < H) {
    float m = -INFINITY, l = 0.f;
    for (int64_t c = c0; c < c1; ++c) {
      const float mc = part[c * S + W + lane], lc = part[c * S + W + H + lane];
      const float mn = fmaxf(m, mc);
      l = l * softmax_weight(m, mn) + lc * softmax_weight(mc, mn);
      m = mn;
    }
    sm[lane] = m;
    sinv[lane] = softmax_inv(m, l, true);  // (a hub row has slots)
  }
  __syncthreads();
  if (out) {
    for (int64_t t = col0 + lane; t < col1; t += kWave) {
      const int h = static_cast<int>(t / C);
      float acc = 0.f;
      for (int64_t c = c0; c < c1; ++c)
        acc = fmaf(part[c * S + t], expf(part[c * S + W + h] - sm[h]), acc);
      out[row * W + t] = acc * sinv[h];
    }
  }
  if (stats && lane < H) {
    stats[hr * 2 * H + lane] = sm[lane];
    stats[hr * 2 * H + H + lane] = sinv[lane];
  }
  if (!rescale_alpha) return;
  const int64_t k0 = static_cast<int64_t>(rowptr[row]) * H;
  const int64_t k1 = static_cast<int64_t>(rowptr[row + 1]) * H;
  for (int64_t t = k0 + lane; t < k1; t += kWave) {
    const int h = static_cast<int>(t % H);
    alpha[t] = expf(alpha[t] - sm[h]) * sinv[h];
  }
}

// ---- host side -------------------------------------------------------------------------------
// The lane shape of the edge variant: the shape of (H, C) with lph widened (idle lanes for the row)
// until kEdgeRegs * lph >= De.  Whether one exists does not depend on `aligned`.
inline bool choose_shape_edge(int64_t H, int64_t C, int64_t De, bool aligned, Shape* s) {
  if (De < 1 || !choose_shape(H, C, aligned, s)) return false;
  int lph = s->lph;
  while (kEdgeRegs * lph < De && lph * 2 * H <= kWave) lph *= 2;
  if (kEdgeRegs * lph < De) return false;
  if (lph != s->lph) {
    const int n = static_cast<int>(((s->vec ? C / 4 : C) + lph - 1) / lph);
    int epl = 1;
    while (epl < n) epl *= 2;
    *s = Shape{lph, s->vec ? 4 * n : epl, s->vec};
  }
  return true;
}

// the checks every entry point shares on its handle `g`, the row count of the other side and the
// head layout; 0 = go on
inline int check_args(const pygamd_csr* g, int64_t n_other, int64_t H, int64_t C) {
  const int rc = check_handle(g, n_other);
  if (rc != PYGAMD_OK) return rc;
  if (H < 1 || C < 1) return PYGAMD_ERR_INVALID_ARG;
  if (H * C > kMaxWidth || H > kAttnMaxHeads) return PYGAMD_ERR_UNSUPPORTED;
  return PYGAMD_OK;
}

}  // namespace attn
}  // namespace pygamd

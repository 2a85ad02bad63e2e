// gatv2.hip — GATv2 attention (nn/conv/gatv2_conv.py:358-378 of the reference) as row-gather
// kernels on a sorted handle.  The score
//     s[i<-j, h] = sum_c att[h,c] * leaky_relu(x_l[j,h,c] + x_r[i,h,c])
// needs the full source row per edge, and so does the aggregation: ONE pass per destination keeps
// x_r[i] in registers, gathers every x_l[j] once, runs an online softmax per head and (AGG)
// accumulates the weighted row.  Nothing of size E x H*C is ever written.  Lane layout (`lph`
// lanes per head, one wave per row or per chunk of a long row): rowwalk_device.h.
//
// Long rows (more slots than the handle's hub threshold) are split into the hub plan's chunks: one
// wave per chunk leaves a partial (m, l, acc) — or a partial gradient row — in the workspace and a
// merge kernel combines the chunks of a row in chunk order.  No float atomics anywhere: every
// result, the att gradient included, is bitwise reproducible.
#include <math.h>

#include "attn_device.h"
#include "common.h"

namespace pygamd {
namespace {

using namespace rowwalk;  // layout, work items and the sum merge: rowwalk_device.h
using namespace attn;     // online softmax and its merge: attn_device.h

constexpr int kGv2MaxBlocks = 1024;  // persistent grid of the by-destination backward

template <int EPL>
struct InFlight {
  static constexpr int fwd = EPL >= 16 ? 2 : 4;   // gathered rows in flight per wave
  static constexpr int src = EPL >= 8 ? 2 : 4;    // (the by-source pass gathers two rows per slot)
};

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC, bool AGG>
__global__ void __launch_bounds__(kBlock)
    gatv2_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const float* __restrict__ xl,
                     const float* __restrict__ xr, const float* __restrict__ att, int H, int C,
                     int lph, float slope, float* __restrict__ alpha, float* __restrict__ out,
                     float* __restrict__ part) {
  constexpr int U = InFlight<EPL>::fwd;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float a[EPL], r[EPL], acc[EPL];
  load_row<EPL, VEC>(att, L, a);
  load_row<EPL, VEC>(xr + s.row * W, L, r);
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float v[U][EPL];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        load_row<EPL, VEC>(xl + j * W, L, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        float p = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const float t = v[u][e] + r[e];
          p = fmaf(a[e], t > 0.f ? t : t * slope, p);
        }
        p = group_sum(p, lph);
        // the raw score; the lane that writes it is the lane that rescales it below
        if (L.head_ok && L.sub == static_cast<int>((k + u - s.row_start) & (lph - 1)))
          alpha[(k + u) * H + L.h] = p;
        const float mn = fmaxf(m, p);
        const float sc = softmax_weight(m, mn), pe = softmax_weight(p, mn);
        l = fmaf(l, sc, pe);
        if constexpr (AGG) {
#pragma unroll
          for (int e = 0; e < EPL; ++e) acc[e] = fmaf(acc[e], sc, pe * v[u][e]);
        }
        m = mn;
      }
    }
  }
  if (s.chunk_id >= 0) {  // partial (acc, m, l) of one chunk of a long row
    float* p = part + s.chunk_id * (W + 2 * H);
    if constexpr (AGG) store_row<EPL, VEC>(p, L, acc);
    if (L.head_ok && L.sub == 0) {
      p[W + L.h] = m;
      p[W + H + L.h] = l;
    }
    return;
  }
  const float inv = softmax_inv(m, l, s.k1 > s.k0);
  if constexpr (AGG) {
#pragma unroll
    for (int e = 0; e < EPL; ++e) acc[e] *= inv;
    store_row<EPL, VEC>(out + s.row * W, L, acc);
  }
  if (L.head_ok) {
    for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
      alpha[k * H + L.h] = expf(alpha[k * H + L.h] - m) * inv;
  }
}

// one 64-lane workgroup per hub row: final (m, l) per head, the output row, the row's alpha
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    gatv2_fwd_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                           const IdxT* __restrict__ hub_cptr, int H, int C,
                           const float* __restrict__ part, float* __restrict__ alpha,
                           float* __restrict__ out) {
  __shared__ float sm[kAttnMaxHeads], sinv[kAttnMaxHeads];
  merge_softmax_row(rowptr, hub_rows, hub_cptr, static_cast<int64_t>(blockIdx.x), H, C, part,
                    alpha, out, sm, sinv, 0, static_cast<int64_t>(H) * C, true, nullptr);
}

// ---- backward, by destination -------------------------------------------------------------------
// d s[k,h] = alpha * (d alpha - D);  grad_x_r[i] = sum_k d pre;  grad_att += sum_k d s * lrelu(pre).
// SCORE: d alpha is given (the layer consumed alpha itself); otherwise d alpha = <grad_out, x_l[j]>
// and D = <grad_out[i,h,:], out[i,h,:]>.
template <typename IdxT, int EPL, bool VEC, bool SCORE>
__global__ void __launch_bounds__(kBlock)
    gatv2_bwd_dst_kernel(Items<IdxT> it, int64_t n_items, const IdxT* __restrict__ col,
                         const float* __restrict__ xl, const float* __restrict__ xr,
                         const float* __restrict__ att, const float* __restrict__ alpha,
                         const float* __restrict__ gout, const float* __restrict__ outp,
                         const float* __restrict__ galpha, int H, int C, int lph, float slope,
                         float* __restrict__ ds, float* __restrict__ gxr,
                         float* __restrict__ part, float* __restrict__ att_part) {
  constexpr int U = InFlight<EPL>::src;
  __shared__ __attribute__((aligned(16))) float sm[kWavesPerBlock][kMaxWidth];
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float a[EPL], ga[EPL];
  load_row<EPL, VEC>(att, L, a);
#pragma unroll
  for (int e = 0; e < EPL; ++e) ga[e] = 0.f;
  const int64_t stride = static_cast<int64_t>(gridDim.x) * kWavesPerBlock;
  for (int64_t item = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
       item < n_items; item += stride) {
    Span s;
    if (!decode(it, item, s)) continue;
    float r[EPL], g[EPL], gr[EPL];
    load_row<EPL, VEC>(xr + s.row * W, L, r);
    float D = 0.f;
    if constexpr (SCORE) {
      if (L.head_ok) {
        for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
          D = fmaf(alpha[k * H + L.h], galpha[k * H + L.h], D);
      }
#pragma unroll
      for (int e = 0; e < EPL; ++e) g[e] = 0.f;
    } else {
      float o[EPL];
      load_row<EPL, VEC>(gout + s.row * W, L, g);
      load_row<EPL, VEC>(outp + s.row * W, L, o);
#pragma unroll
      for (int e = 0; e < EPL; ++e) D = fmaf(g[e], o[e], D);
    }
    D = group_sum(D, lph);
#pragma unroll
    for (int e = 0; e < EPL; ++e) gr[e] = 0.f;
    for (int64_t k = s.k0; k < s.k1; k += U) {
      float v[U][EPL];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (k + u < s.k1) {
          const int64_t j = static_cast<int64_t>(col[k + u]);
          load_row<EPL, VEC>(xl + j * W, L, v[u]);
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
            for (int e = 0; e < EPL; ++e) da = fmaf(g[e], v[u][e], da);
            da = group_sum(da, lph);
          }
          const float al = L.head_ok ? alpha[(k + u) * H + L.h] : 0.f;
          const float d = al * (da - D);
          if (L.head_ok && L.sub == 0) ds[(k + u) * H + L.h] = d;
#pragma unroll
          for (int e = 0; e < EPL; ++e) {
            const float t = v[u][e] + r[e];
            const bool pos = t > 0.f;
            gr[e] = fmaf(d * a[e], pos ? 1.f : slope, gr[e]);
            ga[e] = fmaf(d, pos ? t : t * slope, ga[e]);
          }
        }
      }
    }
    store_row<EPL, VEC>(s.chunk_id >= 0 ? part + s.chunk_id * W : gxr + s.row * W, L, gr);
  }
  // att gradient: per wave -> per workgroup (fixed order) -> one row of the partials buffer
  store_row<EPL, VEC>(sm[threadIdx.x >> 6], L, ga);
  __syncthreads();
  for (int t = threadIdx.x; t < W; t += kBlock) {
    float acc = sm[0][t];
#pragma unroll
    for (int w = 1; w < kWavesPerBlock; ++w) acc += sm[w][t];
    att_part[static_cast<int64_t>(blockIdx.x) * W + t] = acc;
  }
}

// ---- backward, by source ---------------------------------------------------------------------
// grad_x_l[j] = sum over the edges j -> i of alpha * grad_out[i] (not in SCORE mode) + d pre.
template <typename IdxT, int EPL, bool VEC, bool SCORE>
__global__ void __launch_bounds__(kBlock)
    gatv2_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                         const IdxT* __restrict__ slot_map, const float* __restrict__ xl,
                         const float* __restrict__ xr, const float* __restrict__ att,
                         const float* __restrict__ alpha, const float* __restrict__ ds,
                         const float* __restrict__ gout, int H, int C, int lph, float slope,
                         float* __restrict__ gxl, float* __restrict__ part) {
  constexpr int U = InFlight<EPL>::src;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float a[EPL], v[EPL], acc[EPL];
  load_row<EPL, VEC>(att, L, a);
  load_row<EPL, VEC>(xl + s.row * W, L, v);
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  for (int64_t q = s.k0; q < s.k1; q += U) {
    float r[U][EPL], g[SCORE ? 1 : U][EPL];
    float al[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
        const int64_t i = static_cast<int64_t>(col_t[q + u]);
        const int64_t kd = static_cast<int64_t>(slot_map[q + u]);
        load_row<EPL, VEC>(xr + i * W, L, r[u]);
        if constexpr (!SCORE) load_row<EPL, VEC>(gout + i * W, L, g[u]);
        al[u] = (!SCORE && L.head_ok) ? alpha[kd * H + L.h] : 0.f;
        d[u] = L.head_ok ? ds[kd * H + L.h] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
#pragma unroll
        for (int e = 0; e < EPL; ++e) {
          const float t = v[e] + r[u][e];
          acc[e] = fmaf(d[u] * a[e], t > 0.f ? 1.f : slope, acc[e]);
          if constexpr (!SCORE) acc[e] = fmaf(al[u], g[u][e], acc[e]);
        }
      }
    }
  }
  store_row<EPL, VEC>(s.chunk_id >= 0 ? part + s.chunk_id * W : gxl + s.row * W, L, acc);
}

// ---- host side -------------------------------------------------------------------------------
size_t gv2_ws_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  const int64_t W = H * C;
  return sizeof(float) * static_cast<size_t>(n_chunks * (W + 2 * H) + kGv2MaxBlocks * W);
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_gatv2_supported(int64_t H, int64_t C) {
  Shape s;
  return choose_shape(H, C, false, &s) ? 1 : 0;
}

int pygamd_gatv2_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C, size_t* bytes) {
  if (!bytes || n_chunks < 0 || H < 1 || C < 1) return PYGAMD_ERR_INVALID_ARG;
  if (H * C > kMaxWidth || H > kAttnMaxHeads) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = gv2_ws_bytes(n_chunks, H, C);
  return PYGAMD_OK;
}

int pygamd_gatv2_forward(const pygamd_csr* g, const float* x_l, const float* x_r, const float* att,
                         int64_t n_src, int64_t H, int64_t C, float slope, float* alpha, float* out,
                         void* workspace, size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !x_l || !x_r || !att || !alpha) return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < gv2_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(x_l) && aligned16(x_r) && aligned16(att) && aligned16(workspace) &&
                  (!out || aligned16(out)) && (H % 2 == 0 || n_chunks == 0);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (out) {
        hipLaunchKernelGGL((gatv2_fwd_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st, it, c,
                           x_l, x_r, att, static_cast<int>(H), static_cast<int>(C), sh.lph, slope,
                           alpha, out, part);
      } else {
        hipLaunchKernelGGL((gatv2_fwd_kernel<IdxT, EPL, VEC, false>), grid, block, 0, st, it, c,
                           x_l, x_r, att, static_cast<int>(H), static_cast<int>(C), sh.lph, slope,
                           alpha, out, part);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((gatv2_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.rowptr, it.hub_rows, it.hub_cptr,
                         static_cast<int>(H), static_cast<int>(C), part, alpha, out);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_gatv2_backward_dst(const pygamd_csr* g, const float* x_l, const float* x_r,
                              const float* att, const float* alpha, const float* grad_out,
                              const float* out, const float* grad_alpha, int64_t n_src, int64_t H,
                              int64_t C, float slope, float* grad_s, float* grad_x_r,
                              float* grad_att, void* workspace, size_t workspace_bytes,
                              void* stream) {
  const int rc = check_args(g, n_src, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_chunks = g->n_chunks;
  if (!grad_att) return PYGAMD_ERR_INVALID_ARG;
  // exactly one of (grad_out, out) and grad_alpha says where d alpha comes from
  const bool score = grad_alpha != nullptr;
  if (score ? (grad_out || out) : (!grad_out || !out)) return PYGAMD_ERR_INVALID_ARG;
  hipStream_t st = as_stream(stream);
  const int64_t W = H * C;
  if (n_rows == 0) {
    PYGAMD_HIP_CHECK(hipMemsetAsync(grad_att, 0, sizeof(float) * W, st));
    return PYGAMD_OK;
  }
  if (!g->rowptr || !g->col || !x_l || !x_r || !att || !alpha || !grad_s || !grad_x_r)
    return PYGAMD_ERR_INVALID_ARG;
  if (!workspace || workspace_bytes < gv2_ws_bytes(n_chunks, H, C)) return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(x_l) && aligned16(x_r) && aligned16(att) && aligned16(workspace) &&
                  aligned16(grad_x_r) && (score || (aligned16(grad_out) && aligned16(out)));
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  float* part = static_cast<float*>(workspace);
  float* att_part = part + n_chunks * W;
  const int64_t n_items = n_rows + n_chunks;
  int64_t blocks = wave_grid(n_items);
  if (blocks > kGv2MaxBlocks) blocks = kGv2MaxBlocks;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(static_cast<unsigned>(blocks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      if (score) {
        hipLaunchKernelGGL((gatv2_bwd_dst_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st, it,
                           n_items, c, x_l, x_r, att, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, slope, grad_s,
                           grad_x_r, part, att_part);
      } else {
        hipLaunchKernelGGL((gatv2_bwd_dst_kernel<IdxT, EPL, VEC, false>), grid, block, 0, st, it,
                           n_items, c, x_l, x_r, att, alpha, grad_out, out, grad_alpha,
                           static_cast<int>(H), static_cast<int>(C), sh.lph, slope, grad_s,
                           grad_x_r, part, att_part);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    const int rc = launch_sum_merge(it, W, part, grad_x_r, st);
    if (rc != PYGAMD_OK) return rc;
    // (the workgroups' att partials in workgroup order; no bias block)
    return launch_param_reduce(att_part, static_cast<unsigned>(blocks), static_cast<int>(W), 0,
                               grad_att, nullptr, st);
  });
}

int pygamd_gatv2_backward_src(const pygamd_csr* g, const void* slot_map, const float* x_l,
                              const float* x_r, const float* att, const float* alpha,
                              const float* grad_s, const float* grad_out, int64_t n_dst, int64_t H,
                              int64_t C, float slope, float* grad_x_l, void* workspace,
                              size_t workspace_bytes, void* stream) {
  const int rc = check_args(g, n_dst, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_src = g->n_rows, n_chunks = g->n_chunks;
  if (n_src == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !slot_map || !x_l || !x_r || !att || !alpha || !grad_s || !grad_x_l)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < gv2_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(x_l) && aligned16(x_r) && aligned16(att) && aligned16(workspace) &&
                  aligned16(grad_x_l) && (!grad_out || aligned16(grad_out));
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
      if (!grad_out) {
        hipLaunchKernelGGL((gatv2_bwd_src_kernel<IdxT, EPL, VEC, true>), grid, block, 0, st, it,
                           c, sm, x_l, x_r, att, alpha, grad_s, grad_out, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, slope, grad_x_l, part);
      } else {
        hipLaunchKernelGGL((gatv2_bwd_src_kernel<IdxT, EPL, VEC, false>), grid, block, 0, st, it,
                           c, sm, x_l, x_r, att, alpha, grad_s, grad_out, static_cast<int>(H),
                           static_cast<int>(C), sh.lph, slope, grad_x_l, part);
      }
    });
    PYGAMD_LAUNCH_CHECK();
    return launch_sum_merge(it, W, part, grad_x_l, st);
  });
}

}  // extern "C"

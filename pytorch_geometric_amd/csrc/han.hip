// han.hip — HAN's node-level attention (nn/conv/han_conv.py:170-179 of the reference: GAT's additive
// score, the softmax per destination and the 'add' aggregation) for EVERY edge type of a layer call
// in one launch, as row-gather kernels on a stacked by-destination handle.
//
// Stacked graph: row r = row_begin[e] + i is destination i of edge type e (dense: an empty
// neighbourhood is an empty row), column c = src_begin[e] + j is source j of edge type e.  The
// per-node logits a_src [n_cols, H] and a_dst [n_rows, H] are stacked the same way, so a slot reads
// a_src[col] directly; the projected features live ONCE per node type in x_all, and the row a
// column reads is x_all[col + val_shift[e]] — a node type that feeds several edge types is never
// copied.  (row_begin, val_shift) travel in the kernel arguments as a by-value table of at most 64
// entries; a wave finds its edge type by a binary search over it (the row id is wave-uniform).
//
//   s[k,h]    = leaky_relu(a_src[col[k],h] + a_dst[r,h])
//   alpha     = softmax over the row (online: maximum subtracted, 1e-16 on the denominator)
//   out[r,h]  = relu?(sum_k alpha[k,h] * x_all[col[k] + val_shift[e], h, :])
//
// ONE pass per row keeps a_dst[r] in registers and gathers every source row once; nothing of size
// E x H*C is written.  Lane layout, work items and the in-order sum merge of the chunks of a
// long row: rowwalk_device.h.  Online softmax, non-finite rules and its merge: attn_device.h.  No
// float atomics: every result is bitwise reproducible.
#include <math.h>

#include "attn_device.h"
#include "common.h"

namespace pygamd {
namespace {

using namespace rowwalk;  // layout, work items and the sum merge: rowwalk_device.h
using namespace attn;     // online softmax and its merge: attn_device.h

constexpr int kHanMaxTypes = 64;

// by value in the kernel arguments (about 1 KB of the 4 KB there are)
struct HanTypes {
  int64_t row_begin[kHanMaxTypes + 1];  // stacked rows of edge type e: [row_begin[e], row_begin[e + 1])
  int64_t val_shift[kHanMaxTypes];      // column c of edge type e reads row c + val_shift[e] of x_all
  int32_t n_et;
};
static_assert(sizeof(HanTypes) <= 1056, "HanTypes must stay small");

// the edge type e with row_begin[e] <= row < row_begin[e + 1] (empty blocks are skipped)
__device__ __forceinline__ int han_type_of(const HanTypes& t, int64_t row) {
  int lo = 0, hi = t.n_et - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (t.row_begin[mid] <= row) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

template <int EPL>
struct InFlight {
  static constexpr int rows = EPL >= 16 ? 2 : 4;  // gathered rows in flight per wave
};

// torch.relu: NaN passes (v > 0 ? v : 0 would clear it)
__device__ __forceinline__ float relu_keep_nan(float v) { return v < 0.f ? 0.f : v; }

// ---- forward ---------------------------------------------------------------------------------
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    han_fwd_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const HanTypes tab,
                   const float* __restrict__ x, const float* __restrict__ a_src,
                   const float* __restrict__ a_dst, int H, int C, int lph, float slope, int relu,
                   float* __restrict__ alpha, float* __restrict__ out, float* __restrict__ part) {
  constexpr int U = InFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  const int64_t shift = tab.val_shift[han_type_of(tab, s.row)];
  const float ad = L.head_ok ? a_dst[s.row * H + L.h] : 0.f;
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float m = -INFINITY, l = 0.f;
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float v[U][EPL], as[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        as[u] = L.head_ok ? a_src[j * H + L.h] : 0.f;
        load_row<EPL, VEC>(x + (j + shift) * W, L, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const float t = as[u] + ad;
        const float p = t > 0.f ? t : t * slope;  // (every lane of a head holds the same score)
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
  const float inv = softmax_inv(m, l, s.k1 > s.k0);
#pragma unroll
  for (int e = 0; e < EPL; ++e) {
    acc[e] *= inv;
    if (relu) acc[e] = relu_keep_nan(acc[e]);
  }
  store_row<EPL, VEC>(out + s.row * W, L, acc);
  if (L.head_ok) {
    for (int64_t k = s.row_start + L.sub; k < s.row_end; k += lph)
      alpha[k * H + L.h] = expf(alpha[k * H + L.h] - m) * inv;
  }
}

// one 64-lane workgroup per hub row: final (m, l) per head, the output row, the row's alpha; the
// ReLU runs over the finished row (every lane reads back the elements it wrote itself)
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    han_fwd_merge_kernel(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ hub_rows,
                         const IdxT* __restrict__ hub_cptr, int H, int C, int relu,
                         const float* __restrict__ part, float* __restrict__ alpha,
                         float* __restrict__ out) {
  __shared__ float sm[kAttnMaxHeads], sinv[kAttnMaxHeads];
  const int64_t hr = static_cast<int64_t>(blockIdx.x);
  const int64_t W = static_cast<int64_t>(H) * C;
  merge_softmax_row(rowptr, hub_rows, hub_cptr, hr, H, C, part, alpha, out, sm, sinv, 0, W, true,
                    nullptr);
  if (!relu) return;
  float* row = out + static_cast<int64_t>(hub_rows[hr]) * W;
  for (int64_t t = threadIdx.x; t < W; t += kWave) row[t] = relu_keep_nan(row[t]);
}

// partial rows of a hub row summed in chunk order: a [W] row and, if wide2 > 0, a second [W2] row
template <typename IdxT>
__global__ void __launch_bounds__(kWave)
    han_sum_merge_kernel(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_cptr,
                         int64_t W, const float* __restrict__ part, float* __restrict__ dst,
                         int64_t W2, const float* __restrict__ part2, float* __restrict__ dst2) {
  const int64_t hr = static_cast<int64_t>(blockIdx.x);
  if (W > 0) merge_sum_row(hub_rows, hub_cptr, hr, W, part, W, dst, W);
  if (W2 > 0) merge_sum_row(hub_rows, hub_cptr, hr, W2, part2, W2, dst2, W2);
}

// the gradient row that reaches the aggregation: grad_out, masked by the ReLU's [out > 0]
template <int EPL, bool VEC>
__device__ __forceinline__ void load_grad(const float* __restrict__ gout,
                                          const float* __restrict__ outp, int64_t off, const Lay& L,
                                          int relu, float (&g)[EPL]) {
  load_row<EPL, VEC>(gout + off, L, g);
  if (relu) {
    float o[EPL];
    load_row<EPL, VEC>(outp + off, L, o);
#pragma unroll
    for (int e = 0; e < EPL; ++e) g[e] = o[e] > 0.f ? g[e] : 0.f;
  }
}

// ---- backward, by destination -------------------------------------------------------------------
// g = grad_out * [out > 0];  d alpha[k,h] = <g[r,h,:], x[j,h,:]>;  D = sum_k alpha d alpha =
// <g[r,h,:], out[r,h,:]> (where the mask is open, out is the weighted sum itself);
// grad_s[k,h] = alpha (d alpha - D) * leaky_relu'(a_src[j,h] + a_dst[r,h]);  grad_a_dst[r] = sum_k.
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    han_bwd_dst_kernel(Items<IdxT> it, const IdxT* __restrict__ col, const HanTypes tab,
                       const float* __restrict__ x, const float* __restrict__ a_src,
                       const float* __restrict__ a_dst, const float* __restrict__ alpha,
                       const float* __restrict__ gout, const float* __restrict__ outp, int H, int C,
                       int lph, float slope, int relu, float* __restrict__ ds,
                       float* __restrict__ ga_dst, float* __restrict__ part) {
  constexpr int U = InFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  const int64_t shift = tab.val_shift[han_type_of(tab, s.row)];
  const float ad = L.head_ok ? a_dst[s.row * H + L.h] : 0.f;
  float g[EPL];
  load_grad<EPL, VEC>(gout, outp, s.row * W, L, relu, g);
  float D = 0.f;
  {
    float o[EPL];
    load_row<EPL, VEC>(outp + s.row * W, L, o);
#pragma unroll
    for (int e = 0; e < EPL; ++e) D = fmaf(g[e], o[e], D);
  }
  D = group_sum(D, lph);
  float gd = 0.f;
  for (int64_t k = s.k0; k < s.k1; k += U) {
    float v[U][EPL], as[U], al[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        const int64_t j = static_cast<int64_t>(col[k + u]);
        as[u] = L.head_ok ? a_src[j * H + L.h] : 0.f;
        al[u] = L.head_ok ? alpha[(k + u) * H + L.h] : 0.f;
        load_row<EPL, VEC>(x + (j + shift) * W, L, v[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (k + u < s.k1) {
        float da = 0.f;
#pragma unroll
        for (int e = 0; e < EPL; ++e) da = fmaf(g[e], v[u][e], da);
        da = group_sum(da, lph);
        const float d = al[u] * (da - D) * (as[u] + ad > 0.f ? 1.f : slope);
        if (L.head_ok && L.sub == 0) ds[(k + u) * H + L.h] = d;
        gd += d;
      }
    }
  }
  if (L.head_ok && L.sub == 0)
    (s.chunk_id >= 0 ? part + s.chunk_id * H : ga_dst + s.row * H)[L.h] = gd;
}

// ---- backward, by source ---------------------------------------------------------------------
// rows are the stacked (edge type, source) columns of the forward:
// grad_a_src[c] = sum of grad_s over the edges c -> r;  grad_xv[c] = sum alpha * g[r].
template <typename IdxT, int EPL, bool VEC>
__global__ void __launch_bounds__(kBlock)
    han_bwd_src_kernel(Items<IdxT> it, const IdxT* __restrict__ col_t,
                       const IdxT* __restrict__ slot_map, const float* __restrict__ alpha,
                       const float* __restrict__ ds, const float* __restrict__ gout,
                       const float* __restrict__ outp, int H, int C, int lph, int relu,
                       float* __restrict__ ga_src, float* __restrict__ gxv,
                       float* __restrict__ part, float* __restrict__ part_h) {
  constexpr int U = InFlight<EPL>::rows;
  const int64_t item = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  Span s;
  if (!decode(it, item, s)) return;
  const Lay L = make_lay(H, C, lph);
  const int64_t W = static_cast<int64_t>(H) * C;
  float acc[EPL];
#pragma unroll
  for (int e = 0; e < EPL; ++e) acc[e] = 0.f;
  float gs = 0.f;
  for (int64_t q = s.k0; q < s.k1; q += U) {
    float g[U][EPL], al[U], d[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
        const int64_t r = static_cast<int64_t>(col_t[q + u]);
        const int64_t kd = static_cast<int64_t>(slot_map[q + u]);
        load_grad<EPL, VEC>(gout, outp, r * W, L, relu, g[u]);
        al[u] = L.head_ok ? alpha[kd * H + L.h] : 0.f;
        d[u] = L.head_ok ? ds[kd * H + L.h] : 0.f;
      }
    }
#pragma unroll
    for (int u = 0; u < U; ++u) {
      if (q + u < s.k1) {
        gs += d[u];
#pragma unroll
        for (int e = 0; e < EPL; ++e) acc[e] = fmaf(al[u], g[u][e], acc[e]);
      }
    }
  }
  store_row<EPL, VEC>(s.chunk_id >= 0 ? part + s.chunk_id * W : gxv + s.row * W, L, acc);
  if (L.head_ok && L.sub == 0)
    (s.chunk_id >= 0 ? part_h + s.chunk_id * H : ga_src + s.row * H)[L.h] = gs;
}

// ---- host side -------------------------------------------------------------------------------
size_t han_ws_bytes(int64_t n_chunks, int64_t H, int64_t C) {
  return sizeof(float) * static_cast<size_t>(n_chunks * (H * C + 2 * H));
}

// the by-value table from the caller's host arrays; the blocks must tile [0, n_rows)
int make_types(const int64_t* row_begin, const int64_t* val_shift, int64_t n_et, int64_t n_rows,
               HanTypes* t) {
  if (!row_begin || !val_shift || n_et < 1) return PYGAMD_ERR_INVALID_ARG;
  if (n_et > kHanMaxTypes) return PYGAMD_ERR_UNSUPPORTED;
  if (row_begin[0] != 0 || row_begin[n_et] != n_rows) return PYGAMD_ERR_INVALID_ARG;
  for (int64_t e = 0; e < n_et; ++e) {
    if (row_begin[e + 1] < row_begin[e]) return PYGAMD_ERR_INVALID_ARG;
    t->row_begin[e] = row_begin[e];
    t->val_shift[e] = val_shift[e];
  }
  for (int64_t e = n_et; e <= kHanMaxTypes; ++e) t->row_begin[e] = n_rows;
  for (int64_t e = n_et; e < kHanMaxTypes; ++e) t->val_shift[e] = 0;
  t->n_et = static_cast<int32_t>(n_et);
  return PYGAMD_OK;
}

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_han_supported(int64_t H, int64_t C) {
  Shape s;
  return choose_shape(H, C, false, &s) ? 1 : 0;
}

int pygamd_han_workspace_bytes(int64_t n_chunks, int64_t H, int64_t C, size_t* bytes) {
  if (!bytes || n_chunks < 0 || H < 1 || C < 1) return PYGAMD_ERR_INVALID_ARG;
  if (H * C > kMaxWidth || H > kAttnMaxHeads) return PYGAMD_ERR_UNSUPPORTED;
  *bytes = han_ws_bytes(n_chunks, H, C);
  return PYGAMD_OK;
}

int pygamd_han_forward(const pygamd_csr* g, const int64_t* row_begin, const int64_t* val_shift,
                       int64_t n_et, const float* x_all, const float* a_src, const float* a_dst,
                       int64_t n_cols, int64_t H, int64_t C, float slope, int relu, float* alpha,
                       float* out, void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_args(g, n_cols, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  HanTypes tab;
  rc = make_types(row_begin, val_shift, n_et, n_rows, &tab);
  if (rc != PYGAMD_OK) return rc;
  if (!g->rowptr || !g->col || !x_all || !a_src || !a_dst || !alpha || !out)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < han_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(x_all) && aligned16(out) && aligned16(workspace) &&
                  (H % 2 == 0 || n_chunks == 0);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((han_fwd_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, tab, x_all,
                         a_src, a_dst, static_cast<int>(H), static_cast<int>(C), sh.lph, slope,
                         relu, alpha, out, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((han_fwd_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.rowptr, it.hub_rows, it.hub_cptr,
                         static_cast<int>(H), static_cast<int>(C), relu, part, alpha, out);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_han_backward_dst(const pygamd_csr* g, const int64_t* row_begin,
                            const int64_t* val_shift, int64_t n_et, const float* x_all,
                            const float* a_src, const float* a_dst, const float* alpha,
                            const float* grad_out, const float* out, int64_t n_cols, int64_t H,
                            int64_t C, float slope, int relu, float* grad_s, float* grad_a_dst,
                            void* workspace, size_t workspace_bytes, void* stream) {
  int rc = check_args(g, n_cols, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_rows = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (n_rows == 0) return PYGAMD_OK;
  HanTypes tab;
  rc = make_types(row_begin, val_shift, n_et, n_rows, &tab);
  if (rc != PYGAMD_OK) return rc;
  if (!g->rowptr || !g->col || !x_all || !a_src || !a_dst || !alpha || !grad_out || !out ||
      !grad_s || !grad_a_dst)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < han_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(x_all) && aligned16(grad_out) && aligned16(out);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  float* part = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_rows + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((han_bwd_dst_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, tab,
                         x_all, a_src, a_dst, alpha, grad_out, out, static_cast<int>(H),
                         static_cast<int>(C), sh.lph, slope, relu, grad_s, grad_a_dst, part);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((han_sum_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, H, part, grad_a_dst,
                         static_cast<int64_t>(0), static_cast<const float*>(nullptr),
                         static_cast<float*>(nullptr));
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

int pygamd_han_backward_src(const pygamd_csr* g, const void* slot_map, const float* alpha,
                            const float* grad_s, const float* grad_out, const float* out,
                            int64_t n_dst, int64_t H, int64_t C, int relu, float* grad_a_src,
                            float* grad_xv, void* workspace, size_t workspace_bytes,
                            void* stream) {
  const int rc = check_args(g, n_dst, H, C);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n_cols = g->n_rows, n_hub = g->n_hub, n_chunks = g->n_chunks;
  if (n_cols == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col || !slot_map || !alpha || !grad_s || !grad_out || !out ||
      !grad_a_src || !grad_xv)
    return PYGAMD_ERR_INVALID_ARG;
  if (n_chunks > 0 && (!workspace || workspace_bytes < han_ws_bytes(n_chunks, H, C)))
    return PYGAMD_ERR_WORKSPACE;
  Shape sh;
  const bool al = aligned16(grad_out) && aligned16(out) && aligned16(grad_xv) &&
                  aligned16(workspace);
  if (!choose_shape(H, C, al, &sh)) return PYGAMD_ERR_UNSUPPORTED;
  hipStream_t st = as_stream(stream);
  const int64_t W = H * C;
  float* part = static_cast<float*>(workspace);
  float* part_h = part + n_chunks * W;
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    const Items<IdxT> it = make_items<IdxT>(*g);
    const dim3 grid(wave_grid(n_cols + n_chunks)), block(kBlock);
    const IdxT* c = typed_col<IdxT>(*g);
    const IdxT* sm = static_cast<const IdxT*>(slot_map);
    ROWWALK_DISPATCH_SHAPE(sh, {
      hipLaunchKernelGGL((han_bwd_src_kernel<IdxT, EPL, VEC>), grid, block, 0, st, it, c, sm,
                         alpha, grad_s, grad_out, out, static_cast<int>(H), static_cast<int>(C),
                         sh.lph, relu, grad_a_src, grad_xv, part, part_h);
    });
    PYGAMD_LAUNCH_CHECK();
    if (n_hub > 0) {
      hipLaunchKernelGGL((han_sum_merge_kernel<IdxT>), dim3(static_cast<unsigned>(n_hub)),
                         dim3(kWave), 0, st, it.hub_rows, it.hub_cptr, W, part, grad_xv, H, part_h,
                         grad_a_src);
      PYGAMD_LAUNCH_CHECK();
    }
    return PYGAMD_OK;
  });
}

}  // extern "C"

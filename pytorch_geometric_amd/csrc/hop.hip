// hop.hip — one step of a linear propagation x <- A^ x with the combination of the iterates as the
// row epilogue (APPNP, SGConv, SSGConv, TAGConv, LGConv, GCN2Conv; see include/pyg_amd.h):
//
//   t[i,:]   = sum_k (w ? w[e(k)] : 1) x[col[k],:]
//   out[i,:] = a t[i,:] (+ b y[i,:]) (+ c z[i,:]),   sum[i,:] = (sum_init ? 0 : sum[i,:]) + d out[i,:]
//
// The gather is the row walk of spmm.hip (spmm_device.h: one wave per row or per group of rows,
// 64 column ids per coalesced load, U row loads in flight, registers in slot order); what is new
// is the epilogue: the rows of y, z and the old sum are requested BEFORE the gather loop and
// arrive under it, and the [N, F] plane is written once instead of being re-read and re-written
// by three elementwise launches.  Rows longer than hub_threshold go through hop_hub_chunks /
// hop_hub_merge: the chunks' partial sums into the workspace, then one wave per hub row adds them
// in chunk order and applies the epilogue once.
//
// `out` is stored with plain stores: it is the plane the next step gathers (spmm_sum_rows, whose
// output is consumed by a dense product, streams its stores).  PYGAMD_HOP_NT_STORE builds the
// streamed form for the comparison in profiles/propagate_hops.md.
//
// out may be the same plane as y or z: a lane reads its columns of a row before it writes them
// and no other lane touches them; hence no __restrict__ on the epilogue pointers.
#include "common.h"

#include "spmm_device.h"

namespace pygamd {
namespace {

struct HopEpilogue {
  const float* y;
  const float* z;
  float* out;
  float* sum;
  int64_t ldy, ldz, ldo, lds;
  float a, b, c, d;
  int sum_init;
};

// Separately rounded products and sums, as the elementwise chain this replaces: contraction is
// switched off for these two functions (hipcc contracts a * b + c by default, and the _rn
// arithmetic functions of the HIP headers are plain operators that it contracts too).
__device__ __forceinline__ float hop_combine(float t, float a, bool has_y, float y, float b,
                                             bool has_z, float z, float c) {
#pragma clang fp contract(off)
  float o = a * t;
  if (has_y) o = o + b * y;
  if (has_z) o = o + c * z;
  return o;
}

__device__ __forceinline__ float hop_running_sum(float old, float d, float o) {
#pragma clang fp contract(off)
  return old + d * o;
}

__device__ __forceinline__ void hop_store_out(float o, float* p) {
#ifdef PYGAMD_HOP_NT_STORE
  __builtin_nontemporal_store(o, p);
#else
  *p = o;
#endif
}

template <typename IdxT, int VW, int LPR, int CH, int WMODE>
__global__ void __launch_bounds__(kBlock) hop_rows(SpmmDev<IdxT> a, HopEpilogue e) {
  const int lane = lane_id();
  const int64_t row = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  if (row >= a.n_rows) return;
  const IdxT start = a.rowptr[row];
  const IdxT end = a.rowptr[row + 1];
  if (a.hub_threshold > 0 && end - start > a.hub_threshold) return;  // owned by the hub path
  int fo[CH], head[CH];
  bool fv[CH];
  feature_slots<VW, LPR, CH>(lane, a.F, a.head_dim, fo, fv, head);
  float acc[CH][VW];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VW; ++i) acc[c][i] = 0.f;
  }
  // the epilogue operands do not depend on the sum: requested here, they arrive under the gather
  const bool has_y = e.y != nullptr, has_z = e.z != nullptr;
  const bool has_old = e.sum != nullptr && !e.sum_init;
  Vec<VW> yv[CH], zv[CH], sv[CH];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VW; ++i) {
      yv[c].v[i] = 0.f;
      zv[c].v[i] = 0.f;
      sv[c].v[i] = 0.f;
    }
    if (lane < LPR && fv[c]) {
      if (has_y) yv[c] = load_vec_streamed<VW>(e.y + row * e.ldy + fo[c]);
      if (has_z) zv[c] = load_vec_streamed<VW>(e.z + row * e.ldz + fo[c]);
      if (has_old) sv[c] = load_vec_streamed<VW>(e.sum + row * e.lds + fo[c]);
    }
  }
  spmm_accumulate<IdxT, VW, LPR, CH, WMODE, false>(a, start, end, lane, fo, fv, head, acc);
  combine_subgroups<VW, LPR, CH>(acc);
  if (lane < LPR) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (fv[c]) {
#pragma unroll
        for (int i = 0; i < VW; ++i) {
          const float o =
              hop_combine(acc[c][i], e.a, has_y, yv[c].v[i], e.b, has_z, zv[c].v[i], e.c);
          if (e.out) hop_store_out(o, e.out + row * e.ldo + fo[c] + i);
          if (e.sum) e.sum[row * e.lds + fo[c] + i] = hop_running_sum(sv[c].v[i], e.d, o);
        }
      }
    }
  }
}

// One wave per hub chunk: partial[ck, :] = the chunk's slots summed in slot order.
template <typename IdxT, int VW, int LPR, int CH, int WMODE>
__global__ void __launch_bounds__(kBlock)
    hop_hub_chunks(SpmmDev<IdxT> a, const IdxT* __restrict__ hub_rows,
                   const IdxT* __restrict__ hub_chunk_ptr, int64_t n_hub, int64_t n_chunks,
                   int64_t chunk, float* __restrict__ partial) {
  const int lane = lane_id();
  const int64_t ck = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  if (ck >= n_chunks) return;
  int64_t lo = 0, hi = n_hub;  // hub_chunk_ptr[lo] <= ck < hub_chunk_ptr[hi]
  while (hi - lo > 1) {
    const int64_t mid = (lo + hi) >> 1;
    if (static_cast<int64_t>(hub_chunk_ptr[mid]) <= ck) {
      lo = mid;
    } else {
      hi = mid;
    }
  }
  const int64_t row = hub_rows[lo];
  const int64_t ci = ck - static_cast<int64_t>(hub_chunk_ptr[lo]);
  const IdxT re = a.rowptr[row + 1];
  const IdxT start = a.rowptr[row] + static_cast<IdxT>(ci * chunk);
  IdxT end = start + static_cast<IdxT>(chunk);
  if (end > re) end = re;
  int fo[CH], head[CH];
  bool fv[CH];
  feature_slots<VW, LPR, CH>(lane, a.F, a.head_dim, fo, fv, head);
  float acc[CH][VW];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VW; ++i) acc[c][i] = 0.f;
  }
  spmm_accumulate<IdxT, VW, LPR, CH, WMODE, false>(a, start, end, lane, fo, fv, head, acc);
  combine_subgroups<VW, LPR, CH>(acc);
  if (lane < LPR) {
    float* __restrict__ prow = partial + ck * a.F;
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (fv[c]) {
#pragma unroll
        for (int i = 0; i < VW; ++i) prow[fo[c] + i] = acc[c][i];
      }
    }
  }
}

// One wave per hub row: the chunks' partial rows added in chunk order, then the epilogue, once.
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hop_hub_merge(const IdxT* __restrict__ hub_rows, const IdxT* __restrict__ hub_chunk_ptr,
                  int64_t n_hub, const float* __restrict__ partial, int64_t F, HopEpilogue e) {
  const int lane = lane_id();
  const int64_t h = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (h >= n_hub) return;
  const int64_t row = hub_rows[h];
  const int64_t c0 = hub_chunk_ptr[h];
  const int64_t c1 = hub_chunk_ptr[h + 1];
  const bool has_y = e.y != nullptr, has_z = e.z != nullptr;
  const bool has_old = e.sum != nullptr && !e.sum_init;
  for (int64_t f = lane; f < F; f += kWave) {
    const float yv = has_y ? e.y[row * e.ldy + f] : 0.f;
    const float zv = has_z ? e.z[row * e.ldz + f] : 0.f;
    const float sv = has_old ? e.sum[row * e.lds + f] : 0.f;
    float s = 0.f;
    int64_t c = c0;
    for (; c + 8 <= c1; c += 8) {  // eight chunks' loads in flight, added in chunk order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = partial[(c + u) * F + f];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < c1; ++c) s += partial[c * F + f];
    const float o = hop_combine(s, e.a, has_y, yv, e.b, has_z, zv, e.c);
    if (e.out) hop_store_out(o, e.out + row * e.ldo + f);
    if (e.sum) e.sum[row * e.lds + f] = hop_running_sum(sv, e.d, o);
  }
}

// ---- host side -------------------------------------------------------------------------------
template <typename IdxT>
SpmmDev<IdxT> hop_dev(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* p) {
  SpmmDev<IdxT> a = {};
  a.rowptr = static_cast<const IdxT*>(g->rowptr);
  a.col = static_cast<const IdxT*>(g->col);
  a.eid = static_cast<const IdxT*>(edge_id);
  a.w = p->w;
  a.x = p->x;
  a.n_src = p->n_src;
  a.n_rows = g->n_rows;
  a.F = p->F;
  a.ldx = p->ldx;
  a.w_heads = 1;
  a.head_dim = static_cast<int>(p->F < 0x7fffffff ? p->F : 0x7fffffff);
  a.hub_threshold = g->n_hub > 0 ? g->hub_threshold : 0;
  return a;
}

template <typename IdxT, int VW, int LPR, int CH, int WMODE>
int hop_launch(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* p,
               const HopEpilogue& e, const Shape& s, float* partial, hipStream_t st) {
  const SpmmDev<IdxT> a = hop_dev<IdxT>(g, edge_id, p);
  hipLaunchKernelGGL((hop_rows<IdxT, VW, LPR, CH, WMODE>), dim3(wave_grid(g->n_rows), s.tiles),
                     dim3(kBlock), 0, st, a, e);
  PYGAMD_LAUNCH_CHECK();
  if (g->n_hub > 0) {
    const IdxT* hub_rows = static_cast<const IdxT*>(g->hub_rows);
    const IdxT* hub_cptr = static_cast<const IdxT*>(g->hub_chunk_ptr);
    hipLaunchKernelGGL((hop_hub_chunks<IdxT, VW, LPR, CH, WMODE>),
                       dim3(wave_grid(g->n_chunks), s.tiles), dim3(kBlock), 0, st, a, hub_rows,
                       hub_cptr, g->n_hub, g->n_chunks, g->hub_chunk, partial);
    PYGAMD_LAUNCH_CHECK();
    hipLaunchKernelGGL((hop_hub_merge<IdxT>),
                       dim3(static_cast<unsigned>(ceil_div(g->n_hub, kWavesPerBlock))),
                       dim3(kBlock), 0, st, hub_rows, hub_cptr, g->n_hub, partial, p->F, e);
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

template <typename IdxT, int VW, int LPR, int CH>
int hop_launch_w(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* p,
                 const HopEpilogue& e, const Shape& s, float* partial, hipStream_t st) {
  return p->w ? hop_launch<IdxT, VW, LPR, CH, 1>(g, edge_id, p, e, s, partial, st)
              : hop_launch<IdxT, VW, LPR, CH, 0>(g, edge_id, p, e, s, partial, st);
}

template <typename IdxT, int VW>
int hop_launch_vw(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* p,
                  const HopEpilogue& e, const Shape& s, float* partial, hipStream_t st) {
  switch (s.lpr) {
    case 4:
      return hop_launch_w<IdxT, VW, 4, 1>(g, edge_id, p, e, s, partial, st);
    case 8:
      return hop_launch_w<IdxT, VW, 8, 1>(g, edge_id, p, e, s, partial, st);
    case 16:
      return hop_launch_w<IdxT, VW, 16, 1>(g, edge_id, p, e, s, partial, st);
    case 32:
      return hop_launch_w<IdxT, VW, 32, 1>(g, edge_id, p, e, s, partial, st);
    default:
      return s.ch == 2 ? hop_launch_w<IdxT, VW, 64, 2>(g, edge_id, p, e, s, partial, st)
                       : hop_launch_w<IdxT, VW, 64, 1>(g, edge_id, p, e, s, partial, st);
  }
}

bool hop_plane_v4(const float* p, int64_t ld) { return !p || (aligned16(p) && ld % 4 == 0); }

}  // namespace
}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_hop_workspace_size(int64_t n_chunks, int64_t F, size_t* bytes) {
  if (!bytes || n_chunks < 0 || F < 1) return PYGAMD_ERR_INVALID_ARG;
  *bytes = sizeof(float) * static_cast<size_t>(n_chunks) * static_cast<size_t>(F);
  return PYGAMD_OK;
}

int pygamd_hop(const pygamd_csr* g, const void* edge_id, const pygamd_hop_args* p,
               void* workspace, size_t workspace_bytes, void* stream) {
  if (!g || !p) return PYGAMD_ERR_INVALID_ARG;
  if (g->idx_dtype != PYGAMD_IDX_I32 && g->idx_dtype != PYGAMD_IDX_I64)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->reserved0 != 0 || g->n_rows < 0 || g->n_hub < 0 || g->n_chunks < 0)
    return PYGAMD_ERR_INVALID_ARG;
  for (int i = 0; i < 4; ++i) {
    if (p->reserved[i] != 0) return PYGAMD_ERR_INVALID_ARG;
  }
  if (p->F < 1 || p->n_src < 0 || !p->x || (!p->out && !p->sum)) return PYGAMD_ERR_INVALID_ARG;
  if (p->sum_init != 0 && p->sum_init != 1) return PYGAMD_ERR_INVALID_ARG;
  if (p->ldx < p->F || (p->y && p->ldy < p->F) || (p->z && p->ldz < p->F) ||
      (p->out && p->ldo < p->F) || (p->sum && p->lds < p->F))
    return PYGAMD_ERR_INVALID_ARG;
  // a row of out / sum is written while other rows still gather x; out and sum differ by d
  if ((p->out && p->out == p->x) || (p->sum && p->sum == p->x) || (p->out && p->out == p->sum))
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub > 0) {
    if (!g->hub_rows || !g->hub_chunk_ptr || g->hub_threshold < 1 || g->hub_chunk < 1 ||
        g->n_chunks < 1)
      return PYGAMD_ERR_INVALID_ARG;
    if (!workspace || workspace_bytes < sizeof(float) * static_cast<size_t>(g->n_chunks) *
                                            static_cast<size_t>(p->F))
      return PYGAMD_ERR_WORKSPACE;
  }
  if (g->n_rows == 0) return PYGAMD_OK;
  if (!g->rowptr || !g->col) return PYGAMD_ERR_INVALID_ARG;
  const bool v4 = p->F % 4 == 0 && hop_plane_v4(p->x, p->ldx) && hop_plane_v4(p->y, p->ldy) &&
                  hop_plane_v4(p->z, p->ldz) && hop_plane_v4(p->out, p->ldo) &&
                  hop_plane_v4(p->sum, p->lds);
  const Shape s = spmm_shape(p->F, v4);
  HopEpilogue e;
  e.y = p->y;
  e.z = p->z;
  e.out = p->out;
  e.sum = p->sum;
  e.ldy = p->ldy;
  e.ldz = p->ldz;
  e.ldo = p->ldo;
  e.lds = p->lds;
  e.a = p->a;
  e.b = p->b;
  e.c = p->c;
  e.d = p->d;
  e.sum_init = p->sum_init;
  hipStream_t st = as_stream(stream);
  float* partial = static_cast<float*>(workspace);
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    return s.vw == 4 ? hop_launch_vw<IdxT, 4>(g, edge_id, p, e, s, partial, st)
                     : hop_launch_vw<IdxT, 1>(g, edge_id, p, e, s, partial, st);
  });
}

}  // extern "C"

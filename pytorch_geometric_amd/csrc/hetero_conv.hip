// hetero_conv.hip — the typed aggregation of nn.HeteroConv over SAGEConv for gfx950 (MI355X).
//
// A heterogeneous layer aggregates one neighbourhood per (edge type, destination) pair, and the
// features it reads live in one matrix per NODE type.  The per-edge-type loop costs one SpMM launch
// per edge type forward and one backward; on sampled batches those launches are the whole cost.
// Here every edge type of a layer shares ONE stacked CSR (rows = (edge type, destination), dense:
// an empty neighbourhood is an empty row; col = the typed local source id) and one launch:
//
//   pygamd_hetero_spmm            one wavefront per stacked row.  The per-edge-type operands (source
//                                 matrix, pitch, row count, mean / sum, output block) travel in the
//                                 kernel arguments as a by-value table of at most 64 entries; the
//                                 wave finds its edge type by a binary search of row_begin (scalar
//                                 loads: the row id is wave-uniform), fills a local SpmmDev with that
//                                 type's operands and runs spmm_device.h's spmm_accumulate: slot
//                                 ids staged 64 at a time, 16-byte row loads, several in flight.
//                                 Lane shape and mean epilogue are those of pygamd_spmm_csr, so a
//                                 row's result equals that kernel's bit for bit whenever both run
//                                 the same shape.  The shape depends on F and on the alignment of
//                                 the rows: ONE shape per launch, picked from the least aligned
//                                 operand of the table.
//   pygamd_hetero_spmm_backward   one wavefront per stacked SOURCE node over the transposed
//                                 structure: every slot names a stacked (edge type, destination)
//                                 row; the lane that stages the slot finds the row's edge type,
//                                 the address of that row in the edge type's gradient matrix and
//                                 1 / max(deg, 1) where the type aggregates by mean; the rows are
//                                 then read like the forward's.  No floating-point atomics: the
//                                 order of a row's sum is the order of the sorted structure.
//
// Rows of any degree are correct.  There is no two-stage hub path here: a row above the SpMM's
// hub threshold is walked by its one wave (sampled batches bound the degree by the fan-out).
#include "common.h"

#include "spmm_device.h"

namespace pygamd {

constexpr int kMaxHeteroTypes = 64;

struct HeteroSpmmTable {
  int64_t row_begin[kMaxHeteroTypes + 1];  // stacked rows of edge type et: [row_begin[et], row_begin[et + 1])
  const float* x[kMaxHeteroTypes];         // source matrix of the edge type's source node type
  float* out[kMaxHeteroTypes];             // row 0 of the edge type's output block
  int64_t n_src[kMaxHeteroTypes];
  int32_t ldx[kMaxHeteroTypes];
  int32_t ldo[kMaxHeteroTypes];
  uint64_t mean_mask;                      // bit et: mean instead of sum
  int32_t n_et;
};
// kernel arguments are limited to about 4 KB
static_assert(sizeof(HeteroSpmmTable) <= 2592, "HeteroSpmmTable must stay small");

struct HeteroSpmmBwdTable {
  int64_t row_begin[kMaxHeteroTypes + 1];  // as above
  const float* grad[kMaxHeteroTypes];      // gradient of the edge type's output block
  int32_t ldg[kMaxHeteroTypes];
  uint64_t mean_mask;
  int64_t src_begin[kMaxHeteroTypes + 1];  // stacked source nodes of node type t
  float* grad_x[kMaxHeteroTypes];
  int32_t ldgx[kMaxHeteroTypes];
  int32_t n_et, n_nt;
};
static_assert(sizeof(HeteroSpmmBwdTable) <= 2600, "HeteroSpmmBwdTable must stay small");

// the block t with begin[t] <= i < begin[t + 1] (empty blocks are skipped); i < begin[n]
__device__ __forceinline__ int hetero_block_of(const int64_t* begin, int n, int64_t i) {
  int lo = 0, hi = n - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (begin[mid] <= i) {
      lo = mid;
    } else {
      hi = mid - 1;
    }
  }
  return lo;
}

template <typename IdxT, int VW, int LPR, int CH>
__global__ void __launch_bounds__(kBlock)
    hetero_spmm_rows(const IdxT* __restrict__ rowptr, const IdxT* __restrict__ col,
                     const HeteroSpmmTable tab, int64_t F, int32_t* __restrict__ err_flag) {
  const int lane = lane_id();
  const int64_t row = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  if (row >= tab.row_begin[tab.n_et]) return;
  const int et = hetero_block_of(tab.row_begin, tab.n_et, row);
  SpmmDev<IdxT> a = {};
  a.rowptr = rowptr;
  a.col = col;
  a.x = tab.x[et];
  a.ldx = tab.ldx[et];
  a.n_src = tab.n_src[et];
  const IdxT start = rowptr[row];
  IdxT end = rowptr[row + 1];
  const IdxT deg = end - start;
  bool bad = false;
  if (a.n_src <= 0) {  // no source row exists, not even row 0
    bad = deg > 0;
    end = start;
  }
  int fo[CH], head[CH];
  bool fv[CH];
  feature_slots<VW, LPR, CH>(lane, F, static_cast<int>(F), fo, fv, head);
  float acc[CH][VW];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VW; ++i) acc[c][i] = 0.f;
  }
  spmm_accumulate<IdxT, VW, LPR, CH, 0, false, 0, true>(a, start, end, lane, fo, fv, head, acc,
                                                        &bad);
  combine_subgroups<VW, LPR, CH>(acc);
  if (lane < LPR) {
    const bool mean = (tab.mean_mask >> et) & 1u;
    const float cntf = static_cast<float>(deg > 0 ? deg : 1);
    float* __restrict__ orow = tab.out[et] + (row - tab.row_begin[et]) * tab.ldo[et];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (fv[c]) {
        Vec<VW> o;
#pragma unroll
        for (int i = 0; i < VW; ++i) o.v[i] = mean ? acc[c][i] / cntf : acc[c][i];
        store_vec<VW>(orow + fo[c], o);
      }
    }
  }
  if (bad && err_flag) *err_flag = 1;
}

template <typename IdxT, int VW, int LPR, int CH>
__global__ void __launch_bounds__(kBlock)
    hetero_spmm_bwd_rows(const IdxT* __restrict__ rowptr_t, const IdxT* __restrict__ col_t,
                         const IdxT* __restrict__ rowptr, const HeteroSpmmBwdTable tab, int64_t F) {
  constexpr int EPI = kWave / LPR;
  constexpr int U = spmm_unroll<LPR, CH>();
  constexpr int STEP = EPI * U;
  const int lane = lane_id();
  const int sub = lane / LPR;
  const int64_t j = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  if (j >= tab.src_begin[tab.n_nt]) return;
  const int nt = hetero_block_of(tab.src_begin, tab.n_nt, j);
  const int64_t n_rows = tab.row_begin[tab.n_et];
  const IdxT start = rowptr_t[j];
  const IdxT end = rowptr_t[j + 1];
  int fo[CH], head[CH];
  bool fv[CH];
  feature_slots<VW, LPR, CH>(lane, F, static_cast<int>(F), fo, fv, head);
  float acc[CH][VW];
#pragma unroll
  for (int c = 0; c < CH; ++c) {
#pragma unroll
    for (int i = 0; i < VW; ++i) acc[c][i] = 0.f;
  }
  for (IdxT base = start; base < end; base += kWave) {
    const IdxT rem = end - base;
    const int cnt = rem < kWave ? static_cast<int>(rem) : kWave;
    // lane l stages slot base + l: the address of its gradient row and its multiplier
    int64_t myp = 0;
    float mym = 0.f;
    if (lane < cnt) {
      int64_t r = static_cast<int64_t>(__builtin_nontemporal_load(&col_t[base + lane]));
      const bool ok = r >= 0 && r < n_rows;  // (a row id nobody vouches for contributes nothing)
      r = ok ? r : 0;
      const int et = hetero_block_of(tab.row_begin, tab.n_et, r);
      const float* g = tab.grad[et] + (r - tab.row_begin[et]) * tab.ldg[et];
      myp = static_cast<int64_t>(reinterpret_cast<uintptr_t>(g));
      mym = ok ? 1.f : 0.f;
      if ((tab.mean_mask >> et) & 1u) {
        const IdxT deg = rowptr[r + 1] - rowptr[r];
        mym /= static_cast<float>(deg > 0 ? deg : 1);
      }
    }
    for (int s = 0; s < cnt; s += STEP) {
      Vec<VW> v[U][CH];
      float m[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = s + u * EPI + sub;
        const bool valid = k < cnt;
        const int kk = valid ? k : cnt - 1;
        int64_t p;
        float mm;
        if constexpr (EPI == 1) {
          p = bcast_uniform(myp, kk);
          mm = bcast_uniform(mym, kk);
        } else {
          p = bcast_lane(myp, kk);
          mm = bcast_lane(mym, kk);
        }
        m[u] = valid ? mm : 0.f;
        const float* __restrict__ gr = reinterpret_cast<const float*>(static_cast<uintptr_t>(p));
#pragma unroll
        for (int c = 0; c < CH; ++c) {
          if (fv[c] && valid) {
            v[u][c] = load_vec<VW>(gr + fo[c]);
          } else {
#pragma unroll
            for (int i = 0; i < VW; ++i) v[u][c].v[i] = 0.f;
          }
        }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
#pragma unroll
        for (int c = 0; c < CH; ++c) {
#pragma unroll
          for (int i = 0; i < VW; ++i) acc[c][i] = fmaf(v[u][c].v[i], m[u], acc[c][i]);
        }
      }
    }
  }
  combine_subgroups<VW, LPR, CH>(acc);
  if (lane < LPR) {
    float* __restrict__ orow = tab.grad_x[nt] + (j - tab.src_begin[nt]) * tab.ldgx[nt];
#pragma unroll
    for (int c = 0; c < CH; ++c) {
      if (fv[c]) {
        Vec<VW> o;
#pragma unroll
        for (int i = 0; i < VW; ++i) o.v[i] = acc[c][i];
        store_vec<VW>(orow + fo[c], o);
      }
    }
  }
}

template <typename IdxT, int VW>
static int launch_hetero_fwd(const Shape& s, const void* rowptr, const void* col,
                             const HeteroSpmmTable& tab, int64_t F, int32_t* err_flag,
                             hipStream_t st) {
  dim3 grid(wave_grid(tab.row_begin[tab.n_et]), s.tiles);
  const IdxT* rp = static_cast<const IdxT*>(rowptr);
  const IdxT* cl = static_cast<const IdxT*>(col);
#define PYGAMD_HETERO_FWD(LPR, CH)                                                              \
  hipLaunchKernelGGL((hetero_spmm_rows<IdxT, VW, LPR, CH>), grid, dim3(kBlock), 0, st, rp, cl, \
                     tab, F, err_flag)
  switch (s.lpr) {
    case 4: PYGAMD_HETERO_FWD(4, 1); break;
    case 8: PYGAMD_HETERO_FWD(8, 1); break;
    case 16: PYGAMD_HETERO_FWD(16, 1); break;
    case 32: PYGAMD_HETERO_FWD(32, 1); break;
    default:
      if (s.ch == 2) {
        PYGAMD_HETERO_FWD(64, 2);
      } else {
        PYGAMD_HETERO_FWD(64, 1);
      }
  }
#undef PYGAMD_HETERO_FWD
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

template <typename IdxT, int VW>
static int launch_hetero_bwd(const Shape& s, const void* rowptr_t, const void* col_t,
                             const void* rowptr, const HeteroSpmmBwdTable& tab, int64_t F,
                             hipStream_t st) {
  dim3 grid(wave_grid(tab.src_begin[tab.n_nt]), s.tiles);
  const IdxT* rt = static_cast<const IdxT*>(rowptr_t);
  const IdxT* ct = static_cast<const IdxT*>(col_t);
  const IdxT* rp = static_cast<const IdxT*>(rowptr);
#define PYGAMD_HETERO_BWD(LPR, CH)                                                                 \
  hipLaunchKernelGGL((hetero_spmm_bwd_rows<IdxT, VW, LPR, CH>), grid, dim3(kBlock), 0, st, rt, ct, \
                     rp, tab, F)
  switch (s.lpr) {
    case 4: PYGAMD_HETERO_BWD(4, 1); break;
    case 8: PYGAMD_HETERO_BWD(8, 1); break;
    case 16: PYGAMD_HETERO_BWD(16, 1); break;
    case 32: PYGAMD_HETERO_BWD(32, 1); break;
    default:
      if (s.ch == 2) {
        PYGAMD_HETERO_BWD(64, 2);
      } else {
        PYGAMD_HETERO_BWD(64, 1);
      }
  }
#undef PYGAMD_HETERO_BWD
  PYGAMD_LAUNCH_CHECK();
  return PYGAMD_OK;
}

// a block table: n in [1, 64], begin[0] == 0, non-decreasing
static int check_blocks(const int64_t* begin, int n) {
  if (n > kMaxHeteroTypes) return PYGAMD_ERR_UNSUPPORTED;
  if (n <= 0 || !begin || begin[0] != 0) return PYGAMD_ERR_INVALID_ARG;
  for (int t = 0; t < n; ++t) {
    if (begin[t + 1] < begin[t]) return PYGAMD_ERR_INVALID_ARG;
  }
  return PYGAMD_OK;
}

static bool fits_ld(int64_t ld, int64_t F) { return ld >= F && ld <= INT32_MAX; }

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_hetero_spmm(const void* rowptr, const void* col, int idx_dtype,
                       const int64_t* row_begin, const float* const* x, float* const* out,
                       const int64_t* et_table, int n_et, int64_t F, int32_t* err_flag,
                       void* stream) {
  int rc = check_blocks(row_begin, n_et);
  if (rc != PYGAMD_OK) return rc;
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (F < 0 || !x || !out || !et_table) return PYGAMD_ERR_INVALID_ARG;
  HeteroSpmmTable tab = {};
  tab.n_et = n_et;
  tab.row_begin[0] = 0;
  bool v4 = (F % 4 == 0);
  for (int et = 0; et < n_et; ++et) {
    const int64_t ldx = et_table[4 * et], n_src = et_table[4 * et + 1];
    const int64_t mean = et_table[4 * et + 2], ldo = et_table[4 * et + 3];
    const int64_t rows = row_begin[et + 1] - row_begin[et];
    if (n_src < 0 || (mean != 0 && mean != 1) || !fits_ld(ldx, F) || !fits_ld(ldo, F))
      return PYGAMD_ERR_INVALID_ARG;
    if (rows > 0 && F > 0 && (!out[et] || (n_src > 0 && !x[et]))) return PYGAMD_ERR_INVALID_ARG;
    tab.row_begin[et + 1] = row_begin[et + 1];
    tab.x[et] = x[et];
    tab.out[et] = out[et];
    tab.n_src[et] = n_src;
    tab.ldx[et] = static_cast<int32_t>(ldx);
    tab.ldo[et] = static_cast<int32_t>(ldo);
    if (mean) tab.mean_mask |= 1ull << et;
    if (rows > 0)
      v4 = v4 && (ldx % 4 == 0) && (ldo % 4 == 0) && aligned16(x[et]) && aligned16(out[et]);
  }
  const int64_t n_rows = row_begin[n_et];
  if (n_rows == 0 || F == 0) return PYGAMD_OK;
  if (!rowptr) return PYGAMD_ERR_INVALID_ARG;  // (col may be NULL when nothing is stored)
  const Shape s = spmm_shape(F, v4);
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    return s.vw == 4 ? launch_hetero_fwd<IdxT, 4>(s, rowptr, col, tab, F, err_flag, st)
                     : launch_hetero_fwd<IdxT, 1>(s, rowptr, col, tab, F, err_flag, st);
  });
}

int pygamd_hetero_spmm_backward(const void* rowptr_t, const void* col_t, const void* rowptr,
                                int idx_dtype, const int64_t* row_begin,
                                const float* const* grad, const int64_t* et_table, int n_et,
                                const int64_t* src_begin, float* const* grad_x,
                                const int64_t* ld_grad_x, int n_nt, int64_t F, void* stream) {
  int rc = check_blocks(row_begin, n_et);
  if (rc != PYGAMD_OK) return rc;
  rc = check_blocks(src_begin, n_nt);
  if (rc != PYGAMD_OK) return rc;
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (F < 0 || !grad || !et_table || !grad_x || !ld_grad_x) return PYGAMD_ERR_INVALID_ARG;
  HeteroSpmmBwdTable tab = {};
  tab.n_et = n_et;
  tab.n_nt = n_nt;
  bool v4 = (F % 4 == 0);
  for (int et = 0; et < n_et; ++et) {
    const int64_t ldg = et_table[2 * et], mean = et_table[2 * et + 1];
    const int64_t rows = row_begin[et + 1] - row_begin[et];
    if ((mean != 0 && mean != 1) || !fits_ld(ldg, F)) return PYGAMD_ERR_INVALID_ARG;
    if (rows > 0 && F > 0 && !grad[et]) return PYGAMD_ERR_INVALID_ARG;
    tab.row_begin[et + 1] = row_begin[et + 1];
    tab.grad[et] = grad[et];
    tab.ldg[et] = static_cast<int32_t>(ldg);
    if (mean) tab.mean_mask |= 1ull << et;
    if (rows > 0) v4 = v4 && (ldg % 4 == 0) && aligned16(grad[et]);
  }
  for (int t = 0; t < n_nt; ++t) {
    const int64_t rows = src_begin[t + 1] - src_begin[t];
    if (!fits_ld(ld_grad_x[t], F)) return PYGAMD_ERR_INVALID_ARG;
    if (rows > 0 && F > 0 && !grad_x[t]) return PYGAMD_ERR_INVALID_ARG;
    tab.src_begin[t + 1] = src_begin[t + 1];
    tab.grad_x[t] = grad_x[t];
    tab.ldgx[t] = static_cast<int32_t>(ld_grad_x[t]);
    if (rows > 0) v4 = v4 && (ld_grad_x[t] % 4 == 0) && aligned16(grad_x[t]);
  }
  if (src_begin[n_nt] == 0 || F == 0) return PYGAMD_OK;
  if (!rowptr_t || !rowptr) return PYGAMD_ERR_INVALID_ARG;
  const Shape s = spmm_shape(F, v4);
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    return s.vw == 4 ? launch_hetero_bwd<IdxT, 4>(s, rowptr_t, col_t, rowptr, tab, F, st)
                     : launch_hetero_bwd<IdxT, 1>(s, rowptr_t, col_t, rowptr, tab, F, st);
  });
}

}  // extern "C"

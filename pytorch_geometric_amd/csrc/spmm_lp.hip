// spmm_lp.hip — the CSR aggregation over float16 / bfloat16 storage (pygamd_spmm_lp).
//
// The same HBM-bound gather as spmm.hip with half the bytes per source row: x and out are 16-bit,
// everything else (weights, accumulators, hub partials) is float32 and every output is rounded
// once, at its store.
//
// Mapping (wave64):
//   * a lane owns 8 consecutive columns: one 16-byte load = 8 elements = 8 float32 accumulators;
//     LPR = next_pow2(ceil(F / 8)) lanes (1 .. 64) cover a row of up to 512 columns, blockIdx.y
//     walks further column tiles;
//   * the 64 / LPR lane groups of a wave walk different slots of the same row and are folded at
//     the end by an xor butterfly (LPR, 2 LPR, .. 32: a fixed order);
//   * 64 slots' column id and float32 multiplier are staged one per lane and handed out by
//     v_readlane (LPR == 64) or ds_bpermute; U = min(LPR, 8) row loads per lane are issued before
//     the first add (spmm_lp_device.h, lp_unroll);
//   * the vector width is chosen per launch: 8 elements when F, both pitches and both pointers
//     are multiples of 16 bytes, 2 elements when they are multiples of 4 bytes, 1 otherwise;
//     the lane keeps its 8 columns at every width (1, 4 or 8 loads) and the columns past F are
//     predicated, never read;
//   * one launch serves rows and hub chunks: the lowest wave ids take the chunks of the hub plan
//     (float32 partials in the workspace), the others one row each; a second, small launch merges
//     the partials of every hub row in chunk order and narrows AFTER the merge.
// No LDS (nothing is reused between lanes: the staged slots travel by readlane / bpermute, the
// hub merge reads its partials straight from L2) and no matrix instructions (no operand is used
// twice).  No float atomics: results are bit-identical from run to run.
//
// Unroll per LPR and the VGPRs the compiler reports at the 16-byte width (hipcc -O3, gfx950; the
// larger of the int32 / int64 instantiation; all 260 kernels of this file: no spill, no scratch;
// every width and the weighted kernels: profiles/spmm_lp.md):
//     LPR   U   rows in flight   lp_sum_rows f16 / bf16   lp_minmax_rows f16 / bf16
//       1   1        64               28 / 24                  63 / 63
//       2   2        64               36 / 36                  84 / 85
//       4   4        64               46 / 52                  79 / 80
//       8   8        64               66 / 86                 103 / 103
//      16   8        32               66 / 82                  99 / 99
//      32   8        16               62 / 82                  95 / 96
//      64   8         8               60 / 80                  86 / 87
#include "common.h"

#include "spmm_lp_device.h"

namespace pygamd {

// SUM / MEAN.  W: a multiplier per slot (w and / or src_scale).
template <typename T, typename IdxT, int VW, int LPR, bool W>
__global__ void __launch_bounds__(kBlock) lp_sum_rows(LpDev<IdxT> a) {
  const int lane = lane_id();
  LpItem<IdxT> it;
  if (!lp_item(a, it)) return;
  uint32_t pm;
  const int fo = lp_columns<LPR>(lane, a.F, pm);
  float acc[kLpCols];
#pragma unroll
  for (int i = 0; i < kLpCols; ++i) acc[i] = 0.f;
  lp_accumulate<T, IdxT, VW, LPR, W>(a, it.start, it.end, lane, fo, pm, acc);
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) acc[i] += __shfl_xor(acc[i], off, kWave);
  }
  if (lane >= LPR) return;
  if (it.chunk >= 0) {  // a hub chunk: the float32 partial, no post-scale, no rounding
    float* __restrict__ prow = a.partial + it.chunk * a.F + fo;
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) {
      if ((pm >> i) & 1u) prow[i] = acc[i];
    }
    return;
  }
  if (a.mean) {
    const float cntf = static_cast<float>(it.deg > 0 ? it.deg : 1);
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) acc[i] = acc[i] / cntf;
  }
  lp_store<T, VW>(a.out + it.row * a.ldo + fo, pm, acc);
}

// One wave per hub row: out[row, :] = narrow(post * (chunk partials summed in chunk order)).
template <typename T, typename IdxT>
__global__ void __launch_bounds__(kBlock) lp_hub_sum(LpDev<IdxT> a) {
  const int lane = lane_id();
  const int64_t h = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (h >= a.n_hub) return;
  const int64_t row = a.hub_rows[h];
  const int64_t c0 = a.hub_chunk_ptr[h];
  const int64_t c1 = a.hub_chunk_ptr[h + 1];
  const IdxT deg = a.rowptr[row + 1] - a.rowptr[row];
  const float cntf = static_cast<float>(deg > 0 ? deg : 1);
  for (int64_t f = lane; f < a.F; f += kWave) {
    float s = 0.f;
    int64_t c = c0;
    for (; c + 8 <= c1; c += 8) {  // eight chunks' loads in flight, added in chunk order
      float v[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) v[u] = a.partial[(c + u) * a.F + f];
#pragma unroll
      for (int u = 0; u < 8; ++u) s += v[u];
    }
    for (; c < c1; ++c) s += a.partial[c * a.F + f];
    a.out[row * a.ldo + f] = lp_narrow<T>(a.mean ? s / cntf : s);
  }
}

// ---- min / max ------------------------------------------------------------------------------------
// Walked as a MAX over values whose sign bit is flipped for MIN (a.flip): the extremum is one of
// the inputs and is handed back bit for bit.  Per column: the extremum, the slot offset of its
// first occurrence, the low 32 bits of that occurrence's source row, and whether a DIFFERENT
// source row attains it too (parallel edges to one neighbour are no tie: spmm.hip,
// spmm_minmax_rows).  A NaN beats any non-NaN.
struct LpBest {
  float best;
  int32_t arg;  // -1: nothing met yet
  uint32_t src;
  bool tie;
};

// `o` holds later slots than `m` unless its arg says otherwise (the lane groups interleave)
__device__ __forceinline__ void lp_best_merge(LpBest& m, const LpBest& o) {
  const bool o_valid = o.arg >= 0, m_empty = m.arg < 0;
  const bool on = o.best != o.best, mn = m.best != m.best;
  const bool o_better = !mn & (on | (o.best > m.best));
  const bool m_better = !on & (mn | (m.best > o.best));
  const bool equal = o_valid & !m_empty & !o_better & !m_better;
  const bool take_new = o_valid & (m_empty | o_better);
  const bool take = take_new | (equal & (o.arg < m.arg));
  m.tie = equal ? (m.tie | o.tie | (o.src != m.src)) : (take_new ? o.tie : m.tie);
  m.best = take ? o.best : m.best;
  m.arg = take ? o.arg : m.arg;
  m.src = take ? o.src : m.src;
}

template <typename T, typename IdxT, int VW, int LPR>
__global__ void __launch_bounds__(kBlock) lp_minmax_rows(LpDev<IdxT> a) {
  constexpr int EPI = kWave / LPR;
  constexpr int U = lp_unroll<LPR>();
  constexpr int STEP = EPI * U;
  const int lane = lane_id();
  LpItem<IdxT> it;
  if (!lp_item(a, it)) return;
  uint32_t pm;
  const int fo = lp_columns<LPR>(lane, a.F, pm);
  const int sub = lane / LPR;
  LpBest b[kLpCols];
#pragma unroll
  for (int i = 0; i < kLpCols; ++i) b[i] = {-INFINITY, -1, 0u, false};
  for (IdxT base = it.start; base < it.end; base += kWave) {
    const IdxT rem = it.end - base;
    const int cnt = rem < kWave ? static_cast<int>(rem) : kWave;
    IdxT myc = 0;
    if (lane < cnt) myc = __builtin_nontemporal_load(&a.col[base + lane]);  // streamed once
    const int32_t off0 = it.off0 + static_cast<int32_t>(base - it.start);
    for (int j = 0; j < cnt; j += STEP) {
      LpRaw<VW> v[U];
      bool ok[U];
      uint32_t cs[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int k = j + u * EPI + sub;
        ok[u] = k < cnt;
        const IdxT c = lp_bcast<IdxT, LPR>(myc, ok[u] ? k : cnt - 1);
        cs[u] = static_cast<uint32_t>(c);
        lp_load<VW>(a.x + static_cast<int64_t>(c) * a.ldx + fo, pm, ok[u], v[u]);
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int32_t slot = off0 + (j + u * EPI + sub);
#pragma unroll
        for (int i = 0; i < kLpCols; ++i) {
          const float val = __uint_as_float(__float_as_uint(lp_widen<T, VW>(v[u], i)) ^ a.flip);
          const bool vn = val != val, bn = b[i].best != b[i].best;
          const bool gt = !bn & (vn | (val > b[i].best));
          const bool lt = !vn & (bn | (val < b[i].best));
          const bool has = b[i].arg >= 0;
          const bool take = ok[u] & (!has | gt);  // the first slot always wins over "nothing"
          b[i].tie = take ? false : (b[i].tie | (ok[u] & has & !lt & (cs[u] != b[i].src)));
          b[i].best = take ? val : b[i].best;
          b[i].arg = take ? slot : b[i].arg;
          b[i].src = take ? cs[u] : b[i].src;
        }
      }
    }
  }
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) {
      LpBest o;
      o.best = bcast_lane(b[i].best, lane ^ off);
      o.arg = bcast_lane(b[i].arg, lane ^ off);
      o.src = static_cast<uint32_t>(bcast_lane(static_cast<int32_t>(b[i].src), lane ^ off));
      o.tie = bcast_lane(static_cast<int32_t>(b[i].tie), lane ^ off) != 0;
      lp_best_merge(b[i], o);
    }
  }
  if (lane >= LPR) return;
  if (it.chunk >= 0) {
    const int64_t p0 = it.chunk * a.F + fo;
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) {
      if ((pm >> i) & 1u) {
        a.partial[p0 + i] = b[i].best;
        a.part_arg[p0 + i] = (b[i].tie && b[i].arg >= 0) ? -2 - b[i].arg : b[i].arg;
        a.part_src[p0 + i] = b[i].src;
      }
    }
    return;
  }
  float o[kLpCols];
#pragma unroll
  for (int i = 0; i < kLpCols; ++i)
    o[i] = b[i].arg < 0 ? 0.f : __uint_as_float(__float_as_uint(b[i].best) ^ a.flip);
  lp_store<T, VW>(a.out + it.row * a.ldo + fo, pm, o);
  if (a.arg32_out) {
    // -2: the gradient is split (several attaining neighbours, or an extremum of exactly 0, which
    // ties with the zero-initialised output of scatter_reduce_(include_self=False))
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) {
      if ((pm >> i) & 1u) {
        const bool split = b[i].tie | (b[i].best == 0.f);
        a.arg32_out[it.row * a.F + fo + i] = b[i].arg < 0 ? -1 : (split ? -2 : b[i].arg);
      }
    }
  }
}

// One wave per hub row: the chunk partials merged in chunk order (they carry their slot offset
// and first source, so arg32 comes out as if one wave had walked the row).
template <typename T, typename IdxT>
__global__ void __launch_bounds__(kBlock) lp_hub_minmax(LpDev<IdxT> a) {
  const int lane = lane_id();
  const int64_t h = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (h >= a.n_hub) return;
  const int64_t row = a.hub_rows[h];
  const int64_t c0 = a.hub_chunk_ptr[h];
  const int64_t c1 = a.hub_chunk_ptr[h + 1];
  for (int64_t f = lane; f < a.F; f += kWave) {
    LpBest m = {-INFINITY, -1, 0u, false};
    for (int64_t c = c0; c < c1; ++c) {
      const int32_t pa = a.part_arg[c * a.F + f];
      LpBest o;
      o.best = a.partial[c * a.F + f];
      o.src = a.part_src[c * a.F + f];
      o.tie = pa < -1;
      o.arg = pa < -1 ? -2 - pa : pa;
      lp_best_merge(m, o);
    }
    const float r = m.arg < 0 ? 0.f : __uint_as_float(__float_as_uint(m.best) ^ a.flip);
    a.out[row * a.ldo + f] = lp_narrow<T>(r);
    if (a.arg32_out) {
      const bool split = m.tie | (m.best == 0.f);
      a.arg32_out[row * a.F + f] = m.arg < 0 ? -1 : (split ? -2 : m.arg);
    }
  }
}

// ---- host ------------------------------------------------------------------------------------------
struct LpCall {
  const pygamd_csr* g;
  const void* eid;
  const float* w;
  const float* src_scale;
  const void* x;
  void* out;
  int64_t ldx, ldo, F;
  int reduce;
  int32_t* arg32_out;
  void* workspace;
  hipStream_t st;
};

static int lp_lanes(int64_t F) {
  const int64_t units = ceil_div(F, kLpCols);
  int lpr = 1;
  while (lpr < kWave && lpr < units) lpr <<= 1;
  return lpr;
}

static int lp_vector_width(const LpCall& c) {
  const uintptr_t px = reinterpret_cast<uintptr_t>(c.x), po = reinterpret_cast<uintptr_t>(c.out);
  if (c.F % 8 == 0 && c.ldx % 8 == 0 && c.ldo % 8 == 0 && ((px | po) & 15u) == 0) return 8;
  if (c.F % 2 == 0 && c.ldx % 2 == 0 && c.ldo % 2 == 0 && ((px | po) & 3u) == 0) return 2;
  return 1;
}

template <typename T, typename IdxT, int VW, int LPR>
static int lp_launch(const LpCall& c) {
  const pygamd_csr* g = c.g;
  LpDev<IdxT> a;
  a.rowptr = static_cast<const IdxT*>(g->rowptr);
  a.col = static_cast<const IdxT*>(g->col);
  a.eid = static_cast<const IdxT*>(c.eid);
  a.w = c.w;
  a.src_scale = c.src_scale;
  a.x = static_cast<const uint16_t*>(c.x);
  a.out = static_cast<uint16_t*>(c.out);
  a.arg32_out = c.arg32_out;
  a.n_rows = g->n_rows;
  a.F = c.F;
  a.ldx = c.ldx;
  a.ldo = c.ldo;
  a.mean = c.reduce == PYGAMD_MEAN;
  a.flip = c.reduce == PYGAMD_MIN ? 0x80000000u : 0u;
  const bool hubs = g->n_hub > 0;
  a.hub_rows = hubs ? static_cast<const IdxT*>(g->hub_rows) : nullptr;
  a.hub_chunk_ptr = hubs ? static_cast<const IdxT*>(g->hub_chunk_ptr) : nullptr;
  a.n_hub = hubs ? g->n_hub : 0;
  a.n_chunks = hubs ? g->n_chunks : 0;
  a.hub_threshold = g->hub_threshold;
  a.hub_chunk = g->hub_chunk;
  const size_t plane = static_cast<size_t>(a.n_chunks) * static_cast<size_t>(c.F);
  a.partial = static_cast<float*>(c.workspace);
  a.part_arg = reinterpret_cast<int32_t*>(a.partial + plane);
  a.part_src = reinterpret_cast<uint32_t*>(a.partial + 2 * plane);
  const bool mm = c.reduce == PYGAMD_MIN || c.reduce == PYGAMD_MAX;
  dim3 grid(wave_grid(a.n_rows + a.n_chunks),
            static_cast<unsigned>(ceil_div(c.F, static_cast<int64_t>(LPR) * kLpCols)));
  if (mm) {
    hipLaunchKernelGGL((lp_minmax_rows<T, IdxT, VW, LPR>), grid, dim3(kBlock), 0, c.st, a);
  } else if (c.w || c.src_scale) {
    hipLaunchKernelGGL((lp_sum_rows<T, IdxT, VW, LPR, true>), grid, dim3(kBlock), 0, c.st, a);
  } else {
    hipLaunchKernelGGL((lp_sum_rows<T, IdxT, VW, LPR, false>), grid, dim3(kBlock), 0, c.st, a);
  }
  PYGAMD_LAUNCH_CHECK();
  if (hubs) {
    dim3 hgrid(static_cast<unsigned>(ceil_div(a.n_hub, kWavesPerBlock)));
    if (mm) {
      hipLaunchKernelGGL((lp_hub_minmax<T, IdxT>), hgrid, dim3(kBlock), 0, c.st, a);
    } else {
      hipLaunchKernelGGL((lp_hub_sum<T, IdxT>), hgrid, dim3(kBlock), 0, c.st, a);
    }
    PYGAMD_LAUNCH_CHECK();
  }
  return PYGAMD_OK;
}

template <typename T, typename IdxT, int VW>
static int lp_launch_lanes(const LpCall& c) {
  switch (lp_lanes(c.F)) {
    case 1:
      return lp_launch<T, IdxT, VW, 1>(c);
    case 2:
      return lp_launch<T, IdxT, VW, 2>(c);
    case 4:
      return lp_launch<T, IdxT, VW, 4>(c);
    case 8:
      return lp_launch<T, IdxT, VW, 8>(c);
    case 16:
      return lp_launch<T, IdxT, VW, 16>(c);
    case 32:
      return lp_launch<T, IdxT, VW, 32>(c);
    default:
      return lp_launch<T, IdxT, VW, 64>(c);
  }
}

template <typename T, typename IdxT>
static int lp_launch_width(const LpCall& c) {
  switch (lp_vector_width(c)) {
    case 8:
      return lp_launch_lanes<T, IdxT, 8>(c);
    case 2:
      return lp_launch_lanes<T, IdxT, 2>(c);
    default:
      return lp_launch_lanes<T, IdxT, 1>(c);
  }
}

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_spmm_lp_supported(int x_dtype, int64_t F) {
  return (x_dtype == PYGAMD_DTYPE_F16 || x_dtype == PYGAMD_DTYPE_BF16) && F >= 1 &&
         F < (int64_t{1} << 31);
}

size_t pygamd_spmm_lp_workspace_size(const pygamd_csr* g, int64_t F) {
  if (!g || g->n_hub <= 0 || g->n_chunks <= 0 || F <= 0) return 0;
  // float32 partials [n_chunks, F]; MIN / MAX add the slot offsets and first sources
  return static_cast<size_t>(g->n_chunks) * static_cast<size_t>(F) * 12u;
}

int pygamd_spmm_lp(const pygamd_csr* g, const void* eid, const float* w, const float* src_scale,
                   const void* x, int x_dtype, int64_t ldx, int64_t n_src, void* out, int64_t ldo,
                   int64_t F, int reduce, int32_t* arg32_out, void* workspace,
                   size_t workspace_bytes, void* stream) {
  if (!g) return PYGAMD_ERR_INVALID_ARG;
  if (g->idx_dtype != PYGAMD_IDX_I32 && g->idx_dtype != PYGAMD_IDX_I64)
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows < 0 || F < 0 || n_src < 0 || ldx < F || ldo < F) return PYGAMD_ERR_INVALID_ARG;
  if (reduce != PYGAMD_SUM && reduce != PYGAMD_MEAN && reduce != PYGAMD_MIN &&
      reduce != PYGAMD_MAX)
    return PYGAMD_ERR_UNSUPPORTED;
  const bool mm = reduce == PYGAMD_MIN || reduce == PYGAMD_MAX;
  if (mm && (w || src_scale)) return PYGAMD_ERR_UNSUPPORTED;
  if (!mm && arg32_out) return PYGAMD_ERR_INVALID_ARG;
  if (g->n_rows == 0 || F == 0) return PYGAMD_OK;
  if (!pygamd_spmm_lp_supported(x_dtype, F)) return PYGAMD_ERR_UNSUPPORTED;
  if (!g->rowptr || !g->col || !x || !out) return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub > 0 && (!g->hub_rows || !g->hub_chunk_ptr || g->hub_chunk < 1 ||
                       g->hub_threshold < 1 || g->n_chunks < g->n_hub))
    return PYGAMD_ERR_INVALID_ARG;
  if (g->n_hub <= 0 && g->n_chunks != 0) return PYGAMD_ERR_INVALID_ARG;
  const size_t need = pygamd_spmm_lp_workspace_size(g, F);
  if (need > 0 && (!workspace || workspace_bytes < need)) return PYGAMD_ERR_WORKSPACE;
  LpCall c = {g, eid, w, src_scale, x, out, ldx, ldo, F, reduce, arg32_out, workspace,
              as_stream(stream)};
  return PYGAMD_DISPATCH_IDX(g->idx_dtype, [&]() -> int {
    return x_dtype == PYGAMD_DTYPE_BF16 ? lp_launch_width<LpBf16, IdxT>(c)
                                        : lp_launch_width<LpHalf, IdxT>(c);
  });
}

}  // extern "C"

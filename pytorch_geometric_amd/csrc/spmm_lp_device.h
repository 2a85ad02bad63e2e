// spmm_lp_device.h — device-side building blocks of the CSR aggregation over 16-bit storage
// (csrc/spmm_lp.hip): the argument block, the 8-column lane, its loads at three vector widths,
// the widening / narrowing converts and the slot-staged accumulation loop.
#pragma once
#include "common.h"

namespace pygamd {

struct LpHalf {};   // IEEE binary16
struct LpBf16 {};   // bfloat16

constexpr int kLpCols = 8;  // columns per lane: one 16-byte load, 8 float32 accumulators

template <typename IdxT>
struct LpDev {
  const IdxT* __restrict__ rowptr;
  const IdxT* __restrict__ col;
  const IdxT* __restrict__ eid;
  const float* __restrict__ w;
  const float* __restrict__ src_scale;
  const uint16_t* __restrict__ x;
  uint16_t* __restrict__ out;
  int32_t* __restrict__ arg32_out;
  int64_t n_rows, F, ldx, ldo;
  int mean;
  uint32_t flip;  // MIN: 0x80000000 (the walk is a MAX over sign-flipped values), else 0
  // hub plan (n_chunks == 0: no row is split) and the chunk partials
  const IdxT* __restrict__ hub_rows;
  const IdxT* __restrict__ hub_chunk_ptr;
  int64_t n_hub, n_chunks, hub_threshold, hub_chunk;
  float* __restrict__ partial;     // [n_chunks, F]
  int32_t* __restrict__ part_arg;  // MIN/MAX [n_chunks, F]: slot offset; -1 empty; -2 - offset: tie
  uint32_t* __restrict__ part_src; // MIN/MAX [n_chunks, F]: low 32 bits of the first attaining source
};

// Independent row loads per lane before the first add.  A staged index chunk holds 64 slots and a
// wave walks 64 / LPR of them per load, so U <= LPR.  At the same F the float32 kernel uses twice
// the lanes per row (4 columns per lane) and the same min(LPR, 8) rule: this one has twice the
// rows and the same 16 bytes x 64 lanes x U in flight — 8 KiB per wave from F = 64 up, every
// staged slot at once (64 rows) below.
template <int LPR>
constexpr int lp_unroll() {
  return LPR < 8 ? LPR : 8;
}

// A lane's 8 columns as they arrive: VW 8: one 16-byte load; VW 2: four 4-byte loads; VW 1: eight
// 2-byte loads (one element per dword, zero-extended).
template <int VW>
struct LpRaw {
  static constexpr int ND = VW == 1 ? 8 : 4;
  uint32_t d[ND];
};

// pm: bit i set where column fo + i exists (fo + i < F); F % VW == 0, so a load is all or nothing
template <int VW>
__device__ __forceinline__ void lp_load(const uint16_t* __restrict__ p, uint32_t pm, bool ok,
                                        LpRaw<VW>& r) {
#pragma unroll
  for (int i = 0; i < LpRaw<VW>::ND; ++i) r.d[i] = 0u;
  if constexpr (VW == 8) {
    if (ok && (pm & 1u)) {
      const uint4 t = *reinterpret_cast<const uint4*>(p);
      r.d[0] = t.x;
      r.d[1] = t.y;
      r.d[2] = t.z;
      r.d[3] = t.w;
    }
  } else if constexpr (VW == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if (ok && ((pm >> (2 * q)) & 1u)) r.d[q] = *reinterpret_cast<const uint32_t*>(p + 2 * q);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if (ok && ((pm >> i) & 1u)) r.d[i] = p[i];
    }
  }
}

// element i of a lane's 8 as float32: bfloat16 is the upper half of a float32 (a shift or a mask),
// binary16 takes the hardware convert
template <typename T, int VW>
__device__ __forceinline__ float lp_widen(const LpRaw<VW>& r, int i) {
  const uint32_t word = VW == 1 ? r.d[i] : r.d[i >> 1];
  const bool hi = VW != 1 && (i & 1);
  if constexpr (__is_same(T, LpBf16)) {
    return __uint_as_float(hi ? (word & 0xFFFF0000u) : (word << 16));
  } else {
    const uint16_t bits = static_cast<uint16_t>(hi ? (word >> 16) : word);
    return static_cast<float>(__builtin_bit_cast(_Float16, bits));
  }
}

// round-to-nearest-even, NaN stays NaN, binary16 overflow gives +-inf (the compiler's fptrunc:
// v_cvt_pk_bf16_f32 / v_cvt_f16_f32 on gfx950)
template <typename T>
__device__ __forceinline__ uint16_t lp_narrow(float a) {
  if constexpr (__is_same(T, LpBf16)) {
    return __builtin_bit_cast(uint16_t, static_cast<__bf16>(a));
  } else {
    return __builtin_bit_cast(uint16_t, static_cast<_Float16>(a));
  }
}
template <typename T>
__device__ __forceinline__ uint32_t lp_narrow2(float a, float b) {
  typedef float f2 __attribute__((ext_vector_type(2)));
  const f2 v = {a, b};
  if constexpr (__is_same(T, LpBf16)) {
    typedef __bf16 b2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, b2));
  } else {
    typedef _Float16 h2 __attribute__((ext_vector_type(2)));
    return __builtin_bit_cast(uint32_t, __builtin_convertvector(v, h2));
  }
}

// the lane's 8 results -> out row, at the vector width of the launch
template <typename T, int VW>
__device__ __forceinline__ void lp_store(uint16_t* __restrict__ p, uint32_t pm,
                                         const float (&o)[kLpCols]) {
  if constexpr (VW == 8) {
    if (pm & 1u) {
      uint4 t;
      t.x = lp_narrow2<T>(o[0], o[1]);
      t.y = lp_narrow2<T>(o[2], o[3]);
      t.z = lp_narrow2<T>(o[4], o[5]);
      t.w = lp_narrow2<T>(o[6], o[7]);
      *reinterpret_cast<uint4*>(p) = t;
    }
  } else if constexpr (VW == 2) {
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      if ((pm >> (2 * q)) & 1u)
        *reinterpret_cast<uint32_t*>(p + 2 * q) = lp_narrow2<T>(o[2 * q], o[2 * q + 1]);
    }
  } else {
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      if ((pm >> i) & 1u) p[i] = lp_narrow<T>(o[i]);
    }
  }
}

template <typename IdxT, int LPR>
__device__ __forceinline__ IdxT lp_bcast(IdxT v, int k) {
  if constexpr (LPR == kWave) {
    return bcast_uniform(v, k);  // one row per wave: the slot number is uniform (v_readlane)
  } else {
    return bcast_lane(v, k);
  }
}
template <int LPR>
__device__ __forceinline__ float lp_bcastf(float v, int k) {
  if constexpr (LPR == kWave) {
    return bcast_uniform(v, k);
  } else {
    return bcast_lane(v, k);
  }
}

// What a wave works on: a hub chunk (the lowest wave ids: the long rows start first) or one whole
// row that is not a hub.  off0 = the first slot's offset inside its row.
template <typename IdxT>
struct LpItem {
  int64_t row, chunk;  // chunk: -1 for a whole row
  IdxT start, end, deg;
  int32_t off0;
};

template <typename IdxT>
__device__ __forceinline__ bool lp_item(const LpDev<IdxT>& a, LpItem<IdxT>& it) {
  const int64_t wid = xcd_logical_block() * kWavesPerBlock + wave_in_block();
  if (wid < a.n_chunks) {
    int64_t lo = 0, hi = a.n_hub;  // hub_chunk_ptr[lo] <= wid < hub_chunk_ptr[hi]
    while (hi - lo > 1) {
      const int64_t mid = (lo + hi) >> 1;
      if (static_cast<int64_t>(a.hub_chunk_ptr[mid]) <= wid) {
        lo = mid;
      } else {
        hi = mid;
      }
    }
    it.row = a.hub_rows[lo];
    it.chunk = wid;
    const int64_t ci = wid - static_cast<int64_t>(a.hub_chunk_ptr[lo]);
    const IdxT rs = a.rowptr[it.row];
    const IdxT re = a.rowptr[it.row + 1];
    it.deg = re - rs;
    it.start = rs + static_cast<IdxT>(ci * a.hub_chunk);
    it.end = it.start + static_cast<IdxT>(a.hub_chunk);
    if (it.end > re) it.end = re;
    if (it.start > re) it.start = re;  // (a plan that does not fit the row pointer reads nothing)
    it.off0 = static_cast<int32_t>(it.start - rs);
    return true;
  }
  it.row = wid - a.n_chunks;
  it.chunk = -1;
  if (it.row >= a.n_rows) return false;
  it.start = a.rowptr[it.row];
  it.end = a.rowptr[it.row + 1];
  it.deg = it.end - it.start;
  it.off0 = 0;
  return !(a.n_chunks > 0 && it.deg > a.hub_threshold);  // a hub row: its chunk waves own it
}

// the lane's first column and which of its 8 exist
template <int LPR>
__device__ __forceinline__ int lp_columns(int lane, int64_t F, uint32_t& pm) {
  const int fo = (static_cast<int>(blockIdx.y) * LPR + lane % LPR) * kLpCols;
  const int64_t left = F - fo;
  pm = left >= kLpCols ? 0xFFu : (left > 0 ? (1u << left) - 1u : 0u);
  return fo;
}

// One batch of the sum: U row loads per lane, then U x 8 fmas (W: m is the slot's staged
// multiplier; otherwise plain adds) in slot order.
template <typename T, typename IdxT, int VW, int LPR, bool W, bool FULL>
__device__ __forceinline__ void lp_batch(const LpDev<IdxT>& a, int j, int cnt, int sub, IdxT myc,
                                         float mym, int fo, uint32_t pm,
                                         float (&acc)[kLpCols]) {
  constexpr int EPI = kWave / LPR;
  constexpr int U = lp_unroll<LPR>();
  LpRaw<VW> v[U];
  float m[U];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = j + u * EPI + sub;
    const bool valid = FULL || (k < cnt);
    const int kk = FULL ? k : (k < cnt ? k : cnt - 1);
    const IdxT c = lp_bcast<IdxT, LPR>(myc, kk);
    if constexpr (W) {
      const float mm = lp_bcastf<LPR>(mym, kk);
      m[u] = valid ? mm : 0.f;
    } else {
      m[u] = 1.f;
    }
    lp_load<VW>(a.x + static_cast<int64_t>(c) * a.ldx + fo, pm, valid, v[u]);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int i = 0; i < kLpCols; ++i) {
      const float xv = lp_widen<T, VW>(v[u], i);
      if constexpr (W) {
        acc[i] = fmaf(xv, m[u], acc[i]);
      } else {
        acc[i] += xv;
      }
    }
  }
}

// acc += the slots [start, end): 64 slots' column and multiplier staged one per lane, handed out
// by readlane (LPR == 64) or through the crossbar
template <typename T, typename IdxT, int VW, int LPR, bool W>
__device__ __forceinline__ void lp_accumulate(const LpDev<IdxT>& a, IdxT start, IdxT end,
                                              int lane, int fo, uint32_t pm,
                                              float (&acc)[kLpCols]) {
  constexpr int STEP = (kWave / LPR) * lp_unroll<LPR>();
  const int sub = lane / LPR;
  for (IdxT base = start; base < end; base += kWave) {
    const IdxT rem = end - base;
    const int cnt = rem < kWave ? static_cast<int>(rem) : kWave;
    IdxT myc = 0;
    float mym = 1.f;
    if (lane < cnt) {
      const IdxT k = base + lane;
      myc = __builtin_nontemporal_load(&a.col[k]);  // streamed once: keep L2 for feature rows
      if constexpr (W) {
        if (a.src_scale) mym = a.src_scale[myc];
        if (a.w) mym *= a.w[a.eid ? a.eid[k] : k];
      }
    }
    int j = 0;
    for (; j + STEP <= cnt; j += STEP)
      lp_batch<T, IdxT, VW, LPR, W, true>(a, j, cnt, sub, myc, mym, fo, pm, acc);
    if (j < cnt) lp_batch<T, IdxT, VW, LPR, W, false>(a, j, cnt, sub, myc, mym, fo, pm, acc);
  }
}

}  // namespace pygamd

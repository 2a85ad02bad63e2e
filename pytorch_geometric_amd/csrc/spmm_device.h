// spmm_device.h — device-side building blocks of the CSR aggregation shared by spmm.hip (the
// stand-alone SpMM family) and sage_fused.hip (aggregation fused with the feature transform):
// the argument block, the per-lane feature slots, and the slot-staged, U-loads-in-flight row
// accumulation loop.  See spmm.hip for the mapping.
#pragma once
#include "common.h"

namespace pygamd {

template <typename IdxT>
struct SpmmDev {
  const IdxT* __restrict__ rowptr;
  const IdxT* __restrict__ col;
  const IdxT* __restrict__ eid;
  const float* __restrict__ w;
  const float* __restrict__ src_scale;
  const float* __restrict__ x;
  float* __restrict__ out;
  IdxT* __restrict__ arg_out;
  int32_t* __restrict__ arg32_out;  // MIN/MAX: saved for the backward (see pyg_amd.h)
  const float* __restrict__ relu_mask;  // SUM/MEAN: out = relu_mask <= 0 ? 0 : out (or null)
  int64_t ldm;
  const uint32_t* __restrict__ relu_bits;  // the same mask, one bit per element (or null)
  int64_t ldb;
  // null, or one bit per SOURCE row (bit j & 31 of src_bits[j >> 5]): rows whose bit is clear are
  // all-zero and are not read (plain sums only).  src_bits_set (or null): how many bits are set,
  // on the device — with more than half of the n_src rows live the lookup costs more than it
  // saves and the kernel ignores the bits.
  const uint32_t* __restrict__ src_bits;
  const int64_t* __restrict__ src_bits_set;
  int64_t n_src;
  int64_t n_rows, F, ldx, ldo;
  int w_heads, head_dim;
  int mean;
  int accumulate;  // out[i] += result instead of out[i] = result
  int64_t hub_threshold;
  // null, or [n_rows]: the slots of row r are [rowptr[r], rowend[r]) instead of [rowptr[r],
  // rowptr[r + 1]) — rows own fixed-stride slot blocks that are only partly filled (sampled batches
  // at their static fan-out capacity, csrc/minibatch.hip)
  const IdxT* __restrict__ rowend;
  int64_t accumulate_rows;  // with accumulate: rows >= this start from 0 (0 = every row has an old value)
};

template <typename IdxT>
__device__ __forceinline__ IdxT spmm_row_end(const SpmmDev<IdxT>& a, int64_t row) {
  return a.rowend ? a.rowend[row] : a.rowptr[row + 1];
}

// Independent row loads issued per lane before the first add.  A staged index chunk holds 64
// slots, so EPI * U never needs to exceed 64 (U <= LPR).
template <int LPR, int CH>
constexpr int spmm_unroll() {
  return CH == 1 ? (LPR < 8 ? LPR : 8) : 4;
}

// WMODE: 0 = plain sum; 1 = one staged multiplier per slot (w with one head and/or src_scale);
//        2 = per-head weights fetched per slot (+ optional staged src_scale);
//        3 = plain sum over the source rows whose bit in a.src_bits is set (the others are known
//            to be all-zero and are not read);
//        4 = plain sum over COMPRESSED source rows (a.x = the compressed block, a.ldx its pitch in words;
//            see "compressed rows" below).
template <typename IdxT, int VW, int LPR, int CH, int WMODE, bool IDENT, bool FULL, int UF = 0>
__device__ __forceinline__ void spmm_batch(const SpmmDev<IdxT>& a, int j, int cnt, int sub,
                                           IdxT myc, IdxT mye, float mym, const int (&fo)[CH],
                                           const bool (&fv)[CH], const int (&head)[CH],
                                           float (&acc)[CH][VW]) {
  constexpr int EPI = kWave / LPR;
  constexpr int U = UF > 0 ? UF : spmm_unroll<LPR, CH>();
  Vec<VW> v[U][CH];
  float m[U];
  float wv[U][CH];
#pragma unroll
  for (int u = 0; u < U; ++u) {
    const int k = j + u * EPI + sub;
    const bool valid = FULL || (k < cnt);
    const int kk = FULL ? k : (k < cnt ? k : cnt - 1);
    IdxT c;
    if constexpr (EPI == 1) {
      c = bcast_uniform(myc, kk);
    } else {
      c = bcast_lane(myc, kk);
    }
    if constexpr (WMODE == 1 || WMODE == 2) {
      float mm;
      if constexpr (EPI == 1) {
        mm = bcast_uniform(mym, kk);
      } else {
        mm = bcast_lane(mym, kk);
      }
      m[u] = valid ? mm : 0.f;
    } else {
      m[u] = 1.f;
    }
    const float* __restrict__ xr = a.x + static_cast<int64_t>(c) * a.ldx;
    if constexpr (WMODE == 2) {
      IdxT e;
      if constexpr (EPI == 1) {
        e = bcast_uniform(mye, kk);
      } else {
        e = bcast_lane(mye, kk);
      }
      const float* __restrict__ wr = a.w + static_cast<int64_t>(e) * a.w_heads;
#pragma unroll
      for (int c2 = 0; c2 < CH; ++c2) wv[u][c2] = fv[c2] ? wr[head[c2]] : 0.f;
    }
#pragma unroll
    for (int c2 = 0; c2 < CH; ++c2) {
      if (fv[c2] && valid) {
#ifdef PYGAMD_GATHER_NT  // lab: gathered rows with the non-temporal hint (scripts/README.md)
        v[u][c2] = load_vec_streamed<VW>(xr + fo[c2]);
#else
        v[u][c2] = load_vec<VW>(xr + fo[c2]);
#endif
      } else {
#pragma unroll
        for (int i = 0; i < VW; ++i) v[u][c2].v[i] = 0.f;
      }
    }
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int c2 = 0; c2 < CH; ++c2) {
#pragma unroll
      for (int i = 0; i < VW; ++i) {
        if constexpr (WMODE == 0 || WMODE == 3) {
          acc[c2][i] += v[u][c2].v[i];
        } else if constexpr (WMODE == 1) {
          acc[c2][i] = fmaf(v[u][c2].v[i], m[u], acc[c2][i]);
        } else {
          acc[c2][i] = fmaf(v[u][c2].v[i], m[u] * wv[u][c2], acc[c2][i]);
        }
      }
    }
  }
}

// ---- compressed rows ------------------------------------------------------------------------------------
// A [n, F <= 256] activation block with many exact zeros (a ReLU output: half of it) stored row by
// row as  [8 mask words | the kept values in column order]  at a fixed row pitch (ld words, a
// multiple of 32 = 128 bytes, >= F + 12): bit (c & 31) of word (c >> 5) is set where element c is
// kept (its bit pattern is not +0.0).  A gather then touches 32 + 4 nnz bytes of a row instead of
// 4 F — 4.4 instead of 8 lines of 128 bytes for a half-empty 256-float row — and the cost of a
// row gather on this chip is proportional to the lines it touches (scripts/gather_lines_probe.py:
// 10.1 ms for 8 lines per row, 6.0 ms for 5, 4.6 ms for 4 at the products shape).  Lossless: the
// sums below add the same values in the same order as the dense gather (a dropped +0.0 changes no
// sum).
//
// The writers (rows_compress_kernel, fused_compress_tile) own columns 4 l .. 4 l + 3 per lane
// (zrow_lane_offset).  The READER does not: lane l of the wave that decodes a row owns columns
// l, l + 64, l + 128, l + 192.  The mask of column chunk k is then the 64-bit lane mask made of
// header words 2 k, 2 k + 1 — the same for the whole wave, so the eight header words of a row come
// in as ONE scalar load of 32 bytes (the source row id is wave-uniform) — and lane l's value of
// chunk k sits at word  8 + kept(chunks < k) + (set bits of mask_k below lane l): scalar popcounts
// plus v_mbcnt_lo / v_mbcnt_hi.  The lanes whose bit is set read consecutive dwords: one coalesced
// request of exactly the kept bytes per chunk (the slack words behind a row are never read).
constexpr int kZrowHdr = 8;
typedef uint32_t u32x8 __attribute__((ext_vector_type(8)));
typedef const __attribute__((address_space(4))) u32x8* zrow_hdr_ptr;  // read-only: scalar loads
typedef const __attribute__((address_space(1))) uint32_t* zrow_ptr;   // (global, not flat, loads)

// exclusive prefix over the eight 8-lane groups of a wave of a value `t` that is equal inside each
// group (three DPP adds: the other half of the 16-lane row, then row 0 -> 1 / 2 -> 3, then the
// lower half -> rows 2, 3)
__device__ __forceinline__ int group8_exclusive_prefix(int t) {
  const int a1 = t + __builtin_amdgcn_update_dpp(0, t, 0x118 /* row_shr:8 */, 0xF, 0xF, false);
  const int a2 = a1 + __builtin_amdgcn_update_dpp(0, a1, 0x142 /* row_bcast:15 */, 0xA, 0xF, false);
  const int a3 = a2 + __builtin_amdgcn_update_dpp(0, a2, 0x143 /* row_bcast:31 */, 0xC, 0xF, false);
  return a3 - t;
}

// writers: (offset of the lane's first kept value, its mask nibble) from the mask word that holds
// the nibble of the lane's columns 4 l .. 4 l + 3
__device__ __forceinline__ int zrow_lane_offset(uint32_t hw, int lane, uint32_t& nib) {
  const int sh = (lane & 7) * 4;
  nib = (hw >> sh) & 15u;
  const int below = __popc(hw & ((1u << sh) - 1u));
  return group8_exclusive_prefix(__popc(hw)) + below;
}

// the headers of the U source rows of slots j .. j + U - 1 (past cnt: the last slot's again).
// PIN: the slot number passes through an opaque scalar, which keeps the loads at this point of the
// program (hipcc otherwise merges the in-loop call with the one in front of the loop and issues the
// loads at the loop head, behind the wait for the previous batch's values).
// (row id and pitch in bytes are below 2^32: one 32 x 32 -> 64 bit product on the scalar unit)
template <typename IdxT, int U, bool PIN>
__device__ __forceinline__ void zrows_headers(const SpmmDev<IdxT>& a, int j, int cnt, IdxT myc,
                                              zrow_ptr (&base)[U], u32x8 (&h)[U]) {
  const __attribute__((address_space(1))) char* rows =
      (const __attribute__((address_space(1))) char*)(a.x);
  const uint32_t pitch = static_cast<uint32_t>(a.ldx) * 4u;  // bytes
#pragma unroll
  for (int u = 0; u < U; ++u) {
    int k = j + u;
    k = k < cnt ? k : cnt - 1;
    if constexpr (PIN) asm volatile("" : "+s"(k));
    const uint32_t c = static_cast<uint32_t>(bcast_uniform(static_cast<int32_t>(myc), k));
    base[u] = (zrow_ptr)(rows + static_cast<uint64_t>(c) * pitch);
    h[u] = *(zrow_hdr_ptr)(base[u]);
  }
}

// One batch: the 4 U value loads are issued under the chunk masks (a lane whose bit is clear
// issues nothing and keeps +0.0), then the header loads of the NEXT batch — the masks are dead once
// the value loads are out, and the headers complete under them: the mask round trip is paid once
// per staged index chunk, not once per batch — then the values are added in slot order.
// FULL: all U slots exist; otherwise the slots from cnt on add +0.0.
template <typename IdxT, int U, bool FULL>
__device__ __forceinline__ void zrows_batch(const SpmmDev<IdxT>& a, int j, int cnt, IdxT myc,
                                            zrow_ptr (&base)[U], u32x8 (&h)[U],
                                            float (&zacc)[4]) {
  float v[U][4];
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) v[u][k] = 0.f;
    if (FULL || j + u < cnt) {  // (uniform: a slot past the end is one scalar branch)
      int kept = kZrowHdr;
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        const uint32_t lo = h[u][2 * k], hi = h[u][2 * k + 1];
        const uint64_t m = (static_cast<uint64_t>(hi) << 32) | lo;
        if (__builtin_amdgcn_inverse_ballot_w64(m)) {
          const int off = __builtin_amdgcn_mbcnt_hi(hi, __builtin_amdgcn_mbcnt_lo(lo, 0)) + kept;
          v[u][k] = __uint_as_float(base[u][off]);
        }
        kept += __popcll(m);
      }
    }
  }
  if constexpr (FULL) {  // (a partial batch is the chunk's last)
    __builtin_amdgcn_sched_barrier(0);
    zrows_headers<IdxT, U, true>(a, j + U, cnt, myc, base, h);
    __builtin_amdgcn_sched_barrier(0);
  }
#pragma unroll
  for (int u = 0; u < U; ++u) {
#pragma unroll
    for (int k = 0; k < 4; ++k) zacc[k] += v[u][k];
  }
}

// The slots [0, cnt) of one staged index chunk, U source rows at a time, into zacc[k] = column
// lane + 64 k.
template <typename IdxT, int U>
__device__ __forceinline__ void spmm_zrows(const SpmmDev<IdxT>& a, int cnt, IdxT myc,
                                           float (&zacc)[4]) {
  zrow_ptr base[U];
  u32x8 h[U];
  zrows_headers<IdxT, U, false>(a, 0, cnt, myc, base, h);
  int j = 0;
  for (; j + U <= cnt; j += U) zrows_batch<IdxT, U, true>(a, j, cnt, myc, base, h, zacc);
  if (j < cnt) zrows_batch<IdxT, U, false>(a, j, cnt, myc, base, h, zacc);
}

// zacc[k] = column lane + 64 k  ->  o[i] = column 4 lane + i (the lane shape of the dense row
// kernels: 64 lanes x 4 consecutive columns).  Column 4 l + i lives in lane (4 l + i) & 63,
// chunk l >> 4.  Once per destination row.
__device__ __forceinline__ void zrows_to_vec4(const float (&zacc)[4], int lane, float (&o)[4]) {
  const int src = (lane & 15) * 4;
  const int kq = lane >> 4;
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    float t[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) t[k] = __shfl(zacc[k], src + i, kWave);
    o[i] = kq == 0 ? t[0] : (kq == 1 ? t[1] : (kq == 2 ? t[2] : t[3]));
  }
}

// UF > 0 overrides the number of row loads in flight per lane (a kernel with few resident waves
// needs more memory-level parallelism per wave)
// GUARD: a column id outside [0, a.n_src) reads row 0 instead and sets *bad (a per-lane flag of
// the caller; the convention of pygamd_gather_rows) — for callers whose ids nobody vouches for.
template <typename IdxT, int VW, int LPR, int CH, int WMODE, bool IDENT, int UF = 0,
          bool GUARD = false>
__device__ __forceinline__ void spmm_accumulate(const SpmmDev<IdxT>& a, IdxT start, IdxT end,
                                                int lane, const int (&fo)[CH],
                                                const bool (&fv)[CH], const int (&head)[CH],
                                                float (&acc)[CH][VW], bool* bad = nullptr) {
  constexpr int EPI = kWave / LPR;
  constexpr int U = UF > 0 ? UF : spmm_unroll<LPR, CH>();
  constexpr int STEP = EPI * U;
  const int sub = lane / LPR;
  bool sparse_src = false;
  float zacc[4] = {0.f, 0.f, 0.f, 0.f};  // WMODE 4: column lane + 64 k (see "compressed rows")
  if constexpr (WMODE == 3) {
    sparse_src = a.src_bits_set == nullptr || 2 * *a.src_bits_set < a.n_src;
  }
  for (IdxT base = start; base < end; base += kWave) {
    const IdxT rem = end - base;
    int cnt = rem < kWave ? static_cast<int>(rem) : kWave;
    IdxT myc = 0, mye = 0;
    float mym = 1.f;
    if (lane < cnt) {
      const IdxT k = base + lane;
      if constexpr (IDENT) {
        myc = k;
      } else {
        myc = __builtin_nontemporal_load(&a.col[k]);  // streamed once: keep L2 for feature rows
      }
      if constexpr (GUARD) {
        if (myc < 0 || static_cast<int64_t>(myc) >= a.n_src) {
          myc = 0;
          *bad = true;
        }
      }
      if constexpr (WMODE == 1 || WMODE == 2) {
        mye = a.eid ? a.eid[k] : k;
        if (a.src_scale) mym = a.src_scale[myc];
        if constexpr (WMODE == 1) {
          if (a.w) mym *= a.w[mye];
        }
      }
    }
    if constexpr (WMODE == 3) {
      if (sparse_src) {
        // keep the slots whose source row is live, packed into the low lanes in slot order (an
        // all-zero row adds +0.0 to every sum: dropping it changes no result)
        const bool keep =
            lane < cnt && ((a.src_bits[static_cast<int64_t>(myc) >> 5] >> (myc & 31)) & 1u) != 0;
        const uint64_t m = __ballot(keep);
        const int before = __builtin_amdgcn_mbcnt_hi(
            static_cast<uint32_t>(m >> 32), __builtin_amdgcn_mbcnt_lo(static_cast<uint32_t>(m), 0));
        cnt = __popcll(m);
        myc = push_lane(myc, keep ? before : cnt + lane - before);
      }
    }
    int j = 0;
    if constexpr (WMODE == 4) {
      static_assert(LPR == kWave && VW == 4 && CH == 1 && !IDENT, "compressed rows: 64 lanes x 4");
      spmm_zrows<IdxT, U>(a, cnt, myc, zacc);
    } else {
      for (; j + STEP <= cnt; j += STEP) {
        spmm_batch<IdxT, VW, LPR, CH, WMODE, IDENT, true, UF>(a, j, cnt, sub, myc, mye, mym, fo,
                                                              fv, head, acc);
      }
      if (j < cnt) {
        spmm_batch<IdxT, VW, LPR, CH, WMODE, IDENT, false, UF>(a, j, cnt, sub, myc, mye, mym, fo,
                                                               fv, head, acc);
      }
    }
  }
  if constexpr (WMODE == 4) {  // (an accumulator that starts at +0.0 never becomes -0.0: the
    float o[4];                // sum added to a zero acc keeps its bits)
    zrows_to_vec4(zacc, lane, o);
#pragma unroll
    for (int i = 0; i < 4; ++i) acc[0][i] += o[i];
  }
}

// The lane shape of a row kernel: LPR lanes x CH chunks of VW floats cover a row of F floats
// (`tiles` times over when F > 512 floats); v4 = every row start is 16-byte aligned and F % 4 == 0.
struct Shape {
  int vw, lpr, ch;
  unsigned tiles;
};

inline Shape spmm_shape(int64_t F, bool v4) {
  Shape s;
  s.vw = v4 ? 4 : 1;
  const int64_t units = ceil_div(F, s.vw);  // lanes needed to cover a row once
  int lpr = 4;
  while (lpr < 64 && lpr < units) lpr <<= 1;
  s.lpr = lpr;
  s.ch = (lpr == 64 && units > 64) ? 2 : 1;
  s.tiles = static_cast<unsigned>(ceil_div(units, static_cast<int64_t>(s.lpr) * s.ch));
  return s;
}

inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }

template <int VW, int LPR, int CH>
__device__ __forceinline__ void feature_slots(int lane, int64_t F, int head_dim, int (&fo)[CH],
                                              bool (&fv)[CH], int (&head)[CH]) {
  const int lir = lane % LPR;
  const int f0 = blockIdx.y * (LPR * CH * VW);
#pragma unroll
  for (int c = 0; c < CH; ++c) {
    fo[c] = f0 + (lir + LPR * c) * VW;
    fv[c] = fo[c] < F;
    head[c] = fv[c] ? fo[c] / head_dim : 0;
  }
}

template <int VW, int LPR, int CH>
__device__ __forceinline__ void combine_subgroups(float (&acc)[CH][VW]) {
#pragma unroll
  for (int off = LPR; off < kWave; off <<= 1) {
#pragma unroll
    for (int c = 0; c < CH; ++c) {
#pragma unroll
      for (int i = 0; i < VW; ++i) acc[c][i] += __shfl_xor(acc[c][i], off, kWave);
    }
  }
}

}  // namespace pygamd

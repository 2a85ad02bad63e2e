// sample.hip — uniform neighbour sampling (without or with replacement) on a CSC graph (SURVEY.md
// §8(f)-1):
// the device-side counterpart of torch.ops.pyg.neighbor_sample for one hop
// (torch_geometric/sampler/neighbor_sampler.py:550-577: colptr, row, seed nodes, fan-out k).
//
// One wavefront per frontier node v.  If deg(v) <= k every in-neighbour is taken (lanes copy the
// slot range, coalesced).  Otherwise the wave draws a uniform k-subset of the deg(v) slots with
// Floyd's algorithm (k <= 64: lane c makes draw c from a counter-based hash of (seed, v, c), the
// k insertions are k wave-wide membership tests), so a batch is reproducible from its seed
// regardless of scheduling; lanes 0..k-1 then emit one edge each.  With replacement
// (`replace`, the reference's `replace=True`, loader/neighbor_loader.py:209) every node with at
// least one in-neighbour emits exactly k edges, lane c an independent uniform draw of the same
// hash.  HBM-bound integer work: 3 index reads + 3 index writes per sampled edge.
#include "common.h"

namespace pygamd {

constexpr int kMaxFanout = 64;

__device__ __forceinline__ uint64_t mix64(uint64_t z) {  // splitmix64 finaliser
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// deg(v) <= count: lanes copy the slot range [s, s + deg), coalesced, in slot order
// (`perm`, the heterogeneous draw: slot_out receives perm[slot] in place of the slot)
template <typename IdxT>
__device__ __forceinline__ void copy_all_slots(const IdxT* __restrict__ row, int64_t s,
                                               int64_t deg, int64_t o, int64_t f,
                                               IdxT* __restrict__ src_out,
                                               IdxT* __restrict__ dstpos_out,
                                               IdxT* __restrict__ slot_out,
                                               const IdxT* __restrict__ perm = nullptr) {
  for (int64_t t = lane_id(); t < deg; t += kWave) {
    src_out[o + t] = row[s + t];
    dstpos_out[o + t] = static_cast<IdxT>(f);
    slot_out[o + t] = perm ? perm[s + t] : static_cast<IdxT>(s + t);
  }
}

// The hash stream of frontier node v at frontier position f: draw c of the node uses
// mix64(key + c).
__device__ __forceinline__ uint64_t node_key(uint64_t seed, const uint64_t* __restrict__ seed_dev,
                                             int64_t v, int64_t f, int flags) {
  // flags & 2: the draws depend on the frontier position too (disjoint trees)
  const uint64_t salt = (flags & 2) ? mix64(0xD1B54A32D192ED03ull * static_cast<uint64_t>(f + 1)) : 0;
  // (a captured graph bumps this word between replays.  It is mixed in on its own, not added:
  // the host seed is rng * 1000003 + hop, so `seed + word` would hand hop h + 1 of one replay the
  // stream of hop h of the next — ADVICE r3)
  if (seed_dev) seed = mix64(seed ^ mix64(*seed_dev * 0x9E3779B97F4A7C15ull));
  return mix64(seed ^ mix64(static_cast<uint64_t>(v)) ^ salt);
}

// The uniform draw of one frontier node over the slot range [s, s + deg): cnt = offsets[f + 1] -
// offsets[f] > 0 edges written from position o.  The range is the node's whole column or its
// eligible window (temporal draws): the same (key, s, deg, cnt) gives the same edges bit for bit.
template <typename IdxT>
__device__ __forceinline__ void draw_uniform(const IdxT* __restrict__ row, int64_t s, int64_t deg,
                                             int64_t o, int64_t cnt, int64_t f, uint64_t key,
                                             bool replace, IdxT* __restrict__ src_out,
                                             IdxT* __restrict__ dstpos_out,
                                             IdxT* __restrict__ slot_out,
                                             const IdxT* __restrict__ perm = nullptr) {
  const int lane = lane_id();
  if (replace) {  // cnt = k independent draws from the deg in-neighbours (deg > 0 here)
    if (lane < cnt) {
      const uint64_t r = mix64(key + static_cast<uint64_t>(lane));
      const int64_t t = static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(deg)));
      src_out[o + lane] = row[s + t];
      dstpos_out[o + lane] = static_cast<IdxT>(f);
      slot_out[o + lane] = perm ? perm[s + t] : static_cast<IdxT>(s + t);
    }
    return;
  }
  if (deg <= cnt) {  // take every in-neighbour
    copy_all_slots(row, s, deg, o, f, src_out, dstpos_out, slot_out, perm);
    return;
  }
  // Floyd: for j = deg-k .. deg-1: t = U{0..j}; insert t, or j if t is already chosen.  Lane c
  // draws t_c; the k dependent insertions then run as k wave-wide steps (one 64-lane membership
  // test each) instead of an O(k^2) loop on lane 0 — same draws, same result, bit for bit.
  const int k = static_cast<int>(cnt);
  const int64_t jl = deg - cnt + lane;  // Floyd's j of this lane's draw
  int64_t t = 0;
  if (lane < k) {
    const uint64_t r = mix64(key + static_cast<uint64_t>(lane));
    t = static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(jl + 1)));
  }
  int64_t mine = -1;  // final choice of lane c (only lanes < k end up with one)
  for (int c = 0; c < k; ++c) {
    const int64_t tc = bcast_uniform(t, c);
    const bool dup = __ballot(lane < c && mine == tc) != 0;
    if (lane == c) mine = dup ? jl : tc;
  }
  if (lane < k) {
    src_out[o + lane] = row[s + mine];
    dstpos_out[o + lane] = static_cast<IdxT>(f);
    slot_out[o + lane] = perm ? perm[s + mine] : static_cast<IdxT>(s + mine);
  }
}

// The edges drawn from a window of w slots under (k, replace): min(w, k) (k < 0: all of it; with
// replacement and k >= 0: k wherever the window is not empty).  THE count rule of every sampler:
// the plain and the typed counts apply it to a column, the window kernels to the eligible window.
__device__ __forceinline__ int64_t window_count(int64_t w, int64_t k, bool replace) {
  if (replace && k >= 0) return w > 0 ? k : 0;
  return (k >= 0 && w > k) ? k : w;
}

// lo / hi NULL: the slot range of frontier node f is its column, read from colptr.  Given (the
// temporal draws, see below): it is the window [lo[f], hi[f]) and colptr is not read.
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    sample_neighbors_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ row,
                            const IdxT* __restrict__ frontier, int64_t n_frontier,
                            const IdxT* __restrict__ lo, const IdxT* __restrict__ hi,
                            const IdxT* __restrict__ offsets, uint64_t seed, int flags,
                            const uint64_t* __restrict__ seed_dev,
                            IdxT* __restrict__ src_out, IdxT* __restrict__ dstpos_out,
                            IdxT* __restrict__ slot_out) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (f >= n_frontier) return;
  const int64_t v = frontier[f];
  const int64_t s = lo ? lo[f] : colptr[v];
  const int64_t deg = static_cast<int64_t>(lo ? hi[f] : colptr[v + 1]) - s;
  const int64_t o = offsets[f];
  const int64_t cnt = static_cast<int64_t>(offsets[f + 1]) - o;
  if (cnt <= 0) return;
  const uint64_t key = node_key(seed, seed_dev, v, f, flags);
  draw_uniform(row, s, deg, o, cnt, f, key, (flags & 1) != 0, src_out, dstpos_out, slot_out);
}

// ---- temporal draws (the reference's NeighborLoader(..., time_attr=..., temporal_strategy=...)
// -> torch.ops.pyg.neighbor_sample(..., node_time, edge_time, seed_time, ..., temporal_strategy),
// sampler/neighbor_sampler.py:550-571).  The caller's CSC is sorted like the reference's sort_csc
// (sampler/utils.py:24-42): inside every column the slots ascend in time (the source node's time
// or the edge's), ties in edge_index order.  The in-edges of frontier node v (in tree t) that are
// eligible, time <= seed_time[t], are then a PREFIX [s, hi) of its column.
//
// Window kernel: one wave per frontier node.  hi is found by a wave-cooperative search: the
// candidate range [a, b] (key(a - 1) <= t < key(b), with key(s - 1) = -inf, key(end) = +inf) is
// cut into 64 chunks of `step` slots, lane l probes the last slot of chunk l, one ballot gives the
// first chunk whose probe is past t and the range shrinks to that chunk: ceil(log64(deg)) steps
// (deg <= 64: one load per lane and one ballot).  'last' then narrows the window to its last k
// slots, lo = max(s, hi - k) (k >= 0); 'uniform' keeps lo = s.  cnt is window_count on hi - lo.
// The draws of the hop are sample_neighbors_kernel's on the windows [lo[f], hi[f]): draw_uniform
// with the same hash stream, so a window that is the whole column draws what the column draws.
template <typename IdxT>
__device__ __forceinline__ int64_t slot_time_of(const IdxT* __restrict__ row,
                                                const int64_t* __restrict__ time, int level,
                                                int64_t j) {
  return level == 0 ? time[static_cast<int64_t>(row[j])] : time[j];
}

// The search itself, shared by the plain and the typed window kernels: the first slot of [s, end)
// whose time is past t (= end when every slot is eligible).  Wave-uniform arguments and result.
template <typename IdxT>
__device__ __forceinline__ int64_t temporal_window_end(const IdxT* __restrict__ row,
                                                       const int64_t* __restrict__ time, int level,
                                                       int64_t s, int64_t end, int64_t t) {
  const int lane = lane_id();
  int64_t a = s, b = end;  // the answer lies in [a, b]
  while (a < b) {
    const int64_t len = b - a;
    const int64_t step = (len + kWave - 1) / kWave;
    const int64_t q = a + (lane + 1) * step - 1;  // the last slot of chunk `lane`
    const bool past = q >= b || slot_time_of(row, time, level, q) > t;
    const uint64_t m = __ballot(past);
    if (m == 0) {  // every probe is eligible: the last one is b - 1
      a = b;
      break;
    }
    const int p = __ffsll(static_cast<unsigned long long>(m)) - 1;
    const int64_t qp = a + (static_cast<int64_t>(p) + 1) * step - 1;
    a = a + static_cast<int64_t>(p) * step;
    b = qp < b ? qp : b;
  }
  return a;
}

// lo of a window [s, hi): 'last' keeps its last k slots (k >= 0)
__device__ __forceinline__ int64_t temporal_window_lo(int64_t s, int64_t hi, int64_t k,
                                                      bool last) {
  return (last && k >= 0 && hi - k > s) ? hi - k : s;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    sample_temporal_window_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ row,
                                  const int64_t* __restrict__ time, int level,
                                  const IdxT* __restrict__ frontier,
                                  const int64_t* __restrict__ frontier_time, int64_t n_frontier,
                                  int64_t k, int replace, int last,
                                  const int64_t* __restrict__ n_valid, IdxT* __restrict__ lo_out,
                                  IdxT* __restrict__ hi_out, IdxT* __restrict__ cnt_out) {
  const int lane = lane_id();
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (f >= n_frontier) return;
  if (n_valid && f >= *n_valid) {  // padding of a fixed-capacity frontier
    if (lane == 0) {
      lo_out[f] = static_cast<IdxT>(0);
      hi_out[f] = static_cast<IdxT>(0);
      cnt_out[f] = static_cast<IdxT>(0);
    }
    return;
  }
  const int64_t v = frontier[f];
  const int64_t s = colptr[v];
  const int64_t end = colptr[v + 1];
  const int64_t hi = temporal_window_end(row, time, level, s, end, frontier_time[f]);
  const int64_t lo = temporal_window_lo(s, hi, k, last != 0);
  if (lane == 0) {
    lo_out[f] = static_cast<IdxT>(lo);
    hi_out[f] = static_cast<IdxT>(hi);
    cnt_out[f] = static_cast<IdxT>(window_count(hi - lo, k, replace != 0));
  }
}

// ---- weighted draws (the reference's weight_attr -> NeighborSampler.edge_weight,
// sampler/neighbor_sampler.py:110-114, 559-571).  One wave per frontier node, like the uniform
// kernel; `weight` is in CSC slot order.  deg <= count without replacement: every in-neighbour, as
// above.  Otherwise the wave streams ALL deg weights of the node in chunks of 64 slots, kWGroup
// chunks per group, the loads of the next group in flight while the current one is processed.
//   without replacement: Efraimidis-Spirakis — slot j gets key log(-ln u_j) - log(w_j) (u_j the
//     hash of (seed, v, j) in (0, 1)), the k smallest keys are the sample (= successive sampling
//     in proportion to weight).  The wave keeps the 64 smallest keys seen so far as a sorted list
//     (lane c = the c-th smallest; the slot rides in the low word of a 64-bit composite key).  A
//     chunk with no key below the current k-th is skipped on one ballot; otherwise it is bitonic-
//     sorted descending, merged by an elementwise min against the running list and cleaned up by
//     6 bitonic stages.  w = 0 keys sort after every positive weight, among themselves by hash.
//     Lane c < k emits the c-th smallest key: a node's edges come out in key order.
//   with replacement: pass 1 sums W with the same per-chunk inclusive scans pass 2 repeats, so
//     the running prefix of pass 2 ends at W bit for bit; lane c's draw targets u_c * W and is
//     resolved in the chunk whose prefix passes it by a 6-step binary search across the lanes.
//     A target that rounding puts on a zero-weight slot moves to the last positive slot before
//     it.  W = 0 (outside the reference's domain): k uniform draws over the deg slots.
constexpr int kWGroup = 16;

// u in (0, 1) from 23 hash bits: (h + 0.5) / 2^23 is exact in fp32 and never 0 or 1
__device__ __forceinline__ float open_unit(uint64_t r) {
  return (static_cast<float>(static_cast<uint32_t>(r >> 41)) + 0.5f) * 0x1p-23f;
}

// 64-bit composite key of slot j: high word = the ES key as an order-preserving uint (log2 in
// place of ln: a positive scale and a common shift, the same order), or +inf plus 23 hash bits
// for w = 0 (after every positive weight, ties broken by hash); low word = j
__device__ __forceinline__ uint64_t es_key(float w, uint64_t r, uint32_t j) {
  const float k = log2f(-log2f(open_unit(r))) - log2f(w);
  const uint32_t b = __float_as_uint(k);
  const uint32_t ord = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  const uint32_t hi = w > 0.f ? ord : (0xFF800000u | static_cast<uint32_t>(r & 0x7FFFFFu));
  return (static_cast<uint64_t>(hi) << 32) | j;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t x, int m) {
  return static_cast<uint64_t>(__shfl_xor(static_cast<unsigned long long>(x), m, kWave));
}

// bitonic sort of one key per lane across the wave (descending: lane 0 holds the largest)
__device__ __forceinline__ uint64_t wave_sort_desc(uint64_t x) {
  const int lane = lane_id();
#pragma unroll
  for (int size = 2; size <= kWave; size <<= 1) {
#pragma unroll
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      const uint64_t y = shfl_xor_u64(x, stride);
      const bool keep_max = ((lane & stride) == 0) == ((lane & size) == 0);
      x = keep_max ? (x > y ? x : y) : (x < y ? x : y);
    }
  }
  return x;
}

// run ascending, c descending: min(run, c) lane by lane holds the 64 smallest of both as a
// bitonic sequence; 6 half-cleaner stages sort it ascending
__device__ __forceinline__ uint64_t merge_smallest(uint64_t run, uint64_t c) {
  uint64_t x = run < c ? run : c;
  const int lane = lane_id();
#pragma unroll
  for (int stride = kWave >> 1; stride > 0; stride >>= 1) {
    const uint64_t y = shfl_xor_u64(x, stride);
    x = ((lane & stride) == 0) ? (x < y ? x : y) : (x > y ? x : y);
  }
  return x;
}

__device__ __forceinline__ float wave_inclusive_scan(float x) {
  const int lane = lane_id();
#pragma unroll
  for (int d = 1; d < kWave; d <<= 1) {
    const float y = __shfl_up(x, d, kWave);
    if (lane >= d) x += y;
  }
  return x;
}

// weights of slots [g, g + kWGroup * 64) of the node (0 past deg)
__device__ __forceinline__ void load_weight_group(const float* __restrict__ wv, int64_t deg,
                                                  int64_t g, float (&w)[kWGroup]) {
#pragma unroll
  for (int i = 0; i < kWGroup; ++i) {
    const int64_t j = g + i * kWave + lane_id();
    w[i] = j < deg ? wv[j] : 0.f;
  }
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    sample_neighbors_weighted_kernel(const IdxT* __restrict__ colptr,
                                     const IdxT* __restrict__ row,
                                     const float* __restrict__ weight,
                                     const IdxT* __restrict__ frontier, int64_t n_frontier,
                                     const IdxT* __restrict__ offsets, uint64_t seed, int flags,
                                     const uint64_t* __restrict__ seed_dev,
                                     IdxT* __restrict__ src_out, IdxT* __restrict__ dstpos_out,
                                     IdxT* __restrict__ slot_out) {
  constexpr int64_t kGroupSlots = kWGroup * kWave;
  const int lane = lane_id();
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (f >= n_frontier) return;
  const int64_t v = frontier[f];
  const int64_t s = colptr[v];
  const int64_t deg = static_cast<int64_t>(colptr[v + 1]) - s;
  const int64_t o = offsets[f];
  const int64_t cnt = static_cast<int64_t>(offsets[f + 1]) - o;
  if (cnt <= 0) return;
  const bool replace = (flags & 1) != 0;
  if (!replace && deg <= cnt) {  // take every in-neighbour
    copy_all_slots(row, s, deg, o, f, src_out, dstpos_out, slot_out);
    return;
  }
  const uint64_t key = node_key(seed, seed_dev, v, f, flags);
  const float* wv = weight + s;
  float wn[kWGroup];
  int64_t pick = 0;  // lane c < cnt: the chosen slot, relative to s
  if (!replace) {
    const int k = static_cast<int>(cnt);
    uint64_t run = ~0ull;  // lane c: the c-th smallest key so far
    uint64_t thr = ~0ull;  // the k-th smallest (wave-uniform)
    load_weight_group(wv, deg, 0, wn);
    for (int64_t g = 0; g < deg; g += kGroupSlots) {
      float w[kWGroup];
#pragma unroll
      for (int i = 0; i < kWGroup; ++i) w[i] = wn[i];
      if (g + kGroupSlots < deg) load_weight_group(wv, deg, g + kGroupSlots, wn);
#pragma unroll
      for (int i = 0; i < kWGroup; ++i) {
        const int64_t j = g + i * kWave + lane;
        const uint64_t kj = j < deg ? es_key(w[i], mix64(key + static_cast<uint64_t>(j)),
                                             static_cast<uint32_t>(j))
                                    : ~0ull;
        if (__ballot(kj < thr) == 0) continue;  // nothing below the current k-th
        run = merge_smallest(run, wave_sort_desc(kj));
        thr = static_cast<uint64_t>(bcast_uniform(static_cast<int64_t>(run), k - 1));
      }
    }
    pick = static_cast<int64_t>(static_cast<uint32_t>(run));
  } else {
    // pass 1: W as the running sum of the chunks' scan totals
    float base = 0.f;
    load_weight_group(wv, deg, 0, wn);
    for (int64_t g = 0; g < deg; g += kGroupSlots) {
      float w[kWGroup];
#pragma unroll
      for (int i = 0; i < kWGroup; ++i) w[i] = wn[i];
      if (g + kGroupSlots < deg) load_weight_group(wv, deg, g + kGroupSlots, wn);
#pragma unroll
      for (int i = 0; i < kWGroup; ++i)
        base = base + bcast_uniform(wave_inclusive_scan(w[i]), kWave - 1);
    }
    const float W = base;
    const uint64_t r = mix64(key + static_cast<uint64_t>(lane));  // draw `lane`
    if (!(W > 0.f)) {  // every weight 0: uniform over the deg slots
      pick = static_cast<int64_t>(__umul64hi(r, static_cast<uint64_t>(deg)));
    } else {
      // pass 2: the same prefix sums; resolve every target in the chunk whose prefix passes it
      const float target = open_unit(r) * W;
      bool open = lane < cnt;
      int64_t last_pos = -1;  // the last positive-weight slot so far (wave-uniform)
      pick = -1;
      base = 0.f;
      load_weight_group(wv, deg, 0, wn);
      for (int64_t g = 0; g < deg; g += kGroupSlots) {
        float w[kWGroup];
#pragma unroll
        for (int i = 0; i < kWGroup; ++i) w[i] = wn[i];
        if (g + kGroupSlots < deg) load_weight_group(wv, deg, g + kGroupSlots, wn);
#pragma unroll
        for (int i = 0; i < kWGroup; ++i) {
          const float P = base + wave_inclusive_scan(w[i]);
          const float end = bcast_uniform(P, kWave - 1);
          const uint64_t positive = __ballot(w[i] > 0.f);
          const bool here = open && target < end;
          if (__ballot(here) != 0) {
            int p = 0;  // the first lane whose prefix exceeds the target
#pragma unroll
            for (int step = kWave >> 1; step > 0; step >>= 1)
              if (bcast_lane(P, p + step - 1) <= target) p += step;
            const float wp = bcast_lane(w[i], p);
            if (here) {
              int q = p;
              if (!(wp > 0.f)) {  // rounding landed on a zero-weight slot
                const uint64_t below = positive & ((1ull << p) - 1);
                q = below ? 63 - __clzll(static_cast<long long>(below)) : -1;
              }
              pick = q >= 0 ? g + i * kWave + q : last_pos;
              open = false;
            }
          }
          if (positive) last_pos = g + i * kWave + 63 - __clzll(static_cast<long long>(positive));
          base = end;
        }
      }
      if (open || pick < 0) pick = last_pos;  // u * W rounded up to W
    }
  }
  if (lane < cnt) {
    const int64_t t = s + pick;
    src_out[o + lane] = row[t];
    dstpos_out[o + lane] = static_cast<IdxT>(f);
    slot_out[o + lane] = static_cast<IdxT>(t);
  }
}

// cnt[f] = min(deg(frontier[f]), k)   (k < 0: deg; with replacement: k wherever deg > 0)
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    sample_counts_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ frontier,
                         int64_t n, int64_t k, int replace, const int64_t* __restrict__ n_valid,
                         IdxT* __restrict__ cnt) {
  const int64_t f = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (f >= n) return;
  if (n_valid && f >= *n_valid) {  // padding of a fixed-capacity frontier
    cnt[f] = 0;
    return;
  }
  const int64_t v = frontier[f];
  const int64_t deg = static_cast<int64_t>(colptr[v + 1]) - static_cast<int64_t>(colptr[v]);
  cnt[f] = static_cast<IdxT>(window_count(deg, k, replace != 0));
}

// ---- relabelling: global ids of the sampled sources -> local ids, new nodes in order of first
// appearance (what the reference's hash-map insertion produces), deterministic:
//   claim : local[s] = max(local[s], -(e + 2))  -> the smallest e wins among duplicates; entries
//           that already hold a local id (>= 0) are never lowered
//   flag  : flag[e] = (local[src[e]] == -(e + 2))
//   (inclusive scan of flag on the caller's side)
//   assign: the claimant writes local[s] = base + scan[e] - 1 and new_nodes[scan[e] - 1] = s
//   lookup: row[e] = local[src[e]]
template <typename IdxT>
__device__ __forceinline__ void atomic_max_idx(IdxT* p, IdxT v);
template <>
__device__ __forceinline__ void atomic_max_idx<int32_t>(int32_t* p, int32_t v) {
  atomicMax(p, v);
}
template <>
__device__ __forceinline__ void atomic_max_idx<int64_t>(int64_t* p, int64_t v) {
  atomicMax(reinterpret_cast<long long*>(p), static_cast<long long>(v));
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    relabel_claim_kernel(const IdxT* __restrict__ src, int64_t m,
                         const int64_t* __restrict__ m_dev, IdxT* __restrict__ local) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (m_dev && *m_dev < m) m = *m_dev;
  if (e < m) atomic_max_idx<IdxT>(local + src[e], static_cast<IdxT>(-(e + 2)));
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    relabel_flag_kernel(const IdxT* __restrict__ src, int64_t m,
                        const int64_t* __restrict__ m_dev, const IdxT* __restrict__ local,
                        int64_t* __restrict__ flag) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= m) return;
  const bool valid = !m_dev || e < *m_dev;  // the padding flags 0: the scan stays fixed-size
  flag[e] = (valid && static_cast<int64_t>(local[src[e]]) == -(e + 2)) ? 1 : 0;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    relabel_assign_kernel(const IdxT* __restrict__ src, int64_t m,
                          const int64_t* __restrict__ m_dev, const int64_t* __restrict__ scan,
                          int64_t base, const int64_t* __restrict__ base_dev,
                          IdxT* __restrict__ local, IdxT* __restrict__ new_nodes) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (m_dev && *m_dev < m) m = *m_dev;
  if (e >= m) return;
  if (base_dev) base = *base_dev;
  const int64_t prev = (e == 0) ? 0 : scan[e - 1];
  if (scan[e] != prev) {  // this entry claimed its source
    const IdxT s = src[e];
    local[s] = static_cast<IdxT>(base + prev);
    new_nodes[prev] = s;
  }
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    relabel_lookup_kernel(const IdxT* __restrict__ src, int64_t m,
                          const int64_t* __restrict__ m_dev, const IdxT* __restrict__ local,
                          IdxT* __restrict__ out) {
  const int64_t e = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (e >= m) return;
  out[e] = (!m_dev || e < *m_dev) ? local[src[e]] : static_cast<IdxT>(0);
}

// ---- negative draws of link-level sampling (the reference's neg_sample / NegativeSampling.sample,
// sampler/neighbor_sampler.py:1051-1096, sampler/base.py:906-929).  One thread per draw j; round r
// of draw j hashes (seed, j, r).  The candidate is uniform over [0, N) (multiply-high of 64 hash
// bits) or, with a CDF, the first i with cdf[i] > u, u uniform in [0, cdf[N-1]).  With node times a
// candidate is accepted iff node_time[c] <= bound[j % n_bound]; kNegRounds candidates are tried in
// registers (the reference's first draw and its 5 retries), then `fallback` is written.
constexpr int kNegRounds = 6;
constexpr uint64_t kNegSalt = 0x6E65676174697665ull;  // "negative": a stream of its own

__device__ __forceinline__ int64_t negative_candidate(uint64_t h, int64_t num_nodes,
                                                      const double* __restrict__ cdf,
                                                      double total) {
  if (!cdf) return static_cast<int64_t>(__umul64hi(h, static_cast<uint64_t>(num_nodes)));
  // 53 hash bits -> [0, 1); a product that rounds up to `total` is pulled just below it, so the
  // search always lands on a node whose weight moved the CDF
  double u = static_cast<double>(h >> 11) * 0x1p-53 * total;
  if (!(u < total)) u = nextafter(total, 0.0);
  int64_t lo = 0, hi = num_nodes - 1;  // the first i with cdf[i] > u lies in [lo, hi]
  while (lo < hi) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (cdf[mid] > u) hi = mid; else lo = mid + 1;
  }
  return lo;
}

// draw j of the stream `key` (= mix64(seed ^ kNegSalt)): the candidate rounds and the `<=` rule
__device__ __forceinline__ int64_t negative_draw(uint64_t key, int64_t j, int64_t num_nodes,
                                                 const double* __restrict__ cdf,
                                                 const int64_t* __restrict__ node_time, int64_t t,
                                                 int64_t fallback) {
  const double total = cdf ? cdf[num_nodes - 1] : 0.0;
  const uint64_t base = static_cast<uint64_t>(j) * 8u;
  int64_t c = negative_candidate(mix64(key + base), num_nodes, cdf, total);
  if (node_time) {
    bool ok = node_time[c] <= t;
    for (int r = 1; r < kNegRounds && !ok; ++r) {
      c = negative_candidate(mix64(key + base + static_cast<uint64_t>(r)), num_nodes, cdf, total);
      ok = node_time[c] <= t;
    }
    if (!ok) c = fallback;
  }
  return c;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    sample_negatives_kernel(int64_t n, int64_t num_nodes, uint64_t seed,
                            const uint64_t* __restrict__ seed_dev, const double* __restrict__ cdf,
                            const int64_t* __restrict__ node_time,
                            const int64_t* __restrict__ bound, int64_t n_bound, int64_t fallback,
                            IdxT* __restrict__ out) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= n) return;
  if (seed_dev) seed = mix64(seed ^ mix64(*seed_dev * 0x9E3779B97F4A7C15ull));
  const uint64_t key = mix64(seed ^ kNegSalt);
  const int64_t t = node_time ? bound[j % n_bound] : 0;
  out[j] = static_cast<IdxT>(negative_draw(key, j, num_nodes, cdf, node_time, t, fallback));
}

// ---- the typed seed block of a heterogeneous edge batch (the reference's edge_sample, heterogeneous
// branch, sampler/neighbor_sampler.py:852-937): seeds = [source block | destination block] as global
// ids of the stacked id space, one thread per slot.  Slot j of an endpoint is the positive j for
// j < n_pos and otherwise draw j - n_pos of pygamd_sample_negatives' stream seed * 2 + endpoint with
// that endpoint's num_nodes / cdf / node_time / fallback and the bound link_time[j % n_pos];
// seed_time[slot] = link_time[j % n_pos] (the reference's `repeat`).  The two endpoints' values
// travel in the kernel arguments, like the hop table of the typed layer below.
struct LinkEndpoint {
  int64_t n;          // slots of this endpoint: n_pos, or n_pos + num_neg
  int64_t num_nodes;
  int64_t node_base;
  int64_t fallback;
  const double* cdf;          // fp64 [num_nodes] or NULL (uniform)
  const int64_t* node_time;   // int64 [num_nodes] or NULL (untimed type / edge-level time)
};

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_link_seeds_kernel(const IdxT* __restrict__ src, const IdxT* __restrict__ dst,
                             int64_t n_pos, const LinkEndpoint e_src, const LinkEndpoint e_dst,
                             uint64_t seed, const int64_t* __restrict__ link_time,
                             IdxT* __restrict__ seeds, int64_t* __restrict__ seed_time) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= e_src.n + e_dst.n) return;
  const bool is_dst = i >= e_src.n;
  const int64_t j = is_dst ? i - e_src.n : i;
  // (selected field by field: indexing a two-entry argument array would spill it to scratch)
  const int64_t num_nodes = is_dst ? e_dst.num_nodes : e_src.num_nodes;
  const int64_t node_base = is_dst ? e_dst.node_base : e_src.node_base;
  const int64_t t = link_time ? link_time[j % n_pos] : 0;
  int64_t c;
  if (j < n_pos) {
    c = static_cast<int64_t>((is_dst ? dst : src)[j]);
  } else {
    const uint64_t key = mix64((seed * 2u + (is_dst ? 1u : 0u)) ^ kNegSalt);
    c = negative_draw(key, j - n_pos, num_nodes, is_dst ? e_dst.cdf : e_src.cdf,
                      is_dst ? e_dst.node_time : e_src.node_time, t,
                      is_dst ? e_dst.fallback : e_src.fallback);
  }
  seeds[i] = static_cast<IdxT>(c + node_base);
  if (seed_time) seed_time[i] = t;
}

// ---- torch.unique(keys, return_inverse=True) on the output of index_sort: rank[i] = 1 where a run
// of equal sorted keys starts (then scanned inclusively by pygamd_cumsum), and the scatter
// uniq[rank - 1] = key (run heads), inverse[perm[i]] = rank[i] - 1, *n_unique = rank[n - 1].
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    unique_heads_kernel(const IdxT* __restrict__ sorted, int64_t n, int64_t* __restrict__ rank) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  rank[i] = (i == 0 || sorted[i] != sorted[i - 1]) ? 1 : 0;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    unique_scatter_kernel(const IdxT* __restrict__ sorted, const int64_t* __restrict__ perm,
                          int64_t n, const int64_t* __restrict__ rank, IdxT* __restrict__ uniq,
                          int64_t* __restrict__ inverse, int64_t* __restrict__ n_unique) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= n) return;
  const int64_t r = rank[i] - 1;
  if (i == 0 || rank[i - 1] != rank[i]) uniq[r] = sorted[i];
  inverse[perm[i]] = r;
  if (i == n - 1) n_unique[0] = r + 1;
}

// ---- heterogeneous hops (the reference's NeighborLoader(hetero_data, ...) ->
// torch.ops.pyg.hetero_neighbor_sample(..., csc=True, ...), sampler/neighbor_sampler.py:438-548).
// Every edge type lives in ONE stacked CSC: node i of type t is the global id node_base[t] + i, edge
// type et owns the columns [col_base[et], col_base[et] + N_dst(et)), `row` holds global source ids
// and `perm` each slot's position in its own type's edge_index.  A hop's work list is the
// concatenation, in edge-type order, of the frontier block of every edge type's destination type:
// item i belongs to the edge type et with item_begin[et] <= i < item_begin[et + 1] and sits at
// p = i - item_begin[et] in that block, which starts at frontier_off[et] of the type-major frontier
// buffer (global ids).  Its column is frontier[frontier_off[et] + p] + col_off[et] (col_off =
// col_base - node_base[dst]).  The per-edge-type values travel in the kernel arguments, so ONE
// launch serves every edge type of a hop.
constexpr int kMaxEdgeTypes = 64;
constexpr int kMaxNodeTypes = 64;

struct HeteroHop {
  int64_t item_begin[kMaxEdgeTypes + 1];
  int64_t frontier_off[kMaxEdgeTypes];
  int64_t col_off[kMaxEdgeTypes];
  int64_t dst_local[kMaxEdgeTypes];  // typed local id of the block's first node (-> col)
  int32_t k[kMaxEdgeTypes];          // fan-out of the hop, -1 = every in-neighbour
  int32_t n_et;
};

// the edge type of work item i: the last et with item_begin[et] <= i (empty types skipped)
__device__ __forceinline__ int hetero_edge_type(const HeteroHop& h, int64_t i) {
  int lo = 0, hi = h.n_et - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (h.item_begin[mid] <= i) lo = mid; else hi = mid - 1;
  }
  return lo;
}

// work item i decoded: its edge type, its position p in that type's frontier block, its position
// fp in the frontier buffer and its stacked column
struct HeteroItem {
  int et;
  int64_t p, fp, col;
};

template <typename IdxT>
__device__ __forceinline__ HeteroItem hetero_item(const HeteroHop& h,
                                                  const IdxT* __restrict__ frontier, int64_t i) {
  HeteroItem it;
  it.et = hetero_edge_type(h, i);
  it.p = i - h.item_begin[it.et];
  it.fp = h.frontier_off[it.et] + it.p;
  it.col = static_cast<int64_t>(frontier[it.fp]) + h.col_off[it.et];
  return it;
}

// cnt[i] = window_count on item i's column with the k of its edge type
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_counts_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ frontier,
                         const HeteroHop hop, int replace, IdxT* __restrict__ cnt) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (i >= hop.item_begin[hop.n_et]) return;
  const HeteroItem it = hetero_item(hop, frontier, i);
  const int64_t deg =
      static_cast<int64_t>(colptr[it.col + 1]) - static_cast<int64_t>(colptr[it.col]);
  cnt[i] = static_cast<IdxT>(window_count(deg, hop.k[it.et], replace != 0));
}

// One wave per work item: draw_uniform on the item's column, or on its window [lo[i], hi[i]) when
// lo / hi are given (colptr is not read then), keyed by the stacked column id and the item's
// position (a single type with col_base = 0 draws what sample_neighbors_kernel draws);
// replacement only where the item's edge type has a bounded fan-out.  Writes the global source,
// the typed local destination (dst_local + p), the edge id perm[slot] and, when fpos_out is given,
// the destination's position in the frontier buffer.
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_sample_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ row,
                         const IdxT* __restrict__ perm, const IdxT* __restrict__ frontier,
                         const IdxT* __restrict__ lo, const IdxT* __restrict__ hi,
                         const IdxT* __restrict__ offsets, const HeteroHop hop, uint64_t seed,
                         int flags, IdxT* __restrict__ src_out, IdxT* __restrict__ col_out,
                         IdxT* __restrict__ edge_out, IdxT* __restrict__ fpos_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (i >= hop.item_begin[hop.n_et]) return;
  const int64_t o = offsets[i];
  const int64_t cnt = static_cast<int64_t>(offsets[i + 1]) - o;
  if (cnt <= 0) return;
  const HeteroItem it = hetero_item(hop, frontier, i);
  const int64_t s = lo ? lo[i] : colptr[it.col];
  const int64_t deg = static_cast<int64_t>(lo ? hi[i] : colptr[it.col + 1]) - s;
  const uint64_t key = node_key(seed, nullptr, it.col, i, flags);
  const bool rep = (flags & 1) != 0 && hop.k[it.et] >= 0;
  draw_uniform(row, s, deg, o, cnt, hop.dst_local[it.et] + it.p, key, rep, src_out, col_out,
               edge_out, perm);
  if (fpos_out) {
    for (int64_t t = lane_id(); t < cnt; t += kWave) fpos_out[o + t] = static_cast<IdxT>(it.fp);
  }
}

// ---- temporal heterogeneous hops (the reference's NeighborLoader(hetero_data, time_attr=...) ->
// hetero_neighbor_sample(..., node_time, edge_time, seed_time, ..., temporal_strategy)).  The
// stacked CSC keeps the slots of every column of a TIMED edge type ascending in time (bit et of
// `timed`: the source type has node times, or the edge type edge times); `time` is int64 over the
// global node ids (level 0) or over the slots (level 1).  One wave per work item: the window of a
// timed item is the prefix of its column with time <= frontier_time[fp] (the seed time of the tree
// of the destination at frontier position fp), found by temporal_window_end and narrowed by
// 'last'; an untimed item's window is its whole column.  cnt is window_count on the window, so
// this launch takes the place of the counts launch; hetero_sample_kernel then draws on the windows
// (one node type with one edge type: what sample_neighbors_kernel draws on them).
template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_temporal_window_kernel(const IdxT* __restrict__ colptr, const IdxT* __restrict__ row,
                                  const int64_t* __restrict__ time, int level,
                                  const IdxT* __restrict__ frontier,
                                  const int64_t* __restrict__ frontier_time, const HeteroHop hop,
                                  uint64_t timed, int replace, int last,
                                  IdxT* __restrict__ lo_out, IdxT* __restrict__ hi_out,
                                  IdxT* __restrict__ cnt_out) {
  const int64_t i = static_cast<int64_t>(blockIdx.x) * kWavesPerBlock + wave_in_block();
  if (i >= hop.item_begin[hop.n_et]) return;
  const HeteroItem it = hetero_item(hop, frontier, i);
  const int64_t s = colptr[it.col];
  const int64_t end = colptr[it.col + 1];
  const bool is_timed = ((timed >> it.et) & 1ull) != 0;
  const int64_t hi =
      is_timed ? temporal_window_end(row, time, level, s, end, frontier_time[it.fp]) : end;
  const int64_t k = hop.k[it.et];
  const int64_t lo = temporal_window_lo(s, hi, k, last != 0 && is_timed);
  if (lane_id() == 0) {
    lo_out[i] = static_cast<IdxT>(lo);
    hi_out[i] = static_cast<IdxT>(hi);
    cnt_out[i] = static_cast<IdxT>(window_count(hi - lo, k, replace != 0));
  }
}

// ---- the typed split of a hop's new nodes (global ids in order of first appearance, the first
// *n_new of new_nodes[m]): a stable partition by node type.  Phase 0 writes the one-hot matrix
// flag[t * m + j] = (type(new_nodes[j]) == t), which the caller scans inclusively as ONE vector of
// n_t * m entries; then scan[t * m + j] - 1 is node j's position in the type-major order and
// scan[t * m + j] - scan[t * m - 1] - 1 its rank among the new nodes of its type.  Phase 1 turns
// that into the typed local id count_prev[t] + rank (into local[g] and / or typed_out[j]), writes
// the type-major buffers (global id, id inside the type, aux payload) and the hop's stats: the new
// nodes per type, then offsets[item_begin[et]] for et = 0 .. n_et (the edge boundaries).
struct HeteroTypes {
  int64_t node_base[kMaxNodeTypes + 1];
  int64_t count_prev[kMaxNodeTypes];
  int64_t item_begin[kMaxEdgeTypes + 1];
  int32_t n_t;
  int32_t n_et;
};

__device__ __forceinline__ int hetero_node_type(const HeteroTypes& h, int64_t g) {
  int lo = 0, hi = h.n_t - 1;  // the last t with node_base[t] <= g
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (h.node_base[mid] <= g) lo = mid; else hi = mid - 1;
  }
  return lo;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_split_flag_kernel(const IdxT* __restrict__ new_nodes, int64_t m,
                             const int64_t* __restrict__ n_new, const HeteroTypes types,
                             int64_t* __restrict__ flag) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j >= m) return;
  const int t = j < *n_new ? hetero_node_type(types, new_nodes[j]) : -1;
  for (int u = 0; u < types.n_t; ++u) flag[u * m + j] = (u == t) ? 1 : 0;
}

template <typename IdxT>
__global__ void __launch_bounds__(kBlock)
    hetero_split_apply_kernel(const IdxT* __restrict__ new_nodes, int64_t m,
                              const int64_t* __restrict__ n_new, const int64_t* __restrict__ scan,
                              const HeteroTypes types, const IdxT* __restrict__ offsets,
                              const int64_t* __restrict__ aux_in, IdxT* __restrict__ local,
                              IdxT* __restrict__ typed_out, IdxT* __restrict__ sorted_global,
                              IdxT* __restrict__ sorted_local, int64_t* __restrict__ aux_out,
                              int64_t* __restrict__ stats) {
  const int64_t j = static_cast<int64_t>(blockIdx.x) * kBlock + threadIdx.x;
  if (j < types.n_t) {
    stats[j] = scan[(j + 1) * m - 1] - (j > 0 ? scan[j * m - 1] : 0);
  }
  if (j <= types.n_et) {
    stats[types.n_t + j] = offsets ? static_cast<int64_t>(offsets[types.item_begin[j]]) : 0;
  }
  if (j >= m || j >= *n_new) return;
  const int64_t g = new_nodes[j];
  const int t = hetero_node_type(types, g);
  const int64_t before = t > 0 ? scan[t * m - 1] : 0;
  const int64_t r = scan[t * m + j] - 1;
  const int64_t typed = types.count_prev[t] + (r - before);
  if (local) local[g] = static_cast<IdxT>(typed);
  if (typed_out) typed_out[j] = static_cast<IdxT>(typed);
  sorted_global[r] = static_cast<IdxT>(g);
  sorted_local[r] = static_cast<IdxT>(g - types.node_base[t]);
  if (aux_in) aux_out[r] = aux_in[j];
}

}  // namespace pygamd

using namespace pygamd;

extern "C" {

int pygamd_sample_max_fanout(void) { return kMaxFanout; }

// the launch of sample_neighbors_kernel behind both of its entry points (lo / hi NULL: the columns)
static int launch_sample_neighbors(const void* colptr, const void* row, int idx_dtype,
                                   const void* frontier, int64_t n_frontier, const void* lo,
                                   const void* hi, const void* offsets, uint64_t seed, int flags,
                                   const uint64_t* seed_dev, void* src_out, void* dstpos_out,
                                   void* slot_out, void* stream) {
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const unsigned grid = static_cast<unsigned>(ceil_div(n_frontier, kWavesPerBlock));
    hipLaunchKernelGGL((sample_neighbors_kernel<IdxT>), dim3(grid), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(row), static_cast<const IdxT*>(frontier),
                       n_frontier, static_cast<const IdxT*>(lo), static_cast<const IdxT*>(hi),
                       static_cast<const IdxT*>(offsets), seed, flags, seed_dev,
                       static_cast<IdxT*>(src_out), static_cast<IdxT*>(dstpos_out),
                       static_cast<IdxT*>(slot_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_sample_neighbors(const void* colptr, const void* row, int idx_dtype,
                            const void* frontier, int64_t n_frontier, const void* offsets,
                            int64_t max_per_node, uint64_t seed, int flags,
                            const uint64_t* seed_dev, void* src_out,
                            void* dstpos_out, void* slot_out, void* stream) {
  if (n_frontier < 0) return PYGAMD_ERR_INVALID_ARG;
  if (n_frontier == 0) return PYGAMD_OK;
  if (!colptr || !row || !frontier || !offsets || !src_out || !dstpos_out || !slot_out)
    return PYGAMD_ERR_INVALID_ARG;
  // a bounded fan-out larger than the LDS draw table is not supported (k < 0 = "all" is)
  if (max_per_node > kMaxFanout) return PYGAMD_ERR_UNSUPPORTED;
  if ((flags & 1) && max_per_node <= 0) return PYGAMD_ERR_INVALID_ARG;  // "all": no replacement
  return launch_sample_neighbors(colptr, row, idx_dtype, frontier, n_frontier, nullptr, nullptr,
                                 offsets, seed, flags, seed_dev, src_out, dstpos_out, slot_out,
                                 stream);
}

int pygamd_sample_neighbors_weighted(const void* colptr, const void* row, int idx_dtype,
                                     const float* weight_csc, const void* frontier,
                                     int64_t n_frontier, const void* offsets,
                                     int64_t max_per_node, uint64_t seed, int flags,
                                     const uint64_t* seed_dev, void* src_out, void* dstpos_out,
                                     void* slot_out, void* stream) {
  if (n_frontier < 0 || !weight_csc) return PYGAMD_ERR_INVALID_ARG;
  if (max_per_node > kMaxFanout) return PYGAMD_ERR_UNSUPPORTED;  // one key per lane
  if (n_frontier == 0) return PYGAMD_OK;
  if (!colptr || !row || !frontier || !offsets || !src_out || !dstpos_out || !slot_out)
    return PYGAMD_ERR_INVALID_ARG;
  if ((flags & 1) && max_per_node <= 0) return PYGAMD_ERR_INVALID_ARG;  // "all": no replacement
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const unsigned grid = static_cast<unsigned>(ceil_div(n_frontier, kWavesPerBlock));
    hipLaunchKernelGGL((sample_neighbors_weighted_kernel<IdxT>), dim3(grid), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(row), weight_csc,
                       static_cast<const IdxT*>(frontier), n_frontier,
                       static_cast<const IdxT*>(offsets), seed, flags, seed_dev,
                       static_cast<IdxT*>(src_out), static_cast<IdxT*>(dstpos_out),
                       static_cast<IdxT*>(slot_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_sample_temporal_window(const void* colptr, const void* row, int idx_dtype,
                                  const int64_t* time, int level, const void* frontier,
                                  const int64_t* frontier_time, int64_t n_frontier, int64_t k,
                                  int replace, int strategy, const int64_t* n_valid,
                                  void* lo_out, void* hi_out, void* cnt_out, void* stream) {
  if (n_frontier < 0 || !time || !frontier_time) return PYGAMD_ERR_INVALID_ARG;
  if ((level != 0 && level != 1) || (strategy != 0 && strategy != 1))
    return PYGAMD_ERR_INVALID_ARG;
  if (k > kMaxFanout) return PYGAMD_ERR_UNSUPPORTED;
  if (replace && k < 0) return PYGAMD_ERR_INVALID_ARG;  // "all": no replacement
  if (n_frontier == 0) return PYGAMD_OK;
  if (!colptr || !row || !frontier || !lo_out || !hi_out || !cnt_out)
    return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const unsigned grid = static_cast<unsigned>(ceil_div(n_frontier, kWavesPerBlock));
    hipLaunchKernelGGL((sample_temporal_window_kernel<IdxT>), dim3(grid), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(row), time, level,
                       static_cast<const IdxT*>(frontier), frontier_time, n_frontier, k,
                       replace ? 1 : 0, strategy, n_valid, static_cast<IdxT*>(lo_out),
                       static_cast<IdxT*>(hi_out), static_cast<IdxT*>(cnt_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_sample_neighbors_temporal(const void* row, int idx_dtype, const void* frontier,
                                     int64_t n_frontier, const void* lo, const void* hi,
                                     const void* offsets, int64_t max_per_node, uint64_t seed,
                                     int flags, const uint64_t* seed_dev, void* src_out,
                                     void* dstpos_out, void* slot_out, void* stream) {
  if (n_frontier < 0 || !lo || !hi) return PYGAMD_ERR_INVALID_ARG;
  if (max_per_node > kMaxFanout) return PYGAMD_ERR_UNSUPPORTED;
  if ((flags & 1) && max_per_node <= 0) return PYGAMD_ERR_INVALID_ARG;  // "all": no replacement
  if (n_frontier == 0) return PYGAMD_OK;
  if (!row || !frontier || !offsets || !src_out || !dstpos_out || !slot_out)
    return PYGAMD_ERR_INVALID_ARG;
  return launch_sample_neighbors(nullptr, row, idx_dtype, frontier, n_frontier, lo, hi, offsets,
                                 seed, flags, seed_dev, src_out, dstpos_out, slot_out, stream);
}

int pygamd_sample_counts(const void* colptr, int idx_dtype, const void* frontier, int64_t n,
                         int64_t k, int replace, const int64_t* n_valid, void* cnt_out,
                         void* stream) {
  if (n < 0) return PYGAMD_ERR_INVALID_ARG;
  if (n == 0) return PYGAMD_OK;
  if (!colptr || !frontier || !cnt_out) return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((sample_counts_kernel<IdxT>),
                       dim3(static_cast<unsigned>(ceil_div(n, kBlock))), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(frontier), n, k, replace ? 1 : 0, n_valid,
                       static_cast<IdxT*>(cnt_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_relabel(int phase, const void* src, int idx_dtype, int64_t m, const int64_t* m_dev,
                   void* local_map, int64_t* flag_or_scan, int64_t base,
                   const int64_t* base_dev, void* out, void* stream) {
  if (m < 0 || phase < 0 || phase > 3) return PYGAMD_ERR_INVALID_ARG;
  if (m == 0) return PYGAMD_OK;
  if (!src || !local_map) return PYGAMD_ERR_INVALID_ARG;
  if ((phase == 1 || phase == 2) && !flag_or_scan) return PYGAMD_ERR_INVALID_ARG;
  if ((phase == 2 || phase == 3) && !out) return PYGAMD_ERR_INVALID_ARG;
  const dim3 grid(static_cast<unsigned>(ceil_div(m, kBlock)));
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const IdxT* s = static_cast<const IdxT*>(src);
    IdxT* local = static_cast<IdxT*>(local_map);
    switch (phase) {
      case 0:
        hipLaunchKernelGGL((relabel_claim_kernel<IdxT>), grid, dim3(kBlock), 0, st, s, m, m_dev,
                           local);
        break;
      case 1:
        hipLaunchKernelGGL((relabel_flag_kernel<IdxT>), grid, dim3(kBlock), 0, st, s, m, m_dev,
                           local, flag_or_scan);
        break;
      case 2:
        hipLaunchKernelGGL((relabel_assign_kernel<IdxT>), grid, dim3(kBlock), 0, st, s, m, m_dev,
                           flag_or_scan, base, base_dev, local, static_cast<IdxT*>(out));
        break;
      default:
        hipLaunchKernelGGL((relabel_lookup_kernel<IdxT>), grid, dim3(kBlock), 0, st, s, m, m_dev,
                           local, static_cast<IdxT*>(out));
    }
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_sample_negatives(int64_t n, int64_t num_nodes, uint64_t seed, const uint64_t* seed_dev,
                            const double* cdf, const int64_t* node_time, const int64_t* bound,
                            int64_t n_bound, int64_t fallback, int out_dtype, void* out,
                            void* stream) {
  if (n < 0) return PYGAMD_ERR_INVALID_ARG;
  if (out_dtype != PYGAMD_IDX_I32 && out_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (out_dtype == PYGAMD_IDX_I32 && num_nodes > INT32_MAX) return PYGAMD_ERR_INVALID_ARG;
  if (!node_time && bound) return PYGAMD_ERR_INVALID_ARG;  // a bound without times to test
  if (node_time && (!bound || n_bound <= 0 || fallback < 0 || fallback >= num_nodes))
    return PYGAMD_ERR_INVALID_ARG;
  if (n == 0) return PYGAMD_OK;
  if (num_nodes <= 0 || !out) return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_DISPATCH_IDX(out_dtype, [&]() -> int {
    hipLaunchKernelGGL((sample_negatives_kernel<IdxT>),
                       dim3(static_cast<unsigned>(ceil_div(n, kBlock))), dim3(kBlock), 0,
                       as_stream(stream), n, num_nodes, seed, seed_dev, cdf, node_time, bound,
                       n_bound, fallback, static_cast<IdxT*>(out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_unique_inverse(const void* keys_sorted, const int64_t* perm, int idx_dtype, int64_t n,
                          int64_t* rank, void* workspace, size_t workspace_bytes, void* uniq_out,
                          int64_t* inverse_out, int64_t* n_unique, void* stream) {
  if (n < 0) return PYGAMD_ERR_INVALID_ARG;
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  if (n == 0) return PYGAMD_OK;
  if (!keys_sorted || !perm || !rank || !workspace || !uniq_out || !inverse_out || !n_unique)
    return PYGAMD_ERR_INVALID_ARG;
  size_t need = 0;
  int rc = pygamd_cumsum_workspace_bytes(PYGAMD_IDX_I64, n, &need);
  if (rc != PYGAMD_OK) return rc;
  if (workspace_bytes < need) return PYGAMD_ERR_WORKSPACE;
  const dim3 grid(static_cast<unsigned>(ceil_div(n, kBlock)));
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const IdxT* keys = static_cast<const IdxT*>(keys_sorted);
    hipLaunchKernelGGL((unique_heads_kernel<IdxT>), grid, dim3(kBlock), 0, st, keys, n, rank);
    PYGAMD_LAUNCH_CHECK();
    const int scan_rc = pygamd_cumsum(rank, PYGAMD_IDX_I64, n, rank, workspace, workspace_bytes,
                                      stream);
    if (scan_rc != PYGAMD_OK) return scan_rc;
    hipLaunchKernelGGL((unique_scatter_kernel<IdxT>), grid, dim3(kBlock), 0, st, keys, perm, n,
                       rank, static_cast<IdxT*>(uniq_out), inverse_out, n_unique);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_hetero_link_seeds(const void* src, const void* dst, int idx_dtype, int64_t n_pos,
                             int64_t num_neg, int mode, const int64_t* link_time,
                             const int64_t* ep_table, const double* src_cdf, const double* dst_cdf,
                             const int64_t* src_node_time, const int64_t* dst_node_time,
                             uint64_t seed, void* seeds_out, int64_t* seed_time_out,
                             void* stream) {
  if (mode < PYGAMD_LINK_NEG_NONE || mode > PYGAMD_LINK_NEG_TRIPLET) return PYGAMD_ERR_INVALID_ARG;
  if (n_pos < 0 || num_neg < 0 || !ep_table) return PYGAMD_ERR_INVALID_ARG;
  if (mode == PYGAMD_LINK_NEG_NONE && num_neg != 0) return PYGAMD_ERR_INVALID_ARG;
  if (idx_dtype != PYGAMD_IDX_I32 && idx_dtype != PYGAMD_IDX_I64) return PYGAMD_ERR_INVALID_ARG;
  LinkEndpoint ep[2];
  for (int e = 0; e < 2; ++e) {
    ep[e].num_nodes = ep_table[3 * e];
    ep[e].node_base = ep_table[3 * e + 1];
    ep[e].fallback = ep_table[3 * e + 2];
    ep[e].cdf = e ? dst_cdf : src_cdf;
    ep[e].node_time = e ? dst_node_time : src_node_time;
    const bool draws = mode == PYGAMD_LINK_NEG_BINARY || (e == 1 && mode == PYGAMD_LINK_NEG_TRIPLET);
    ep[e].n = n_pos + (draws ? num_neg : 0);
    if (ep[e].num_nodes < 0 || ep[e].node_base < 0) return PYGAMD_ERR_INVALID_ARG;
    if (idx_dtype == PYGAMD_IDX_I32 && ep[e].node_base + ep[e].num_nodes > INT32_MAX)
      return PYGAMD_ERR_INVALID_ARG;
    if (ep[e].node_time && !link_time) return PYGAMD_ERR_INVALID_ARG;  // times without a bound
    if (ep[e].node_time && (ep[e].fallback < 0 || ep[e].fallback >= ep[e].num_nodes))
      return PYGAMD_ERR_INVALID_ARG;
    if (draws && num_neg > 0 && n_pos > 0 && ep[e].num_nodes <= 0) return PYGAMD_ERR_INVALID_ARG;
  }
  if (link_time && !seed_time_out) return PYGAMD_ERR_INVALID_ARG;
  if (n_pos == 0) return num_neg == 0 ? PYGAMD_OK : PYGAMD_ERR_INVALID_ARG;  // no link to bound by
  if (!src || !dst || !seeds_out) return PYGAMD_ERR_INVALID_ARG;
  const int64_t n = ep[0].n + ep[1].n;
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((hetero_link_seeds_kernel<IdxT>),
                       dim3(static_cast<unsigned>(ceil_div(n, kBlock))), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(src),
                       static_cast<const IdxT*>(dst), n_pos, ep[0], ep[1], seed, link_time,
                       static_cast<IdxT*>(seeds_out), link_time ? seed_time_out : nullptr);
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

// the kernel-argument table of a hop from the caller's host arrays (see pyg_amd.h)
static int fill_hetero_hop(const int64_t* item_begin, const int64_t* et_table, int n_et,
                           HeteroHop* hop) {
  if (n_et <= 0 || n_et > kMaxEdgeTypes || !item_begin || !et_table) return PYGAMD_ERR_INVALID_ARG;
  if (item_begin[0] != 0) return PYGAMD_ERR_INVALID_ARG;
  hop->n_et = n_et;
  for (int e = 0; e < n_et; ++e) {
    if (item_begin[e + 1] < item_begin[e]) return PYGAMD_ERR_INVALID_ARG;
    const int64_t k = et_table[4 * e + 3];
    if (k > kMaxFanout) return PYGAMD_ERR_UNSUPPORTED;
    if (k < -1 || et_table[4 * e] < 0 || et_table[4 * e + 2] < 0) return PYGAMD_ERR_INVALID_ARG;
    hop->item_begin[e] = item_begin[e];
    hop->frontier_off[e] = et_table[4 * e];
    hop->col_off[e] = et_table[4 * e + 1];
    hop->dst_local[e] = et_table[4 * e + 2];
    hop->k[e] = static_cast<int32_t>(k);
  }
  hop->item_begin[n_et] = item_begin[n_et];
  return PYGAMD_OK;
}

int pygamd_hetero_sample_counts(const void* colptr, int idx_dtype, const void* frontier,
                                const int64_t* item_begin, const int64_t* et_table, int n_et,
                                int replace, void* cnt_out, void* stream) {
  HeteroHop hop;
  const int rc = fill_hetero_hop(item_begin, et_table, n_et, &hop);
  if (rc != PYGAMD_OK) return rc;
  const int64_t n = hop.item_begin[n_et];
  if (n == 0) return PYGAMD_OK;
  if (!colptr || !frontier || !cnt_out) return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    hipLaunchKernelGGL((hetero_counts_kernel<IdxT>),
                       dim3(static_cast<unsigned>(ceil_div(n, kBlock))), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(frontier), hop, replace ? 1 : 0,
                       static_cast<IdxT*>(cnt_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

// the launch of hetero_sample_kernel behind both of its entry points (lo / hi NULL: the columns)
static int launch_hetero_sample(const void* colptr, const void* row, const void* perm,
                                int idx_dtype, const void* frontier, const void* lo,
                                const void* hi, const void* offsets, const HeteroHop& hop,
                                uint64_t seed, int flags, void* src_out, void* col_out,
                                void* edge_out, void* fpos_out, void* stream) {
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const unsigned grid =
        static_cast<unsigned>(ceil_div(hop.item_begin[hop.n_et], kWavesPerBlock));
    hipLaunchKernelGGL((hetero_sample_kernel<IdxT>), dim3(grid), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(row), static_cast<const IdxT*>(perm),
                       static_cast<const IdxT*>(frontier), static_cast<const IdxT*>(lo),
                       static_cast<const IdxT*>(hi), static_cast<const IdxT*>(offsets), hop, seed,
                       flags, static_cast<IdxT*>(src_out), static_cast<IdxT*>(col_out),
                       static_cast<IdxT*>(edge_out), static_cast<IdxT*>(fpos_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_hetero_sample_neighbors(const void* colptr, const void* row, const void* perm,
                                   int idx_dtype, const void* frontier, const void* offsets,
                                   const int64_t* item_begin, const int64_t* et_table, int n_et,
                                   uint64_t seed, int flags, void* src_out, void* col_out,
                                   void* edge_out, void* fpos_out, void* stream) {
  HeteroHop hop;
  const int rc = fill_hetero_hop(item_begin, et_table, n_et, &hop);
  if (rc != PYGAMD_OK) return rc;
  if (hop.item_begin[n_et] == 0) return PYGAMD_OK;
  if (!colptr || !row || !perm || !frontier || !offsets || !src_out || !col_out || !edge_out)
    return PYGAMD_ERR_INVALID_ARG;
  return launch_hetero_sample(colptr, row, perm, idx_dtype, frontier, nullptr, nullptr, offsets,
                              hop, seed, flags, src_out, col_out, edge_out, fpos_out, stream);
}

int pygamd_hetero_sample_temporal_window(const void* colptr, const void* row, int idx_dtype,
                                         const int64_t* time, int level, const void* frontier,
                                         const int64_t* frontier_time, const int64_t* item_begin,
                                         const int64_t* et_table, int n_et, uint64_t timed_mask,
                                         int replace, int strategy, void* lo_out, void* hi_out,
                                         void* cnt_out, void* stream) {
  if ((level != 0 && level != 1) || (strategy != 0 && strategy != 1))
    return PYGAMD_ERR_INVALID_ARG;
  HeteroHop hop;
  const int rc = fill_hetero_hop(item_begin, et_table, n_et, &hop);
  if (rc != PYGAMD_OK) return rc;
  if (n_et < kMaxEdgeTypes && (timed_mask >> n_et) != 0) return PYGAMD_ERR_INVALID_ARG;
  if (!time || !frontier_time) return PYGAMD_ERR_INVALID_ARG;
  const int64_t n = hop.item_begin[n_et];
  if (n == 0) return PYGAMD_OK;
  if (!colptr || !row || !frontier || !lo_out || !hi_out || !cnt_out)
    return PYGAMD_ERR_INVALID_ARG;
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const unsigned grid = static_cast<unsigned>(ceil_div(n, kWavesPerBlock));
    hipLaunchKernelGGL((hetero_temporal_window_kernel<IdxT>), dim3(grid), dim3(kBlock), 0,
                       as_stream(stream), static_cast<const IdxT*>(colptr),
                       static_cast<const IdxT*>(row), time, level,
                       static_cast<const IdxT*>(frontier), frontier_time, hop, timed_mask,
                       replace ? 1 : 0, strategy, static_cast<IdxT*>(lo_out),
                       static_cast<IdxT*>(hi_out), static_cast<IdxT*>(cnt_out));
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

int pygamd_hetero_sample_neighbors_temporal(const void* row, const void* perm, int idx_dtype,
                                            const void* frontier, const void* lo, const void* hi,
                                            const void* offsets, const int64_t* item_begin,
                                            const int64_t* et_table, int n_et, uint64_t seed,
                                            int flags, void* src_out, void* col_out,
                                            void* edge_out, void* fpos_out, void* stream) {
  HeteroHop hop;
  const int rc = fill_hetero_hop(item_begin, et_table, n_et, &hop);
  if (rc != PYGAMD_OK) return rc;
  if (!lo || !hi) return PYGAMD_ERR_INVALID_ARG;
  if (hop.item_begin[n_et] == 0) return PYGAMD_OK;
  if (!row || !perm || !frontier || !offsets || !src_out || !col_out || !edge_out)
    return PYGAMD_ERR_INVALID_ARG;
  return launch_hetero_sample(nullptr, row, perm, idx_dtype, frontier, lo, hi, offsets, hop, seed,
                              flags, src_out, col_out, edge_out, fpos_out, stream);
}

int pygamd_hetero_split(int phase, const void* new_nodes, int idx_dtype, int64_t m,
                        const int64_t* n_new, const int64_t* node_base, const int64_t* count_prev,
                        int n_t, int64_t* flag_or_scan, const void* offsets,
                        const int64_t* item_begin, int n_et, const int64_t* aux_in,
                        void* local_map, void* typed_out, void* sorted_global,
                        void* sorted_local, int64_t* aux_out, int64_t* stats, void* stream) {
  if (phase < 0 || phase > 1 || m < 0) return PYGAMD_ERR_INVALID_ARG;
  if (n_t <= 0 || n_t > kMaxNodeTypes || n_et < 0 || n_et > kMaxEdgeTypes || !node_base)
    return PYGAMD_ERR_INVALID_ARG;
  if (phase == 1 && (!count_prev || (n_et > 0 && !item_begin))) return PYGAMD_ERR_INVALID_ARG;
  if (m == 0) return PYGAMD_OK;
  if (!new_nodes || !n_new || !flag_or_scan) return PYGAMD_ERR_INVALID_ARG;
  if (phase == 1 && (!sorted_global || !sorted_local || !stats || (aux_in && !aux_out) ||
                     (n_et > 0 && !offsets)))
    return PYGAMD_ERR_INVALID_ARG;
  HeteroTypes types;
  types.n_t = n_t;
  types.n_et = n_et;
  for (int t = 0; t <= n_t; ++t) types.node_base[t] = node_base[t];
  for (int t = 0; t < n_t; ++t) types.count_prev[t] = phase == 1 ? count_prev[t] : 0;
  for (int e = 0; e <= n_et; ++e) types.item_begin[e] = phase == 1 && item_begin ? item_begin[e] : 0;
  hipStream_t st = as_stream(stream);
  return PYGAMD_DISPATCH_IDX(idx_dtype, [&]() -> int {
    const IdxT* nn = static_cast<const IdxT*>(new_nodes);
    if (phase == 0) {
      hipLaunchKernelGGL((hetero_split_flag_kernel<IdxT>),
                         dim3(static_cast<unsigned>(ceil_div(m, kBlock))), dim3(kBlock), 0, st,
                         nn, m, n_new, types, flag_or_scan);
    } else {
      const int64_t n = m > n_et + 1 ? m : n_et + 1;  // (n_t <= m: one flag row per type)
      hipLaunchKernelGGL((hetero_split_apply_kernel<IdxT>),
                         dim3(static_cast<unsigned>(ceil_div(n > n_t ? n : n_t, kBlock))),
                         dim3(kBlock), 0, st, nn, m, n_new, flag_or_scan, types,
                         static_cast<const IdxT*>(offsets), aux_in, static_cast<IdxT*>(local_map),
                         static_cast<IdxT*>(typed_out), static_cast<IdxT*>(sorted_global),
                         static_cast<IdxT*>(sorted_local), aux_out, stats);
    }
    PYGAMD_LAUNCH_CHECK();
    return PYGAMD_OK;
  });
}

}  // extern "C"

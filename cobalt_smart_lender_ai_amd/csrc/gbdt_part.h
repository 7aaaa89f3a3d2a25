// ------------------------------------------------------------------------------------------
// Row partition of the split nodes of a level (K18), one launch: the node-ordered k_partition, the
// position-ordered k_part_pos and k_eval_part, which evaluates a node's split in the partition blocks.
//
// All three partition a block's rows the same way (the pieces below, each defined once). A block of 16
// wavefronts takes <= 8192 rows of one node; each wavefront owns a contiguous share and keeps its <= 8 rows
// per lane in registers: pass 1 takes the split feature's bins and counts, the block claims its left range
// (from the node start, ascending) and right range (from the node end, descending) with one atomic per
// block, pass 2 scatters with ballot ranks -- rows are read once. Left rows keep their relative order
// inside a block; only whole blocks interleave, so a node's row list stays sorted in runs of a block's rows
// (the root level reads rows in identity order).
// The claim is a same-address device-scope atomic, whose latency / serialisation across the 8 XCDs dominates
// a level when the blocks are many and small (measured: removing the claims took a 10M-row level from 58 to
// 24 us); hence 1024-thread blocks (16 waves x 8 steps per 8192 rows, 4096 rows while the blocks fit one
// per CU; see chunk_part).
// kSteps: 64-row steps per wave, sized by the host to the item (chunk <= kPartWaves * kSteps * 64): steps
// past the item would still issue their (unconditional) bin loads and ballots.
// ------------------------------------------------------------------------------------------
// Part of the trainer's one translation unit: csrc/gbdt.hip includes this file after the code it builds on
// (it is not self-contained). The host half (launch_eval_part, launch_partition) is at the end.
#pragma once

constexpr int kPartWaves = 16;  // wavefronts of a partition block

// Zero the next level's reduce destination (hist_b of the other parity, free at this point, or the next IPC
// send slot): zero_next int64 cells as int4s, the calling thread every stride-th one from start.
__device__ __forceinline__ void zero_next_reduce(const GbdtDev& d, int parity, int64_t zero_next, int64_t start,
                                                 int64_t stride) {
  int4* zp = reinterpret_cast<int4*>(d.zero_red ? d.zero_red : d.hist_b[parity ^ 1]);
  const int64_t nz = zero_next / 2;
  for (int64_t e = start; e < nz; e += stride) zp[e] = make_int4(0, 0, 0, 0);
}

// Which of a lane's kSteps rows are rows, in a form that folds at compile time: ok(k) is 1 or 0.
// Rows of an item: padding carries the row id -1.
template <int kSteps>
struct ItemRows {
  const int (&r)[kSteps];
  __device__ __forceinline__ uint32_t ok(int k) const { return ~(uint32_t)r[k] >> 31; }
};
// Positions of a wave: the first nv are rows.
struct WavePositions {
  int lane, nv;
  __device__ __forceinline__ uint32_t ok(int k) const { return (uint32_t)(k * kWave + lane < nv); }
};

// The row ids of the wave's share [wb, we) of an item that ends at `end`: unconditional loads at a clamped
// index (end - 1 is a row of the item), masked after; -1 for padding. kMayBeEmpty: an item of a data-parallel
// plan may hold no rows (end - 1 = -1).
template <bool kMayBeEmpty, int kSteps>
__device__ __forceinline__ void load_item_rows(int (&r)[kSteps], const int32_t* cur, bool identity, int wb, int we,
                                               int end, int lane) {
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const int i = wb + k * kWave + lane;
    const int ic = kMayBeEmpty ? max(min(i, end - 1), 0) : min(i, end - 1);
    const int rv = identity ? ic : cur[ic];
    r[k] = i < we ? rv : -1;
  }
}

// Pass 1 in integer arithmetic (boolean forms compiled to per-step branches and spilled masks): the
// direction bit of each row (bin <= j, or the default direction dlv for the missing code) goes to bit k of
// lbits (0 where rows.ok(k) is 0); returns the wave's left count. The caller loads bv[] unconditionally
// (padding rows read row 0), so all kSteps loads are in flight at once -- a load guarded per step made hipcc
// wait for each in turn. The valid rows of a step are a prefix of the lanes, so the wave's valid count needs
// no ballots (the caller has it from its bounds).
template <int kSteps, class Rows>
__device__ __forceinline__ int part_pass1(const uint8_t (&bv)[kSteps], int jm1, uint32_t dlv, const Rows& rows,
                                          uint32_t& lbits) {
  static_assert(kSteps <= 32, "step bit masks are 32-bit");
  int nl = 0;
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const uint32_t b = bv[k];
    const uint32_t lt = (uint32_t)((int)b - jm1) >> 31;  // bin <= j (jm1 = j + 1)
    const uint32_t ms = (b + 1u) >> 8;                    // bin == 255 (missing)
    const uint32_t left = (lt | (ms & dlv)) & rows.ok(k);
    lbits |= left << k;
    nl += __popcll(__ballot(left != 0u));
  }
  return nl;
}

// The claim: the waves' left / right counts (nl of nv rows) to LDS, then ONE atomic per block for both of
// the node's cursors (left = low word, right = high word), then this wave's offsets bl / br into the
// claimed ranges (the block's base + the waves before it). The two probes are the caller's stamp points
// after the counts and after the claim. kAblate: d.ablate == 12 skips the atomic (timing only).
template <bool kAblate>
__device__ __forceinline__ void part_claim(const GbdtDev& d, int node, int nl, int nv, int wv, int lane,
                                           int32_t (&s_cnt)[2][kPartWaves], int32_t (&s_base)[2], BlockStamp& stamp_,
                                           int probe_counted, int probe_claimed, int& bl, int& br) {
  if (lane == 0) { s_cnt[0][wv] = nl; s_cnt[1][wv] = nv - nl; }
  __syncthreads();
  stamp_.probe(probe_counted);
  if (threadIdx.x == 0) {
    int tl = 0, tr = 0;
    for (int k = 0; k < kPartWaves; ++k) { tl += s_cnt[0][k]; tr += s_cnt[1][k]; }
    const unsigned long long c =
        kAblate && d.ablate == 12 ? 0ull
                                  : atomicAdd(reinterpret_cast<unsigned long long*>(d.cursors + 2 * node),
                                              ((unsigned long long)(uint32_t)tr << 32) | (uint32_t)tl);
    s_base[0] = (int32_t)(uint32_t)c;
    s_base[1] = (int32_t)(c >> 32);
  }
  __syncthreads();
  stamp_.probe(probe_claimed);
  bl = s_base[0], br = s_base[1];
  for (int k = 0; k < wv; ++k) { bl += s_cnt[0][k]; br += s_cnt[1][k]; }
}

// Pass 2: one destination per lane (left rows ascending from pl_, the node start + bl; right rows descending
// from pr_, the node's last slot - br), one store per step under the valid-lane mask. lbits is read packed
// (not as 32 live per-step values).
template <int kSteps, class Rows>
__device__ __forceinline__ void part_pass2(const GbdtDev& d, int32_t* nxt, const int (&r)[kSteps], uint32_t lbits,
                                           const Rows& rows, uint32_t pl_, uint32_t pr_, int lane) {
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const bool valid = rows.ok(k) != 0u;
    const uint32_t left = (lbits >> k) & 1u;
    const uint64_t lm = __ballot(left != 0u), vm = __ballot(valid);
    const uint32_t rk_l = mask_rank(lm);
    // valid lanes are a prefix: a right row's rank among the right rows is lane - rk_l
    const uint32_t dst = rk_l + (left ? pl_ : pr_ - (uint32_t)lane);
    if (valid) store_wt(nxt + dst, r[k], (d.wt & 2) != 0);
    const uint32_t cl = (uint32_t)__popcll(lm);
    pl_ += cl;
    pr_ -= (uint32_t)__popcll(vm) - cl;
  }
}

// Node-ordered items: a block plans its item (<= chunk rows of one split node) from the level's node table.
template <int kSteps>
__global__ __launch_bounds__(kPartWaves * 64) void k_partition(GbdtDev d, int parity, int64_t zero_next, int level,
                                                               int chunk) {
  BlockStamp stamp_(d);
  __shared__ int32_t s_cnt[2][kPartWaves];
  __shared__ int32_t s_base[2];
  __shared__ int s_plan[5];
  zero_next_reduce(d, parity, zero_next, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  const int item = blockIdx.x;
  const int first = (1 << level) - 1;
  const PlanOut pl = block_plan(1 << level, chunk, item, [&](int e) {
    const Node& n = d.nodes[first + e];
    const int st = n.status, cnt = n.count, start = n.start;  // loaded together (no per-load branch)
    return (st == kSplit && cnt > 0) ? PlanEntry{first + e, 0, start, cnt} : PlanEntry{-1, 0, 0, 0};
  }, s_plan);
  stamp_.probe(1);
  if (pl.node < 0) return;
  WorkItem w;
  w.node = pl.node;
  w.slot = 0;
  w.begin = pl.begin;
  w.end = pl.end;
  const Node nd = d.nodes[w.node];
  const bool identity = parity == 0 && w.node == 0;
  const int32_t* cur = d.ridx[parity];
  int32_t* nxt = d.ridx[parity ^ 1];
  const uint8_t* col = d.binsT + (int64_t)nd.feat * d.ldt;
  const int j = nd.bin;
  const bool dl = nd.default_left != 0;
  // wave index as a uniform (SGPR) value: the per-step row counts and prefix masks stay scalar
  const int wv = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int len = w.end - w.begin;
  const int per = ((len + kPartWaves - 1) / kPartWaves + kWave - 1) / kWave * kWave;
  const int wb = min(w.end, w.begin + wv * per), we = min(w.end, wb + per);
  int r[kSteps];
  load_item_rows<false>(r, cur, identity, wb, we, w.end, lane);
  uint8_t bv[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; ++k) bv[k] = col[max(r[k], 0)];
  const ItemRows<kSteps> rows{r};
  uint32_t lbits = 0;
  const int nl = part_pass1(bv, j + 1, dl ? 1u : 0u, rows, lbits);
  asm volatile("" : "+v"(lbits));  // pass 2 reads the packed bits
  int bl, br;
  part_claim<true>(d, w.node, nl, max(0, we - wb), wv, lane, s_cnt, s_base, stamp_, 2, 3, bl, br);
  part_pass2(d, nxt, r, lbits, rows, (uint32_t)(nd.start + bl), (uint32_t)(nd.start + nd.count - 1 - br), lane);
}

// Row partition by POSITION (levels with <= 64 nodes): block b takes the row-id positions [b C, (b + 1) C)
// of the level's ridx buffer (C = 16 waves x kSteps x 64), whatever nodes they belong to. A level's nodes
// own disjoint, position-ordered ranges of that buffer (every child range lies inside its parent's), so the
// block's row-id loads depend on nothing but the block index: they are issued at kernel entry, in the same
// round trip as the level's node records -- where the node-ordered k_partition first plans its item from
// the node table and only then loads its row ids (~1.1-1.4 us per block at 10M rows, one of ~4 dependent
// round trips). A wave's 512 positions cover a few ranges: a uniform walk over the split ranges that start
// before each 64-row step gives every lane its node; positions of leaves (and gaps) route nowhere. Counts
// are kept per (wave, range) in LDS, one cursor claim per range per block (all in one round trip), and the
// scatter advances per-(wave, range) pointers as the shared pass 2 does per-wave ones (left rows ascending
// from the node start, right rows descending from its end).
constexpr int kPartPosNodes = 64;

template <int kSteps>
__global__ __launch_bounds__(1024) __attribute__((amdgpu_waves_per_eu(8))) void k_part_pos(GbdtDev d, int parity, int64_t zero_next, int level) {
  constexpr int kPW = kPartWaves;
  constexpr int kN = kPartPosNodes;
  BlockStamp stamp_(d);
  __shared__ int s_rs[kN], s_re[kN];  // split ranges (position order): start, end
  __shared__ uint32_t s_rm[kN];        // feature | (j + 1) << 16 | dl << 25
  __shared__ int s_rn[kN];             // node index
  __shared__ int s_nr;
  __shared__ int32_t s_cnt[kPW][kN][2];  // per (wave, range): left / right rows, then the wave's scatter bases
  __shared__ int s_one, s_one_node, s_one_start, s_one_end;  // the block's one range (s_one < 0: several)
  __shared__ uint32_t s_one_meta;
  __shared__ int32_t s_wc[2][kPW];
  __shared__ int32_t s_wbase[2];
  zero_next_reduce(d, parity, zero_next, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  const int n = (int)d.n;
  const int wv = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int wb = blockIdx.x * (kPW * kSteps * kWave) + wv * (kSteps * kWave);
  const bool identity = parity == 0 && level == 0;  // the root's rows in identity order (never written)
  const int32_t* cur = d.ridx[parity];
  int32_t* nxt = d.ridx[parity ^ 1];
  // row ids first: unconditional loads at clamped positions (no dependence on the node table)
  int r[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const int p = min(wb + k * kWave + lane, n - 1);
    r[k] = identity ? p : cur[p];
  }
  // the level's split nodes with rows -> LDS, in position order (wave 0, one lane per node)
  const int first = (1 << level) - 1, nlev = 1 << level;
  if (wv == 0) {
    const int e = lane;
    const Node& nd = d.nodes[first + min(e, nlev - 1)];
    const int st = nd.status, start = nd.start, cnt = nd.count, f = nd.feat, j = nd.bin, dl = nd.default_left;
    const bool on = e < nlev && st == kSplit && cnt > 0;
    const uint64_t m = __ballot(on);
    if (on) {
      const int k = mask_rank(m);
      s_rs[k] = start;
      s_re[k] = start + cnt;
      s_rm[k] = (uint32_t)f | ((uint32_t)(j + 1) & 0x1FFu) << 16 | (uint32_t)(dl & 1) << 25;
      s_rn[k] = first + e;
    }
    if (e == 0) s_nr = __popcll(m);
    // the block's positions inside ONE split range (nearly every block: a node's range spans ~10^5 rows)?
    const int b0 = blockIdx.x * (kPW * kSteps * kWave), b1 = min(n, b0 + kPW * kSteps * kWave);
    const uint64_t hit = __ballot(on && start <= b0 && start + cnt >= b1);
    if (e == 0) s_one = hit ? __ffsll((unsigned long long)hit) - 1 : -1;
    if (hit && e == __ffsll((unsigned long long)hit) - 1) {
      s_one_node = first + e;
      s_one_start = start;
      s_one_end = start + cnt;
      s_one_meta = (uint32_t)f | ((uint32_t)(j + 1) & 0x1FFu) << 16 | (uint32_t)(dl & 1) << 25;
    }
  }
  for (int i = threadIdx.x; i < kPW * kN * 2; i += blockDim.x) (&s_cnt[0][0][0])[i] = 0;
  __syncthreads();
  stamp_.probe(1);
  const int nr = s_nr;
  if (nr == 0) return;
  if (s_one >= 0) {
    // One range: the shared per-wave passes (counts by ballot, one claim, running per-wave pointers)
    const int node = s_one_node, nstart = s_one_start, nend = s_one_end;
    const uint32_t m = s_one_meta;
    const uint8_t* col = d.binsT + (int64_t)(m & 0xFFFFu) * d.ldt;
    uint8_t bv1[kSteps];
#pragma unroll
    for (int k = 0; k < kSteps; ++k) bv1[k] = col[r[k]];
    const int nv = max(0, min(n, wb + kSteps * kWave) - wb);  // valid positions of this wave (a prefix)
    const WavePositions rows{lane, nv};
    uint32_t lb = 0;
    const int nl = part_pass1(bv1, (int)((m >> 16) & 0x1FFu), (m >> 25) & 1u, rows, lb);
    asm volatile("" : "+v"(lb));
    int bl, br;
    part_claim<true>(d, node, nl, nv, wv, lane, s_wc, s_wbase, stamp_, 2, 3, bl, br);
    part_pass2(d, nxt, r, lb, rows, (uint32_t)(nstart + bl), (uint32_t)(nend - 1 - br), lane);
    return;
  }
  // first range that ends past the wave's first position (uniform binary search over the LDS ends)
  int k0 = 0;
  {
    int lo = 0, hi = nr;  // first k with re[k] > wb
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (__builtin_amdgcn_readfirstlane(s_re[mid]) > wb) hi = mid; else lo = mid + 1;
    }
    k0 = lo;
  }
  // pass 1: each lane's range (uniform walk over the ranges that start inside or before the step), the
  // split feature's bin, the direction; per (wave, range) counts
  // each row's range, packed 8 bits per step (0xFF: routes nowhere) -- 2 VGPRs instead of kSteps (the kernel
  // must stay within 64 VGPRs for two 1024-thread blocks per CU)
  uint32_t klp[(kSteps + 3) / 4];
#pragma unroll
  for (int i = 0; i < (kSteps + 3) / 4; ++i) klp[i] = 0xFFFFFFFFu;
  auto kl_of = [&](int k) -> int {
    const uint32_t v = (klp[k >> 2] >> (8 * (k & 3))) & 0xFFu;
    return v == 0xFFu ? -1 : (int)v;
  };
  uint32_t lbits = 0, inbits = 0;
  uint8_t bv[kSteps];
  // Fast path (nearly every wave: a node's range spans ~10^5 positions): the wave's positions lie inside one
  // range -- every lane's node is k0, no per-lane search. Otherwise each lane binary-searches the ranges
  // from k0 on (the last one starting at or before its position) and checks the range's end.
  const bool one = k0 < nr && __builtin_amdgcn_readfirstlane(s_rs[k0]) <= wb &&
                   __builtin_amdgcn_readfirstlane(s_re[k0]) >= wb + kSteps * kWave;
  if (one) {
    const uint32_t m = __builtin_amdgcn_readfirstlane(s_rm[k0]);
    const uint8_t* col = d.binsT + (int64_t)(m & 0xFFFFu) * d.ldt;
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      klp[k >> 2] &= ~((uint32_t)(0xFFu ^ (uint32_t)k0) << (8 * (k & 3)));
      bv[k] = col[max(r[k], 0)];
    }
    inbits = (1u << kSteps) - 1u;
  } else {
#pragma unroll
    for (int k = 0; k < kSteps; ++k) {
      const int p = wb + k * kWave + lane;
      int lo = k0, hi = nr - 1, kk = -1;  // last t in [k0, nr) with rs[t] <= p
      while (lo <= hi) {
        const int mid = (lo + hi) >> 1;
        if (s_rs[mid] <= p) { kk = mid; lo = mid + 1; } else hi = mid - 1;
      }
      const bool in = kk >= 0 && p < n && p < s_re[max(kk, 0)];
      if (in) klp[k >> 2] &= ~((uint32_t)(0xFFu ^ (uint32_t)kk) << (8 * (k & 3)));
      inbits |= (in ? 1u : 0u) << k;
      // the split feature's bin: an unconditional load (lanes outside a range read their nearest one's column)
      const uint32_t m = s_rm[max(kk, 0)];
      bv[k] = d.binsT[(int64_t)(m & 0xFFFFu) * d.ldt + max(r[k], 0)];
    }
  }
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const int klk = kl_of(k);
    const uint32_t m = s_rm[max(klk, 0)];
    const uint32_t b = bv[k];
    const int jm1 = (int)((m >> 16) & 0x1FFu);  // j + 1
    const uint32_t lt = (uint32_t)((int)b - jm1) >> 31;
    const uint32_t ms = (b + 1u) >> 8;
    const uint32_t left = (lt | (ms & ((m >> 25) & 1u))) & ((inbits >> k) & 1u);
    lbits |= left << k;
    // per-range counts of this step (uniform loop over the ranges present in it; usually one)
    uint64_t rem = __ballot((inbits >> k) & 1u);
    const uint64_t lm = __ballot(left != 0u);
    while (rem) {
      const int src = __ffsll((unsigned long long)rem) - 1;
      const int kk = __builtin_amdgcn_readlane(klk, src);
      const uint64_t mk = __ballot(klk == kk) & rem;
      if (lane == 0) {
        s_cnt[wv][kk][0] += __popcll(mk & lm);
        s_cnt[wv][kk][1] += __popcll(mk & ~lm);
      }
      rem &= ~mk;
    }
  }
  __syncthreads();
  stamp_.probe(2);
  // one claim per range for the whole block (thread t: range t), then each wave's bases
  if ((int)threadIdx.x < nr) {
    const int t = threadIdx.x;
    int tl = 0, tr = 0;
    for (int w = 0; w < kPW; ++w) { tl += s_cnt[w][t][0]; tr += s_cnt[w][t][1]; }
    if (tl + tr > 0) {
      const unsigned long long c =
          d.ablate == 12 ? 0ull
                         : atomicAdd(reinterpret_cast<unsigned long long*>(d.cursors + 2 * s_rn[t]),
                                     ((unsigned long long)(uint32_t)tr << 32) | (uint32_t)tl);
      int bl = s_rs[t] + (int)(uint32_t)c;                // next left slot
      int br = s_re[t] - 1 - (int)(uint32_t)(c >> 32);    // next right slot (descending)
      for (int w = 0; w < kPW; ++w) {
        const int cl = s_cnt[w][t][0], cr = s_cnt[w][t][1];
        s_cnt[w][t][0] = bl;
        s_cnt[w][t][1] = br;
        bl += cl;
        br -= cr;
      }
    }
  }
  __syncthreads();
  stamp_.probe(3);
  // pass 2: scatter with ballot ranks inside each (step, range)
#pragma unroll
  for (int k = 0; k < kSteps; ++k) {
    const bool in = (inbits >> k) & 1u;
    const uint32_t left = (lbits >> k) & 1u;
    const int klk = kl_of(k);
    uint64_t rem = __ballot(in);
    const uint64_t lm = __ballot(left != 0u);
    while (rem) {
      const int src = __ffsll((unsigned long long)rem) - 1;
      const int kk = __builtin_amdgcn_readlane(klk, src);
      const uint64_t mk = __ballot(klk == kk) & rem;
      const int pl = __builtin_amdgcn_readfirstlane(s_cnt[wv][kk][0]);
      const int pr = __builtin_amdgcn_readfirstlane(s_cnt[wv][kk][1]);
      const uint64_t ml = mk & lm, mr = mk & ~lm;
      if (klk == kk) {
        const int dst = left ? pl + mask_rank(ml) : pr - mask_rank(mr);
        store_wt(nxt + dst, r[k], (d.wt & 2) != 0);
      }
      if (lane == 0) {
        s_cnt[wv][kk][0] = pl + __popcll(ml);
        s_cnt[wv][kk][1] = pr - __popcll(mr);
      }
      rem &= ~mk;
    }
  }
}

// ------------------------------------------------------------------------------------------
// Split evaluation fused with the row partition (one GPU, a level's items <= CUs, levels 0 .. max_depth - 2).
// At small row counts a level is a chain of short launches whose fixed costs dominate (1M rows:
// k_eval ~6.6 us + a ~1.5 us boundary per level), so every block of the partition pass evaluates its
// OWN node (the same eval_core, redundantly: ~2 us of fp64 work per block on its own CU, with the
// node's ~42 KB of histograms hot in L2) and partitions its rows by the result -- one launch per level
// fewer. The item's row ids are loaded before the evaluation (they do not depend on the split), so
// their latency hides behind it. The block holding the node's first item finalises the node record
// and stores its histogram for the children (eval_finalize / eval_core's store, as k_eval does).
// The plan covers every node of the level with rows (a block that finalised its node changes the
// status from active to split / leaf; the other blocks accept any status but kNone). A leaf's blocks
// stop after the evaluation.
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ bool split_decision(const GbdtDev& d, const Cand& best, int nb, int& f, int& j, bool& dl) {
  const float loss = (float)best.gain;
  const bool ok = best.key != 0x7fffffff && loss > 1e-6f && loss >= (float)d.gamma;
  f = best.key >> 10;
  const int r = best.key & 1023;
  if (r < 512) { j = r; dl = false; } else { j = (nb - 1 - (r - 512)) - 1; dl = true; }
  return ok;
}

// A node's split decision as ONE 8-byte granule {tag, decision} (evaluator-block modes): written by the
// node's evaluator block with a write-through store, polled by the node's partition blocks.
__device__ __forceinline__ uint64_t decision_word(uint32_t tag, bool ok, bool fail, int f, int j, bool dl) {
  const uint32_t v = (ok ? 1u : 0u) | (fail ? 2u : 0u) | (dl ? 4u : 0u) | ((uint32_t)(j + 1) & 0x3FFu) << 3 |
                     (uint32_t)f << 13;
  return ((uint64_t)tag << 32) | v;
}

// Every block evaluates its node (the items fit one block per CU):
//   kMode 0: one GPU. 1: data parallel with the level's global histograms already in hist_b (RCCL / the
//   separate IPC exchange kernel); every active node gets an item (possibly empty), so each rank
//   finalises every node of the level, also those it holds no rows of.
// kMode 2, EVALUATOR blocks (data parallel over the fused IPC exchange): blocks 0 .. 2^level - 1
// evaluate one node position each, exactly as k_eval<false, true, true> does (block 0 publishes the
// epoch, every evaluator sums its node's cells over the ranks; node ownership on the deep levels; the
// replica digest), publish its decision granule and finalise it; the blocks after them are the
// partition items, which plan and load their row ids while the evaluation runs and then poll their
// node's granule (one lane, bounded by the group's deadline). One evaluation per node -- no xGMI
// traffic multiplied by the items -- and no k_eval -> k_partition boundary, at any item count: blocks
// are dispatched in index order on every XCD, so the evaluators hold CUs before any item does, and no
// evaluator waits on an item. (The same form for one GPU beyond one block per CU measured slower than
// k_eval + k_partition -- 10M rows 238.6 vs 231.9 ms: the fused kernel's 110 VGPRs hold the partition
// to one block per CU; profiles/round5/eval_blocks_10M.txt.)
template <int kSteps, int kMode>
__global__ __launch_bounds__(1024) void k_eval_part(GbdtDev d, int parity, int64_t zero_next, int level, int chunk,
                                                    int tree, EvalSlots es, uint32_t tag) {
  constexpr bool kDP = kMode != 0;
  constexpr bool kEvalBlocks = kMode == 2;
  constexpr bool kIpc = kMode == 2;
  BlockStamp stamp_(d);
  __shared__ int32_t s_cnt[2][kPartWaves];
  __shared__ int32_t s_base[2];
  __shared__ EvalOut s_out;
  if (!kIpc)  // (kMode 2: the evaluators do, see below)
    zero_next_reduce(d, parity, zero_next, (int64_t)blockIdx.x * blockDim.x + threadIdx.x, (int64_t)gridDim.x * blockDim.x);
  const int nlev = 1 << level;
  const int first = nlev - 1;
  if (kIpc && (int)blockIdx.x < nlev) {  // the evaluator of node first + blockIdx.x
    const int pos = blockIdx.x, n = first + pos;
    const IpcFusedView* iv = d.ipcv + (d.ipc_epoch & 1u);
    const bool owned = d.own_level >= 0 && level >= d.own_level;
    const bool mine = !owned || node_owner(d, level, n, iv->n) == iv->me;
    const bool good = eval_core<false, true, true>(d, level, parity, tree, d.F, es, pos, stamp_, &s_out);
    if (threadIdx.x == 0) {
      if (good) {  // the decision first (the items wait on it; they need nothing else of the finalisation)
        int f = 0, j = -1;
        bool dl = false;
        const bool ok = split_decision(d, s_out.best, s_out.nb, f, j, dl);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(d.dec) + n,
                           (unsigned long long)decision_word(tag, ok, false, f, j, dl), __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
        eval_finalize<true>(d, level, n, s_out.G, s_out.H, s_out.best, s_out.cut, s_out.nb);
        if (owned) own_publish(d, iv, n);
      } else {
        const Node nd = d.nodes[n];  // a non-owner's copy of the owner's record (own_copy), or inactive
        if (owned && mine && nd.status != kActive) own_publish(d, iv, n);  // (as k_eval: a diverged peer learns)
        const bool failed =
            __hip_atomic_load(iv->myflag + kIpcStickyWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) != 0u;
        // Always published: a node that is inactive here has no items, but one this rank planned items
        // for can come back inactive from its owner's record (a diverged replica) -- its items then
        // route no rows (and the replica digest reports the divergence at the next tree) instead of
        // waiting for a decision that never comes.
        const uint64_t w = decision_word(tag, nd.status == kSplit, failed || nd.status == kActive, nd.feat, nd.bin,
                                         nd.default_left != 0);
        __hip_atomic_store(reinterpret_cast<unsigned long long*>(d.dec) + n, (unsigned long long)w, __ATOMIC_RELAXED,
                           __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    // The next send slot (this epoch - 1's) is zeroed once every peer has published this epoch: a peer
    // then has finished reading its previous contents. The evaluators that exchanged waited for that in
    // eval_core; a non-owner (it waited only for its node's owner) polls the flags once more, after its
    // decision is out. A failed exchange zeroes nothing (the fit is aborted).
    const bool synced =
        mine ? __hip_atomic_load(iv->myflag + kIpcStickyWord, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0u
             : ipc_wait<false>(iv->ftab, iv->n, iv->me, iv->myflag, d.ipc_epoch, iv->err_host, iv->timeout);
    if (!synced) return;
    zero_next_reduce(d, parity, zero_next, (int64_t)pos * blockDim.x + threadIdx.x, (int64_t)nlev * blockDim.x);
    return;
  }
  const int item = kEvalBlocks ? (int)blockIdx.x - nlev : (int)blockIdx.x;
  // this block's item: the root's rows are fixed slices; deeper levels' items are planned by every
  // block (block_plan over the level's node table)
  PlanOut pl;
  __shared__ int s_plan[5];
  if (level == 0) {
    const int n = (int)d.n, b = item * chunk;
    const int items = max((n + chunk - 1) / chunk, kDP ? 1 : 0);
    pl = PlanOut{item < items ? 0 : -1, 0, min(b, n), min(n, b + chunk), items};
  } else {
    pl = block_plan<kDP>(1 << level, chunk, item, [&](int e) {
      const Node& n = d.nodes[first + e];
      const int st = n.status, cnt = n.count, start = n.start;  // loaded together (no per-load branch)
      return (st != kNone && (kDP || cnt > 0)) ? PlanEntry{first + e, 0, start, cnt} : PlanEntry{-1, 0, 0, 0};
    }, s_plan);
  }
  if (pl.node < 0) return;
  const int node = pl.node;
  // the item's row ids and the node's range: independent of the split, in flight during the evaluation
  const bool identity = parity == 0 && node == 0;
  const int32_t* cur = d.ridx[parity];
  int32_t* nxt = d.ridx[parity ^ 1];
  const int wv = __builtin_amdgcn_readfirstlane(wave_id()), lane = lane_id();
  const int len = pl.end - pl.begin;
  const int per = ((len + kPartWaves - 1) / kPartWaves + kWave - 1) / kWave * kWave;
  const int wb = min(pl.end, pl.begin + wv * per), we = min(pl.end, wb + per);
  int r[kSteps];
  const int nstart = d.nodes[node].start, ncount = d.nodes[node].count;
  const bool lead = pl.begin == nstart;  // the node's first item
  int f, j;
  bool dlb, ok;
  load_item_rows<true>(r, cur, identity, wb, we, pl.end, lane);
  if constexpr (kEvalBlocks) {  // the node's evaluator decides; the row ids are in flight meanwhile
    if (len == 0) return;
    __shared__ uint32_t s_dec;
    if (threadIdx.x == 0) {
      // (bounded: the exchange's deadline; without an exchange 20 s, which no evaluator approaches)
      const IpcFusedView* iv = kIpc ? d.ipcv + (d.ipc_epoch & 1u) : nullptr;
      const uint64_t limit = kIpc ? iv->timeout : 2000000000ull;
      const uint64_t t0 = __builtin_amdgcn_s_memrealtime();
      uint32_t v = 2u;  // failed unless the evaluator's granule arrives
      for (;;) {
        const uint64_t w = __hip_atomic_load(reinterpret_cast<const unsigned long long*>(d.dec) + node,
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if ((uint32_t)(w >> 32) == tag) { v = (uint32_t)w; break; }
        if (__builtin_amdgcn_s_memrealtime() - t0 > limit) {
          if (kIpc) ipc_fail(iv->myflag, iv->err_host);
          break;
        }
        __builtin_amdgcn_s_sleep(1);
      }
      s_dec = v;
    }
    __syncthreads();
    const uint32_t v = s_dec;
    if (v & 2u) return;  // the exchange failed (the host watchdog reports it)
    ok = (v & 1u) != 0;
    dlb = (v & 4u) != 0;
    j = (int)((v >> 3) & 0x3FFu) - 1;
    f = (int)(v >> 13);
  } else {
    // every block evaluates its node itself (the histograms are L2-hot; the row ids are in flight)
    eval_core<false, false, kDP, true>(d, level, parity, tree, d.F, es, node - first, stamp_, &s_out, lead);
    __syncthreads();
    const Cand best = s_out.best;
    ok = split_decision(d, best, s_out.nb, f, j, dlb);
    if (lead && threadIdx.x == 0) eval_finalize<kDP>(d, level, node, s_out.G, s_out.H, best, s_out.cut, s_out.nb);
  }
  stamp_.probe(4);
  if (!ok || len == 0) return;  // a leaf (its rows are not routed) or an empty item (block-uniform)
  const uint8_t* col = d.binsT + (int64_t)f * d.ldt;
  uint8_t bv[kSteps];
#pragma unroll
  for (int k = 0; k < kSteps; ++k) bv[k] = col[max(r[k], 0)];
  const ItemRows<kSteps> rows{r};
  uint32_t lbits = 0;
  const int nl = part_pass1(bv, j + 1, dlb ? 1u : 0u, rows, lbits);
  int bl, br;
  // (probe 5: the split bins are in, pass 1 done; probe 6: the item's ranges are claimed)
  part_claim<false>(d, node, nl, max(0, we - wb), wv, lane, s_cnt, s_base, stamp_, 5, 6, bl, br);
  part_pass2(d, nxt, r, lbits, rows, (uint32_t)(nstart + bl), (uint32_t)(nstart + ncount - 1 - br), lane);
}

// ------------------------------------------------------------------------------------------
// Host half: which instantiation a level's partition launch takes. steps = ceil(item rows / 1024), <= 8.
// ------------------------------------------------------------------------------------------
static void launch_eval_part(int steps, int mode, dim3 grid, size_t lds, hipStream_t stream, const GbdtDev& d,
                             int parity, int64_t zero_next, int level, int chunk, int tree, const EvalSlots& es,
                             uint32_t tag) {
#define EP_LAUNCH(S, M) \
  hipLaunchKernelGGL((k_eval_part<S, M>), grid, dim3(1024), lds, stream, d, parity, zero_next, level, chunk, tree, es, tag)
  if (steps <= 4) {
    switch (mode) {
      case 0: EP_LAUNCH(4, 0); break;
      case 1: EP_LAUNCH(4, 1); break;
      default: EP_LAUNCH(4, 2); break;
    }
  } else if (steps <= 6 && mode <= 1) {  // (1.25M rows: 6144-row items; the 8-step form spills 2 VGPRs)
    if (mode == 0) EP_LAUNCH(6, 0); else EP_LAUNCH(6, 1);
  } else {
    switch (mode) {
      case 0: EP_LAUNCH(8, 0); break;
      case 1: EP_LAUNCH(8, 1); break;
      default: EP_LAUNCH(8, 2); break;
    }
  }
#undef EP_LAUNCH
}

// The separate partition pass: position-ordered blocks (by_pos; the grid from the instantiation's rows per block:
// COBALT_PART_CHUNK may give 1-3 or 5-7 steps) or `items` node-ordered items of `chunk` rows.
static void launch_partition(bool by_pos, int steps, int items, hipStream_t stream, const GbdtDev& d, int parity,
                             int64_t zero_next, int level, int chunk) {
  const dim3 block(kPartWaves * kWave);
  const int ps = steps <= 4 ? 4 : 8;
  if (by_pos) {
    const dim3 pg(std::max(1, (int)ceil_div(d.n, (int64_t)kPartWaves * kWave * ps)));
    if (ps == 4)
      hipLaunchKernelGGL(k_part_pos<4>, pg, block, 0, stream, d, parity, zero_next, level);
    else
      hipLaunchKernelGGL(k_part_pos<8>, pg, block, 0, stream, d, parity, zero_next, level);
  } else if (ps == 4) {
    hipLaunchKernelGGL(k_partition<4>, dim3(items), block, 0, stream, d, parity, zero_next, level, chunk);
  } else {
    hipLaunchKernelGGL(k_partition<8>, dim3(items), block, 0, stream, d, parity, zero_next, level, chunk);
  }
}

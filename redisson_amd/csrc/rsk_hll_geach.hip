// rsk_hll_geach.hip -- grouped PFADD with per-element replies
// (rsk_hll_add_grouped_each), gfx950.
//
// An RBatch of RHyperLogLog.add over many keys: element i goes to sketch
// groups[i] and out[i] is the reply Redis gives to the i-th PFADD when the n
// commands run one by one, 1 iff the element's rank is above its register as
// the sketch stood after elements 0..i-1.
//
// Registers only grow, so an element whose rank is not above its register's
// value at the start of the call replies 0 whatever ran before it; only the
// survivors, whose rank is above that value, need ordering among themselves.
//
//   hll_geach_filter   hashes every element (MurmurHash64A), gathers its
//       register byte and stores out[i] = 0.  Survivors become records
//       {key = sketch << 14 | index, value = seq << 6 | rank}.  A tile of 2048
//       elements compacts its survivors IN INPUT ORDER (ballot + wave counts
//       through LDS) into its own slot and writes its count; one workgroup
//       scans the counts; a pack pass moves each tile's run to its dense
//       place.  The survivor count goes back to the host (the one sync that
//       sizes the rest); at zero nothing else is launched.
//   hll_geach_sort     stable radix sort of the records on the key's
//       14 + ceil(log2 G) bits (hipcub): input order survives inside a register.
//   hll_geach_scan     three launches over tiles of 1024 sorted records, none
//       of which waits for another workgroup.  (1) per tile: first key, last
//       key, the maximum rank of the last key's trailing run, and every
//       record's register byte as the call found it (so launch 3 never reads a
//       register another workgroup may already have raised).  (2) one
//       workgroup walks the aggregates in order and gives every tile the
//       maximum rank of the records before it that share its first key: a
//       register hit by millions of survivors costs O(n).  (3) an in-tile
//       exclusive segmented max-scan in sorted (= input) order; reply = rank >
//       max(register, carry, prefix), out[seq] = 1 where it is 1; the last
//       record of a register's run stores the new byte (one writer per
//       register, a plain store) and the first record of a sketch's run
//       invalidates its card cache, retires its precomputed PFCOUNT and
//       appends the sketch to the list of changed sketches.  Every register
//       among the survivors grows (its first survivor replies 1), so that list
//       is exactly the set of sketches whose registers changed.
//
// Bytes per element: 16 (key) + 4 (sketch id) + 1 (reply) streamed and one
// random register byte gathered; per survivor 12 written + 12 read (compact,
// pack), the sort's passes over 12-byte pairs, and 12 + 13 read, 1 written by
// the scan's launches, plus the scattered reply and register bytes.
#include <hipcub/hipcub.hpp>

#include "rsk_internal.h"

namespace rsk {

namespace {

constexpr uint32_t GE_T = 256;                  // lanes per workgroup (4 waves)
constexpr uint32_t GE_FR = 8;                   // filter: rounds of 256 elements per tile
constexpr uint32_t GE_FTILE = GE_T * GE_FR;     // filter tile
constexpr uint32_t GE_SI = 4;                   // scan: consecutive records per lane
constexpr uint32_t GE_STILE = GE_T * GE_SI;     // scan tile
constexpr uint64_t GE_NOKEY = ~0ull;            // no record (a key has at most 46 bits)

// ------------------------------------------------------------------ filter
// K16: 16-byte keys, 16-byte aligned (non-temporal key and id loads); else any
// fixed stride or blob + offsets.  n < 2^26 + 1, so seq << 6 fits 32 bits.
template <bool K16>
__global__ __launch_bounds__(GE_T) void hll_geach_filter_kernel(
    const uint8_t* __restrict__ data, const uint64_t* __restrict__ offsets, uint32_t fixed_len,
    const uint32_t* __restrict__ groups, uint32_t n, const uint8_t* __restrict__ regs, uint64_t G,
    uint8_t* __restrict__ out, uint64_t* __restrict__ skey, uint32_t* __restrict__ sval,
    uint32_t* __restrict__ tile_cnt, uint32_t ntiles) {
  __shared__ uint32_t wcnt[2][4];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t base = tile * GE_FTILE;
    uint64_t key[GE_FR];
    uint32_t val[GE_FR];  // 0: not a survivor (a rank is >= 1)
#pragma unroll
    for (uint32_t r = 0; r < GE_FR; ++r) {
      const uint32_t i = base + r * GE_T + t;
      key[r] = 0;
      val[r] = 0;
      if (i < n) {
        uint64_t h;
        uint32_t g;
        if (K16) {
          const uint4 v = ld_nt16(reinterpret_cast<const uint4*>(data) + i);
          g = __builtin_nontemporal_load(&groups[i]);
          h = murmur64a_16(((uint64_t)v.y << 32) | v.x, ((uint64_t)v.w << 32) | v.z);
        } else {
          g = groups[i];
          const uint64_t s = offsets ? offsets[i] : (uint64_t)i * fixed_len;
          const uint64_t len = offsets ? offsets[i + 1] - s : fixed_len;
          h = murmur64a(data + s, len);
        }
        out[i] = 0;
        if (g < G) {  // (validated by the caller; an id outside the pool is never dereferenced)
          const uint64_t at = ((uint64_t)g << HLL_P) | hll_index(h);
          const uint32_t rank = hll_rank(h);
          if (rank > regs[at]) {
            key[r] = at;
            val[r] = (i << 6) | rank;
          }
        }
      }
    }
    uint32_t run = 0;  // survivors of the rounds before this one (the same in every lane)
#pragma unroll
    for (uint32_t r = 0; r < GE_FR; ++r) {
      const bool s = val[r] != 0;
      const unsigned long long m = __ballot(s);
      if (lane == 0) wcnt[r & 1][w] = (uint32_t)__popcll(m);
      __syncthreads();  // (round r + 2 rewrites this buffer only after every lane passed round r + 1's barrier)
      const uint32_t c0 = wcnt[r & 1][0], c1 = wcnt[r & 1][1], c2 = wcnt[r & 1][2], c3 = wcnt[r & 1][3];
      const uint32_t woff = (w > 0 ? c0 : 0) + (w > 1 ? c1 : 0) + (w > 2 ? c2 : 0);
      if (s) {
        const uint32_t pos = base + run + woff + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        skey[pos] = key[r];
        sval[pos] = val[r];
      }
      run += c0 + c1 + c2 + c3;
    }
    if (t == 0) tile_cnt[tile] = run;
    __syncthreads();
  }
}

// Exclusive scan of the tile counts by one workgroup; *total = their sum, and
// the changed-sketch list's cursor is reset.
__global__ __launch_bounds__(GE_T) void hll_geach_tilescan_kernel(const uint32_t* __restrict__ cnt, uint32_t ntiles,
                                                                 uint32_t* __restrict__ off,
                                                                 uint32_t* __restrict__ total,
                                                                 uint32_t* __restrict__ list_n) {
  __shared__ uint32_t part[GE_T];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (ntiles + GE_T - 1) / GE_T;
  const uint32_t b = min(t * per, ntiles), e = min(b + per, ntiles);
  uint32_t s = 0;
  for (uint32_t i = b; i < e; ++i) s += cnt[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    uint32_t acc = 0;
    for (uint32_t j = 0; j < GE_T; ++j) {
      const uint32_t v = part[j];
      part[j] = acc;
      acc += v;
    }
    *total = acc;
    *list_n = 0;
  }
  __syncthreads();
  uint32_t acc = part[t];
  for (uint32_t i = b; i < e; ++i) {
    off[i] = acc;
    acc += cnt[i];
  }
}

// Each tile's run of survivors from its slot to its dense place.
__global__ __launch_bounds__(GE_T) void hll_geach_pack_kernel(const uint64_t* __restrict__ skey,
                                                             const uint32_t* __restrict__ sval,
                                                             const uint32_t* __restrict__ cnt,
                                                             const uint32_t* __restrict__ off, uint32_t ntiles,
                                                             uint64_t* __restrict__ dkey, uint32_t* __restrict__ dval) {
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t c = cnt[tile], o = off[tile], s = tile * GE_FTILE;
    for (uint32_t j = threadIdx.x; j < c; j += GE_T) {
      dkey[o + j] = skey[s + j];
      dval[o + j] = sval[s + j];
    }
  }
}

// -------------------------------------------------------------------- scan
// Launch 1: a tile's aggregates, and base[p] = the register byte of record p
// as the call found it.
__global__ __launch_bounds__(GE_T) void hll_geach_agg_kernel(const uint64_t* __restrict__ key,
                                                            const uint32_t* __restrict__ val, uint32_t S,
                                                            const uint8_t* __restrict__ regs,
                                                            uint8_t* __restrict__ base, uint64_t* __restrict__ a_first,
                                                            uint64_t* __restrict__ a_last,
                                                            uint32_t* __restrict__ a_trail, uint32_t ntiles) {
  __shared__ uint32_t wmax[4];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t b = tile * GE_STILE;
    const uint32_t end = min(b + GE_STILE, S);
    const uint64_t kl = key[end - 1];
    uint32_t m = 0;
#pragma unroll
    for (uint32_t e = 0; e < GE_SI; ++e) {
      const uint32_t p = b + e * GE_T + t;
      if (p < end) {
        const uint64_t k = key[p];
        base[p] = regs[k];
        if (k == kl) m = max(m, val[p] & 63u);
      }
    }
    for (int o = 32; o > 0; o >>= 1) m = max(m, (uint32_t)__shfl_down(m, o, 64));
    if (lane == 0) wmax[w] = m;
    __syncthreads();
    if (t == 0) {
      a_first[tile] = key[b];
      a_last[tile] = kl;
      a_trail[tile] = max(max(wmax[0], wmax[1]), max(wmax[2], wmax[3]));
    }
    __syncthreads();
  }
}

// Launch 2: carry[t] = the maximum rank of the records before tile t that
// share its first key.  With link(t) = last[t - 1] == first[t] and A[t] = the
// maximum rank of the run of last[t] that ends tile t (reaching back across
// tiles): carry[t] = link(t) ? A[t - 1] : 0 and A[t] = (tile t is one key and
// link(t)) ? max(A[t - 1], trail[t]) : trail[t] -- a segmented max-scan, done by
// one workgroup: every lane folds a contiguous slice, lane 0 chains the 256
// slice results, every lane walks its slice again.
__global__ __launch_bounds__(GE_T) void hll_geach_carry_kernel(const uint64_t* __restrict__ a_first,
                                                              const uint64_t* __restrict__ a_last,
                                                              const uint32_t* __restrict__ a_trail, uint32_t ntiles,
                                                              uint32_t* __restrict__ carry) {
  __shared__ uint32_t sf[GE_T], sv[GE_T];
  const uint32_t t = threadIdx.x;
  const uint32_t per = (ntiles + GE_T - 1) / GE_T;
  const uint32_t b = min(t * per, ntiles), e = min(b + per, ntiles);
  uint32_t f = 0, v = 0;  // the slice as one scan element: a head inside it, the running maximum at its end
  for (uint32_t i = b; i < e; ++i) {
    const uint64_t fi = a_first[i];
    const bool link = i > 0 && a_last[i - 1] == fi;
    const uint32_t tr = a_trail[i];
    if (fi == a_last[i] && link) {
      v = max(v, tr);
    } else {
      f = 1;
      v = tr;
    }
  }
  sf[t] = f;
  sv[t] = v;
  __syncthreads();
  if (t == 0) {
    uint32_t acc = 0;  // A at the end of the slices before j
    for (uint32_t j = 0; j < GE_T; ++j) {
      const uint32_t jf = sf[j], jv = sv[j];
      sv[j] = acc;
      acc = jf ? jv : max(acc, jv);
    }
  }
  __syncthreads();
  uint32_t run = sv[t];  // A[b - 1]
  for (uint32_t i = b; i < e; ++i) {
    const uint64_t fi = a_first[i];
    const bool link = i > 0 && a_last[i - 1] == fi;
    const uint32_t tr = a_trail[i];
    carry[i] = link ? run : 0;
    run = (fi == a_last[i] && link) ? max(run, tr) : tr;
  }
}

// Launch 3: replies, new register bytes, changed sketches.
__global__ __launch_bounds__(GE_T) void hll_geach_apply_kernel(
    const uint64_t* __restrict__ key, const uint32_t* __restrict__ val, uint32_t S, const uint8_t* __restrict__ base,
    const uint32_t* __restrict__ carry, uint32_t ntiles, uint8_t* __restrict__ regs, uint8_t* __restrict__ out,
    unsigned long long* __restrict__ card, uint32_t* __restrict__ pepoch, uint32_t* __restrict__ list,
    uint32_t* __restrict__ list_n, uint32_t list_cap) {
  __shared__ uint32_t wf[4], wv[4];
  const uint32_t t = threadIdx.x, lane = t & 63, w = t >> 6;
  for (uint32_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const uint32_t b = tile * GE_STILE;
    const uint32_t p0 = b + t * GE_SI;
    uint64_t k[GE_SI + 2];  // k[e + 1] = record p0 + e; k[0] the record before them, k[GE_SI + 1] the one after
    uint32_t rk[GE_SI], sq[GE_SI], ex[GE_SI];
    bool open[GE_SI];  // no head at or before the record inside this lane
    k[0] = (p0 > 0 && p0 - 1 < S) ? key[p0 - 1] : GE_NOKEY;
    uint32_t f = 0, v = 0;
#pragma unroll
    for (uint32_t e = 0; e < GE_SI; ++e) {
      const uint32_t p = p0 + e;
      const bool valid = p < S;
      k[e + 1] = valid ? key[p] : GE_NOKEY;
      const uint32_t vv = valid ? val[p] : 0;
      rk[e] = vv & 63u;
      sq[e] = vv >> 6;
      if (p > b && k[e + 1] != k[e]) {  // a run starts here (the tile's first record continues the carry)
        f = 1;
        v = 0;
      }
      ex[e] = v;
      open[e] = f == 0;
      v = max(v, rk[e]);
    }
    k[GE_SI + 1] = (p0 + GE_SI < S) ? key[p0 + GE_SI] : GE_NOKEY;
    // inclusive segmented max-scan of the lanes' (f, v) across the wave, then the waves before through LDS
    uint32_t sf = f, sv = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const uint32_t pf = __shfl_up(sf, o, 64), pv = __shfl_up(sv, o, 64);
      if ((int)lane >= o) {
        if (!sf) sv = max(sv, pv);
        sf |= pf;
      }
    }
    uint32_t ef = __shfl_up(sf, 1, 64), ev = __shfl_up(sv, 1, 64);
    if (lane == 0) ef = 0, ev = 0;
    if (lane == 63) wf[w] = sf, wv[w] = sv;
    __syncthreads();
    uint32_t pf = 0, pv = 0;
    for (uint32_t j = 0; j < w; ++j) {
      const uint32_t jf = wf[j], jv = wv[j];
      pv = jf ? jv : max(pv, jv);
      pf |= jf;
    }
    const uint32_t in_v = ef ? ev : max(pv, ev);  // maximum rank of the open run's records before this lane, in the tile
    const uint32_t in_f = pf | ef;                // a run started before this lane in the tile
    const uint32_t cr = carry[tile];
    __syncthreads();
#pragma unroll
    for (uint32_t e = 0; e < GE_SI; ++e) {
      const uint32_t p = p0 + e;
      if (p >= S) continue;
      const uint64_t kk = k[e + 1];
      uint32_t pre = ex[e];
      if (open[e]) {
        pre = max(pre, in_v);
        if (!in_f) pre = max(pre, cr);
      }
      pre = max(pre, (uint32_t)base[p]);
      const bool reply = rk[e] > pre;
      if (reply) out[sq[e]] = 1;
      if (k[e + 2] != kk) regs[kk] = (uint8_t)(reply ? rk[e] : pre);  // the run's last record: its only writer
      const uint64_t g = kk >> HLL_P;
      if (k[e] == GE_NOKEY || (k[e] >> HLL_P) != g) {  // the sketch's first record: one per sketch
        card[g] |= 1ull << 63;
        pepoch[g] = 0;
        const uint32_t slot = atomicAdd(list_n, 1u);
        if (slot < list_cap) list[slot] = (uint32_t)g;
      }
    }
  }
}

uint64_t al256(uint64_t x) { return (x + 255) & ~uint64_t(255); }

uint32_t grid_for(const rsk_ctx* c, uint64_t tiles) {
  return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(tiles, (uint64_t)c->num_cus * 8));
}

}  // namespace

uint64_t hll_add_grouped_each_launch(rsk_ctx* c, const DevKeys& k, const uint32_t* d_groups, uint8_t* d_regs, uint64_t G,
                                     uint64_t* d_card, uint32_t* d_pepoch, uint8_t* d_out,
                                     std::vector<uint32_t>* changed) {
  const uint64_t n = k.n;
  if (n == 0) return 0;
  if (n > (1ull << 26)) throw RskError{RSK_ERR_INVALID_ARG, "hll_add_grouped_each_launch: sub-chunk above 2^26"};
  const uint32_t ftiles = (uint32_t)((n + GE_FTILE - 1) / GE_FTILE);
  const uint64_t cap = (uint64_t)ftiles * GE_FTILE;
  const uint32_t stiles_max = (uint32_t)((n + GE_STILE - 1) / GE_STILE);
  const uint64_t list_cap = std::min<uint64_t>(n, G);
  int end_bit = HLL_P;
  while (end_bit < 64 && (1ull << (end_bit - HLL_P)) < G) ++end_bit;
  size_t sort_bytes = 0;
  RSK_HIP(hipcub::DeviceRadixSort::SortPairs(nullptr, sort_bytes, (const uint64_t*)nullptr, (uint64_t*)nullptr,
                                             (const uint32_t*)nullptr, (uint32_t*)nullptr, (int)n, 0, end_bit,
                                             c->stream));
  // The slots are sized for every element surviving; the sorted records reuse them once packed.
  uint64_t at = 0;
  auto take = [&](uint64_t bytes) {
    const uint64_t o = at;
    at += al256(bytes);
    return o;
  };
  const uint64_t o_hdr = take(256), o_skey = take(8 * cap), o_sval = take(4 * cap), o_dkey = take(8 * n),
                 o_dval = take(4 * n), o_base = take(n), o_tcnt = take(4ull * ftiles), o_toff = take(4ull * ftiles),
                 o_first = take(8ull * stiles_max), o_last = take(8ull * stiles_max),
                 o_trail = take(4ull * stiles_max), o_carry = take(4ull * stiles_max), o_list = take(4 * list_cap),
                 o_tmp = take(sort_bytes);
  uint8_t* w = c->work(at);
  auto* d_total = reinterpret_cast<uint32_t*>(w + o_hdr);
  auto* d_list_n = d_total + 1;
  auto* skey = reinterpret_cast<uint64_t*>(w + o_skey);
  auto* sval = reinterpret_cast<uint32_t*>(w + o_sval);
  auto* dkey = reinterpret_cast<uint64_t*>(w + o_dkey);
  auto* dval = reinterpret_cast<uint32_t*>(w + o_dval);
  uint8_t* base = w + o_base;
  auto* tcnt = reinterpret_cast<uint32_t*>(w + o_tcnt);
  auto* toff = reinterpret_cast<uint32_t*>(w + o_toff);
  auto* a_first = reinterpret_cast<uint64_t*>(w + o_first);
  auto* a_last = reinterpret_cast<uint64_t*>(w + o_last);
  auto* a_trail = reinterpret_cast<uint32_t*>(w + o_trail);
  auto* carry = reinterpret_cast<uint32_t*>(w + o_carry);
  auto* list = reinterpret_cast<uint32_t*>(w + o_list);
  uint32_t* h_res = reinterpret_cast<uint32_t*>(c->h_small + 448);

  {
    ProfScope ps(c, "hll_geach_filter");
    const uint32_t grid = grid_for(c, ftiles);
    if (k.offsets == nullptr && k.fixed_len == 16 && (reinterpret_cast<uintptr_t>(k.data) & 15) == 0) {
      hipLaunchKernelGGL(hll_geach_filter_kernel<true>, dim3(grid), dim3(GE_T), 0, c->stream, k.data, nullptr, 16u,
                         d_groups, (uint32_t)n, d_regs, G, d_out, skey, sval, tcnt, ftiles);
    } else {
      hipLaunchKernelGGL(hll_geach_filter_kernel<false>, dim3(grid), dim3(GE_T), 0, c->stream, k.data, k.offsets,
                         k.fixed_len, d_groups, (uint32_t)n, d_regs, G, d_out, skey, sval, tcnt, ftiles);
    }
    RSK_CHECK_LAUNCH("hll_geach_filter");
    hipLaunchKernelGGL(hll_geach_tilescan_kernel, dim3(1), dim3(GE_T), 0, c->stream, tcnt, ftiles, toff, d_total,
                       d_list_n);
    RSK_CHECK_LAUNCH("hll_geach_tilescan");
    hipLaunchKernelGGL(hll_geach_pack_kernel, dim3(grid), dim3(GE_T), 0, c->stream, skey, sval, tcnt, toff, ftiles,
                       dkey, dval);
    RSK_CHECK_LAUNCH("hll_geach_pack");
  }
  RSK_HIP(hipMemcpyAsync(h_res, d_total, 4, hipMemcpyDeviceToHost, c->stream));
  RSK_HIP(hipStreamSynchronize(c->stream));
  const uint32_t S = h_res[0];
  if (S == 0) return 0;
  if (S > n) throw RskError{RSK_ERR_DEVICE, "hll_add_grouped_each: survivor count out of range"};

  // sorted records land in the (now free) slots
  {
    ProfScope ps(c, "hll_geach_sort");
    RSK_HIP(hipcub::DeviceRadixSort::SortPairs(w + o_tmp, sort_bytes, (const uint64_t*)dkey, skey,
                                               (const uint32_t*)dval, sval, (int)S, 0, end_bit, c->stream));
  }
  {
    ProfScope ps(c, "hll_geach_scan");
    const uint32_t stiles = (S + GE_STILE - 1) / GE_STILE;
    const uint32_t grid = grid_for(c, stiles);
    hipLaunchKernelGGL(hll_geach_agg_kernel, dim3(grid), dim3(GE_T), 0, c->stream, (const uint64_t*)skey,
                       (const uint32_t*)sval, S, (const uint8_t*)d_regs, base, a_first, a_last, a_trail, stiles);
    RSK_CHECK_LAUNCH("hll_geach_agg");
    hipLaunchKernelGGL(hll_geach_carry_kernel, dim3(1), dim3(GE_T), 0, c->stream, (const uint64_t*)a_first,
                       (const uint64_t*)a_last, (const uint32_t*)a_trail, stiles, carry);
    RSK_CHECK_LAUNCH("hll_geach_carry");
    hipLaunchKernelGGL(hll_geach_apply_kernel, dim3(grid), dim3(GE_T), 0, c->stream, (const uint64_t*)skey,
                       (const uint32_t*)sval, S, (const uint8_t*)base, (const uint32_t*)carry, stiles, d_regs, d_out,
                       reinterpret_cast<unsigned long long*>(d_card), d_pepoch, list, d_list_n, (uint32_t)list_cap);
    RSK_CHECK_LAUNCH("hll_geach_apply");
  }
  RSK_HIP(hipMemcpyAsync(h_res, d_list_n, 4, hipMemcpyDeviceToHost, c->stream));
  RSK_HIP(hipStreamSynchronize(c->stream));
  const uint32_t nl = h_res[0];
  if (nl > list_cap) throw RskError{RSK_ERR_DEVICE, "hll_add_grouped_each: changed-sketch count out of range"};
  const size_t old = changed->size();
  changed->resize(old + nl);
  RSK_HIP(hipMemcpy(changed->data() + old, list, 4ull * nl, hipMemcpyDeviceToHost));
  return S;
}

}  // namespace rsk

// rsk_bloom_pool.hip -- pools of equal Bloom filters (rsk_bloom_pool), gfx950.
//
// Many small RBloomFilters driven from one RBatch (one dedup filter per
// tenant / user / shard): F filters of one (size, k) held as F rows of one
// Redis-layout (MSB-first) bit string, row r at bit r * stride, stride = size
// rounded up to a multiple of 32 bits (so bloom_bit_mask holds at any row base
// and a row starts on a u32 word; the padding bits are never set).  Key i of a
// batch goes to row groups[i]: its probes are groups[i] * stride + idx_t with
// idx_t exactly RedissonBloomFilter.hash's (:116-131) for `size`.
//
// Rows occupy disjoint bit ranges, so the pool IS a single filter of
// F * stride bits with another probe generator (RowGroups, rsk_device.h): the
// insert's slice partition (rsk_bloom_st.hip, rsk_bloom_part.hip), add()'s
// first-setter replies (rsk_bloom_reply.hip, the (bit, sequence) sort of
// rsk_bloom.hip) and the early-exit contains (rsk_bloom_kern.h) are the
// single filter's kernels instantiated with that generator -- "first probe of
// a bit" per global bit is "first probe of the bit in its row", which is what
// the per-filter sequential replies ask for.  This file holds what only a pool
// needs: the reduction that validates a batch's row ids before anything is
// written, and BITCOUNT per row.
#include "rsk_internal.h"

namespace rsk {

namespace {

// max over groups[0..n): one atomicMax per wave.
__global__ __launch_bounds__(256) void pool_max_group_kernel(const uint32_t* __restrict__ groups, uint64_t n,
                                                             uint32_t* __restrict__ out) {
  uint32_t m = 0;
  for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (uint64_t)gridDim.x * blockDim.x)
    m = max(m, groups[i]);
  for (int off = 32; off > 0; off >>= 1) m = max(m, (uint32_t)__shfl_down(m, off, 64));
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

// BITCOUNT of one row per wave: the row's first row_bytes bytes (whole u32
// words, then the low bytes of the last one: the string is little-endian in
// its words), so the stride's padding is outside the count.
__global__ __launch_bounds__(256) void pool_bitcount_kernel(const uint32_t* __restrict__ bits, uint64_t stride_words,
                                                            uint64_t row_bytes, const uint64_t* __restrict__ ids,
                                                            uint64_t n, uint64_t* __restrict__ out) {
  const uint32_t lane = threadIdx.x & 63;
  const uint64_t wave = ((uint64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
  const uint64_t nwaves = ((uint64_t)gridDim.x * blockDim.x) >> 6;
  const uint64_t full = row_bytes / 4;
  const uint32_t rem = (uint32_t)(row_bytes & 3);
  for (uint64_t i = wave; i < n; i += nwaves) {
    const uint32_t* row = bits + (ids ? ids[i] : i) * stride_words;
    uint32_t acc = 0;
    for (uint64_t w = lane; w < full; w += 64) acc += __popc(row[w]);
    if (rem && lane == 0) acc += __popc(row[full] & ((1u << (8 * rem)) - 1u));
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
    if (lane == 0) out[i] = acc;
  }
}

}  // namespace

uint32_t bloom_pool_max_group(rsk_ctx* c, const uint32_t* d_groups, uint64_t n) {
  if (n == 0) return 0;
  uint32_t* d = reinterpret_cast<uint32_t*>(c->d_small + 192);
  RSK_HIP(hipMemsetAsync(d, 0, 4, c->stream));
  uint64_t g = (n + 255) / 256;
  const uint64_t cap = (uint64_t)c->num_cus * 8;
  if (g > cap) g = cap;
  {
    ProfScope ps(c, "bloom_pool_check");
    hipLaunchKernelGGL(pool_max_group_kernel, dim3((uint32_t)g), dim3(256), 0, c->stream, d_groups, n, d);
    RSK_CHECK_LAUNCH("bloom_pool_check");
  }
  RSK_HIP(hipMemcpyAsync(c->h_small + 192, d, 4, hipMemcpyDeviceToHost, c->stream));
  RSK_HIP(hipStreamSynchronize(c->stream));
  uint32_t m = 0;
  __builtin_memcpy(&m, c->h_small + 192, 4);
  return m;
}

void bloom_pool_bitcount_launch(rsk_ctx* c, const uint32_t* d_bits, uint64_t stride_words, uint64_t row_bytes,
                                const uint64_t* d_ids, uint64_t n, uint64_t* d_out) {
  if (n == 0) return;
  uint64_t g = (n + 3) / 4;  // 4 waves per workgroup, one row per wave
  const uint64_t cap = (uint64_t)c->num_cus * 8;
  if (g > cap) g = cap;
  ProfScope ps(c, "bloom_pool_bitcount");
  hipLaunchKernelGGL(pool_bitcount_kernel, dim3((uint32_t)g), dim3(256), 0, c->stream, d_bits, stride_words, row_bytes,
                     d_ids, n, d_out);
  RSK_CHECK_LAUNCH("bloom_pool_bitcount");
}

}  // namespace rsk

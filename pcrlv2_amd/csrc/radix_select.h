// Exact order statistics without a sort: byte-wise radix selection of R ranks at once over unsigned keys whose integer order is the values' order.
// sizeof(Key) passes, most significant byte first.  A pass is a grid-wide histogram launch -- per block a 256-bin LDS histogram PER RANK of the keys
// that share the rank's prefix so far (LDS integer atomics), then one 64-bit integer atomic per non-empty (block, rank, bin) -- and a tiny pick launch
// in which thread r walks the bins of rank r, extends its prefix by the byte that holds the rank, and clears its row.  No host read-back in between and
// only integer atomics: the result does not depend on any order.  Equal keys serialise on one bin, which is what counting them takes.
//
// The users (seg_prep.hip: 32-bit keys of float32 values, 4 ranks; surface_dist.hip: the 64-bit patterns of non-negative doubles, 3 ranks) keep what
// differs: which keys a voxel yields, how the state is started (ranks set, prefixes and histogram zero) and where the final prefix goes.
#pragma once
#include "common.h"

template <typename Key, int R>
struct RadixSelect {
  static constexpr int PASSES = (int)sizeof(Key);
  unsigned long long rank[R];         // what is left of each rank inside its current prefix
  Key prefix[R];                      // the leading bytes found so far
  unsigned long long hist[R][256];    // all zero between passes
};

// One block's share of histogram pass `pass` (0: the most significant byte), for blocks of THREADS threads; every thread of the block calls
// begin (it zeroes the LDS histogram `h` [R * 256] and synchronises), add for each of its keys, and flush (it synchronises first).
template <typename Key, int R, int THREADS>
struct RadixPass {
  unsigned* h;
  Key prefix[R];
  int pass, shift;

  __device__ __forceinline__ void begin(const RadixSelect<Key, R>* __restrict__ st, int pass_, unsigned* lds) {
    h = lds;
    for (int i = threadIdx.x; i < R * 256; i += THREADS) h[i] = 0u;
#pragma unroll
    for (int r = 0; r < R; ++r) prefix[r] = st->prefix[r];
    __syncthreads();
    pass = pass_;
    shift = 8 * ((int)sizeof(Key) - 1 - pass_);
  }
  __device__ __forceinline__ void add(Key k) const {
    const unsigned byte = (unsigned)(k >> shift) & 255u;
    const Key head = pass ? k >> (shift + 8) : (Key)0;
#pragma unroll
    for (int r = 0; r < R; ++r)
      if (head == prefix[r]) atomicAdd(&h[r * 256 + byte], 1u);
  }
  __device__ __forceinline__ void flush(RadixSelect<Key, R>* __restrict__ st) const {
    __syncthreads();
    unsigned long long* gh = &st->hist[0][0];
    for (int i = threadIdx.x; i < R * 256; i += THREADS)
      if (h[i]) atomicAdd(&gh[i], (unsigned long long)h[i]);
  }
};

// The pick of rank r, by ONE thread per rank after a pass's histogram is complete -> the prefix so far (after the last pass: the key at that rank).
template <typename Key, int R>
__device__ __forceinline__ Key radix_pick(RadixSelect<Key, R>* __restrict__ st, int r) {
  unsigned long long rank = st->rank[r], cum = 0;
  int b = 0;
  for (; b < 255; ++b) {
    const unsigned long long c = st->hist[r][b];
    if (rank < cum + c) break;
    cum += c;
  }
  for (int i = 0; i < 256; ++i) st->hist[r][i] = 0;
  const Key pre = (Key)(st->prefix[r] << 8) | (Key)b;
  st->rank[r] = rank - cum;
  st->prefix[r] = pre;
  return pre;
}

// Connected components of one class of a 3D bitmask (uint8 [X][Y][Z], bit k = class k) under connectivity 6, 18 or 26, numbered as
// scipy.ndimage.label numbers them, and the clean-up rules on top (keep the largest component, drop components below a volume).  Integer only.
//
// Everything is a union-find forest over linear voxel indices whose links ALWAYS run from a larger index to a smaller one: the root of a component
// is its minimum linear index whatever order the atomics land in, so every output is order-independent.  Nothing here waits on another block.
//
// local     block = one tile at a time (the grid is capped at 2^20 blocks, a block walks the tiles b, b + grid, ...), a tile = CCL_TX x CCL_TY x CCL_TZ (4 x 4 x 64) voxels = 16 whole Z-runs, 256 threads x 4 voxels; wave w, pass i owns the
//           Z-run (lx, ly) = (i, w), lane = lz.  The Z-links cost no atomic: a ballot of the run's class bits gives every lane the first voxel of its
//           stretch of consecutive class voxels, which becomes its first parent.  The other backward neighbours inside the tile (2 / 8 / 12 offsets
//           at 6 / 18 / 26) are united in LDS: find both roots, atomicMin(&lab[larger], smaller), and if the value returned is not the root that
//           was held, go on from that value.  Then every voxel finds its root (read-only), counts itself on it (LDS atomic), and the tile writes
//           L[v] = global index of the tile-local root (-1: background) and S[v] = the voxels of the tile-local component at its root, 0 elsewhere.
// merge     thread = voxel; only voxels with a backward neighbour in ANOTHER tile do anything (faces; edges and corners at 18 / 26).  The same
//           lock-free union on L in global memory; parent reads are relaxed agent-scope atomic loads -- a stale copy is an older, larger, still
//           valid ancestor, and the loop is correct because it always continues from the value its atomicMin returned.
// flatten   block = a chunk of CCL_CHUNK (1024) consecutive voxels; L is read-only here: R[v] = root of v (-1: background); a tile-local root adds
//           its tile's count to its final root, ONE integer atomic per (tile, tile-local component); the chunk's number of roots goes to bsum.
// scan      one block walks bsum in strips of 256 in a fixed order: exclusive offsets per chunk, and n.
// rank      chunk again, 4 consecutive voxels per thread: rank of a root = offset of its chunk + exclusive scan inside it, i.e. roots are numbered by
//           ascending linear index -- scipy's numbering; sizes[rank] = S[root], then S[root] = rank + 1.
// relabel   labels[v] = S[R[v]], 0 for background (labels is the buffer L lived in; L is dead by now).
//
// Loop bounds.  find: a parent is strictly smaller than its child, so a walk from v takes at most v steps (in LDS at most 1023).  union: after an
// iteration the pair (a, b) has become (old, b) with old < a and b < a: max(a, b) strictly falls, at most max(a, b) iterations.  Every other loop has
// a trip count fixed at launch.
// LDS       lab and cnt, 4 KiB each.  Staging and the final write touch lab[i * 256 + t]: 64 consecutive words per wave, conflict-free.  The union
//           and find walks are data-dependent (as is any union-find); equal addresses broadcast, atomics on one root serialise.
#include "common.h"

namespace {

constexpr int CCL_TX = 4, CCL_TY = 4, CCL_TZ = 64, CCL_TILE = CCL_TX * CCL_TY * CCL_TZ;
constexpr int CCL_THREADS = 256, CCL_CHUNK = 1024, CCL_PER = CCL_CHUNK / CCL_THREADS;
// the tile grid's cap: a launch takes fewer than 2^32 threads in all, and a tile may hold as little as one Z-run of real voxels (tiles up to 2^31 / 16)
constexpr int CCL_MAX_BLOCKS = 1 << 20;
static_assert(CCL_TZ == 64 && CCL_TY * 64 == CCL_THREADS && CCL_TX == CCL_PER, "wave w, pass i owns the Z-run (i, w)");

// offset (dx, dy, dz) is a backward neighbour (smaller linear index) within the connectivity: NORM = 1, 2, 3 for 6, 18, 26
template <int NORM>
__host__ __device__ constexpr bool ccl_backward(int dx, int dy, int dz) {
  const int n = (dx < 0 ? -dx : dx) + (dy < 0 ? -dy : dy) + (dz < 0 ? -dz : dz);
  return n >= 1 && n <= NORM && (dx < 0 || (dx == 0 && (dy < 0 || (dy == 0 && dz < 0))));
}

// a relaxed atomic read: other threads of the block lower entries meanwhile; whatever it returns is an ancestor
__device__ __forceinline__ int lds_load(const int* lab, int a) { return __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }

__device__ __forceinline__ int lds_find(const int* lab, int a) {
  int p;
  while ((p = lds_load(lab, a)) != a) a = p;
  return a;
}

__device__ __forceinline__ void lds_union(int* lab, int a, int b) {
  a = lds_find(lab, a);
  b = lds_find(lab, b);
  while (a != b) {
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&lab[a], b);
    if (old == a) break;
    a = old;
  }
}

__device__ __forceinline__ int g_load(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

__device__ __forceinline__ int g_find(const int* L, int a) {
  int p;
  while ((p = g_load(L + a)) != a) a = p;
  return a;
}

__device__ __forceinline__ void g_union(int* L, int a, int b) {
  a = g_find(L, a);
  b = g_find(L, b);
  while (a != b) {
    if (a < b) {
      const int s = a;
      a = b;
      b = s;
    }
    const int old = atomicMin(&L[a], b);
    if (old == a) break;
    a = old;
  }
}

// grid = min(tiles, CCL_MAX_BLOCKS), a block takes the tiles blockIdx.x, blockIdx.x + gridDim.x, ... (z fastest); block = 256
template <int NORM>
__global__ void __launch_bounds__(CCL_THREADS) ccl_local_kernel(const uint8_t* __restrict__ mask, unsigned bit, int* __restrict__ L, int* __restrict__ S, int X,
                                                               int Y, int Z, int nty, int ntz, int64_t tiles) {
  __shared__ int lab[CCL_TILE];
  __shared__ int cnt[CCL_TILE];
  const int t = threadIdx.x, lz = t & 63, ly = t >> 6;
  for (int64_t tile = blockIdx.x; tile < tiles; tile += gridDim.x) {      // uniform over the block: every barrier below is reached by all of it
    const int z0 = (int)(tile % ntz) * CCL_TZ;
    const int64_t col = tile / ntz;
    const int y0 = (int)(col % nty) * CCL_TY, x0 = (int)(col / nty) * CCL_TX;
    const int y = y0 + ly, z = z0 + lz;
#pragma unroll
    for (int i = 0; i < CCL_PER; ++i) {      // lx = i
      const int x = x0 + i, e = i * CCL_THREADS + t;
      const bool on = x < X && y < Y && z < Z && (mask[((int64_t)x * Y + y) * Z + z] & bit) != 0;
      const unsigned long long run = __ballot(on);
      const unsigned long long gaps = ~run & ((1ull << lz) - 1ull);      // the voxels below this one in its Z-run that are not in the class
      const int first = gaps ? 64 - __clzll((long long)gaps) : 0;
      lab[e] = on ? e - lz + first : -1;
      cnt[e] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CCL_PER; ++i) {
      const int e = i * CCL_THREADS + t;
      if (lds_load(lab, e) < 0) continue;      // the sign of an entry never changes
#pragma unroll
      for (int dx = -1; dx <= 0; ++dx)
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
          for (int dz = -1; dz <= 1; ++dz) {
            if (!ccl_backward<NORM>(dx, dy, dz) || (dx == 0 && dy == 0)) continue;      // (0, 0, -1): the ballot has linked it
            const int nx = i + dx, ny = ly + dy, nz = lz + dz;
            if (nx < 0 || ny < 0 || ny >= CCL_TY || nz < 0 || nz >= CCL_TZ) continue;
            const int ne = (nx * CCL_TY + ny) * CCL_TZ + nz;
            if (lds_load(lab, ne) >= 0) lds_union(lab, e, ne);      // a voxel outside the volume is background
          }
    }
    __syncthreads();
    int root[CCL_PER];
#pragma unroll
    for (int i = 0; i < CCL_PER; ++i) {      // lab is read-only from here on
      const int e = i * CCL_THREADS + t;
      root[i] = lab[e] >= 0 ? lds_find(lab, e) : -1;
      if (root[i] >= 0) atomicAdd(&cnt[root[i]], 1);
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < CCL_PER; ++i) {
      const int x = x0 + i, e = i * CCL_THREADS + t;
      if (x >= X || y >= Y || z >= Z) continue;
      const int64_t g = ((int64_t)x * Y + y) * Z + z;
      const int r = root[i];
      int gr = -1;
      if (r >= 0) gr = (int)(((int64_t)(x0 + r / (CCL_TY * CCL_TZ)) * Y + (y0 + (r / CCL_TZ) % CCL_TY)) * Z + (z0 + r % CCL_TZ));
      L[g] = gr;
      S[g] = r == e ? cnt[e] : 0;
    }
    __syncthreads();      // cnt has been read: the next tile may be staged
  }
}

// grid = ceil(V / 256); block = 256
template <int NORM>
__global__ void __launch_bounds__(CCL_THREADS) ccl_merge_kernel(int* __restrict__ L, int X, int Y, int Z, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
  if (v >= V) return;
  const int z = (int)(v % Z);
  const int64_t row = v / Z;
  const int y = (int)(row % Y), x = (int)(row / Y);
  const int lx = x % CCL_TX, ly = y % CCL_TY, lz = z % CCL_TZ;
  if (!(lx == 0 || ly == 0 || ly == CCL_TY - 1 || lz == 0 || lz == CCL_TZ - 1)) return;      // every backward neighbour is in this voxel's tile
  if (g_load(L + v) < 0) return;
#pragma unroll
  for (int dx = -1; dx <= 0; ++dx)
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy)
#pragma unroll
      for (int dz = -1; dz <= 1; ++dz) {
        if (!ccl_backward<NORM>(dx, dy, dz)) continue;
        const int nx = x + dx, ny = y + dy, nz = z + dz;
        if (nx < 0 || ny < 0 || ny >= Y || nz < 0 || nz >= Z) continue;
        if (nx / CCL_TX == x / CCL_TX && ny / CCL_TY == y / CCL_TY && nz / CCL_TZ == z / CCL_TZ) continue;      // the tile has united them
        const int64_t nv = ((int64_t)nx * Y + ny) * Z + nz;
        if (g_load(L + nv) >= 0) g_union(L, (int)v, (int)nv);
      }
}

// inclusive scan over the 64 lanes
__device__ __forceinline__ int ccl_wave_scan(int v, int lane) {
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const int u = __shfl_up(v, o, 64);
    if (lane >= o) v += u;
  }
  return v;
}

// grid = chunks; block = 256
__global__ void __launch_bounds__(CCL_THREADS) ccl_flatten_kernel(const int* __restrict__ L, int* __restrict__ R, int* __restrict__ S, int* __restrict__ bsum,
                                                                 int64_t V) {
  __shared__ int red[CCL_THREADS / 64];
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * CCL_CHUNK;
  int roots = 0;
#pragma unroll
  for (int i = 0; i < CCL_PER; ++i) {
    const int64_t v = base + i * CCL_THREADS + t;
    if (v >= V) continue;
    int p = L[v], r = -1;
    if (p >= 0) {
      r = (int)v;
      while (p != r) {
        r = p;
        p = L[r];
      }
      if (r == (int)v) {
        ++roots;
      } else {
        const int s = S[v];      // v is no final root: nobody adds to S[v]
        if (s > 0) atomicAdd(&S[r], s);
      }
    }
    R[v] = r;
  }
  roots = wave_sum(roots);
  if ((t & 63) == 0) red[t >> 6] = roots;
  __syncthreads();
  if (t == 0) bsum[blockIdx.x] = red[0] + red[1] + red[2] + red[3];
}

// one block of 256
__global__ void __launch_bounds__(CCL_THREADS) ccl_scan_kernel(const int* __restrict__ bsum, int* __restrict__ boff, int nchunks, int* __restrict__ n) {
  __shared__ int wsum[CCL_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  int carry = 0;
  for (int base = 0; base < nchunks; base += CCL_THREADS) {
    const int i = base + t;
    const int x = i < nchunks ? bsum[i] : 0;
    const int incl = ccl_wave_scan(x, lane);
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    int before = 0, total = 0;
#pragma unroll
    for (int k = 0; k < CCL_THREADS / 64; ++k) {
      before += k < w ? wsum[k] : 0;
      total += wsum[k];
    }
    if (i < nchunks) boff[i] = carry + before + incl - x;
    carry += total;
    __syncthreads();
  }
  if (t == 0) *n = carry;
}

// grid = chunks; block = 256; thread t owns the voxels base + 4 t .. + 3
__global__ void __launch_bounds__(CCL_THREADS) ccl_rank_kernel(const int* __restrict__ R, int* __restrict__ S, const int* __restrict__ boff, int* __restrict__ sizes,
                                                              int64_t V) {
  __shared__ int wsum[CCL_THREADS / 64];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t v0 = (int64_t)blockIdx.x * CCL_CHUNK + t * CCL_PER;
  bool is_root[CCL_PER];
  int c = 0;
#pragma unroll
  for (int i = 0; i < CCL_PER; ++i) {
    is_root[i] = v0 + i < V && R[v0 + i] == (int)(v0 + i);
    c += is_root[i] ? 1 : 0;
  }
  const int incl = ccl_wave_scan(c, lane);
  if (lane == 63) wsum[w] = incl;
  __syncthreads();
  int rank = boff[blockIdx.x] + incl - c;
#pragma unroll
  for (int k = 0; k < CCL_THREADS / 64; ++k) rank += k < w ? wsum[k] : 0;
#pragma unroll
  for (int i = 0; i < CCL_PER; ++i) {
    if (!is_root[i]) continue;
    sizes[rank] = S[v0 + i];
    S[v0 + i] = ++rank;
  }
}

// grid = ceil(V / 256); block = 256
__global__ void __launch_bounds__(CCL_THREADS) ccl_relabel_kernel(const int* __restrict__ R, const int* __restrict__ S, int* __restrict__ labels, int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
  if (v >= V) return;
  const int r = R[v];
  labels[v] = r >= 0 ? S[r] : 0;
}

// one block of 256: the component with the most voxels, the lowest label among equals -> *winner (a label, 1-based; -1: no component).  Thread t
// looks at sizes[t], sizes[t + 256], ...; the keys (size << 32) | ~label are distinct, so their maximum does not depend on the order.
__global__ void __launch_bounds__(CCL_THREADS) ccl_winner_kernel(const int* __restrict__ sizes, const int* __restrict__ n, int* __restrict__ winner) {
  __shared__ unsigned long long red[CCL_THREADS / 64];
  const int t = threadIdx.x, count = *n;
  unsigned long long best = 0;
  for (int i = t; i < count; i += CCL_THREADS) {
    const unsigned long long key = ((unsigned long long)(unsigned)sizes[i] << 32) | (unsigned)~(unsigned)(i + 1);
    best = key > best ? key : best;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const unsigned long long other = __shfl_xor(best, o, 64);
    best = other > best ? other : best;
  }
  if ((t & 63) == 0) red[t >> 6] = best;
  __syncthreads();
  if (t == 0) {
#pragma unroll
    for (int k = 1; k < CCL_THREADS / 64; ++k) best = red[k] > best ? red[k] : best;
    *winner = best ? (int)~(unsigned)best : -1;
  }
}

// grid = ceil(V / 256); block = 256
__global__ void __launch_bounds__(CCL_THREADS) ccl_filter_kernel(const uint8_t* __restrict__ mask, const int* __restrict__ labels, const int* __restrict__ sizes,
                                                                const int* __restrict__ winner, uint8_t* __restrict__ out, unsigned bit, int min_voxels,
                                                                int64_t V) {
  const int64_t v = (int64_t)blockIdx.x * CCL_THREADS + threadIdx.x;
  if (v >= V) return;
  unsigned m = mask[v];
  const int l = labels[v];
  if (l > 0) {
    bool keep = true;
    if (winner) keep = l == *winner;
    if (min_voxels > 0) keep = keep && sizes[l - 1] >= min_voxels;
    if (!keep) m &= ~bit;
  }
  out[v] = (uint8_t)m;
}

inline int64_t ccl_chunks(int64_t V) { return (V + CCL_CHUNK - 1) / CCL_CHUNK; }
inline bool ccl_shape_ok(int X, int Y, int Z) { return X > 0 && Y > 0 && Z > 0 && (int64_t)X * Y < ((int64_t)1 << 31) && (int64_t)X * Y * Z < ((int64_t)1 << 31); }

}  // namespace

extern "C" int pcrl_ccl_tile(int* tx, int* ty, int* tz) {
  PCRL_REQUIRE(tx && ty && tz, "ccl_tile: null pointer");
  *tx = CCL_TX;
  *ty = CCL_TY;
  *tz = CCL_TZ;
  return PCRL_OK;
}

extern "C" size_t pcrl_ccl_ws_bytes(int X, int Y, int Z) {
  if (!ccl_shape_ok(X, Y, Z)) return 0;
  const int64_t V = (int64_t)X * Y * Z;
  return (size_t)(2 * V + 2 * ccl_chunks(V)) * sizeof(int);      // R, S, bsum, boff
}

extern "C" int pcrl_ccl_label(const uint8_t* mask, int bit, int connectivity, int* labels, int* sizes, int* n, void* ws, size_t ws_bytes, int X, int Y, int Z,
                              pcrl_stream_t stream) {
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "ccl_label: empty volume %d x %d x %d", X, Y, Z);
  PCRL_REQUIRE(ccl_shape_ok(X, Y, Z), "ccl_label: volume %d x %d x %d has 2^31 voxels or more (voxel indices are 32-bit)", X, Y, Z);
  PCRL_REQUIRE(connectivity == 6 || connectivity == 18 || connectivity == 26, "ccl_label: connectivity %d is not 6, 18 or 26", connectivity);
  PCRL_REQUIRE(bit >= 0 && bit <= 6, "ccl_label: bit %d outside 0..6", bit);
  PCRL_REQUIRE(mask && labels && sizes && n, "ccl_label: null pointer");
  if (!ws || ws_bytes < pcrl_ccl_ws_bytes(X, Y, Z)) return pcrl_fail(PCRL_EWORKSPACE, "ccl_label: workspace too small");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0 && reinterpret_cast<uintptr_t>(labels) % 4 == 0, "ccl_label: labels and the workspace must be 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const int64_t V = (int64_t)X * Y * Z, chunks = ccl_chunks(V);
  int* R = static_cast<int*>(ws);
  int* S = R + V;
  int* bsum = S + V;
  int* boff = bsum + chunks;
  const int ntx = (X + CCL_TX - 1) / CCL_TX, nty = (Y + CCL_TY - 1) / CCL_TY, ntz = (Z + CCL_TZ - 1) / CCL_TZ;
  const int64_t tiles = (int64_t)ntx * nty * ntz;
  const unsigned tile_blocks = (unsigned)(tiles < CCL_MAX_BLOCKS ? tiles : CCL_MAX_BLOCKS);
  const unsigned per_voxel = (unsigned)((V + CCL_THREADS - 1) / CCL_THREADS);
  const unsigned b = 1u << bit;
  int* L = labels;
  if (connectivity == 6)
    hipLaunchKernelGGL(ccl_local_kernel<1>, dim3(tile_blocks), dim3(CCL_THREADS), 0, st, mask, b, L, S, X, Y, Z, nty, ntz, tiles);
  else if (connectivity == 18)
    hipLaunchKernelGGL(ccl_local_kernel<2>, dim3(tile_blocks), dim3(CCL_THREADS), 0, st, mask, b, L, S, X, Y, Z, nty, ntz, tiles);
  else
    hipLaunchKernelGGL(ccl_local_kernel<3>, dim3(tile_blocks), dim3(CCL_THREADS), 0, st, mask, b, L, S, X, Y, Z, nty, ntz, tiles);
  if (hipPeekAtLastError() != hipSuccess) return pcrl_check_launch("ccl_label");      // nothing that walks L is queued behind a launch that did not write it
  if (connectivity == 6)
    hipLaunchKernelGGL(ccl_merge_kernel<1>, dim3(per_voxel), dim3(CCL_THREADS), 0, st, L, X, Y, Z, V);
  else if (connectivity == 18)
    hipLaunchKernelGGL(ccl_merge_kernel<2>, dim3(per_voxel), dim3(CCL_THREADS), 0, st, L, X, Y, Z, V);
  else
    hipLaunchKernelGGL(ccl_merge_kernel<3>, dim3(per_voxel), dim3(CCL_THREADS), 0, st, L, X, Y, Z, V);
  hipLaunchKernelGGL(ccl_flatten_kernel, dim3((unsigned)chunks), dim3(CCL_THREADS), 0, st, L, R, S, bsum, V);
  hipLaunchKernelGGL(ccl_scan_kernel, dim3(1), dim3(CCL_THREADS), 0, st, bsum, boff, (int)chunks, n);
  hipLaunchKernelGGL(ccl_rank_kernel, dim3((unsigned)chunks), dim3(CCL_THREADS), 0, st, R, S, boff, sizes, V);
  hipLaunchKernelGGL(ccl_relabel_kernel, dim3(per_voxel), dim3(CCL_THREADS), 0, st, R, S, labels, V);
  return pcrl_check_launch("ccl_label");
}

extern "C" size_t pcrl_ccl_filter_ws_bytes(void) { return sizeof(int); }      // the winner's label

extern "C" int pcrl_ccl_filter(const uint8_t* mask, const int* labels, const int* sizes, const int* n, uint8_t* out, int bit, int keep_largest,
                               int64_t min_voxels, void* ws, size_t ws_bytes, int X, int Y, int Z, pcrl_stream_t stream) {
  PCRL_REQUIRE(X > 0 && Y > 0 && Z > 0, "ccl_filter: empty volume %d x %d x %d", X, Y, Z);
  PCRL_REQUIRE(ccl_shape_ok(X, Y, Z), "ccl_filter: volume %d x %d x %d has 2^31 voxels or more (voxel indices are 32-bit)", X, Y, Z);
  PCRL_REQUIRE(bit >= 0 && bit <= 6, "ccl_filter: bit %d outside 0..6", bit);
  PCRL_REQUIRE(min_voxels >= 0, "ccl_filter: min_voxels %lld is negative", (long long)min_voxels);
  PCRL_REQUIRE(mask && labels && sizes && n && out, "ccl_filter: null pointer");
  PCRL_REQUIRE(out != mask, "ccl_filter: the output mask must not be the input mask");
  if (!ws || ws_bytes < pcrl_ccl_filter_ws_bytes()) return pcrl_fail(PCRL_EWORKSPACE, "ccl_filter: workspace too small");
  PCRL_REQUIRE(reinterpret_cast<uintptr_t>(ws) % 4 == 0, "ccl_filter: the workspace must be 4-byte aligned");
  hipStream_t st = as_stream(stream);
  const int64_t V = (int64_t)X * Y * Z;
  int* winner = static_cast<int*>(ws);
  if (keep_largest) hipLaunchKernelGGL(ccl_winner_kernel, dim3(1), dim3(CCL_THREADS), 0, st, sizes, n, winner);
  const int mv = min_voxels > 0x7fffffff ? 0x7fffffff : (int)min_voxels;      // a component has fewer than 2^31 voxels
  hipLaunchKernelGGL(ccl_filter_kernel, dim3((unsigned)((V + CCL_THREADS - 1) / CCL_THREADS)), dim3(CCL_THREADS), 0, st, mask, labels, sizes,
                     keep_largest ? winner : (const int*)nullptr, out, 1u << bit, mv, V);
  return pcrl_check_launch("ccl_filter");
}

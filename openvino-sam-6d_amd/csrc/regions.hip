// SAM's min_mask_region_area clean-up (ISM/segment_anything/utils/amg.py:267-291 remove_small_regions,
// ISM/segment_anything/automatic_mask_generator.py:324-372 postprocess_small_regions) without the host: 8-connected component
// labelling of K binary masks, the component areas, and the two passes (fill small holes, then drop small islands) in place.
//
// LABELLING.  Every foreground pixel gets a parent L[p], a pixel index of its own component that is never larger than p (L = -1 off the
// foreground); the trees are joined by a lock-free union-find:
//   find(a):      follow L until L[a] == a
//   union(a, b):  a = find(a), b = find(b); while a != b: order a > b; old = atomicMin(&L[a], b); a = (old == a) ? b : old
// A parent only ever decreases, and always to a pixel of the same component, so whatever order the atomics land in, every tree ends
// rooted at the component's smallest pixel index (its first pixel in row-major order); when the atomicMin meets a node that stopped
// being a root (old < a), the union simply continues from (old, b), which restores the link the minimum may have replaced.
// Which pixel pairs are joined -- for every pair of touching row runs exactly one:
//   left:  a pixel in the first column of a 64-pixel chunk with its left neighbour (a row run that crosses a chunk border)
//   up:    U = (x, y-1) on: join with U unless the left pixel and UL = (x-1, y-1) are both on (then the left pixel joins the same runs)
//          U off: join with UL unless the left pixel is on (it has UL as its U), join with UR unless the right pixel is on (it has UR as
//          its U).  This covers the diagonal neighbours, across tile corners as anywhere else.
// Three launches:
//   1. rg_init_kernel labels tiles of 16 rows x 64 columns in LDS.  A wave owns a row of the tile: one ballot gives the row runs, a
//      pixel's first parent is its run's first pixel, the rule above (with the tile's edge for the image's) joins the runs of the tile on
//      LDS atomics, and every pixel leaves with the tile-local root as its parent; the local root's area slot gets the local count.
//   2. rg_merge_kernel joins across tile borders: the same rule on the whole image, evaluated for the pixels of a tile's first row and
//      first and last column, and carried out where the two pixels lie in different tiles (pairs inside a tile are joined already).
//      Every access to L in this launch is an agent-scope atomic (relaxed loads, atomicMin): workgroups on different XCDs read and
//      write the same words, and a plain load may be served stale from the reader's own L1 / L2.  A stale parent would still be an
//      ancestor (parents only move towards the root), so it could cost steps, never the result; the atomics make it a matter of contract.
//   3. rg_flatten_kernel finds the root once per row run (its first lane, broadcast to the run) and writes it to the run's pixels; a
//      tile-local root that is not the root adds its count to the root's slot: one integer atomic per tile-local component, order-free.
//      Run starts are the only pixels other workgroups walk through while this launch rewrites them (always to an ancestor): they are
//      read and stored as agent-scope atomics.
// Launch boundaries publish everything else.  Afterwards L[p] is the component's first pixel and A[L[p]] its area.
//
// CLEAN-UP.  holes pass: label ~m, a per-mask flag says whether any component is smaller than min_area, and if so every pixel of such
// a component is set.  islands pass, on that result: label m; flags say whether a component is smaller than min_area and whether one
// is not; where none is not, a per-mask atomicMax over (area << 32 | ~first pixel) picks the largest component, the one that comes
// first in row-major order among equals (the package's rule: cv2's numbering is not pinned).  The same launch reduces the box of the
// cleaned mask (per lane, per workgroup in LDS, then integer atomics).  Flags, key and box corners of a mask live in 48 bytes of the
// workspace behind the two 4-byte-per-pixel planes.
#include "common.h"
#include "../../include/sam6d_hip.h"

#define RG_ROWS 4                 // rows (= waves) per workgroup of the per-pixel kernels
#define RG_TILE 16                // rows of a labelling tile (64 columns wide)
#define RG_MAX_BLOCKS (1 << 20)   // tiles beyond this are walked by a grid-stride loop
#define RG_BIG 0x7fffffff

struct RgState {  // per mask
  unsigned small_holes, small_islands, big_islands, pad;
  unsigned long long key;  // (area << 32) | ~first pixel of the largest island
  int x0, y0, x1, y1;
  unsigned pad2[2];
};
static_assert(sizeof(RgState) == 48, "RgState");

template <class T>
__device__ __forceinline__ T rg_load(const T* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// parents strictly decrease towards the root; anything else (a mask rewritten under the call) ends the walk instead of leaving the plane
__device__ __forceinline__ int rg_find(const int* L, int a) {
  for (;;) {
    const int n = rg_load(L + a);
    if (n >= a || n < 0) return a;
    a = n;
  }
}

__device__ __forceinline__ void rg_union(int* L, int a, int b) {
  a = rg_find(L, a);
  b = rg_find(L, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(L + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    a = (old == a || old < 0) ? b : old;
  }
}

// the same on a tile's parents in LDS (indices row * 64 + column)
__device__ __forceinline__ int rg_find_lds(const int* lab, int a) {
  for (;;) {
    const int n = __hip_atomic_load(lab + a, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    if (n >= a || n < 0) return a;
    a = n;
  }
}
__device__ __forceinline__ void rg_union_lds(int* lab, int a, int b) {
  a = rg_find_lds(lab, a);
  b = rg_find_lds(lab, b);
  while (a != b) {
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = __hip_atomic_fetch_min(lab + a, b, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    a = (old == a || old < 0) ? b : old;
  }
}

// tiles of `rows` rows x 64 columns over the image, walked by every kernel with a trip count that is uniform over the workgroup
struct RgTiles {
  int ntx, rows;
  long ntiles;
  __host__ __device__ RgTiles(int H, int W, int rows_)
      : ntx((W + 63) >> 6), rows(rows_), ntiles((long)((W + 63) >> 6) * ((H + rows_ - 1) / rows_)) {}
  __device__ __forceinline__ void origin(long tile, int& x0, int& y0) const {
    x0 = (int)(tile % ntx) * 64;
    y0 = (int)(tile / ntx) * rows;
  }
  __device__ __forceinline__ void at(long tile, int& x, int& y) const {  // blocks of 64 x rows threads
    origin(tile, x, y);
    x += (int)threadIdx.x;
    y += (int)threadIdx.y;
  }
};

__device__ __forceinline__ bool rg_on(const unsigned char* m, int H, int W, int x, int y, int invert) {
  if (x < 0 || y < 0 || x >= W || y >= H) return false;
  return (m[(size_t)y * W + x] != 0) != (invert != 0);
}

// lane of the first pixel of the lane's run inside the chunk, and the run's length from this lane on
__device__ __forceinline__ int rg_run_start(unsigned long long bits, int lane) {
  const unsigned long long z = ~bits & ((1ull << lane) - 1ull);
  return z ? 64 - __builtin_clzll(z) : 0;
}
__device__ __forceinline__ int rg_run_len(unsigned long long bits, int lane) {
  const unsigned long long z = ~bits >> lane;
  return z ? __builtin_ctzll(z) : 64 - lane;
}

__global__ __launch_bounds__(64 * RG_ROWS) void rg_init_kernel(const unsigned char* __restrict__ masks, int H, int W, int invert,
                                                               int* __restrict__ Lall, int* __restrict__ Aall) {
  __shared__ unsigned long long rb[RG_TILE];  // the foreground of the tile's rows
  __shared__ int lab[RG_TILE * 64];           // parents
  __shared__ int cnt[RG_TILE * 64];           // pixel counts, at the local roots
  const size_t hw = (size_t)H * W;
  const unsigned char* m = masks + blockIdx.y * hw;
  int* L = Lall + blockIdx.y * hw;
  int* A = Aall + blockIdx.y * hw;
  const RgTiles tiles(H, W, RG_TILE);
  const int lane = threadIdx.x, wave = threadIdx.y;
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x0, y0;
    tiles.origin(tile, x0, y0);
    const int x = x0 + lane;
#pragma unroll
    for (int s = 0; s < RG_TILE / RG_ROWS; ++s) {
      const int r = s * RG_ROWS + wave;
      const bool on = rg_on(m, H, W, x, y0 + r, invert);
      const unsigned long long bits = __ballot(on);
      if (lane == 0) rb[r] = bits;
      lab[r * 64 + lane] = on ? r * 64 + rg_run_start(bits, lane) : -1;
      cnt[r * 64 + lane] = 0;
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RG_TILE / RG_ROWS; ++s) {
      const int r = s * RG_ROWS + wave;
      if (r == 0) continue;
      const unsigned long long bits = rb[r], up = rb[r - 1];
      if (!((bits >> lane) & 1ull)) continue;
      const bool left = lane > 0 && ((bits >> (lane - 1)) & 1ull), right = lane < 63 && ((bits >> (lane + 1)) & 1ull);
      const bool ul = lane > 0 && ((up >> (lane - 1)) & 1ull), ur = lane < 63 && ((up >> (lane + 1)) & 1ull);
      const int me = r * 64 + lane, above = me - 64;
      if ((up >> lane) & 1ull) {
        if (!(left && ul)) rg_union_lds(lab, me, above);
      } else {
        if (ul && !left) rg_union_lds(lab, me, above - 1);
        if (ur && !right) rg_union_lds(lab, me, above + 1);
      }
    }
    __syncthreads();
    int root[RG_TILE / RG_ROWS];
#pragma unroll
    for (int s = 0; s < RG_TILE / RG_ROWS; ++s) {
      const int r = s * RG_ROWS + wave;
      const unsigned long long bits = rb[r];
      root[s] = -1;
      if (((bits >> lane) & 1ull) && rg_run_start(bits, lane) == lane) {
        root[s] = rg_find_lds(lab, r * 64 + lane);
        atomicAdd(&cnt[root[s]], rg_run_len(bits, lane));
      }
    }
    __syncthreads();
#pragma unroll
    for (int s = 0; s < RG_TILE / RG_ROWS; ++s) {
      const int r = s * RG_ROWS + wave, y = y0 + r;
      const unsigned long long bits = rb[r];
      const int rt = __shfl(root[s], rg_run_start(bits, lane), 64);
      if (x < W && y < H) {
        const int p = y * W + x;
        const bool on = (bits >> lane) & 1ull;
        L[p] = on ? (y0 + (rt >> 6)) * W + x0 + (rt & 63) : -1;
        A[p] = cnt[r * 64 + lane];
      }
    }
    __syncthreads();
  }
}

// one workgroup of 128 threads per tile: threads 0 .. 63 the tile's first row, 64 .. 79 its first column, 80 .. 95 its last
__global__ __launch_bounds__(128) void rg_merge_kernel(const unsigned char* __restrict__ masks, int H, int W, int invert,
                                                       int* __restrict__ Lall) {
  const size_t hw = (size_t)H * W;
  const unsigned char* m = masks + blockIdx.y * hw;
  int* L = Lall + blockIdx.y * hw;
  const RgTiles tiles(H, W, RG_TILE);
  const int t = threadIdx.x;
  if (t >= 96) return;
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x0, y0;
    tiles.origin(tile, x0, y0);
    // rows 1 .. 15 of the columns (row 0 belongs to the first 64 threads)
    const int x = t < 64 ? x0 + t : (t < 80 ? x0 : x0 + 63);
    const int y = t < 64 ? y0 : y0 + 1 + ((t - 64) & 15);
    if (t >= 64 && ((t - 64) & 15) == 15) continue;
    if (!rg_on(m, H, W, x, y, invert)) continue;
    const int p = y * W + x;
    const bool first_col = x == x0, last_col = x == x0 + 63, first_row = y == y0;
    const bool left = rg_on(m, H, W, x - 1, y, invert);
    if (first_col && left) rg_union(L, p, p - 1);
    if (y == 0) continue;
    const bool ul = rg_on(m, H, W, x - 1, y - 1, invert);
    if (rg_on(m, H, W, x, y - 1, invert)) {
      if (first_row && !(left && ul)) rg_union(L, p, p - W);
    } else {
      if ((first_row || first_col) && ul && !left) rg_union(L, p, p - W - 1);
      if ((first_row || last_col) && rg_on(m, H, W, x + 1, y - 1, invert) && !rg_on(m, H, W, x + 1, y, invert)) rg_union(L, p, p - W + 1);
    }
  }
}

__global__ __launch_bounds__(64 * RG_ROWS) void rg_flatten_kernel(int H, int W, int* __restrict__ Lall, int* __restrict__ Aall) {
  const size_t hw = (size_t)H * W;
  int* L = Lall + blockIdx.y * hw;
  int* A = Aall + blockIdx.y * hw;
  const RgTiles tiles(H, W, RG_ROWS);
  const int lane = threadIdx.x;
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x, y;
    tiles.at(tile, x, y);
    const bool in = x < W && y < H;
    const int p = in ? y * W + x : 0;
    const bool on = in && rg_load(L + p) >= 0;
    const unsigned long long bits = __ballot(on);
    const int sl = rg_run_start(bits, lane);
    int root = -1;
    if (on && sl == lane) {
      root = rg_find(L, p);
      if (root != p) {
        const int a = A[p];  // > 0 at tile-local roots only; nobody adds to a slot that is not a root's
        if (a > 0) atomicAdd(A + root, a);
        __hip_atomic_store(L + p, root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    root = __shfl(root, sl, 64);
    if (on && sl != lane) L[p] = root;
  }
}

// labels = root + 1, areas = the root's count; 0 off the foreground
__global__ __launch_bounds__(64 * RG_ROWS) void rg_emit_kernel(int H, int W, const int* __restrict__ Lall, const int* __restrict__ Aall,
                                                               int* __restrict__ labels, int* __restrict__ areas) {
  const size_t hw = (size_t)H * W;
  const size_t base = blockIdx.y * hw;
  const RgTiles tiles(H, W, RG_ROWS);
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x, y;
    tiles.at(tile, x, y);
    if (x >= W || y >= H) continue;
    const size_t p = base + (size_t)y * W + x;
    const int l = Lall[p];
    labels[p] = l + 1;
    areas[p] = l >= 0 ? Aall[base + l] : 0;
  }
}

__global__ __launch_bounds__(64) void rg_state_init_kernel(RgState* __restrict__ st, int K) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  RgState s;
  s.small_holes = s.small_islands = s.big_islands = s.pad = 0u;
  s.key = 0ull;
  s.x0 = s.y0 = RG_BIG;
  s.x1 = s.y1 = -1;
  s.pad2[0] = s.pad2[1] = 0u;
  st[k] = s;
}

// one look at every root: is any component small, is any not, which is the largest.  A workgroup walks its share of the mask's tiles
// (rg_reduce_grid: a few dozen workgroups per mask, so that the per-mask words are not a hot spot), reduces over its waves and issues
// its atomics once.
__global__ __launch_bounds__(64 * RG_ROWS) void rg_roots_kernel(int H, int W, int min_area, int islands, const int* __restrict__ Lall,
                                                                const int* __restrict__ Aall, RgState* st) {
  __shared__ unsigned long long wkey[RG_ROWS];
  __shared__ unsigned wflags[RG_ROWS];
  const size_t hw = (size_t)H * W;
  const int* L = Lall + blockIdx.y * hw;
  const int* A = Aall + blockIdx.y * hw;
  RgState* s = st + blockIdx.y;
  const RgTiles tiles(H, W, RG_ROWS);
  bool small = false, big = false;
  unsigned long long key = 0ull;
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x, y;
    tiles.at(tile, x, y);
    if (x >= W || y >= H) continue;
    const int p = y * W + x;
    if (L[p] != p) continue;
    const int a = A[p];
    small |= a < min_area;
    big |= a >= min_area;
    const unsigned long long k = ((unsigned long long)(unsigned)a << 32) | (unsigned)~(unsigned)p;
    key = k > key ? k : key;
  }
  const unsigned flags = (__ballot(small) != 0ull ? 1u : 0u) | (__ballot(big) != 0ull ? 2u : 0u);
  key = wave_max_u64(key);
  if (threadIdx.x == 0) wflags[threadIdx.y] = flags, wkey[threadIdx.y] = key;
  __syncthreads();
  if (threadIdx.x == 0 && threadIdx.y == 0) {
    unsigned f = 0u;
    unsigned long long k = 0ull;
    for (int w = 0; w < RG_ROWS; ++w) {
      f |= wflags[w];
      k = wkey[w] > k ? wkey[w] : k;
    }
    if (f & 1u) atomicOr(islands ? &s->small_islands : &s->small_holes, 1u);
    if (islands && (f & 2u)) atomicOr(&s->big_islands, 1u);
    if (islands && k != 0ull) atomicMax(&s->key, k);
  }
}

// holes pass: L / A label ~m.  m becomes 0 / 1; where the mask has a small hole, every pixel of a small hole is set.
__global__ __launch_bounds__(64 * RG_ROWS) void rg_fill_kernel(unsigned char* __restrict__ masks, int H, int W, int min_area,
                                                               const int* __restrict__ Lall, const int* __restrict__ Aall,
                                                               const RgState* __restrict__ st) {
  const size_t hw = (size_t)H * W;
  const size_t base = blockIdx.y * hw;
  const bool any_small = st[blockIdx.y].small_holes != 0u;
  const RgTiles tiles(H, W, RG_ROWS);
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x, y;
    tiles.at(tile, x, y);
    if (x >= W || y >= H) continue;
    const size_t p = base + (size_t)y * W + x;
    const int l = Lall[p];  // >= 0 on ~m
    const bool on = l < 0 || (any_small && Aall[base + l] < min_area);
    masks[p] = on ? 1 : 0;
  }
}

// islands pass: L / A label m (already 0 / 1).  Where the mask has a small island: keep the islands that are not small, or, if there is
// none, the largest.  The box of the result goes to the mask's state: per lane over the workgroup's tiles, then over the workgroup in
// LDS, then four atomics (rg_reduce_grid, as above).
__global__ __launch_bounds__(64 * RG_ROWS) void rg_keep_kernel(unsigned char* __restrict__ masks, int H, int W, int min_area,
                                                               const int* __restrict__ Lall, const int* __restrict__ Aall, RgState* st) {
  __shared__ int bx[4];
  const size_t hw = (size_t)H * W;
  const size_t base = blockIdx.y * hw;
  RgState* s = st + blockIdx.y;
  const bool any_small = s->small_islands != 0u, any_big = s->big_islands != 0u;
  const int largest = (int)~(unsigned)(s->key & 0xffffffffull);
  const int tid = threadIdx.y * 64 + threadIdx.x;
  if (tid == 0) bx[0] = RG_BIG, bx[1] = RG_BIG, bx[2] = -1, bx[3] = -1;
  __syncthreads();
  int x_min = RG_BIG, y_min = RG_BIG, x_max = -1, y_max = -1;
  const RgTiles tiles(H, W, RG_ROWS);
  for (long tile = blockIdx.x; tile < tiles.ntiles; tile += gridDim.x) {
    int x, y;
    tiles.at(tile, x, y);
    if (x >= W || y >= H) continue;
    const size_t p = base + (size_t)y * W + x;
    const int l = Lall[p];
    bool on = l >= 0;
    if (on && any_small) {
      on = any_big ? Aall[base + l] >= min_area : l == largest;
      if (!on) masks[p] = 0;
    }
    if (on) {
      x_min = min(x_min, x), x_max = max(x_max, x);
      y_min = min(y_min, y), y_max = max(y_max, y);
    }
  }
  if (x_max >= 0) {
    atomicMin(&bx[0], x_min), atomicMin(&bx[1], y_min);
    atomicMax(&bx[2], x_max), atomicMax(&bx[3], y_max);
  }
  __syncthreads();
  if (tid == 0 && bx[2] >= 0) {
    atomicMin(&s->x0, bx[0]), atomicMin(&s->y0, bx[1]);
    atomicMax(&s->x1, bx[2]), atomicMax(&s->y1, bx[3]);
  }
}

__global__ __launch_bounds__(64) void rg_finish_kernel(const RgState* __restrict__ st, int K, unsigned char* __restrict__ changed,
                                                       int* __restrict__ box) {
  const int k = blockIdx.x * 64 + threadIdx.x;
  if (k >= K) return;
  const RgState s = st[k];
  changed[k] = (s.small_holes | s.small_islands) ? 1 : 0;
  const bool empty = s.x1 < 0;
  box[4 * k + 0] = empty ? 0 : s.x0;
  box[4 * k + 1] = empty ? 0 : s.y0;
  box[4 * k + 2] = empty ? 0 : s.x1;
  box[4 * k + 3] = empty ? 0 : s.y1;
}

// ---- host side -------------------------------------------------------------------------------------------------------------------------
static bool rg_sizes_ok(int K, int H, int W) {
  return K >= 1 && K <= 65535 && H >= 1 && W >= 1 && (long long)H * W <= 2147483646LL;
}
static size_t rg_planes_bytes(int K, int H, int W) { return (size_t)K * H * W * 2 * sizeof(int); }

static dim3 rg_grid(int K, int H, int W, int rows) {
  const RgTiles tiles(H, W, rows);
  return dim3((unsigned)(tiles.ntiles < RG_MAX_BLOCKS ? tiles.ntiles : RG_MAX_BLOCKS), K);
}

// the kernels that end in per-mask atomics: about 4096 workgroups in all, each walking its share of a mask's tiles
static dim3 rg_reduce_grid(int K, int H, int W) {
  const RgTiles tiles(H, W, RG_ROWS);
  const long per_mask = (4096 + K - 1) / K;
  return dim3((unsigned)(tiles.ntiles < per_mask ? tiles.ntiles : per_mask), K);
}

// init, merge, flatten: the planes L and A of `masks` (or of their complement)
static int rg_label(const unsigned char* masks, int K, int H, int W, int invert, int* L, int* A, hipStream_t s, const char* who) {
  const dim3 block(64, RG_ROWS);
  hipLaunchKernelGGL(rg_init_kernel, rg_grid(K, H, W, RG_TILE), block, 0, s, masks, H, W, invert, L, A);
  SAM6D_LAUNCH_CHECK_CONT(who);
  hipLaunchKernelGGL(rg_merge_kernel, rg_grid(K, H, W, RG_TILE), dim3(128), 0, s, masks, H, W, invert, L);
  SAM6D_LAUNCH_CHECK_CONT(who);
  hipLaunchKernelGGL(rg_flatten_kernel, rg_grid(K, H, W, RG_ROWS), block, 0, s, H, W, L, A);
  SAM6D_LAUNCH_CHECK(who);
}

extern "C" size_t sam6d_mask_components_workspace_bytes(int K, int H, int W) {
  if (!rg_sizes_ok(K, H, W)) return 0;
  return rg_planes_bytes(K, H, W);
}

extern "C" int sam6d_mask_components(const unsigned char* masks, int K, int H, int W, int invert, int* labels, int* areas, void* ws,
                                     size_t ws_bytes, void* stream) {
  SAM6D_REQUIRE(K >= 1 && K <= 65535, "mask_components: 1 <= K <= 65535 (got %d)", K);
  SAM6D_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 2147483646LL, "mask_components: H * W <= 2^31 - 2 (got %d x %d)", H, W);
  SAM6D_REQUIRE(masks && labels && areas && ws, "mask_components: null pointer");
  SAM6D_REQUIRE(ws_bytes >= sam6d_mask_components_workspace_bytes(K, H, W), "mask_components: workspace too small (%zu < %zu bytes)",
                ws_bytes, sam6d_mask_components_workspace_bytes(K, H, W));
  SAM6D_REQUIRE(((uintptr_t)ws & 3u) == 0, "mask_components: the workspace must be 4-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int* L = (int*)ws;
  int* A = L + (size_t)K * H * W;
  const int rc = rg_label(masks, K, H, W, invert, L, A, s, "mask_components");
  if (rc != 0) return rc;
  hipLaunchKernelGGL(rg_emit_kernel, rg_grid(K, H, W, RG_ROWS), dim3(64, RG_ROWS), 0, s, H, W, (const int*)L, (const int*)A, labels, areas);
  SAM6D_LAUNCH_CHECK("mask_components");
}

extern "C" size_t sam6d_amg_small_regions_workspace_bytes(int K, int H, int W) {
  if (!rg_sizes_ok(K, H, W)) return 0;
  return rg_planes_bytes(K, H, W) + (size_t)K * sizeof(RgState);
}

extern "C" int sam6d_amg_small_regions(unsigned char* masks, int K, int H, int W, int min_area, unsigned char* changed, int* box, void* ws,
                                       size_t ws_bytes, void* stream) {
  SAM6D_REQUIRE(K >= 1 && K <= 65535, "amg_small_regions: 1 <= K <= 65535 (got %d)", K);
  SAM6D_REQUIRE(H >= 1 && W >= 1 && (long long)H * W <= 2147483646LL, "amg_small_regions: H * W <= 2^31 - 2 (got %d x %d)", H, W);
  SAM6D_REQUIRE(min_area >= 1, "amg_small_regions: min_area >= 1 (got %d)", min_area);
  SAM6D_REQUIRE(masks && changed && box && ws, "amg_small_regions: null pointer");
  SAM6D_REQUIRE(ws_bytes >= sam6d_amg_small_regions_workspace_bytes(K, H, W), "amg_small_regions: workspace too small (%zu < %zu bytes)",
                ws_bytes, sam6d_amg_small_regions_workspace_bytes(K, H, W));
  SAM6D_REQUIRE(((uintptr_t)ws & 7u) == 0, "amg_small_regions: the workspace must be 8-byte aligned");
  hipStream_t s = (hipStream_t)stream;
  int* L = (int*)ws;
  int* A = L + (size_t)K * H * W;
  RgState* st = (RgState*)(A + (size_t)K * H * W);  // 8-byte aligned: the planes are a multiple of 8 bytes
  const dim3 grid = rg_grid(K, H, W, RG_ROWS), rgrid = rg_reduce_grid(K, H, W), block(64, RG_ROWS);
  hipLaunchKernelGGL(rg_state_init_kernel, dim3(cdiv(K, 64)), dim3(64), 0, s, st, K);
  SAM6D_LAUNCH_CHECK_CONT("amg_small_regions");
  int rc = rg_label(masks, K, H, W, 1, L, A, s, "amg_small_regions");  // holes
  if (rc != 0) return rc;
  hipLaunchKernelGGL(rg_roots_kernel, rgrid, block, 0, s, H, W, min_area, 0, (const int*)L, (const int*)A, st);
  SAM6D_LAUNCH_CHECK_CONT("amg_small_regions");
  hipLaunchKernelGGL(rg_fill_kernel, grid, block, 0, s, masks, H, W, min_area, (const int*)L, (const int*)A, (const RgState*)st);
  SAM6D_LAUNCH_CHECK_CONT("amg_small_regions");
  rc = rg_label(masks, K, H, W, 0, L, A, s, "amg_small_regions");  // islands
  if (rc != 0) return rc;
  hipLaunchKernelGGL(rg_roots_kernel, rgrid, block, 0, s, H, W, min_area, 1, (const int*)L, (const int*)A, st);
  SAM6D_LAUNCH_CHECK_CONT("amg_small_regions");
  hipLaunchKernelGGL(rg_keep_kernel, rgrid, block, 0, s, masks, H, W, min_area, (const int*)L, (const int*)A, st);
  SAM6D_LAUNCH_CHECK_CONT("amg_small_regions");
  hipLaunchKernelGGL(rg_finish_kernel, dim3(cdiv(K, 64)), dim3(64), 0, s, (const RgState*)st, K, changed, box);
  SAM6D_LAUNCH_CHECK("amg_small_regions");
}

// dense_speckle_device.hpp — the kernels of the speckle filter for disparity planes (include/vo_hip.h, "Speckle filter", has the
// definition): connected-component labelling in four launches that follow each other on one stream — tile-local
// union-find in LDS, the merge across the tiles' edges, root finding with the sizes summed per tile, and the removal. Read by
// csrc/dense_speckle.hip for gfx950 and by tests/emu/emu_dense_speckle.cpp on CPU threads. The includer supplies
//   SPK_LD_LDS(p)     a relaxed load of an LDS word that other lanes of the workgroup change with atomics
//   SPK_LD_AGENT(p)   a relaxed agent-scope load of a global word that other workgroups change with atomics
// and, on the CPU, atomicMin and atomicCAS. A parent word only ever decreases and always names a pixel of its own component, so
// every walk over parent links ends at a root, whatever the order in which lanes and workgroups arrive; each walk also stops after n
// = W H steps. Nothing waits for another lane or workgroup; every index is clamped before it forms an address; integer atomics only.
#pragma once
#include <stdint.h>

#define SPK_NT 256  // threads per workgroup, all four kernels
#define SPK_TW 64   // tile: 64 x 16 pixels, four a lane
#define SPK_TH 16
#define SPK_TILE (SPK_TW * SPK_TH)
#define SPK_PIX (SPK_TILE / SPK_NT)

struct SpkArgs {
  float *disp, *sigma;  // W x H planes, tightly packed; sigma may be null
  uint8_t *status;
  int32_t *label, *size;  // W x H words each: the parent / root plane and the sizes (a root's word; after the removal every pixel's)
  int *counters;          // [0] n_removed, [1] n_components
  int W, H, n;            // n = W H
  int ntx, nty;           // tiles a row, a column
  int max_size;
  float max_diff;
};

// two valid 4-neighbours are joined: one float32 subtraction, rounded; a NaN fails
__device__ __forceinline__ bool spk_joined(float a, float b, float max_diff) { return fabsf(a - b) <= max_diff; }

__device__ __forceinline__ int spk_clamp(int i, int n) { return i < 0 ? 0 : i > n - 1 ? n - 1 : i; }

// ---- union-find on LDS indices ---------------------------------------------------------------------------------------------------
__device__ __forceinline__ int spk_find_lds(int *par, int x, int n) {
  for (int it = 0; it < n; ++it) {
    const int p = SPK_LD_LDS(&par[spk_clamp(x, SPK_TILE)]);
    if (p == x || p < 0) break;
    x = p;
  }
  return x;
}
// lock-free: the larger root's word takes the smaller root by atomicMin; where that word had changed meanwhile, go on from what it held
__device__ __forceinline__ void spk_unite_lds(int *par, int a, int b, int n) {
  for (int it = 0; it < n; ++it) {
    a = spk_find_lds(par, a, n);
    b = spk_find_lds(par, b, n);
    if (a == b) break;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&par[spk_clamp(a, SPK_TILE)], b);
    if (old == a) break;
    a = old;
  }
}

// ---- the same on the label plane's global words ----------------------------------------------------------------------------------
__device__ __forceinline__ int spk_find(int32_t *label, int x, int n) {
  for (int it = 0; it < n; ++it) {
    const int p = SPK_LD_AGENT(&label[spk_clamp(x, n)]);
    if (p == x || p < 0) break;
    x = p;
  }
  return x;
}
__device__ __forceinline__ void spk_unite(int32_t *label, int a, int b, int n) {
  for (int it = 0; it < n; ++it) {
    a = spk_find(label, a, n);
    b = spk_find(label, b, n);
    if (a == b) break;
    if (a < b) {
      const int t = a;
      a = b;
      b = t;
    }
    const int old = atomicMin(&label[spk_clamp(a, n)], b);
    if (old == a) break;
    a = old;
  }
}

// [1] grid (ntx, nty): a tile's components. The parent of every valid pixel is written as a GLOBAL raster index (the smallest of its
// tile-local component: local and global raster order agree inside a tile), -1 on invalid pixels; the tile's size words and (the
// first workgroup) the counters are zeroed for the launches behind this one.
__global__ __launch_bounds__(SPK_NT) void speckle_local_kernel(SpkArgs a) {
  __shared__ float sd[SPK_TILE];
  __shared__ int par[SPK_TILE];
  const int t = (int)threadIdx.x, tx0 = (int)blockIdx.x * SPK_TW, ty0 = (int)blockIdx.y * SPK_TH;
  if (blockIdx.x == 0 && blockIdx.y == 0 && t < 2) a.counters[t] = 0;
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int li = t + k * SPK_NT, gx = tx0 + (li & (SPK_TW - 1)), gy = ty0 + li / SPK_TW;
    const bool in = gx < a.W && gy < a.H;
    const int g = in ? gy * a.W + gx : 0;
    const bool v = in && a.status[g] == 1;
    sd[li] = v ? a.disp[g] : 0.0f;
    par[li] = v ? li : -1;
    if (in) a.size[g] = 0;
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int li = t + k * SPK_NT, lx = li & (SPK_TW - 1), ly = li / SPK_TW;
    if (SPK_LD_LDS(&par[li]) < 0) continue;
    const float d = sd[li];
    if (lx > 0 && SPK_LD_LDS(&par[li - 1]) >= 0 && spk_joined(d, sd[li - 1], a.max_diff)) spk_unite_lds(par, li, li - 1, a.n);
    if (ly > 0 && SPK_LD_LDS(&par[li - SPK_TW]) >= 0 && spk_joined(d, sd[li - SPK_TW], a.max_diff)) spk_unite_lds(par, li, li - SPK_TW, a.n);
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int li = t + k * SPK_NT, gx = tx0 + (li & (SPK_TW - 1)), gy = ty0 + li / SPK_TW;
    if (gx >= a.W || gy >= a.H) continue;
    int out = -1;
    if (par[li] >= 0) {
      const int r = spk_clamp(spk_find_lds(par, li, a.n), SPK_TILE);
      out = (ty0 + r / SPK_TW) * a.W + tx0 + (r & (SPK_TW - 1));
    }
    a.label[gy * a.W + gx] = out;
  }
}

// [2] a lane per pixel on a tile's right edge ((ntx - 1) H of them), then per pixel on a bottom edge ((nty - 1) W): joined with its
// neighbour across the edge, the two trees are united. Only words that were roots after [1] are ever changed, and only downwards.
// A pair whose predecessor along the edge (inside the same tile) is joined too and, as read now, hangs under the same two words
// is left to that predecessor: equal words mean equal components, so its union — or the one it defers to — covers this pair.
__global__ __launch_bounds__(SPK_NT) void speckle_merge_kernel(SpkArgs a) {
  const int i = (int)blockIdx.x * SPK_NT + (int)threadIdx.x, nr = (a.ntx - 1) * a.H, nb = (a.nty - 1) * a.W;
  if (i >= nr + nb) return;
  int x, y, step, prev;  // the pair is (p, p + step), its predecessor (p - prev, p - prev + step); prev = 0: none
  if (i < nr) {
    x = (i / a.H + 1) * SPK_TW - 1;
    y = i % a.H;
    step = 1;
    prev = (y % SPK_TH) != 0 ? a.W : 0;
  } else {
    const int j = i - nr;
    x = j % a.W;
    y = (j / a.W + 1) * SPK_TH - 1;
    step = a.W;
    prev = (x % SPK_TW) != 0 ? 1 : 0;
  }
  const int p = spk_clamp(y * a.W + x, a.n), q = spk_clamp(p + step, a.n);
  if (p == q || a.status[p] != 1 || a.status[q] != 1 || !spk_joined(a.disp[p], a.disp[q], a.max_diff)) return;
  if (prev) {
    const int pp = spk_clamp(p - prev, a.n), qp = spk_clamp(q - prev, a.n);
    if (a.status[pp] == 1 && a.status[qp] == 1 && spk_joined(a.disp[pp], a.disp[qp], a.max_diff) &&
        SPK_LD_AGENT(&a.label[p]) == SPK_LD_AGENT(&a.label[pp]) && SPK_LD_AGENT(&a.label[q]) == SPK_LD_AGENT(&a.label[qp]))
      return;
  }
  spk_unite(a.label, p, q, a.n);
}

// [3] grid (ntx, nty): every valid pixel's root, and the sizes summed per tile. A pixel's word as [1] and [2] left it names a pixel
// of its component inside the tile (its tile-local root) or, for a tile-local root that [2] hung under another tile, outside: the
// pixels are counted per such in-tile word in LDS (a lane's equal neighbours combined first), only the counted words walk to their
// roots through global memory, and a second LDS table keyed by root combines the tile-local components of one root: one global add
// per tile and distinct root. Roots are counted into counters[1], one add per workgroup. The label words other workgroups walk over
// meanwhile only change to their own roots.
__global__ __launch_bounds__(SPK_NT) void speckle_flatten_kernel(SpkArgs a) {
  __shared__ int cnt[SPK_TILE], root[SPK_TILE], hkey[SPK_TILE], hval[SPK_TILE];
  __shared__ int n_roots;
  const int t = (int)threadIdx.x, tx0 = (int)blockIdx.x * SPK_TW, ty0 = (int)blockIdx.y * SPK_TH;
  if (t == 0) n_roots = 0;
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) cnt[t + k * SPK_NT] = 0, hkey[t + k * SPK_NT] = -1, hval[t + k * SPK_NT] = 0;
  __syncthreads();
  // a lane's four pixels are neighbours in a row here: li = 4 (t % 16) + k, row t / 16
  const int lrow = t / (SPK_TW / SPK_PIX), lcol = (t % (SPK_TW / SPK_PIX)) * SPK_PIX, gy = ty0 + lrow;
  int key[SPK_PIX];
  int run_key = -1, run = 0;
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int gx = tx0 + lcol + k;
    key[k] = -1;
    if (gx < a.W && gy < a.H) {
      const int g = gy * a.W + gx, l = a.label[g];
      if (l >= 0) {
        const int ly = l / a.W - ty0, lx = l % a.W - tx0;
        key[k] = (ly >= 0 && ly < SPK_TH && lx >= 0 && lx < SPK_TW) ? ly * SPK_TW + lx : lrow * SPK_TW + lcol + k;
      }
    }
    if (key[k] != run_key) {
      if (run_key >= 0) atomicAdd(&cnt[spk_clamp(run_key, SPK_TILE)], run);
      run_key = key[k];
      run = 0;
    }
    ++run;
  }
  if (run_key >= 0) atomicAdd(&cnt[spk_clamp(run_key, SPK_TILE)], run);
  __syncthreads();
  int mine = 0;
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int li = t + k * SPK_NT, c = cnt[li];
    if (c == 0) continue;
    const int g = spk_clamp((ty0 + li / SPK_TW) * a.W + tx0 + (li & (SPK_TW - 1)), a.n);
    const int r = spk_find(a.label, g, a.n);
    root[li] = r;
    mine += r == g;
    unsigned h = ((unsigned)r * 2654435761u) >> 22;  // 10 bits: SPK_TILE slots, at most SPK_TILE / 2 + 1 keys (a checkerboard)
    for (int it = 0; it < SPK_TILE; ++it) {
      const int old = atomicCAS(&hkey[h & (SPK_TILE - 1)], -1, r);
      if (old == -1 || old == r) {
        atomicAdd(&hval[h & (SPK_TILE - 1)], c);
        break;
      }
      ++h;
    }
  }
  if (mine) atomicAdd(&n_roots, mine);
  __syncthreads();
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int li = t + k * SPK_NT, r = hkey[li];
    if (r >= 0) atomicAdd(&a.size[spk_clamp(r, a.n)], hval[li]);
  }
  if (t == 0 && n_roots) atomicAdd(&a.counters[1], n_roots);
#pragma unroll
  for (int k = 0; k < SPK_PIX; ++k) {
    const int gx = tx0 + lcol + k;
    if (key[k] >= 0 && gx < a.W && gy < a.H) a.label[gy * a.W + gx] = root[spk_clamp(key[k], SPK_TILE)];
  }
}

// [4] grid ceil(n / SPK_NT): a pixel per lane. The size of its root becomes the pixel's own size word (a root's word keeps its value,
// and only roots' words are read by others); a component of at most max_size pixels is removed. counters[0]: one add per workgroup.
__global__ __launch_bounds__(SPK_NT) void speckle_apply_kernel(SpkArgs a) {
  __shared__ int n_removed;
  if (threadIdx.x == 0) n_removed = 0;
  __syncthreads();
  const int i = (int)blockIdx.x * SPK_NT + (int)threadIdx.x;
  if (i < a.n) {
    const int l = a.label[i];
    if (l >= 0) {
      const int s = a.size[spk_clamp(l, a.n)];
      if (l != i) a.size[i] = s;
      if (s <= a.max_size) {
        a.status[i] = 6;  // VO_DISPARITY_SPECKLE
        a.disp[i] = 0.0f;
        if (a.sigma) a.sigma[i] = 0.0f;
        atomicAdd(&n_removed, 1);
      }
    }
  }
  __syncthreads();
  if (threadIdx.x == 0 && n_removed) atomicAdd(&a.counters[0], n_removed);
}

// clahe_device.hpp — the two kernels of the CLAHE equalisation in front of the image ingestion (include/vo_hip.h:
// vo_set_equalize has the arithmetic). Included by clahe.hip and, through tests/emu/hip_emu.h, by the CPU
// harness (tests/emu/emu_clahe.cpp) that runs this text against the numpy restatement (tests/clahe_restatement.py).
//
// The arithmetic restates cv::CLAHE::apply for 8-bit images (OpenCV 4.x imgproc/src/clahe.cpp) from knowledge of upstream; it
// is NOT pinned against an OpenCV build (like every third-party restatement here).
//
//   clahe_hist_kernel   grid (slabs, tiles, images). A workgroup takes `slab_rows` rows of one tile of the image as extended to
//                       the right and the bottom with BORDER_REFLECT_101 and counts them in an LDS histogram. A tile of up to
//                       about 8192 pixels is one workgroup's (every usual grid): it goes straight on. A larger tile is split:
//                       each workgroup adds its counts to the tile's 256 global counters, and the last one to arrive (by
//                       ticket) reads them back and puts counters and ticket back to zero. That workgroup clips the
//                       histogram, spreads the excess, scans it and writes the tile's 256-byte look-up table.
//                       All of this is integer arithmetic: the order in which the counts arrive does not show in the result.
//   clahe_blend_kernel  grid (ceil(w / 256), ceil(h / 8), images). A workgroup stages the look-up tables its 256 x 8 pixels
//                       interpolate between in LDS; a lane blends four neighbouring pixels and stores them as one dword.
//                       Every product and every sum of the blend is rounded to float on its own (no FMA).
//
// What the includer provides: CLAHE_LD_AGENT / CLAHE_ST_AGENT / CLAHE_ATOMIC_ADD_AGENT (relaxed, agent scope),
// CLAHE_FENCE_RELEASE / CLAHE_FENCE_ACQUIRE (agent scope), CLAHE_DYN_LDS(name) (the blend kernel's dynamic LDS).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIP_DEVICE_COMPILE__)
#define CLAHE_FMUL(a, b) __fmul_rn((a), (b))
#define CLAHE_FADD(a, b) __fadd_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define CLAHE_FMUL(a, b) ((a) * (b))
#define CLAHE_FADD(a, b) ((a) + (b))
#endif

#define CLAHE_NT 256         // threads of both kernels: one per histogram bin in the finishing step
#define CLAHE_BLEND_COLS 256 // pixels per workgroup row of the blend: 64 lanes x 4
#define CLAHE_BLEND_ROWS 8
#define CLAHE_MAX_TILES 32   // per dimension (vo_set_equalize)
#define CLAHE_HIST_UNROLL 8  // dwords a thread of the histogram kernel has in flight

struct ClaheImage {
  const uint8_t *src;  // w x h, sstride bytes per row
  uint8_t *dst;        // w x h, dstride bytes per row; 4-byte aligned rows with room for (w + 3) & ~3 bytes
  uint8_t *lut;        // tiles_y * tiles_x tables of 256 bytes, row-major by tile
  int *hist;           // tiles_y * tiles_x * 256 counters, zero between launches
  int *ticket;         // one per tile, zero between launches
};
struct ClaheArgs {
  ClaheImage img[2];
  int w, h, sstride, dstride;
  int tiles_x, tiles_y, tw, th;  // tile grid and tile size of the EXTENDED image
  int slab_rows, slabs;          // histogram launch: rows of a tile per workgroup, workgroups per tile
  int cpr;                       // dwords per tile row, ceil(tw / 4)
  unsigned cpr_magic;            // ceil(2^32 / cpr) for cpr > 1: i / cpr == umulhi(i, cpr_magic) while i * cpr < 2^32
  int limit;                     // a bin's clip limit (>= tw * th: nothing is clipped)
  float lut_scale;               // (float)255 / (float)(tw * th)
  float inv_tw, inv_th;          // 1.0f / tw, 1.0f / th
  int lds_cols, lds_rows;        // blend launch: room of the LDS stage, in tables
};

// What both launches need to know about an image w x h (w > tiles_x, h > tiles_y) — host code, shared by the launcher and the
// emulation harness. slab_px: pixels of a tile per histogram workgroup, about. The product's 8192 gives a tile of
// the usual grids (8 x 8 on 1241 x 376: 7488 pixels) to ONE workgroup, which then needs no global counters at all; larger tiles are split.
static inline void clahe_plan(ClaheArgs *a, int w, int h, int tiles_x, int tiles_y, double clip, int slab_px) {
  a->w = w;
  a->h = h;
  a->tiles_x = tiles_x;
  a->tiles_y = tiles_y;
  // the extension: both amounts whenever either remainder is non-zero (a dividing dimension then grows by a full tile count)
  const bool ext = (w % tiles_x) != 0 || (h % tiles_y) != 0;
  a->tw = (ext ? w + (tiles_x - w % tiles_x) : w) / tiles_x;
  a->th = (ext ? h + (tiles_y - h % tiles_y) : h) / tiles_y;
  const int total = a->tw * a->th;
  a->limit = total;
  if (clip > 0.0) {
    const double lim = clip * (double)total / 256.0;
    if (lim < (double)total) a->limit = (int)lim > 1 ? (int)lim : 1;  // (a limit of `total` or more cuts nothing)
  }
  a->lut_scale = (float)255 / (float)total;
  a->inv_tw = 1.0f / (float)a->tw;
  a->inv_th = 1.0f / (float)a->th;
  int slabs = (total + slab_px - 1) / slab_px;
  slabs = slabs < 1 ? 1 : (slabs > a->th ? a->th : slabs);
  a->slab_rows = (a->th + slabs - 1) / slabs;
  a->slabs = (a->th + a->slab_rows - 1) / a->slab_rows;
  a->cpr = (a->tw + 3) / 4;
  a->cpr_magic = a->cpr > 1 ? (unsigned)((0x100000000ull + (unsigned)a->cpr - 1) / (unsigned)a->cpr) : 0u;
  // blend: 256 x 8 pixels lie in at most floor(255 / tw) + 2 cells along x (floor(7 / th) + 2 along y), one more table than cells
  a->lds_cols = (CLAHE_BLEND_COLS - 1) / a->tw + 3;
  a->lds_rows = (CLAHE_BLEND_ROWS - 1) / a->th + 3;
  if (a->lds_cols > tiles_x) a->lds_cols = tiles_x;
  if (a->lds_rows > tiles_y) a->lds_rows = tiles_y;  // tw, th >= 2: at most 32 x 6 tables = 48 KiB
}

// Host check of that sizing, for the launcher in front of the blend launch: walks the workgroups along one axis with the kernel's
// own float expression for the cell index and returns whether each of them touches at most `room` tables.
static inline bool clahe_stage_axis_fits(int n, int per_group, float inv_t, int tiles, int room) {
  for (int p0 = 0; p0 < n; p0 += per_group) {
    const int pl = p0 + per_group - 1 < n - 1 ? p0 + per_group - 1 : n - 1;
    int t0 = (int)__builtin_floorf((float)p0 * inv_t + -0.5f), t1 = (int)__builtin_floorf((float)pl * inv_t + -0.5f) + 1;
    t0 = t0 < 0 ? 0 : (t0 > tiles - 1 ? tiles - 1 : t0);
    t1 = t1 > tiles - 1 ? tiles - 1 : t1;
    if (t1 - t0 + 1 > room) return false;
  }
  return true;
}
static inline bool clahe_stage_fits(const ClaheArgs *a) {
  return clahe_stage_axis_fits(a->w, CLAHE_BLEND_COLS, a->inv_tw, a->tiles_x, a->lds_cols) &&
         clahe_stage_axis_fits(a->h, CLAHE_BLEND_ROWS, a->inv_th, a->tiles_y, a->lds_rows);
}

// saturate_cast<uchar>(float): round half to even, clamped
__device__ __forceinline__ int clahe_sat_u8(float v) {
  const float r = __builtin_rintf(v);
  return r <= 0.0f ? 0 : (r >= 255.0f ? 255 : (int)r);
}

// the interpolation cell of pixel coordinate p along one axis: the unclamped lower tile index (the weights use it)
__device__ __forceinline__ int clahe_cell(int p, float inv_t, float *wa, float *wa1) {
  const float tf = CLAHE_FADD(CLAHE_FMUL((float)p, inv_t), -0.5f);
  const int t1 = (int)__builtin_floorf(tf);
  const float a = CLAHE_FADD(tf, -(float)t1);
  *wa = a;
  *wa1 = CLAHE_FADD(1.0f, -a);
  return t1;
}

__global__ __launch_bounds__(CLAHE_NT) void clahe_hist_kernel(ClaheArgs a) {
  __shared__ int s_h[256];
  __shared__ int s_v[2][256], s_c[2][256];
  __shared__ int s_last;
  const int tid = (int)threadIdx.x;
  const int tile = (int)blockIdx.y;
  const ClaheImage I = a.img[blockIdx.z];
  const int tx = tile % a.tiles_x, ty = tile / a.tiles_x;
  s_h[tid] = 0;
  __syncthreads();
  // ---- this workgroup's rows of the tile, four neighbouring pixels (one dword) at a time --------------------------------------------
  // All loads of a round are issued before the first count: the kernel is as long as its chain of dependent memory round trips.
  const int r0 = (int)blockIdx.x * a.slab_rows;
  const int r1 = r0 + a.slab_rows < a.th ? r0 + a.slab_rows : a.th;
  const int n = (r1 - r0) * a.cpr;  // dwords: cpr = ceil(tw / 4) per row of the tile
  const int tx0 = tx * a.tw, ty0 = ty * a.th + r0;
  for (int base = 0; base < n; base += CLAHE_HIST_UNROLL * CLAHE_NT) {
    uint32_t px[CLAHE_HIST_UNROLL];
    int cnt[CLAHE_HIST_UNROLL];
#pragma unroll
    for (int k = 0; k < CLAHE_HIST_UNROLL; ++k) {
      const int i = base + k * CLAHE_NT + tid;
      px[k] = 0;
      cnt[k] = 0;
      if (i < n) {
        const int r = a.cpr == 1 ? i : (int)__umulhi((unsigned)i, a.cpr_magic);  // i / cpr (exact: i, cpr < 2^16)
        const int cx = 4 * (i - r * a.cpr);
        int y = ty0 + r;
        // the extension (at most tiles_x columns / tiles_y rows, and w > tiles_x, h > tiles_y): one reflection, never below 0
        if (y >= a.h) y = 2 * a.h - 2 - y;
        const uint8_t *row = I.src + (size_t)y * a.sstride;
        const int x = tx0 + cx;
        cnt[k] = a.tw - cx < 4 ? a.tw - cx : 4;
        if (cnt[k] == 4 && x + 3 < a.w) {
          __builtin_memcpy(&px[k], row + x, 4);  // (any byte address: the caller's image makes no alignment promise)
        } else {
          for (int b = 0; b < cnt[k]; ++b) {
            const int xb = x + b < a.w ? x + b : 2 * a.w - 2 - (x + b);
            px[k] |= (uint32_t)row[xb] << (8 * b);
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CLAHE_HIST_UNROLL; ++k)
      for (int b = 0; b < cnt[k]; ++b) atomicAdd(&s_h[(px[k] >> (8 * b)) & 255u], 1);
  }
  __syncthreads();
  int v = s_h[tid];  // bin tid
  if (a.slabs > 1) {
    int *gh = I.hist + (size_t)tile * 256;
    if (v) CLAHE_ATOMIC_ADD_AGENT(&gh[tid], v);
    CLAHE_FENCE_RELEASE();  // every thread: its counts have been performed ...
    __syncthreads();        // ... before thread 0 takes the workgroup's ticket
    if (tid == 0) s_last = (CLAHE_ATOMIC_ADD_AGENT(&I.ticket[tile], 1) == a.slabs - 1) ? 1 : 0;
    __syncthreads();
    if (!s_last) return;
    CLAHE_FENCE_ACQUIRE();
    v = CLAHE_LD_AGENT(&gh[tid]);
    // back to zero for the next image (every workgroup of the tile has added its counts: this one holds the last ticket)
    CLAHE_ST_AGENT(&gh[tid], 0);
    if (tid == 0) CLAHE_ST_AGENT(&I.ticket[tile], 0);
  }
  // ---- clip; the running sums of the clipped bins and of what was cut, in one double-buffered scan ----------------------------------
  int cut = 0;
  if (v > a.limit) {
    cut = v - a.limit;
    v = a.limit;
  }
  int p = 0;
  s_v[0][tid] = v;
  s_c[0][tid] = cut;
  __syncthreads();
  for (int d = 1; d < 256; d <<= 1) {
    const int tv = s_v[p][tid] + (tid >= d ? s_v[p][tid - d] : 0), tc = s_c[p][tid] + (tid >= d ? s_c[p][tid - d] : 0);
    p ^= 1;
    s_v[p][tid] = tv;
    s_c[p][tid] = tc;
    __syncthreads();
  }
  // ---- spread what was cut: `batch` to every bin, one more to bins 0, step, 2 step, ... (`residual` of them) — in the running sum
  // up to bin tid that is batch * (tid + 1) and the number of those bins at or below tid
  const int clipped = s_c[p][255];
  const int batch = clipped / 256, residual = clipped - 256 * batch;
  int sum = s_v[p][tid] + batch * (tid + 1);
  if (residual != 0) {
    const int step = 256 / residual > 1 ? 256 / residual : 1;
    const int below = tid / step + 1;
    sum += below < residual ? below : residual;
  }
  I.lut[(size_t)tile * 256 + tid] = (uint8_t)clahe_sat_u8(CLAHE_FMUL((float)sum, a.lut_scale));
}

__global__ __launch_bounds__(CLAHE_NT) void clahe_blend_kernel(ClaheArgs a) {
  CLAHE_DYN_LDS(s_lut);  // [rows][cols][256] bytes of the tables this workgroup's pixels touch
  const int tid = (int)threadIdx.x;
  const ClaheImage I = a.img[blockIdx.z];
  const int x0 = (int)blockIdx.x * CLAHE_BLEND_COLS, y0 = (int)blockIdx.y * CLAHE_BLEND_ROWS;
  const int xl = x0 + CLAHE_BLEND_COLS - 1 < a.w - 1 ? x0 + CLAHE_BLEND_COLS - 1 : a.w - 1;
  const int yl = y0 + CLAHE_BLEND_ROWS - 1 < a.h - 1 ? y0 + CLAHE_BLEND_ROWS - 1 : a.h - 1;
  float u0, u1;
  // the cell index grows with the coordinate: the first and the last pixel bound the tables of all of them
  int c0 = clahe_cell(x0, a.inv_tw, &u0, &u1), c1 = clahe_cell(xl, a.inv_tw, &u0, &u1) + 1;
  int q0 = clahe_cell(y0, a.inv_th, &u0, &u1), q1 = clahe_cell(yl, a.inv_th, &u0, &u1) + 1;
  c0 = c0 < 0 ? 0 : (c0 > a.tiles_x - 1 ? a.tiles_x - 1 : c0);
  q0 = q0 < 0 ? 0 : (q0 > a.tiles_y - 1 ? a.tiles_y - 1 : q0);
  c1 = c1 > a.tiles_x - 1 ? a.tiles_x - 1 : c1;
  q1 = q1 > a.tiles_y - 1 ? a.tiles_y - 1 : q1;
  const int ncols = c1 - c0 + 1, nrows = q1 - q0 + 1;
  // (never taken: the launcher refuses a plan whose stage does not hold every workgroup's tables, clahe_stage_fits; this only
  // keeps a workgroup inside its LDS if a launcher forgot to ask)
  if (ncols > a.lds_cols || nrows > a.lds_rows) return;
  {
    uint32_t *s32 = (uint32_t *)s_lut;
    const int nd = ncols * nrows * 64;
    for (int i = tid; i < nd; i += CLAHE_NT) {
      const int l = i >> 6, rr = l / ncols, cc = l - rr * ncols;
      s32[i] = ((const uint32_t *)(I.lut + ((size_t)(q0 + rr) * a.tiles_x + (c0 + cc)) * 256))[i & 63];
    }
  }
  __syncthreads();
  const int x = x0 + 4 * (tid & 63);
  if (x >= a.w) return;
  // the four columns of this lane: weights and table columns (as offsets into the stage)
  float xa[4], xa1[4];
  int o1[4], o2[4];
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int t1 = clahe_cell(x + k, a.inv_tw, &xa[k], &xa1[k]);
    int t2 = t1 + 1 < a.tiles_x - 1 ? t1 + 1 : a.tiles_x - 1;
    int t1c = t1 > 0 ? t1 : 0;
    // (columns past the image's last one belong to no pixel: kept inside the stage, their bytes are not stored as pixels)
    t1c = t1c > c1 ? c1 : t1c;
    t2 = t2 > c1 ? c1 : t2;
    o1[k] = (t1c - c0) * 256;
    o2[k] = (t2 - c0) * 256;
  }
  for (int rr = tid >> 6; rr < CLAHE_BLEND_ROWS; rr += CLAHE_NT / 64) {
    const int y = y0 + rr;
    if (y >= a.h) break;
    float ya, ya1;
    const int q = clahe_cell(y, a.inv_th, &ya, &ya1);
    const int qb = q + 1 < a.tiles_y - 1 ? q + 1 : a.tiles_y - 1;
    const int qa = q > 0 ? q : 0;
    const uint8_t *L1 = s_lut + (size_t)(qa - q0) * ncols * 256, *L2 = s_lut + (size_t)(qb - q0) * ncols * 256;
    const uint8_t *sp = I.src + (size_t)y * a.sstride + x;
    uint32_t in = 0;
    if (x + 3 < a.w) {
      __builtin_memcpy(&in, sp, 4);  // (any byte address: the caller's image makes no alignment promise)
    } else {
      for (int k = 0; x + k < a.w; ++k) in |= (uint32_t)sp[k] << (8 * k);
    }
    uint32_t out = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int pv = (int)((in >> (8 * k)) & 255u);
      const float top = CLAHE_FADD(CLAHE_FMUL((float)L1[o1[k] + pv], xa1[k]), CLAHE_FMUL((float)L1[o2[k] + pv], xa[k]));
      const float bot = CLAHE_FADD(CLAHE_FMUL((float)L2[o1[k] + pv], xa1[k]), CLAHE_FMUL((float)L2[o2[k] + pv], xa[k]));
      const float res = CLAHE_FADD(CLAHE_FMUL(top, ya1), CLAHE_FMUL(bot, ya));
      if (x + k < a.w) out |= (uint32_t)clahe_sat_u8(res) << (8 * k);
    }
    *(uint32_t *)(I.dst + (size_t)y * a.dstride + x) = out;
  }
}

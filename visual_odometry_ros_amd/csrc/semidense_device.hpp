// semidense_device.hpp — the kernels of the semi-dense stereo depth (include/vo_hip.h, "Semi-dense stereo", has the definition;
// DESIGN.md §17). Included by semidense.hip and, through tests/emu/hip_emu.h, by the CPU harness (tests/emu/emu_semidense.cpp)
// that runs this text against the numpy restatement (tests/semidense_restatement.py).
//
//   semidense_kernel   grid (ceil(W / SD_SEG), H), SD_NT threads. A workgroup owns SD_SEG columns of one row. It stages the
//                      2 my + 1 rows (my = max(hh, 1)) of the left segment with a halo of hw, and of the right segment with
//                      hw + d_max more columns to the left, as bytes in LDS; columns outside the image read 0 (no valid
//                      (candidate, disparity) pair touches them). Column sums over the window's rows, then row sums over its
//                      columns, leave S_l, S_ll per left column and S_r, S_rr per right column in LDS: integers, shared by every
//                      candidate of the row. Wavefront 0 evaluates the selection test for its 64 columns, writes the planes of
//                      the pixels that are no candidates and leaves the ballot in LDS. The wavefronts then take the candidates
//                      in turn (the k-th set bit goes to wavefront k % SD_WAVES), lanes as disparities in chunks of 64: a lane
//                      forms S_lr from packed 4-byte dot products — the left words, aligned and with the bytes beyond the window
//                      zeroed, are laid down once per candidate; the right words come from two aligned reads and a byte shift
//                      (vo_bytes4's rule: no misaligned LDS read) — and its score. Arg-max with the smallest-d tie rule: wave
//                      maximum, then the first lane that holds it; a later chunk replaces the best only where strictly larger.
//                      The extent of s > thres_peak: first and last set bit of the chunk's ballot. Scores also go to a per-wave
//                      LDS array, from which lane 0 takes the neighbours of the best. Plain vector stores only, no atomics: where
//                      the caller asks for the number of accepted pixels, every workgroup stores its own count and the host adds
//                      them (one counter for the whole image, 60 000 atomic adds to one word, quadrupled the kernel's time).
//   semidense_points_kernel   one thread per accepted pixel of the compacted index list.
//
// What the includer provides: SD_DYN_LDS(name) (the dynamic LDS block as uint8_t *name, 16-byte aligned), SD_BALLOT(p) (64-bit
// ballot of the caller's wavefront), SD_WAVE_MAX_F32(v) (the maximum over the wavefront in every lane), SD_WAVE_SYNC() (LDS
// writes of the wavefront's lanes are visible to its other lanes), SD_UDOT4(a, b, c) (c + the sum of the four byte products),
// VO_ALIGNBYTE (vo_layout.hpp). Every thread of a wavefront reaches the first four together.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "vo_layout.hpp"

#if defined(__HIP_DEVICE_COMPILE__)
#define SD_FMUL(a, b) __fmul_rn((a), (b))
#define SD_FADD(a, b) __fadd_rn((a), (b))
#define SD_FSUB(a, b) __fsub_rn((a), (b))
#else  // host text (the emulation harness): compiled with -ffp-contract=off
#define SD_FMUL(a, b) ((a) * (b))
#define SD_FADD(a, b) ((a) + (b))
#define SD_FSUB(a, b) ((a) - (b))
#endif

#define SD_SEG 64    // columns per workgroup: one lane of wavefront 0 each
#define SD_WAVES 4   // wavefronts per workgroup
#define SD_NT (64 * SD_WAVES)
#define SD_MAX_HW 15
#define SD_MAX_HH 3
#define SD_MAX_D 1023

struct SdArgs {
  const uint8_t *L, *R;  // level-0 pixel (0, 0) of the left / right image, W x H each
  int strideL, strideR;  // bytes per row
  int W, H;
  const uint8_t *mask;   // the left image's ignore mask (0 = ignore), null: none
  int mask_stride;
  int hw, hh, d_min, d_max, g_min2, peak_px, edge_px;
  float thres_best, thres_peak, eps_edge, eps_epi, bf;
  float *disp, *score, *sigma;  // W x H planes, tightly packed; any may be null
  uint8_t *status;
  int *wg_accepted;      // [gridDim.y][gridDim.x]: the workgroup's number of accepted pixels; null: not counted
  // the plan (sd_plan)
  int my, rows, G, n, pitchL, pitchR, ncR, Dpad;
  unsigned last_mask;    // the bytes of a left row's last word that lie inside the window
  int oL, oR, oVL, oVR, oHL, oHR, oW, oSc, lds_bytes;  // byte offsets of the LDS arrays
};

static inline int sd_round(int v, int m) { return (v + m - 1) / m * m; }

// parameters -> the launch's numbers (host code, shared by the launcher and the harness)
static inline void sd_plan(SdArgs *a) {
  const int hw = a->hw, hh = a->hh;
  a->my = hh > 1 ? hh : 1;
  a->rows = 2 * a->my + 1;
  const int width = 2 * hw + 1;
  a->G = (width + 3) / 4;
  a->n = width * (2 * hh + 1);
  const int rem = width - 4 * (a->G - 1);  // 1 .. 4 bytes of the last word
  a->last_mask = rem >= 4 ? 0xFFFFFFFFu : ((1u << (8 * rem)) - 1u);
  const int ncL = SD_SEG + 2 * hw;
  a->ncR = ncL + a->d_max;
  a->pitchL = sd_round(ncL + 8, 4);  // (a lane's last word starts up to 3 bytes before the window's end and is read with the next one)
  a->pitchR = sd_round(a->ncR + 8, 4);
  a->Dpad = sd_round(a->d_max - a->d_min + 1, 64);
  int o = 0;
  a->oL = o, o += a->rows * a->pitchL;
  a->oR = o, o += a->rows * a->pitchR;
  o = sd_round(o, 16);
  a->oVL = o, o += 2 * 4 * ncL;
  a->oVR = o, o += 2 * 4 * a->ncR;
  a->oHL = o, o += 2 * 4 * SD_SEG;
  a->oHR = o, o += 2 * 4 * (SD_SEG + a->d_max);
  a->oW = o, o += 4 * SD_WAVES * (2 * SD_MAX_HH + 1) * 8;
  a->oSc = o, o += 4 * SD_WAVES * a->Dpad;
  a->lds_bytes = o + 32;  // (+ the ballot and the wavefronts' counts)
}

__global__ __launch_bounds__(SD_NT) void semidense_kernel(SdArgs a) {
  SD_DYN_LDS(lds);
  const int tid = (int)threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int x0 = (int)blockIdx.x * SD_SEG, y = (int)blockIdx.y;
  const int hw = a.hw, hh = a.hh, my = a.my, mx = hw > 1 ? hw : 1;
  const size_t px = (size_t)y * (size_t)a.W + (size_t)(x0 + lane);
  const bool row_in = y >= my && y <= a.H - 1 - my;
  if (!row_in) {  // (the whole workgroup: no candidate in this row)
    if (wave == 0 && x0 + lane < a.W) {
      if (a.disp) a.disp[px] = 0.0f;
      if (a.score) a.score[px] = 0.0f;
      if (a.sigma) a.sigma[px] = 0.0f;
      if (a.status) a.status[px] = 0;
    }
    if (tid == 0 && a.wg_accepted) a.wg_accepted[blockIdx.y * gridDim.x + blockIdx.x] = 0;
    return;
  }
  uint8_t *sL = lds + a.oL, *sR = lds + a.oR;
  int *vL = (int *)(lds + a.oVL), *vR = (int *)(lds + a.oVR), *hL = (int *)(lds + a.oHL), *hR = (int *)(lds + a.oHR);
  uint32_t *sW = (uint32_t *)(lds + a.oW) + wave * (2 * SD_MAX_HH + 1) * 8;
  float *sc = (float *)(lds + a.oSc) + wave * a.Dpad;
  unsigned long long *s_bal = (unsigned long long *)(lds + a.lds_bytes - 32);
  int *s_cnt = (int *)(lds + a.lds_bytes - 16);
  int n_acc = 0;  // (lane 0 of each wavefront counts)
  const int ncL = SD_SEG + 2 * hw, ncR = a.ncR;
  // ---- the rows y - my .. y + my: left columns x0 - hw .., right columns x0 - hw - d_max ..; 0 outside the image and in the pad
  for (int r = 0; r < a.rows; ++r) {
    const uint8_t *gl = a.L + (size_t)(y - my + r) * (size_t)a.strideL, *gr = a.R + (size_t)(y - my + r) * (size_t)a.strideR;
    for (int i = tid; i < a.pitchL; i += SD_NT) {
      const int x = x0 - hw + i;
      sL[r * a.pitchL + i] = (i < ncL && x >= 0 && x < a.W) ? gl[x] : (uint8_t)0;
    }
    for (int i = tid; i < a.pitchR; i += SD_NT) {
      const int x = x0 - hw - a.d_max + i;
      sR[r * a.pitchR + i] = (i < ncR && x >= 0 && x < a.W) ? gr[x] : (uint8_t)0;
    }
  }
  __syncthreads();
  // ---- column sums over the window's rows my - hh .. my + hh
  for (int i = tid; i < ncL + ncR; i += SD_NT) {
    const bool left = i < ncL;
    const uint8_t *p = left ? sL + i : sR + (i - ncL);
    const int pitch = left ? a.pitchL : a.pitchR;
    int s1 = 0, s2 = 0;
    for (int r = my - hh; r <= my + hh; ++r) {
      const int v = p[r * pitch];
      s1 += v;
      s2 += v * v;
    }
    int *o = left ? vL + 2 * i : vR + 2 * (i - ncL);
    o[0] = s1;
    o[1] = s2;
  }
  __syncthreads();
  // ---- row sums over the window's columns: hL[2 j] of left column x0 + j, hR[2 j] of right column x0 - d_max + j
  for (int i = tid; i < SD_SEG + SD_SEG + a.d_max; i += SD_NT) {
    const bool left = i < SD_SEG;
    const int *p = left ? vL + 2 * i : vR + 2 * (i - SD_SEG);
    int s1 = 0, s2 = 0;
    for (int k = 0; k <= 2 * hw; ++k) {
      s1 += p[2 * k];
      s2 += p[2 * k + 1];
    }
    int *o = left ? hL + 2 * i : hR + 2 * (i - SD_SEG);
    o[0] = s1;
    o[1] = s2;
  }
  // ---- the selection test, one column per lane of wavefront 0
  if (wave == 0) {
    const int x = x0 + lane;
    bool cand = false;
    if (x >= mx && x <= a.W - 1 - mx) {
      const uint8_t *c = sL + my * a.pitchL + hw + lane;
      const int gx = (int)c[1] - (int)c[-1], gy = (int)c[a.pitchL] - (int)c[-a.pitchL];
      const int gx2 = gx * gx, gy2 = gy * gy;
      cand = gx2 + gy2 >= a.g_min2 && 3 * gx2 >= gy2;
      if (cand && a.mask) cand = a.mask[(size_t)y * (size_t)a.mask_stride + (size_t)x] != 0;
    }
    if (!cand && x < a.W) {
      if (a.disp) a.disp[px] = 0.0f;
      if (a.score) a.score[px] = 0.0f;
      if (a.sigma) a.sigma[px] = 0.0f;
      if (a.status) a.status[px] = 0;
    }
    const unsigned long long b = SD_BALLOT(cand);
    if (lane == 0) *s_bal = b;
  }
  __syncthreads();
  unsigned long long todo = *s_bal;
  const int nwords = (2 * hh + 1) * a.G;
  for (int k = 0; todo; ++k) {
    const int j = __builtin_ctzll(todo);  // the candidate's column within the segment
    todo &= todo - 1;
    if (k % SD_WAVES != wave) continue;
    const int x = x0 + j;
    // the left patch as aligned words, bytes beyond the window zeroed
    SD_WAVE_SYNC();  // (the previous candidate's reads of sW and sc are over)
    if (lane < nwords) {
      const int r = lane / a.G, g = lane - r * a.G;
      const uint32_t w = vo_bytes4(sL + (my - hh + r) * a.pitchL, j + 4 * g);
      sW[r * 8 + g] = g == a.G - 1 ? (w & a.last_mask) : w;
    }
    SD_WAVE_SYNC();
    const long long S_l = hL[2 * j], S_ll = hL[2 * j + 1], n = a.n;
    const long long A = n * S_ll - S_l * S_l;
    const int d_last = a.d_max < x - hw ? a.d_max : x - hw;
    const int nd = d_last - a.d_min + 1;
    float best_s = -__builtin_inff();
    int best_d = a.d_min, lo = 0x7FFFFFFF, hi = -1;
    const bool search = nd >= 2 * a.edge_px + 3 && A != 0;
    if (search) {
      for (int base = a.d_min; base <= d_last; base += 64) {
        const int d = base + lane;
        const bool valid = d <= d_last;
        const int dr = valid ? d : d_last;  // (a lane beyond the range reads where the last one does)
        // the right window's first column in the staged row: (x - dr - hw) - (x0 - hw - d_max)
        const int o = j + a.d_max - dr;
        const int sh = o & 3;
        unsigned acc = 0;
        for (int r = 0; r <= 2 * hh; ++r) {
          const uint32_t *rw = (const uint32_t *)(sR + (my - hh + r) * a.pitchR) + (o >> 2);
          const uint32_t *lw = sW + r * 8;
          uint32_t w_lo = rw[0];
          for (int g = 0; g < a.G; ++g) {
            const uint32_t w_hi = rw[g + 1];
            acc = SD_UDOT4(lw[g], VO_ALIGNBYTE(w_hi, w_lo, sh), acc);
            w_lo = w_hi;
          }
        }
        const int jc = j + a.d_max - dr;  // the right window's centre column x - dr as an index of hR
        const long long S_r = hR[2 * jc], S_rr = hR[2 * jc + 1], S_lr = acc;
        const long long B = n * S_rr - S_r * S_r, num = n * S_lr - S_l * S_r;
        float s = -1.0f;
        if (B != 0) s = (float)num / sqrtf(SD_FMUL((float)A, (float)B));
        if (valid) sc[d - a.d_min] = s;
        const float sv = valid ? s : -__builtin_inff();
        const unsigned long long pk = SD_BALLOT(valid && s > a.thres_peak);
        if (pk) {
          const int f = base + __builtin_ctzll(pk), l = base + 63 - __builtin_clzll(pk);
          lo = f < lo ? f : lo;
          hi = l > hi ? l : hi;
        }
        const float m = SD_WAVE_MAX_F32(sv);
        const unsigned long long at = SD_BALLOT(valid && s == m);
        if (m > best_s) {  // (strictly: a tie stays with the smaller disparity of an earlier chunk)
          best_s = m;
          best_d = base + __builtin_ctzll(at);
        }
      }
      SD_WAVE_SYNC();
    }
    if (lane == 0) {
      int st;
      if (!search) st = 5;
      else if (best_s <= a.thres_best) st = 2;
      else if (hi >= 0 && (lo < best_d - a.peak_px || hi > best_d + a.peak_px)) st = 3;
      else if (!(a.d_min + a.edge_px < best_d && best_d < d_last - a.edge_px)) st = 4;
      else st = 1;
      float disp = 0.0f, sig = 0.0f;
      if (st == 1) {
        const float s0 = best_s, sm = sc[best_d - 1 - a.d_min], sp = sc[best_d + 1 - a.d_min];
        const float den = SD_FSUB(SD_FADD(sm, sp), SD_FADD(s0, s0));
        const float off = den != 0.0f ? SD_FMUL(0.5f, SD_FSUB(sm, sp)) / den : 0.0f;
        disp = SD_FADD((float)best_d, off);
        const uint8_t *c = sL + my * a.pitchL + hw + j;
        const int gx = (int)c[1] - (int)c[-1], gy = (int)c[a.pitchL] - (int)c[-a.pitchL];
        const float g = sqrtf((float)(gx * gx + gy * gy));
        const float du = (float)gx / g, dv = (float)gy / g;
        const float e = SD_FMUL(a.eps_epi, dv);
        sig = (sqrtf(SD_FADD(SD_FMUL(a.eps_edge, a.eps_edge), SD_FMUL(e, e))) / fabsf(du)) / a.bf;
        ++n_acc;
      }
      const size_t q = (size_t)y * (size_t)a.W + (size_t)x;
      if (a.disp) a.disp[q] = disp;
      if (a.score) a.score[q] = st == 5 ? 0.0f : best_s;
      if (a.sigma) a.sigma[q] = sig;
      if (a.status) a.status[q] = (uint8_t)st;
    }
  }
  if (a.wg_accepted) {
    if (lane == 0) s_cnt[wave] = n_acc;
    __syncthreads();
    if (tid == 0) {
      int n = 0;
      for (int w = 0; w < SD_WAVES; ++w) n += s_cnt[w];
      a.wg_accepted[blockIdx.y * gridDim.x + blockIdx.x] = n;
    }
  }
}

// ---- the points list -------------------------------------------------------------------------------------------------------
// key[i] = status[i] == 1 for the library's stable compaction (compact_kernel takes byte masks)
__global__ void semidense_key_kernel(const uint8_t *status, uint8_t *key, int n) {
  const int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
  if (i < n) key[i] = status[i] == 1;
}

struct SdPointArgs {
  const int32_t *idx;   // the accepted pixels' indices y * W + x, raster order
  const int *n;         // their number (device)
  int cap, W;
  const float *disp, *sigma;
  float fx, fy, cx, cy, bf;
  int has_T;
  float T[12];
  float *xyz, *sig;
  uint16_t *pixel;
};
__global__ void semidense_points_kernel(SdPointArgs a) {
  const int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
  const int n = *a.n < a.cap ? *a.n : a.cap;
  if (i >= n) return;
  const int p = a.idx[i], y = p / a.W, x = p - y * a.W;
  const float z = a.bf / a.disp[p];
  float X[3] = {SD_FMUL(SD_FSUB((float)x, a.cx) / a.fx, z), SD_FMUL(SD_FSUB((float)y, a.cy) / a.fy, z), z};
  if (a.has_T) {
    float Y[3];
    for (int r = 0; r < 3; ++r)
      Y[r] = SD_FADD(SD_FADD(SD_FMUL(a.T[4 * r], X[0]), SD_FADD(SD_FMUL(a.T[4 * r + 1], X[1]), SD_FMUL(a.T[4 * r + 2], X[2]))), a.T[4 * r + 3]);
    X[0] = Y[0], X[1] = Y[1], X[2] = Y[2];
  }
  a.xyz[3 * i] = X[0];
  a.xyz[3 * i + 1] = X[1];
  a.xyz[3 * i + 2] = X[2];
  if (a.sig) a.sig[i] = a.sigma[p];
  if (a.pixel) {
    a.pixel[2 * i] = (uint16_t)x;
    a.pixel[2 * i + 1] = (uint16_t)y;
  }
}

// semidense_temporal_device.hpp — the kernels of the temporal semi-dense search and its fusion (include/vo_hip.h, "Semi-dense
// temporal", has the definition). Included by semidense_temporal.hip and, through tests/emu/hip_emu.h, by the CPU
// harness (tests/emu/emu_semidense_temporal.cpp) that runs this text against the numpy restatement
// (tests/semidense_temporal_restatement.py).
//
//   semidense_temporal_kernel   grid (ceil(W / SDT_SEG), H), SDT_NT threads. A workgroup owns SDT_SEG columns of one key row.
//                      Lane c of wavefront 0 owns column c from the first instruction to the last: it evaluates the selection
//                      tests and the geometry of its pixel (the search range, p(rho_lo), l_c, the signed key direction, the
//                      number of positions), writes tstatus where the pixel is decided without a search and leaves what the
//                      other wavefronts need in LDS. Thread 0 cuts the columns into batches of at most SDT_NB candidates and
//                      SDT_SC positions. Per batch the 256 threads (a) lay the candidates' key patches down in LDS as 12-bit
//                      integers, taps as threads, (b) score the batch's positions, one (candidate, position) pair per thread
//                      wherever the candidate's range is short or long — a pixel with a prior has about ten positions, one
//                      without up to max_search, and neither leaves lanes idle — with the key taps read from LDS (neighbouring
//                      lanes mostly share a candidate: a broadcast) and the current taps from global memory (L2), and (c) the
//                      owner lanes walk their candidates' scores in LDS, decide, fuse and store. No cross-lane operation, no
//                      atomics, plain vector stores: a pixel's four map entries are written by its owner lane only.
//                      Every global load of a tap goes through sdt_sample, which clamps the cell to [0, W-2] x [0, H-2] before
//                      it forms the address; a position whose tap fails the integer inside test is scored "outside" and its
//                      (clamped) sample values are discarded.
//   semidense_map_seed_kernel, semidense_map_key_kernel   one thread per pixel.
//
// The includer provides nothing but __global__, __shared__, __syncthreads and the built-in indices.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "semidense_map_fuse.hpp"  // sdm_seed_entry: a static result's map entry, shared with the map merge
#include "semidense_sample.hpp"    // SDT_MUL / SDT_ADD / SDT_SUB, sdt_q, sdt_in, sdt_sample

#define SDT_SEG 64           // columns per workgroup: one lane of wavefront 0 each
#define SDT_NT 256
#define SDT_NB 16            // candidates per batch
#define SDT_SC 2048          // positions per batch (>= SDT_MAX_SEARCH)
#define SDT_KP 224           // a candidate's key taps in LDS (>= 31 x 7)
#define SDT_MAX_HW 15
#define SDT_MAX_HH 3
#define SDT_MAX_SEARCH 512
#define SDT_EPS_DK2 1e-6f    // |d_k|^2 below this: the pixel sits on the epipole
#define SDT_FRONT 0.1f       // a2 + rho t2 (the depth in the current camera over the depth in the key camera) must exceed this
#define SDT_OUTSIDE (-3.0f)  // the score of a position with a tap outside the image (real scores lie in [-1, 1] but for rounding)

struct SdtArgs {
  const uint8_t *Lk, *Lc;  // level-0 pixel (0, 0) of the key / current left image, W x H each
  int strideK, strideC;    // bytes per row
  int W, H;
  const uint8_t *mask;     // the key pixels' ignore mask (0 = ignore), null: none
  int mask_stride;
  int hw, hh, g_min2, peak_px, edge_px, max_search;
  float thres_best, thres_peak, eps_edge, eps_epi, eps_scale, r_min, r_max, j_min;  // r_min = 1 / z_max, r_max = 1 / z_min
  float fx, fy, cx, cy;
  float R[9], t[3], C[3];  // X_c = R X_k + t; C = -R^T t
  float *invd, *sigma;     // the map, W x H planes, tightly packed
  uint8_t *n_obs, *tstatus;
  float *score;            // may be null
};

// T_ck (row-major 4 x 4) -> R, t, C; C[i] = -((R[0][i] t0 + R[1][i] t1) + R[2][i] t2)
static inline void sdt_pose(SdtArgs *a, const float T[16]) {
  for (int r = 0; r < 3; ++r) {
    for (int c = 0; c < 3; ++c) a->R[3 * r + c] = T[4 * r + c];
    a->t[r] = T[4 * r + 3];
  }
  for (int i = 0; i < 3; ++i) a->C[i] = -((a->R[i] * a->t[0] + a->R[3 + i] * a->t[1]) + a->R[6 + i] * a->t[2]);  // (host code: -ffp-contract=off)
}

__global__ __launch_bounds__(SDT_NT) void semidense_temporal_kernel(SdtArgs a) {
  __shared__ float s_geo[6][SDT_SEG];  // p(rho_lo).x, .y, l_c.x, .y, the signed key direction .x, .y
  __shared__ int s_npos[SDT_SEG];      // positions of the column's search, 0: none
  __shared__ int s_bcol[SDT_SEG + 2];  // batch b: columns s_bcol[b] .. s_bcol[b + 1] - 1
  __shared__ int s_nb;
  __shared__ int s_slot_col[SDT_NB], s_slot_off[SDT_NB + 1], s_ns;
  __shared__ uint16_t s_key[SDT_NB * SDT_KP];
  __shared__ float s_sc[SDT_SC];
  const int tid = (int)threadIdx.x;
  const int x0 = (int)blockIdx.x * SDT_SEG, y = (int)blockIdx.y, x = x0 + tid;
  const int W = a.W, H = a.H, hw = a.hw, hh = a.hh, width = 2 * hw + 1, n = width * (2 * hh + 1);
  const int j0 = -(a.edge_px + 1);
  const size_t px = (size_t)y * (size_t)W + (size_t)x;
  // ---- the owner lanes: selection and geometry --------------------------------------------------------------------------------
  const bool owner = tid < SDT_SEG && x < W;
  int st = 0, npos = 0, jp = -1, gx = 0, gy = 0;
  float P0x = 0.f, P0y = 0.f, lx = 0.f, ly = 0.f, J = 1.f, a0 = 0.f, a1 = 0.f, a2 = 0.f, dot = 0.f, dk2 = 1.f, invd = 0.f, sig = 0.f;
  if (tid < SDT_SEG) s_npos[tid] = 0;
  if (owner && y >= 1 && y <= H - 2 && x >= 1 && x <= W - 2) {
    const uint8_t *c = a.Lk + (size_t)y * (size_t)a.strideK + (size_t)x;
    gx = (int)c[1] - (int)c[-1];
    gy = (int)c[a.strideK] - (int)c[-a.strideK];
    bool cand = gx * gx + gy * gy >= a.g_min2;
    if (cand && a.mask) cand = a.mask[(size_t)y * (size_t)a.mask_stride + (size_t)x] != 0;
    if (cand) {
      const float xc = SDT_SUB((float)x, a.cx), yc = SDT_SUB((float)y, a.cy);
      const float u = xc / a.fx, v = yc / a.fy;
      a0 = SDT_ADD(SDT_ADD(SDT_MUL(a.R[0], u), SDT_MUL(a.R[1], v)), a.R[2]);
      a1 = SDT_ADD(SDT_ADD(SDT_MUL(a.R[3], u), SDT_MUL(a.R[4], v)), a.R[5]);
      a2 = SDT_ADD(SDT_ADD(SDT_MUL(a.R[6], u), SDT_MUL(a.R[7], v)), a.R[8]);
      const float dkx = SDT_SUB(SDT_MUL(a.fx, a.C[0]), SDT_MUL(xc, a.C[2])), dky = SDT_SUB(SDT_MUL(a.fy, a.C[1]), SDT_MUL(yc, a.C[2]));
      dk2 = SDT_ADD(SDT_MUL(dkx, dkx), SDT_MUL(dky, dky));
      if (dk2 < SDT_EPS_DK2) {
        st = 7;
      } else {
        dot = SDT_ADD(SDT_MUL((float)gx, dkx), SDT_MUL((float)gy, dky));
        const float g2 = (float)(gx * gx + gy * gy);
        bool ok = !(SDT_MUL(SDT_MUL(4.0f, dot), dot) < SDT_MUL(g2, dk2));  // within 60 degrees of the key epipolar line
        const float dkl = sqrtf(dk2), ux = dkx / dkl, uy = dky / dkl;
        if (ok) {  // the key patch (the sign of the direction does not change the set of taps)
          for (int vv = -hh; vv <= hh && ok; ++vv)
            for (int k = -hw; k <= hw; ++k) {
              const float tx = SDT_ADD(SDT_ADD((float)x, SDT_MUL((float)k, ux)), SDT_MUL((float)vv, -uy));
              const float ty = SDT_ADD(SDT_ADD((float)y, SDT_MUL((float)k, uy)), SDT_MUL((float)vv, ux));
              ok = ok && sdt_in(sdt_q(tx), sdt_q(ty), W, H);
            }
        }
        if (ok) {
          invd = a.invd[px];
          sig = a.sigma[px];
          float lo = a.r_min, hi = a.r_max;
          if (sig > 0.0f) {
            const float two = SDT_MUL(2.0f, sig);
            lo = SDT_SUB(invd, two);
            hi = SDT_ADD(invd, two);
            lo = lo < a.r_min ? a.r_min : lo;
            hi = hi > a.r_max ? a.r_max : hi;
          }
          const float Dlo = SDT_ADD(a2, SDT_MUL(lo, a.t[2])), Dhi = SDT_ADD(a2, SDT_MUL(hi, a.t[2]));
          if (!(lo < hi) || !(Dlo > SDT_FRONT && Dhi > SDT_FRONT)) {
            st = 8;
          } else {
            const float N0 = SDT_ADD(a0, SDT_MUL(lo, a.t[0])), N1 = SDT_ADD(a1, SDT_MUL(lo, a.t[1]));
            P0x = SDT_ADD(SDT_MUL(a.fx, N0 / Dlo), a.cx);
            P0y = SDT_ADD(SDT_MUL(a.fy, N1 / Dlo), a.cy);
            const float P1x = SDT_ADD(SDT_MUL(a.fx, SDT_ADD(a0, SDT_MUL(hi, a.t[0])) / Dhi), a.cx);
            const float P1y = SDT_ADD(SDT_MUL(a.fy, SDT_ADD(a1, SDT_MUL(hi, a.t[1])) / Dhi), a.cy);
            const float ex = SDT_SUB(P1x, P0x), ey = SDT_SUB(P1y, P0y);
            const float len = sqrtf(SDT_ADD(SDT_MUL(ex, ex), SDT_MUL(ey, ey)));
            J = len / SDT_SUB(hi, lo);
            if (!(J >= a.j_min)) {
              st = 7;
            } else {
              lx = ex / len;
              ly = ey / len;
              const float tl = floorf(SDT_ADD(len, 0.5f));
              if (!(tl <= (float)a.max_search) || (int)tl + 2 * a.edge_px + 3 > a.max_search) {
                st = 6;
              } else {
                npos = (int)tl + 2 * a.edge_px + 3;
                // the key direction that corresponds to l_c: the derivative of p(rho_lo) along the key direction, times Dlo^2
                const float bx = ux / a.fx, by = uy / a.fy;
                const float b0 = SDT_ADD(SDT_MUL(a.R[0], bx), SDT_MUL(a.R[1], by)), b1 = SDT_ADD(SDT_MUL(a.R[3], bx), SDT_MUL(a.R[4], by));
                const float b2 = SDT_ADD(SDT_MUL(a.R[6], bx), SDT_MUL(a.R[7], by));
                const float wx = SDT_MUL(a.fx, SDT_SUB(SDT_MUL(b0, Dlo), SDT_MUL(N0, b2))), wy = SDT_MUL(a.fy, SDT_SUB(SDT_MUL(b1, Dlo), SDT_MUL(N1, b2)));
                const bool pos = SDT_ADD(SDT_MUL(lx, wx), SDT_MUL(ly, wy)) >= 0.0f;
                s_geo[0][tid] = P0x, s_geo[1][tid] = P0y, s_geo[2][tid] = lx, s_geo[3][tid] = ly;
                s_geo[4][tid] = pos ? ux : -ux, s_geo[5][tid] = pos ? uy : -uy;
                s_npos[tid] = npos;
                if (sig > 0.0f) {  // the prior's position
                  const float Dp = SDT_ADD(a2, SDT_MUL(invd, a.t[2]));
                  if (Dp > SDT_FRONT) {
                    const float qx = SDT_ADD(SDT_MUL(a.fx, SDT_ADD(a0, SDT_MUL(invd, a.t[0])) / Dp), a.cx);
                    const float qy = SDT_ADD(SDT_MUL(a.fy, SDT_ADD(a1, SDT_MUL(invd, a.t[1])) / Dp), a.cy);
                    const float tj = floorf(SDT_ADD(SDT_ADD(SDT_MUL(SDT_SUB(qx, P0x), lx), SDT_MUL(SDT_SUB(qy, P0y), ly)), 0.5f));
                    if (tj >= (float)j0 && tj <= (float)(j0 + npos - 1)) jp = (int)tj - j0;
                  }
                }
              }
            }
          }
        }
      }
    }
  }
  if (owner && npos == 0) {  // decided without a search
    a.tstatus[px] = (uint8_t)st;
    if (a.score) a.score[px] = 0.0f;
  }
  __syncthreads();
  // ---- batches: at most SDT_NB candidates and SDT_SC positions each ------------------------------------------------------------
  if (tid == 0) {
    int nb = 0, cnt = 0, tot = 0, any = 0;
    s_bcol[0] = 0;
    for (int c = 0; c < SDT_SEG; ++c) {
      const int m = s_npos[c];
      if (m <= 0) continue;
      if (cnt == SDT_NB || tot + m > SDT_SC) s_bcol[++nb] = c, cnt = 0, tot = 0;
      ++cnt, tot += m, any = 1;
    }
    s_bcol[++nb] = SDT_SEG;
    s_nb = any ? nb : 0;
  }
  __syncthreads();
  const int nb = s_nb;
  for (int b = 0; b < nb; ++b) {
    const int c0 = s_bcol[b], c1 = s_bcol[b + 1];
    if (tid == 0) {
      int ns = 0, off = 0;
      for (int c = c0; c < c1; ++c)
        if (s_npos[c] > 0) s_slot_col[ns] = c, s_slot_off[ns] = off, off += s_npos[c], ++ns;
      s_slot_off[ns] = off;
      s_ns = ns;
    }
    __syncthreads();
    const int ns = s_ns, total = s_slot_off[ns];
    // (a) the key patches: 12-bit samples at (x, y) + k d + v n, n the left normal (-d.y, d.x)
    for (int i = tid; i < ns * n; i += SDT_NT) {
      const int s = i / n, t = i - s * n, c = s_slot_col[s];
      const int vv = t / width - hh, k = t - (t / width) * width - hw;
      const float dx = s_geo[4][c], dy = s_geo[5][c];
      const float tx = SDT_ADD(SDT_ADD((float)(x0 + c), SDT_MUL((float)k, dx)), SDT_MUL((float)vv, -dy));
      const float ty = SDT_ADD(SDT_ADD((float)y, SDT_MUL((float)k, dy)), SDT_MUL((float)vv, dx));
      s_key[s * SDT_KP + t] = (uint16_t)sdt_sample(a.Lk, a.strideK, W, H, sdt_q(tx), sdt_q(ty));
    }
    __syncthreads();
    // (b) the scores: one (candidate, position) pair per thread
    for (int i = tid; i < total; i += SDT_NT) {
      int s = 0;
      while (s + 1 < ns && s_slot_off[s + 1] <= i) ++s;
      const int c = s_slot_col[s], j = j0 + (i - s_slot_off[s]);
      const float qx = s_geo[0][c], qy = s_geo[1][c], ex = s_geo[2][c], ey = s_geo[3][c];
      const float pjx = SDT_ADD(qx, SDT_MUL((float)j, ex)), pjy = SDT_ADD(qy, SDT_MUL((float)j, ey));
      const uint16_t *kp = s_key + s * SDT_KP;
      unsigned Sk = 0, Skk = 0, Sc = 0, Scc = 0, Skc = 0;
      bool in = true;
      int t = 0;
      for (int vv = -hh; vv <= hh; ++vv) {
        const float fvx = SDT_MUL((float)vv, -ey), fvy = SDT_MUL((float)vv, ex);
        for (int k = -hw; k <= hw; ++k, ++t) {
          const int X = sdt_q(SDT_ADD(SDT_ADD(pjx, SDT_MUL((float)k, ex)), fvx)), Y = sdt_q(SDT_ADD(SDT_ADD(pjy, SDT_MUL((float)k, ey)), fvy));
          in = in && sdt_in(X, Y, W, H);
          const unsigned cv = (unsigned)sdt_sample(a.Lc, a.strideC, W, H, X, Y), kv = kp[t];
          Sk += kv, Skk += kv * kv, Sc += cv, Scc += cv * cv, Skc += kv * cv;
        }
      }
      float sc = SDT_OUTSIDE;
      if (in) {
        const long long nn = n;
        const long long A = nn * (long long)Skk - (long long)Sk * (long long)Sk, B = nn * (long long)Scc - (long long)Sc * (long long)Sc;
        const long long num = nn * (long long)Skc - (long long)Sk * (long long)Sc;
        sc = (A != 0 && B != 0) ? (float)num / sqrtf(SDT_MUL((float)A, (float)B)) : -1.0f;
      }
      s_sc[i] = sc;
    }
    __syncthreads();
    // (c) the owner lanes decide
    if (owner && npos > 0 && tid >= c0 && tid < c1) {
      int s = 0;
      while (s_slot_col[s] != tid) ++s;
      const float *sc = s_sc + s_slot_off[s];
      const uint16_t *kp = s_key + s * SDT_KP;
      unsigned Sk = 0, Skk = 0;
      for (int t = 0; t < n; ++t) {
        const unsigned kv = kp[t];
        Sk += kv, Skk += kv * kv;
      }
      const long long A = (long long)n * (long long)Skk - (long long)Sk * (long long)Sk;
      // the searched run: the inside positions around the prior's, or else the first run
      int r0 = -1, r1 = -1;
      if (jp >= 0 && sc[jp] > -2.5f) {
        r0 = r1 = jp;
      } else {
        for (int i = 0; i < npos; ++i)
          if (sc[i] > -2.5f) {
            r0 = r1 = i;
            break;
          }
      }
      if (r0 >= 0) {
        while (r0 > 0 && sc[r0 - 1] > -2.5f) --r0;
        while (r1 < npos - 1 && sc[r1 + 1] > -2.5f) ++r1;
      }
      float best_s = 0.0f, rho = 0.0f, sg_new = 0.0f;
      int have_best = 0;
      if (r0 < 0 || r1 - r0 + 1 < 2 * a.edge_px + 3 || A == 0) {
        st = 5;
      } else {
        int best = r0, lo = 0x7FFFFFFF, hi = -1;
        best_s = sc[r0];
        for (int i = r0; i <= r1; ++i) {
          const float v = sc[i];
          if (v > best_s) best_s = v, best = i;  // (strictly: a tie stays with the smaller j)
          if (v > a.thres_peak) {
            lo = i < lo ? i : lo;
            hi = i;
          }
        }
        have_best = 1;
        if (best_s <= a.thres_best) st = 2;
        else if (hi >= 0 && (lo < best - a.peak_px || hi > best + a.peak_px)) st = 3;
        else if (!(r0 + a.edge_px < best && best < r1 - a.edge_px)) st = 4;
        else {
          const float sm = sc[best - 1], sp = sc[best + 1];
          const float den = SDT_SUB(SDT_ADD(sm, sp), SDT_ADD(best_s, best_s));
          const float off = den != 0.0f ? SDT_MUL(0.5f, SDT_SUB(sm, sp)) / den : 0.0f;
          const float js = SDT_ADD((float)(j0 + best), off);
          if (fabsf(lx) >= fabsf(ly)) {
            const float uu = SDT_SUB(SDT_ADD(P0x, SDT_MUL(js, lx)), a.cx) / a.fx;
            rho = SDT_SUB(a0, SDT_MUL(uu, a2)) / SDT_SUB(SDT_MUL(uu, a.t[2]), a.t[0]);
          } else {
            const float uu = SDT_SUB(SDT_ADD(P0y, SDT_MUL(js, ly)), a.cy) / a.fy;
            rho = SDT_SUB(a1, SDT_MUL(uu, a2)) / SDT_SUB(SDT_MUL(uu, a.t[2]), a.t[1]);
          }
          const float Ds = SDT_ADD(a2, SDT_MUL(rho, a.t[2]));
          if (!(rho >= a.r_min && rho <= a.r_max) || !(Ds > SDT_FRONT)) {
            st = 8;
          } else {
            st = 1;
            const float g = sqrtf((float)(gx * gx + gy * gy));
            const float cs = dot / SDT_MUL(g, sqrtf(dk2));
            float sn2 = SDT_SUB(1.0f, SDT_MUL(cs, cs));
            sn2 = sn2 < 0.0f ? 0.0f : sn2;
            const float e2 = SDT_MUL(SDT_MUL(a.eps_epi, a.eps_epi), sn2);
            const float str = SDT_MUL(SDT_MUL(a.eps_scale, (float)hw), fabsf(SDT_SUB(1.0f, 1.0f / Ds)));  // the patch's unmodelled stretch
            sg_new = (sqrtf(SDT_ADD(SDT_ADD(SDT_MUL(a.eps_edge, a.eps_edge), e2), SDT_MUL(str, str))) / fabsf(cs)) / J;
          }
        }
      }
      if (st == 1) {  // fusion
        if (sig > 0.0f) {
          const float s2 = SDT_MUL(sig, sig), m2 = SDT_MUL(sg_new, sg_new), sum = SDT_ADD(s2, m2);
          a.invd[px] = SDT_ADD(SDT_MUL(invd, m2), SDT_MUL(rho, s2)) / sum;
          a.sigma[px] = sqrtf(SDT_MUL(s2, m2) / sum);
          const int no = a.n_obs[px];
          a.n_obs[px] = (uint8_t)(no < 255 ? no + 1 : 255);
        } else {
          a.invd[px] = rho;
          a.sigma[px] = sg_new;
          a.n_obs[px] = 1;
        }
      }
      a.tstatus[px] = (uint8_t)st;
      if (a.score) a.score[px] = have_best ? best_s : 0.0f;
    }
    __syncthreads();
  }
}

// ---- the map from a static result; the points list's key -------------------------------------------------------------------------
__global__ void semidense_map_seed_kernel(const float *disp, const float *sigma_invd, const uint8_t *status, float bf, float *invd, float *sigma,
                                          uint8_t *n_obs, uint8_t *tstatus, int n) {
  const int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
  if (i >= n) return;
  float r, sg;
  int no;
  sdm_seed_entry(status[i], disp[i], sigma_invd[i], bf, &r, &sg, &no);
  invd[i] = r;
  sigma[i] = sg;
  n_obs[i] = (uint8_t)no;
  tstatus[i] = 0;
}
__global__ void semidense_map_key_kernel(const uint8_t *n_obs, uint8_t *key, int min_obs, int n) {
  const int i = (int)blockIdx.x * (int)blockDim.x + (int)threadIdx.x;
  if (i < n) key[i] = (int)n_obs[i] >= min_obs;
}

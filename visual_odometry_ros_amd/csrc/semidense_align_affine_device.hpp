// semidense_align_affine_device.hpp — the kernel of the alignment with affine brightness (include/vo_hip.h, "Semi-dense alignment with
// affine brightness", has the definition). Included by semidense_align.hip behind semidense_align_device.hpp and,
// through tests/emu/hip_emu.h, by the CPU harness (tests/emu/emu_semidense_align_affine.cpp) that runs this text against the numpy
// restatement (tests/semidense_align_affine_restatement.py).
//
//   semidense_affine_kernel   the launch shape of semidense_align_kernel: grid ceil(W H / SDA_BLOCK), SDA_NT threads, one launch per
//                      iteration, (a) the ballot-packed LDS list, (b) one listed pixel per thread and turn, (c) the block's exact
//                      sums, (d) the ticket, the last workgroup adding the rows in block order, thread 0 solving and updating the
//                      state block. What differs: the residual is taken against the key grey level mapped by the state's G and O;
//                      the record keeps eight words per listed pixel all the same, the key's grey level (which is q_6 / 16) riding in
//                      bits 12..19 of the weight word; 47 sums, formed by 64 columns x 4 parts; a staged row holds 48 doubles, so
//                      SDAA_STAGE = 85 rows fill the records' 32 KB; the solve is 8 x 8 and the update moves G and O next to the pose
//                      or ends with SDAA_STATUS_RANGE. `first` and `level` mean what they mean there, G and O travelling with T.
//
// The includer provides what semidense_align_device.hpp asks for.
#pragma once
#include "semidense_align_device.hpp"

#define SDAA_NSUM 47    // 36 H, 8 b, sum w r^2, sum w, count
#define SDAA_ROW 48     // doubles per staged row
#define SDAA_STAGE 85   // rows of `partial` staged in LDS at a time (85 * 48 doubles = 32640 bytes of the records' 32 KB)
#define SDAA_STATUS_RANGE 5
#define SDAA_G_MIN 8192.0     // 2^13
#define SDAA_G_MAX 524288.0   // 2^19
#define SDAA_O_MAX 4080.0

struct SdaaLevel {  // one level's last evaluated system and the brightness it left
  int status, iters, count, pad;
  double swrr, sw;
  int G, O;
};

struct SdaaState {  // the small device block: pose, brightness, status and the "done" word; the last evaluated system
  float T[16];
  int status, iters, done, count;
  unsigned ticket;
  int pad;
  int G, O;         // gain in 2^-16, offset in 1/16 grey level
  double swrr, sw;  // sum w r^2, sum w (unscaled)
  double H[36], b[8];
  SdaaLevel lv[SDA_MAX_LEVELS];
  int start_prev, pad2;
};

struct SdaaArgs {
  SdaArgs a;  // the plain kernel's arguments (its `st` is not used; `partial` holds SDAA_NSUM sums per block)
  int G0, O0;
  SdaaState *st;
};

// host: gain0, offset0 as the kernel takes them (host code: -ffp-contract=off)
static inline void sdaa_params(SdaaArgs *a, float gain0, float offset0) {
  a->G0 = (int)floorf(65536.0f * gain0 + 0.5f);
  a->O0 = (int)floorf(16.0f * offset0 + 0.5f);
}

// the last workgroup's thread 0: S = the 47 sums in f64 (unscaled). Solves, updates pose and brightness, writes the state block.
__device__ static inline void sdaa_finish(const SdaaArgs &aa, const double *S, const float Tin[12], int Gin, int Oin, bool from_start) {
  const SdaArgs &a = aa.a;
  SdaaState *st = aa.st;
  double A[8][8], bv[8];
  {
    int n = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i)
#pragma unroll
      for (int j = i; j < 8; ++j, ++n) {
        const double h = S[n] * (1.0 / 65536.0);
        A[i][j] = A[j][i] = h;
        st->H[n] = h;
      }
#pragma unroll
    for (int i = 0; i < 8; ++i) st->b[i] = bv[i] = S[36 + i] * (1.0 / 65536.0);
  }
  const int count = (int)S[46], iters = (a.first ? 0 : st->iters) + 1;
  st->count = count;
  st->iters = iters;
  st->swrr = S[44];
  st->sw = S[45];
  int status = 1, done = iters >= a.max_iters ? 1 : 0;
  int Go = Gin, Oo = Oin;
  float To[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) To[i] = Tin[i];
  if (count < a.min_pixels) {
    status = 2;
    done = 1;
  } else {
    double L[8][8], Dg[8], y[8], x[8];
    bool ok = true;
    // (no early exit: every loop has constant bounds and unrolls, so that the arrays stay in registers; after a refused pivot the
    // values that follow are not used)
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      double d = A[j][j];
#pragma unroll
      for (int k = 0; k < j; ++k) d = d - (L[j][k] * L[j][k]) * Dg[k];
      ok = ok && d > 0.0 && d > A[j][j] * SDA_PIVOT && d <= 1.7976931348623157e308;
      Dg[j] = d;
#pragma unroll
      for (int i = j + 1; i < 8; ++i) {
        double s = A[i][j];
#pragma unroll
        for (int k = 0; k < j; ++k) s = s - (L[i][k] * L[j][k]) * Dg[k];
        L[i][j] = s / d;
      }
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      double s = bv[i];
#pragma unroll
      for (int k = 0; k < i; ++k) s = s - L[i][k] * y[k];
      y[i] = s;
    }
#pragma unroll
    for (int i = 7; i >= 0; --i) {
      double s = y[i] / Dg[i];
#pragma unroll
      for (int k = i + 1; k < 8; ++k) s = s - L[k][i] * x[k];
      x[i] = s;
    }
#pragma unroll
    for (int i = 0; i < 8; ++i) ok = ok && fabs(x[i]) <= 1.7976931348623157e308;
    if (!ok) {
      status = 3;
      done = 1;
    } else {
      const double Gn = (double)Gin + floor(65536.0 * x[6] + 0.5), On = (double)Oin + floor(16.0 * x[7] + 0.5);
      if (!(Gn >= SDAA_G_MIN && Gn <= SDAA_G_MAX && On >= -SDAA_O_MAX && On <= SDAA_O_MAX)) {  // (false for NaN)
        status = SDAA_STATUS_RANGE;
        done = 1;
      } else {
        const double nrm2 = ((((x[0] * x[0] + x[1] * x[1]) + x[2] * x[2]) + x[3] * x[3]) + x[4] * x[4]) + x[5] * x[5];
        float xi[6], E[12];
#pragma unroll
        for (int i = 0; i < 6; ++i) xi[i] = -(float)x[i];
        sda_se3_exp(xi, E);
#pragma unroll
        for (int i = 0; i < 3; ++i)  // T <- T * exp(-xi) in svo_mul44's order (row 3 of both: 0 0 0 1)
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            float r = SDT_MUL(Tin[i * 4 + 0], E[j]);
            r = SDT_ADD(SDT_MUL(Tin[i * 4 + 1], E[4 + j]), r);
            r = SDT_ADD(SDT_MUL(Tin[i * 4 + 2], E[8 + j]), r);
            r = SDT_ADD(SDT_MUL(Tin[i * 4 + 3], j == 3 ? 1.0f : 0.0f), r);
            To[i * 4 + j] = r;
          }
        Go = (int)Gn;
        Oo = (int)On;
        if (nrm2 < a.eps2) {
          status = 0;
          done = 1;
        }
      }
    }
  }
#pragma unroll
  for (int i = 0; i < 12; ++i) st->T[i] = To[i];
  st->T[12] = st->T[13] = st->T[14] = 0.0f;
  st->T[15] = 1.0f;
  st->G = Go;
  st->O = Oo;
  st->status = status;
  st->done = done;
  SdaaLevel *lv = &st->lv[a.level];
  lv->status = status;
  lv->iters = iters;
  lv->count = count;
  lv->pad = 0;
  lv->swrr = S[44];
  lv->sw = S[45];
  lv->G = Go;
  lv->O = Oo;
  if (a.first == SDA_FIRST_CALL || a.first == SDA_FIRST_PREV) st->start_prev = from_start ? 0 : 1;
}

__global__ __launch_bounds__(SDA_NT) void semidense_affine_kernel(SdaaArgs aa) {
  __shared__ union {
    int rec[8 * SDA_BLOCK];  // field f of listed pixel e at [f * SDA_BLOCK + e]: q0..q5, w | Lk << 12 | valid << 24, r
    double stage[SDAA_STAGE * SDAA_ROW];  // then the staged rows of `partial`
  } s_u;
  int *const s_rec = s_u.rec;
  __shared__ uint16_t s_list[SDA_BLOCK];
  __shared__ long long s_part[4][64];
  __shared__ int s_wn[SDA_NT / 64];
  __shared__ int s_last;
  __shared__ double s_sum[SDAA_ROW];
  const SdaArgs &a = aa.a;
  SdaaState *const st = aa.st;
  const int tid = (int)threadIdx.x, wave = tid >> 6;
  if (!a.first && st->done) return;  // (written by an earlier launch: every thread reads the same word)
  const int W = a.W, H = a.H;
  const long long np = (long long)W * (long long)H, base = (long long)blockIdx.x * SDA_BLOCK;
  // (the state block's words read here were written by an earlier launch: every thread of every workgroup reads the same)
  const bool from_start = a.first == SDA_FIRST_CALL || (a.first == SDA_FIRST_PREV && (unsigned)st->status > 1u);
  float T[12];
#pragma unroll
  for (int i = 0; i < 12; ++i) T[i] = from_start ? a.T0[i] : st->T[i];
  const int G = from_start ? aa.G0 : st->G, O = from_start ? aa.O0 : st->O;
  // ---- (a) the block's pixels of the set, packed ----------------------------------------------------------------------------------
  int n = 0;
  for (int k = 0; k < SDA_BLOCK / SDA_NT; ++k) {
    const int li = k * SDA_NT + tid;
    const long long i = base + li;
    bool in = false;
    if (i < np) {
      const int y = (int)(i / W), x = (int)(i - (long long)y * W);
      if (x >= 1 && x <= W - 2 && y >= 1 && y <= H - 2 && (int)a.n_obs[i] >= a.min_obs) in = a.sigma[i] > 0.0f && a.invd[i] > 0.0f;
    }
    int cnt;
    const int r = sda_wave_rank(in, &cnt);
    if ((tid & 63) == 0) s_wn[wave] = cnt;
    __syncthreads();
    int off = n;
    for (int v = 0; v < SDA_NT / 64; ++v) {
      off += v < wave ? s_wn[v] : 0;
      n += s_wn[v];
    }
    if (in) s_list[off + r] = (uint16_t)li;
    __syncthreads();
  }
  // ---- (b) one listed pixel per thread and turn ----------------------------------------------------------------------------------
  for (int e = tid; e < n; e += SDA_NT) {
    const long long i = base + (int)s_list[e];
    const int y = (int)(i / W), x = (int)(i - (long long)y * W);
    const uint8_t *c = a.Lk + (size_t)y * (size_t)a.strideK + (size_t)x;
    const float gx = (float)((int)c[1] - (int)c[-1]), gy = (float)((int)c[a.strideK] - (int)c[-a.strideK]);
    const int lk = (int)c[0];
    const float invd = a.invd[i];
    const float Z = 1.0f / invd;
    const float u = SDT_SUB((float)x, a.cx) / a.fx, v = SDT_SUB((float)y, a.cy) / a.fy;
    const float X = SDT_MUL(u, Z), Y = SDT_MUL(v, Z);
    const float fu = SDT_MUL(a.fx, u), fv = SDT_MUL(a.fy, v);
    const float Ju[6] = {SDT_MUL(a.fx, invd), 0.0f, -SDT_MUL(fu, invd), -SDT_MUL(fu, v), SDT_ADD(a.fx, SDT_MUL(fu, u)), -SDT_MUL(a.fx, v)};
    const float Jv[6] = {0.0f, SDT_MUL(a.fy, invd), -SDT_MUL(fv, invd), -SDT_ADD(a.fy, SDT_MUL(fv, v)), SDT_MUL(fv, u), SDT_MUL(a.fy, u)};
    bool keep = fabsf(X) <= 3.40282347e+38f && fabsf(Y) <= 3.40282347e+38f && fabsf(Z) <= 3.40282347e+38f;
    int q[6];
#pragma unroll
    for (int j = 0; j < 6; ++j) {
      const float J16 = SDT_MUL(16.0f, SDT_MUL(0.5f, SDT_ADD(SDT_MUL(gx, Ju[j]), SDT_MUL(gy, Jv[j]))));
      const bool okj = fabsf(J16) < SDA_QMAX;  // (false for NaN)
      keep = keep && okj;
      q[j] = okj ? (int)floorf(SDT_ADD(J16, 0.5f)) : 0;
    }
    int wv = 0, r = 0;
    if (keep) {
      const float Xc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[0], X), SDT_MUL(T[1], Y)), SDT_MUL(T[2], Z)), T[3]);
      const float Yc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[4], X), SDT_MUL(T[5], Y)), SDT_MUL(T[6], Z)), T[7]);
      const float Zc = SDT_ADD(SDT_ADD(SDT_ADD(SDT_MUL(T[8], X), SDT_MUL(T[9], Y)), SDT_MUL(T[10], Z)), T[11]);
      if (Zc > SDA_FRONT) {
        const int QX = sdt_q(SDT_ADD(SDT_MUL(a.fx, Xc / Zc), a.cx)), QY = sdt_q(SDT_ADD(SDT_MUL(a.fy, Yc / Zc), a.cy));
        if (sdt_in(QX, QY, W, H)) {
          const int model = (int)(((long long)G * (long long)(16 * lk) + 32768ll) >> 16) + O;  // (below 2^16: G <= 2^19, |O| <= 4080)
          r = sdt_sample(a.Lc, a.strideC, W, H, QX, QY) - model;
          const int ar = r < 0 ? -r : r;
          wv = (ar <= a.kq ? 256 : (256 * a.kq) / ar) | (lk << 12) | (1 << 24);
        }
      }
    }
#pragma unroll
    for (int j = 0; j < 6; ++j) s_rec[j * SDA_BLOCK + e] = keep ? q[j] : 0;
    s_rec[6 * SDA_BLOCK + e] = wv;
    s_rec[7 * SDA_BLOCK + e] = r;
  }
  __syncthreads();
  // ---- (c) the block's 47 sums ---------------------------------------------------------------------------------------------------
  {
    const int s = tid & 63, part = tid >> 6;
    // sum s: weight * A * B with (A, B) = (q_i, q_j) for the 36 pairs i <= j row by row, (q_i, r), (r, r), (1, 1), and the count.
    // A factor is named by a field: 0..5 the record's q, 6 = 16 Lk, 7 = 16, 8 = r, 9 = 1
    const int i = (s >= 8) + (s >= 15) + (s >= 21) + (s >= 26) + (s >= 30) + (s >= 33) + (s >= 35), j = i + (s - (i * 8 - (i * (i - 1)) / 2));
    const int fa = s < 36 ? i : (s < 44 ? s - 36 : (s == 44 ? 8 : 9)), fb = s < 36 ? j : (s < 45 ? 8 : 9);
    // (a dense coarse level lists nearly all 1024 pixels of a block, so this loop is the launch's longest part: no branch in it — a
    // factor is rec * m + 16 Lk * c6 + r * c8 + c with the thread's own 0 / 1 / constant multipliers — and one 32-bit product in front
    // of the 64-bit one: w <= 2^8 and |factor| < 2^22, so w * A stays below 2^30)
    const int ra = fa < 6 ? fa : 0, ma = fa < 6 ? 1 : 0, a6 = fa == 6 ? 1 : 0, a8 = fa == 8 ? 1 : 0, ca = fa == 7 ? 16 : (fa == 9 ? 1 : 0);
    const int rb = fb < 6 ? fb : 0, mb = fb < 6 ? 1 : 0, b6 = fb == 6 ? 1 : 0, b8 = fb == 8 ? 1 : 0, cb = fb == 7 ? 16 : (fb == 9 ? 1 : 0);
    long long acc = 0;
    if (s < SDAA_NSUM)
      for (int e = part; e < n; e += 4) {
        const int wv = s_rec[6 * SDA_BLOCK + e], rr = s_rec[7 * SDA_BLOCK + e], k16 = 16 * ((wv >> 12) & 0xFF);
        const int wt = s == 46 ? (wv >> 24) : (wv & 0xFFF);
        const int A = s_rec[ra * SDA_BLOCK + e] * ma + k16 * a6 + rr * a8 + ca;
        const int B = s_rec[rb * SDA_BLOCK + e] * mb + k16 * b6 + rr * b8 + cb;
        acc += (long long)(wt * A) * (long long)B;
      }
    s_part[part][s] = acc;
  }
  __syncthreads();
  if (tid < SDAA_NSUM) {
    long long t = 0;
    for (int p = 0; p < 4; ++p) t += s_part[p][tid];
    a.partial[(size_t)blockIdx.x * SDAA_NSUM + tid] = t;
  }
  // ---- (d) the ticket: the last workgroup reduces, solves and updates ---------------------------------------------------------------
  SDA_DRAIN();      // every wavefront: its row entries have left ...
  __syncthreads();  // ... before thread 0 publishes them (one agent-scope release) and takes the workgroup's ticket
  if (tid == 0) {
    SDA_FENCE_RELEASE();
    s_last = (SDA_ATOMIC_ADD_AGENT(&st->ticket, 1u) == (unsigned)a.n_blocks - 1u) ? 1 : 0;
    if (s_last) SDA_FENCE_ACQUIRE();  // one agent-scope acquire covers the workgroup: the barrier below stands behind its wait
  }
  __syncthreads();
  if (!s_last) return;
  double *const stage = s_u.stage;  // [SDAA_STAGE][SDAA_ROW]
  double sum = 0.0;
  for (int b0 = 0; b0 < a.n_blocks; b0 += SDAA_STAGE) {
    const int nb = a.n_blocks - b0 < SDAA_STAGE ? a.n_blocks - b0 : SDAA_STAGE;
#pragma unroll 8
    for (int k = tid; k < nb * SDAA_NSUM; k += SDA_NT) {  // (plain vector loads behind the acquire: independent, so they overlap)
      const int b = k / SDAA_NSUM, s = k - b * SDAA_NSUM;
      stage[b * SDAA_ROW + s] = (double)a.partial[(size_t)(b0 + b) * SDAA_NSUM + s];
    }
    __syncthreads();
    if (tid < SDAA_NSUM) {
#pragma unroll 16
      for (int b = 0; b < nb; ++b) sum = sum + stage[b * SDAA_ROW + tid];  // block order, block 0 first (unrolled: the reads run ahead of the adds)
    }
    __syncthreads();
  }
  if (tid < SDAA_NSUM) s_sum[tid] = sum;
  __syncthreads();
  if (tid == 0) {
    sdaa_finish(aa, s_sum, T, G, O, from_start);
    SDA_ST_AGENT(&st->ticket, 0u);  // back to zero for the next launch (every workgroup has taken its ticket: this one holds the last)
  }
}

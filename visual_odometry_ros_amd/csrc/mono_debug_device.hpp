// mono_debug_device.hpp — what MonoVO's steady-state debug image is drawn from (mono_vo.cpp:799-904): the pose-only BA's input
// pixels pts1_ba and their projections pts1_proj_ba under the pose the BA found, gathered from the frame's own device arrays
// before the next frame overwrites them. Included by mono_vo.hip (mvo_debug_gather_kernel, one lane per feature) and, through
// tests/emu/hip_emu.h, by the CPU harness that runs this text against the numpy restatement.
//
//   member i      stage[i] >= 2 (refined) and ba_ok[i] (BA class and Xp(2) > 0.1): index_ba of :799-826, in feature order
//   pts1_ba[i]    the refined pixel pts1[i], whatever the BA and the Sampson gate did to the feature afterwards
//   pts1_proj_ba  projectToPixel(dR10 * Xp + dt10) (:893-897, camera.cpp:208-213), dT10 = inverseSE3_f(dT01) of the frame's pose
// Every operation is a float operation rounded on its own (the library is compiled without contraction).
//
// The sets are NOT compacted: entry i belongs to feature i, valid[i] says whether it is a member, and a non-member's two pixels
// are NaN — the drawing rules skip a NaN point, and overlap depends on the relative order of the primitives only, so the picture
// is the one the compacted sets give. A frame whose BA gave no pose (need_five_point) draws nothing in the reference: the
// gather then writes "keep" into the control word and touches nothing else.
#pragma once
#include <stdint.h>

enum { MVO_DBG_GO = 0, MVO_DBG_N = 1, MVO_DBG_WORDS = 4 };  // ctl[GO]: 1 draw / 0 keep; ctl[N]: entries the sets span
struct MonoDbgArgs {
  int n;                       // features of the frame
  const uint8_t *stage;        // [n] the frame's result
  const uint8_t *ba_ok;        // [n]
  const float *pts1;           // [n][2] the frame's result pixels (refined for stage >= 2)
  const float *Xp;             // [n][3] the point in the previous camera frame, as the frame kernel computed it
  const float *dT01;           // [16] the frame's pose, device-resident
  const int *need_five_point;  // the frame's count word: non-zero = the reference draws nothing
  float K[4];                  // fx fy cx cy
  int *ctl;                    // out [MVO_DBG_WORDS]
  float *pts_ba, *pts_proj;    // out [n][2] each
  uint8_t *valid;              // out [n]
};

// geometry::inverseSE3_f, the operations of svo_inv_se3 (stereo_vo.hip): R10 = R01^T, t10 = ((-R10_r0 t0) + (-R10_r1 t1)) + (-R10_r2 t2)
__host__ __device__ __forceinline__ void mono_dbg_inv_se3(const float *T, float R[9], float t[3]) {
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) R[i * 3 + j] = T[j * 4 + i];
  const float t0 = T[3], t1 = T[7], t2 = T[11];
  for (int i = 0; i < 3; ++i) t[i] = ((-R[i * 3 + 0]) * t0 + (-R[i * 3 + 1]) * t1) + (-R[i * 3 + 2]) * t2;
}
__host__ __device__ __forceinline__ bool mono_dbg_member(int stage, int ba_ok) { return stage >= 2 && ba_ok != 0; }
// Xc = R Xp + t in the order of Eigen's fixed-size product, then Camera::projectToPixel. Xc(2) <= 0 gives negative, infinite or
// NaN pixels: the drawing rules deal with those.
__host__ __device__ __forceinline__ void mono_dbg_project(const float R[9], const float t[3], const float K[4], const float *Xp, float &u,
                                                          float &v) {
  float Xc[3];
  for (int r = 0; r < 3; ++r) Xc[r] = ((R[r * 3 + 0] * Xp[0] + R[r * 3 + 1] * Xp[1]) + R[r * 3 + 2] * Xp[2]) + t[r];
  const float invz = 1.0f / Xc[2];
  u = (K[0] * Xc[0]) * invz + K[2];
  v = (K[1] * Xc[1]) * invz + K[3];
}

// lane i of a launch that covers at least max(n, 1) lanes
__host__ __device__ __forceinline__ void mono_dbg_gather(const MonoDbgArgs &a, int i) {
  const bool go = a.n > 0 && *a.need_five_point == 0;
  if (i == 0) {
    a.ctl[MVO_DBG_GO] = go ? 1 : 0;
    if (go) a.ctl[MVO_DBG_N] = a.n;
  }
  if (!go || i >= a.n) return;
  const bool in = mono_dbg_member(a.stage[i], a.ba_ok[i]);
  const float nan = __builtin_nanf("");
  float px = nan, py = nan, u = nan, v = nan;
  if (in) {
    float R[9], t[3];
    mono_dbg_inv_se3(a.dT01, R, t);
    px = a.pts1[2 * i];
    py = a.pts1[2 * i + 1];
    mono_dbg_project(R, t, a.K, a.Xp + 3 * i, u, v);
  }
  a.pts_ba[2 * i] = px;
  a.pts_ba[2 * i + 1] = py;
  a.pts_proj[2 * i] = u;
  a.pts_proj[2 * i + 1] = v;
  a.valid[i] = in ? 1 : 0;
}

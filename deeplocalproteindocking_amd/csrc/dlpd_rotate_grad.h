// The adjoint of the trilinear volume rotation (k_rotate of dlpd_corr.hip; TPL VolumeRotation is a differentiable operator,
// call site src/Docker/Docker.py:218): what carries a gradient from rotated copies of a volume back to the volume -- the
// ligand's gradient through the poses of a search's top list.
//
//   out[b,c,i]  = sum_q w_b(i, q) vol[c, q]          (the forward: w the trilinear weight sample p_b(i) gives corner q)
//   gvol[c,q]   = sum_b sum_i w_b(i, q) gout[b,c,i]  (this kernel; per batch entry without the sum over b)
//   p_b(i)      = c0 + A_b (i - c0),  A[a][k] = m[3k + a]  (k_rotate's expression, evaluated here in the same form)
//   with `off` (B, 3), the per-pose offset of dlpd_rotate_shift.h: p_b(i) = (c0 + off_b) + A_b (i - c0); the candidates of q are
//   then centred on c0 + A^-1 (q - c0 - off_b).  off null: zeros, the bits of the plain position.
//
// A GATHER, not a scatter: a thread owns a source voxel q (lanes along z, the contiguous axis) and walks the output voxels i
// that can reach it.  w(i, q) != 0 needs p(i) in the open cube q + (-1, 1)^3, i.e. i in c0 + A^-1 (q - c0 + (-1, 1)^3): along
// axis k within h_k = sum_j |A^-1[k][j]| of i0 = c0 + A^-1 (q - c0) (<= sqrt 3 for a rotation: at most 4 integers per axis,
// 64 candidates, 8 of them with weight on average).  A^-1 comes from the cofactors, per matrix, in the kernel (block-uniform).
// The bounds carry a rounding slack and are clamped to the box, so ANY invertible map is exact; bounds that are not finite (a
// singular map) fall back to the whole axis.  The weight of a candidate is recomputed from p(i) exactly as trilinear_fetch
// does (trilinear_axis_weight, dlpd_trilinear.h); candidates of weight 0 are skipped before anything is loaded.
//
// The geometry does not depend on the channel: a thread carries DLPD_ROT_GRAD_CC = 16 channels in registers (16 sums of the
// pose + 16 of the element), candidates and weights are computed once per chunk of channels.  Order of the additions, per
// element: the candidates in (x, y, z) ascending give the pose's sum s_b; then acc = acc + s_b, b ascending, acc starting at 0
// or (accumulate) at the stored value -- so B poses split over several calls give the bits of one call.  No float atomics, no
// workspace, every element written exactly once (zeros included): the same bits run to run.
// gfx950: 115 VGPRs (4 waves per SIMD), no scratch, no LDS (-Rpass-analysis=kernel-resource-usage).
#pragma once
#include "dlpd_local.h"

#ifndef DLPD_ROT_GRAD_CC
#define DLPD_ROT_GRAD_CC 16          // channels a thread carries in registers (A/B builds: -DDLPD_ROT_GRAD_CC=8, 4)
#endif
#ifndef DLPD_ROT_GRAD_SKIP
#define DLPD_ROT_GRAD_SKIP 1         // 0 (A/B builds only): load and add the candidates of weight 0 too
#endif

// candidate range along one axis: the integers within e of i0, clamped to the box; not finite: the whole axis
DLPD_D void rot_grad_range(float i0, float e, int L, int* lo, int* hi) {
  const float a = i0 - e, b = i0 + e, top = (float)(L - 1);
  *lo = 0;
  *hi = L - 1;
  if (!(fabsf(a) <= 3.0e38f) || !(fabsf(b) <= 3.0e38f)) return;
  *lo = a <= 0.f ? 0 : (a > top ? L : (int)ceilf(a));
  *hi = b >= top ? L - 1 : (b < 0.f ? -1 : (int)floorf(b));
}

// grid (NO * nchunk * nvb), NO = B (gvol_bstride != 0: a gradient per batch entry) or 1 (one gradient, summed over b);
// block 256 source voxels.  gout (B, C, L^3), R (B, 9), off (B, 3) or null, gvol (NO, C, L^3).
__global__ void __launch_bounds__(256)
k_rotate_adjoint(const float* __restrict__ gout, const float* __restrict__ R, const float* __restrict__ off,
                 float* __restrict__ gvol, int B, int C, int L, int nvb, int nchunk, long long gvol_bstride, float c0,
                 int accumulate) {
  constexpr int CC = DLPD_ROT_GRAD_CC;
  const int vb = blockIdx.x % nvb, oc = blockIdx.x / nvb, ch = oc % nchunk, bo = oc / nchunk;
  const size_t L3 = (size_t)L * L * L;
  const size_t q = (size_t)vb * 256 + threadIdx.x;
  if (q >= L3) return;
  const int qz = (int)(q % L), qy = (int)((q / L) % L), qx = (int)(q / ((size_t)L * L));
  const int cb = ch * CC, nc = min(CC, C - cb);
  const int b_beg = gvol_bstride ? bo : 0, b_end = gvol_bstride ? bo + 1 : B;
  float* dst = gvol + (size_t)bo * gvol_bstride + (size_t)cb * L3 + q;
  float acc[CC];
#pragma unroll
  for (int k = 0; k < CC; k++) acc[k] = (accumulate && k < nc) ? dst[(size_t)k * L3] : 0.f;
  for (int b = b_beg; b < b_end; b++) {
    float m[9];
    for (int i = 0; i < 9; i++) m[i] = R[(size_t)b * 9 + i];
    const float ox = off ? off[(size_t)b * 3 + 0] : 0.f, oy = off ? off[(size_t)b * 3 + 1] : 0.f, oz = off ? off[(size_t)b * 3 + 2] : 0.f;
    const float cx = c0 + ox, cy = c0 + oy, cz = c0 + oz;              // the pivot the rotated term is added to
    const float ex = (qx - c0) - ox, ey = (qy - c0) - oy, ez = (qz - c0) - oz;
    // A = [m0 m3 m6; m1 m4 m7; m2 m5 m8]; its inverse by cofactors
    const float k00 = m[4] * m[8] - m[7] * m[5], k01 = m[6] * m[5] - m[3] * m[8], k02 = m[3] * m[7] - m[6] * m[4];
    const float k10 = m[7] * m[2] - m[1] * m[8], k11 = m[0] * m[8] - m[6] * m[2], k12 = m[6] * m[1] - m[0] * m[7];
    const float k20 = m[1] * m[5] - m[4] * m[2], k21 = m[3] * m[2] - m[0] * m[5], k22 = m[0] * m[4] - m[3] * m[1];
    const float rdet = 1.0f / (m[0] * k00 + m[3] * k10 + m[6] * k20);
    int lo[3], hi[3];
    {
      const float ix0 = c0 + rdet * (k00 * ex + k01 * ey + k02 * ez), hx = fabsf(rdet) * (fabsf(k00) + fabsf(k01) + fabsf(k02));
      const float iy0 = c0 + rdet * (k10 * ex + k11 * ey + k12 * ez), hy = fabsf(rdet) * (fabsf(k10) + fabsf(k11) + fabsf(k12));
      const float iz0 = c0 + rdet * (k20 * ex + k21 * ey + k22 * ez), hz = fabsf(rdet) * (fabsf(k20) + fabsf(k21) + fabsf(k22));
      rot_grad_range(ix0, hx + 1e-3f * (1.f + fabsf(ix0) + hx), L, &lo[0], &hi[0]);      // (+ rounding slack)
      rot_grad_range(iy0, hy + 1e-3f * (1.f + fabsf(iy0) + hy), L, &lo[1], &hi[1]);
      rot_grad_range(iz0, hz + 1e-3f * (1.f + fabsf(iz0) + hz), L, &lo[2], &hi[2]);
    }
    const float* g = gout + ((size_t)b * C + cb) * L3;
    float s[CC];
#pragma unroll
    for (int k = 0; k < CC; k++) s[k] = 0.f;
    for (int ix = lo[0]; ix <= hi[0]; ix++) {
      const float dx = ix - c0;
      for (int iy = lo[1]; iy <= hi[1]; iy++) {
        const float dy = iy - c0;
        for (int iz = lo[2]; iz <= hi[2]; iz++) {
          const float dz = iz - c0;
          const float px = cx + (m[0] * dx + m[3] * dy + m[6] * dz);
          const float py = cy + (m[1] * dx + m[4] * dy + m[7] * dz);
          const float pz = cz + (m[2] * dx + m[5] * dy + m[8] * dz);
          const float wx = trilinear_axis_weight(px, qx), wy = trilinear_axis_weight(py, qy), wz = trilinear_axis_weight(pz, qz);
          const float w = wx * wy * wz;
          if (DLPD_ROT_GRAD_SKIP && w == 0.f) continue;
          const float* gi = g + ((size_t)ix * L + iy) * L + iz;
#pragma unroll
          for (int k = 0; k < CC; k++)
            if (k < nc) s[k] = fmaf(gi[(size_t)k * L3], w, s[k]);
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CC; k++) acc[k] = acc[k] + s[k];
  }
#pragma unroll
  for (int k = 0; k < CC; k++)
    if (k < nc) dst[(size_t)k * L3] = acc[k];
}

// the body of dlpd_rotate_trilinear_grad and, with `off`, of dlpd_rotate_trilinear_shift_grad (dlpd_rotate_shift.h)
static int rot_adjoint_run(const float* gout, const float* R, const float* off, float* gvol, int B, int C, int L,
                           long long gvol_bstride, float center, int accumulate, void* stream) {
  if (!gout || !R || !gvol || B <= 0 || C <= 0 || gvol_bstride < 0) return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL) return DLPD_ERR_UNSUPPORTED;
  const size_t L3 = (size_t)L * L * L, nvb = (L3 + 255) / 256, nchunk = ((size_t)C + DLPD_ROT_GRAD_CC - 1) / DLPD_ROT_GRAD_CC;
  const size_t per = nvb * nchunk, most = (0xffffffffull / 256) / per;      // a launch holds < 2^32 threads
  if (most == 0) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const size_t NO = gvol_bstride ? (size_t)B : 1;
  for (size_t beg = 0; beg < NO; beg += most) {                            // (a gradient per batch entry: slices of b)
    const size_t n = NO - beg < most ? NO - beg : most;
    const float* go = gout + (gvol_bstride ? beg * C * L3 : 0);
    const float* Rb = R + (gvol_bstride ? beg * 9 : 0);
    const float* ob = off ? off + (gvol_bstride ? beg * 3 : 0) : nullptr;
    float* gv = gvol + beg * (size_t)gvol_bstride;
    DLPD_LAUNCH(k_rotate_adjoint, dim3((unsigned)(n * per)), dim3(256), 0, st, go, Rb, ob, gv, gvol_bstride ? (int)n : B, C, L,
                (int)nvb, (int)nchunk, gvol_bstride, center, accumulate ? 1 : 0);
  }
  return dlpd_check_launch();
}

extern "C" {

// gout (B, C, L^3) the gradient of dlpd_rotate_trilinear's output, R (B, 9) and center as that call took them.
// gvol: the gradient of its `vol`, laid out as vol was -- (B, C, L^3) with batch stride gvol_bstride floats, or, for stride 0
// (one volume set for all b), (C, L^3) = the sum over b, added in the order of b.  accumulate: the sums start at the stored
// values (the next chunk of a long list of poses) instead of 0.  Every element is written.
int dlpd_rotate_trilinear_grad(const float* gout, const float* R, float* gvol, int B, int C, int L, long long gvol_bstride,
                               float center, int accumulate, void* stream) {
  return rot_adjoint_run(gout, R, nullptr, gvol, B, C, L, gvol_bstride, center, accumulate, stream);
}

}  // extern "C"

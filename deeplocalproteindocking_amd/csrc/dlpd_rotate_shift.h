// Sub-voxel translations: the trilinear rotation with a per-pose OFFSET of the sample position, through every kernel of the
// local-docking stack that evaluates it -- what lets a pose move by a fraction of a voxel, and a descent (Docker.minimize with
// translation=True) move all six degrees of freedom of a rigid body.
//
//   p_a(i) = (c0 + off[b][a]) + sum_j R[b][3j + a] (i_j - c0)        off (B, 3) f32, voxels of the source volume, null: zeros
//
// c0 + off is added FIRST and the rotated term then, the rotated term in k_rotate's own form: with off = 0 (or null) every
// entry below returns the bits of the plain entry without a branch on the value.  A ligand displaced by s voxels of the
// output grid is off = -R^T s (the caller's arithmetic: ops.VolumeRotation(shift=)).
//
//   dlpd_rotate_trilinear_shift       out[b,c,i]  = vol_c( p_b(i) )                        k_rotate_shift, this file
//   dlpd_rotate_trilinear_shift_grad  gvol[c,q]   = sum_b sum_i w_b(i, q) gout[b,c,i]      k_rotate_adjoint (dlpd_rotate_grad.h)
//   dlpd_rotate_trilinear_pgrad       gR[b][3j+a] = sum_c sum_i gout d_a vol_c( p_b(i) ) (i_j - c0)
//                                     goff[b][a]  = sum_c sum_i gout d_a vol_c( p_b(i) )   k_rotate_rgrad<true> (dlpd_rotate_rgrad.h)
//   dlpd_local_correlate_shift        corr[p,c,d] = sum_x rec[c, x + tau] vol_c( (c0 + off_p) + M^T (x - c0) )
//   dlpd_local_correlate_shift_grad   its receptor gradient                                k_local_corr, k_local_corr_grad
//
// The offset is one more argument (nullable) of the kernels that already evaluate p(i); only the forward is a kernel of its
// own, because k_rotate lives with the search pipeline, which does not change.  The pose gradient is k_rotate_rgrad's body with
// three more float64 sums (template flag OFF): the same loads, the same order of additions, twelve partials per block.
// gfx950 (-Rpass-analysis=kernel-resource-usage): k_rotate_shift 34 VGPRs, no scratch, no LDS; k_rotate_rgrad<true> 50 VGPRs
// (8 waves per SIMD), no scratch, 384 bytes of LDS; k_rotate_rgrad<false> 50 VGPRs, no scratch, 288 bytes of LDS, as before;
// k_rotate_adjoint with its nullable offset 115 VGPRs (4 waves per SIMD, as before), no scratch, no LDS.
#pragma once
#include "dlpd_local_grad.h"
#include "dlpd_rotate_grad.h"
#include "dlpd_rotate_rgrad.h"

// grid-stride over the B * C * L^3 output voxels, block 256 (k_rotate's shape).  off (B, 3) or null.
__global__ void __launch_bounds__(256)
k_rotate_shift(const float* __restrict__ vol, const float* __restrict__ R, const float* __restrict__ off, float* __restrict__ out,
               int B, int C, int L, long long vol_bstride, float c0) {
  const size_t L3 = (size_t)L * L * L;
  const size_t total = (size_t)B * C * L3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int z = (int)(i % L), y = (int)((i / L) % L), x = (int)((i / ((size_t)L * L)) % L);
    const int c = (int)((i / L3) % C), b = (int)(i / (L3 * C));
    const float* r = R + (size_t)b * 9;
    const float ox = off ? off[(size_t)b * 3 + 0] : 0.f, oy = off ? off[(size_t)b * 3 + 1] : 0.f, oz = off ? off[(size_t)b * 3 + 2] : 0.f;
    const float cx = c0 + ox, cy = c0 + oy, cz = c0 + oz;
    const float dx = x - c0, dy = y - c0, dz = z - c0;
    const float px = cx + (r[0] * dx + r[3] * dy + r[6] * dz);
    const float py = cy + (r[1] * dx + r[4] * dy + r[7] * dz);
    const float pz = cz + (r[2] * dx + r[5] * dy + r[8] * dz);
    out[i] = trilinear_fetch(vol + (size_t)b * vol_bstride + (size_t)c * L3, L, px, py, pz);
  }
}

extern "C" {

// vol (B, C, L^3) with batch stride vol_bstride floats (0: one volume set for all b), R (B, 9), off (B, 3) or null,
// out (B, C, L^3): every element is written.
int dlpd_rotate_trilinear_shift(const float* vol, const float* R, const float* off, float* out, int B, int C, int L,
                                long long vol_bstride, float center, void* stream) {
  if (!vol || !R || !out || B <= 0 || C <= 0 || vol_bstride < 0) return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL) return DLPD_ERR_UNSUPPORTED;
  const size_t total = (size_t)B * C * L * L * L;
  size_t nblk = (total + 255) / 256;
  if (nblk > 8192) nblk = 8192;
  DLPD_LAUNCH(k_rotate_shift, dim3((unsigned)nblk), dim3(256), 0, (hipStream_t)stream, vol, R, off, out, B, C, L, vol_bstride, center);
  return dlpd_check_launch();
}

// dlpd_rotate_trilinear_grad with the offset the forward took: the same kernel, the same guarantees
int dlpd_rotate_trilinear_shift_grad(const float* gout, const float* R, const float* off, float* gvol, int B, int C, int L,
                                     long long gvol_bstride, float center, int accumulate, void* stream) {
  return rot_adjoint_run(gout, R, off, gvol, B, C, L, gvol_bstride, center, accumulate, stream);
}

// bytes of workspace dlpd_rotate_trilinear_pgrad needs: twelve float64 partial sums per block; 0 for an unsupported shape
size_t dlpd_rotate_trilinear_pgrad_ws_bytes(int B, int L) {
  if (B <= 0 || L < 2 || L > DLPD_LOCAL_MAXL) return 0;
  return (size_t)B * rot_rgrad_nblk(L) * 12 * sizeof(double);
}

// gout, vol, R, vol_bstride, center as dlpd_rotate_trilinear_rgrad takes them, off (B, 3) or null as the forward took it.
// gR (B, 9) and goff (B, 3): either may be null (not wanted), not both; every element of the others is written.
int dlpd_rotate_trilinear_pgrad(const float* gout, const float* vol, const float* R, const float* off, float* gR, float* goff,
                                void* ws, int B, int C, int L, long long vol_bstride, float center, void* stream) {
  if (!gout || !vol || !R || (!gR && !goff) || !ws || B <= 0 || C <= 0 || vol_bstride < 0) return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL) return DLPD_ERR_UNSUPPORTED;
  return rot_rgrad_run<true>(gout, vol, R, off, gR, goff, ws, B, C, L, vol_bstride, center, stream);
}

// dlpd_local_correlate with the ligand sampled at the offset position; off (P, 3) or null; off without R: DLPD_ERR_ARG
int dlpd_local_correlate_shift(const float* rec, const float* lig, const float* R, const float* off, const int* T, float* corr,
                               void* ws, int P, int C, int L, int r, int scale, int coarse_mode, float center,
                               long long rec_pstride, long long lig_pstride, void* stream) {
  return local_correlate_run(rec, lig, R, off, T, corr, ws, P, C, L, r, scale, coarse_mode, center, rec_pstride, lig_pstride, stream);
}

// dlpd_local_correlate_grad likewise (glig with R stays DLPD_ERR_UNSUPPORTED: dlpd_rotate_trilinear_shift_grad carries it)
int dlpd_local_correlate_shift_grad(const float* rec, const float* lig, const float* R, const float* off, const int* T,
                                    const float* gcorr, float* grec, float* glig, int P, int C, int L, int r, int scale,
                                    int coarse_mode, float center, long long rec_pstride, long long lig_pstride, void* stream) {
  return local_correlate_grad_run(rec, lig, R, off, T, gcorr, grec, glig, P, C, L, r, scale, coarse_mode, center, rec_pstride,
                                  lig_pstride, stream);
}

}  // extern "C"

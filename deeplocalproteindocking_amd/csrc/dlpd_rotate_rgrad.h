// The gradient of the trilinear volume rotation (k_rotate of dlpd_corr.hip) with respect to its MATRIX: what carries a
// gradient from rotated copies of a volume back to the nine numbers of every pose -- the descent of a docking score in the
// rotation itself (Docker.minimize).
//
//   out[b,c,i]    = vol_c( p_b(i) ),   p_a(i) = c0 + sum_j R[b][3j + a] (i_j - c0)          (the forward, k_rotate's expression)
//   gR[b][3j + a] = sum_c sum_i gout[b,c,i] * d_a vol_c( p_b(i) ) * (i_j - c0)              (this file)
//
// d_a vol_c the derivative of the trilinear sample along axis a (trilinear_fetch_grad, dlpd_trilinear.h: the forward's floorf,
// masks, clamped addresses and pair loads).  The sample is piecewise trilinear in p, so this is the derivative of the forward
// everywhere but on the cell faces, where it is the right-hand one.
//
// k_rotate_rgrad: one block per (b, chunk of DLPD_ROT_RGRAD_VT * 256 output voxels), 256 threads, lanes along z (the
// contiguous axis): gout is read once, coalesced, and the volume is gathered exactly as the forward gathers it.  The position
// of a voxel does not depend on the channel: floorf, masks and addresses are computed once per voxel, the channels loop sits
// inside.  Order of the additions: per voxel the three sums s_a = sum_c g_c d_a vol_c are f32 fmaf chains, c ascending; the
// nine sums acc[3j + a] += s_a (i_j - c0) are float64 per thread, its voxels ascending (one by default); then lanes by halving, the four waves
// one after the other (as k_local_corr), and the block's nine float64 partials go to the workspace (B, nblk, 9).
// k_rotate_rgrad_reduce adds them in block order and writes gR (B, 9) as float32, every element, zeros included.  No float
// atomics: the same bits run to run, and a pose's nine numbers do not depend on which other poses share its call.
// DLPD_ROT_RGRAD_VT = 1 voxel per thread, measured (MI355X, 64 poses, kernel + reduce, ms at 16 @ 80^3 / 32 @ 40^3):
// 1: 7.68 / 1.13, 2: 8.97 / 1.55, 4: 10.52 / 1.68, 8: 11.40 / 1.92.  The kernel is bound by the latency of its gathers (4 pair
// loads per voxel and channel, nothing reused); a thread's voxels run one after the other, so more of them per thread means
// fewer loads in flight, and that outweighs the block's 9 x 6 float64 shuffles and the longer reduce (2000 partials per pose
// at box 80, 8192 at box 128).
// gfx950: 50 VGPRs (8 waves per SIMD), no scratch, 288 bytes of LDS (-Rpass-analysis=kernel-resource-usage).
//
// The kernel is a template on OFF: false is the kernel above, nine numbers per block.  true (dlpd_rotate_shift.h: the pose
// gradient with a per-pose offset of the sample position) adds `off` to the pivot before the rotated term and carries three
// more sums, goff[a] = sum_c sum_i g d_a vol -- the s_a of the same voxels without the factor (i_j - c0) -- through the same
// float64 path: twelve partials per block, the nine of gR first.
#pragma once
#include "dlpd_local.h"

#ifndef DLPD_ROT_RGRAD_VT
#define DLPD_ROT_RGRAD_VT 1          // output voxels a thread takes (A/B builds: -DDLPD_ROT_RGRAD_VT=2, 4, 8)
#endif

static inline size_t rot_rgrad_nblk(int L) {
  const size_t L3 = (size_t)L * L * L, per = (size_t)DLPD_ROT_RGRAD_VT * 256;
  return (L3 + per - 1) / per;
}

// grid (B * nblk), block 256.  gout (B, C, L^3), vol (C, L^3) with batch stride vol_bstride, R (B, 9), off (B, 3) or null
// (OFF only), part (B, nblk, NA) f64, NA = 9 or (OFF) 12.
template <bool OFF> __global__ void __launch_bounds__(256)
k_rotate_rgrad(const float* __restrict__ gout, const float* __restrict__ vol, const float* __restrict__ R,
               const float* __restrict__ off, double* __restrict__ part, int C, int L, int nblk, long long vol_bstride, float c0) {
  constexpr int NA = OFF ? 12 : 9;
  __shared__ double sm[4 * NA];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int blk = blockIdx.x % nblk, b = blockIdx.x / nblk;
  const size_t L3 = (size_t)L * L * L;
  float m[9];
  for (int i = 0; i < 9; i++) m[i] = R[(size_t)b * 9 + i];
  const float* volb = vol + (size_t)b * vol_bstride;
  const float* gb = gout + (size_t)b * C * L3;
  // the pivot the rotated term is added to: center + off first, so that off = 0 gives the bits of the plain position
  const float cx = (OFF && off) ? c0 + off[(size_t)b * 3 + 0] : c0, cy = (OFF && off) ? c0 + off[(size_t)b * 3 + 1] : c0,
              cz = (OFF && off) ? c0 + off[(size_t)b * 3 + 2] : c0;
  double acc[NA];
#pragma unroll
  for (int a = 0; a < NA; a++) acc[a] = 0.0;
  for (int k = 0; k < DLPD_ROT_RGRAD_VT; k++) {
    const size_t i = ((size_t)blk * DLPD_ROT_RGRAD_VT + k) * 256 + tid;
    if (i >= L3) break;
    const int z = (int)(i % L), y = (int)((i / L) % L), x = (int)(i / ((size_t)L * L));
    const float dx = x - c0, dy = y - c0, dz = z - c0;
    const float px = cx + (m[0] * dx + m[3] * dy + m[6] * dz);
    const float py = cy + (m[1] * dx + m[4] * dy + m[7] * dz);
    const float pz = cz + (m[2] * dx + m[5] * dy + m[8] * dz);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f;
    for (int c = 0; c < C; c++) {
      float d0, d1, d2;
      trilinear_fetch_grad(volb + (size_t)c * L3, L, px, py, pz, &d0, &d1, &d2);
      const float g = gb[(size_t)c * L3 + i];
      s0 = fmaf(g, d0, s0);
      s1 = fmaf(g, d1, s1);
      s2 = fmaf(g, d2, s2);
    }
    const double e[3] = {(double)dx, (double)dy, (double)dz}, s[3] = {(double)s0, (double)s1, (double)s2};
#pragma unroll
    for (int j = 0; j < 3; j++)
#pragma unroll
      for (int a = 0; a < 3; a++) acc[3 * j + a] += s[a] * e[j];
    if (OFF) {
#pragma unroll
      for (int a = 0; a < 3; a++) acc[9 + a] += s[a];
    }
  }
  // block sum in a fixed order: lanes by halving, then the four waves one after the other
#pragma unroll
  for (int a = 0; a < NA; a++) {
    double v = acc[a];
    for (int d = 32; d > 0; d >>= 1) v += __shfl_down(v, d);
    if (lane == 0) sm[wave * NA + a] = v;
  }
  __syncthreads();
  if (tid < NA) part[((size_t)b * nblk + blk) * NA + tid] = ((sm[tid] + sm[NA + tid]) + sm[2 * NA + tid]) + sm[3 * NA + tid];
}

// gR (B, 9) [NA = 12: and goff (B, 3); either may be null] = the blocks' partial sums added in block order, rounded to float32
// once; n = B * NA
__global__ void __launch_bounds__(256) k_rotate_rgrad_reduce(const double* __restrict__ part, float* __restrict__ gR,
                                                             float* __restrict__ goff, size_t n, int nblk, int NA) {
  const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const size_t b = i / NA, a = i - b * NA;
  float* dst = a < 9 ? (gR ? gR + b * 9 + a : nullptr) : (goff ? goff + b * 3 + (a - 9) : nullptr);
  if (!dst) return;
  const double* src = part + b * (size_t)nblk * NA + a;
  double v = 0.0;
#pragma unroll 8
  for (int k = 0; k < nblk; k++) v += src[(size_t)k * NA];
  *dst = (float)v;
}

// the kernel over slices of b that fit a launch, then the reduce: the body of both entry points (this file's and, with OFF,
// dlpd_rotate_trilinear_pgrad of dlpd_rotate_shift.h)
template <bool OFF>
static int rot_rgrad_run(const float* gout, const float* vol, const float* R, const float* off, float* gR, float* goff, void* ws,
                         int B, int C, int L, long long vol_bstride, float center, void* stream) {
  constexpr int NA = OFF ? 12 : 9;
  const size_t L3 = (size_t)L * L * L, nblk = rot_rgrad_nblk(L), most = (0xffffffffull / 256) / nblk;   // a launch holds < 2^32 threads
  hipStream_t st = (hipStream_t)stream;
  double* part = (double*)ws;
  for (size_t beg = 0; beg < (size_t)B; beg += most) {
    const size_t n = (size_t)B - beg < most ? (size_t)B - beg : most;
    DLPD_LAUNCH((k_rotate_rgrad<OFF>), dim3((unsigned)(n * nblk)), dim3(256), 0, st, gout + beg * C * L3,
                vol + beg * (size_t)vol_bstride, R + beg * 9, off ? off + beg * 3 : nullptr, part + beg * nblk * NA, C, L, (int)nblk,
                vol_bstride, center);
  }
  const size_t total = (size_t)B * NA;
  DLPD_LAUNCH(k_rotate_rgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, (const double*)part, gR, goff, total,
              (int)nblk, NA);
  return dlpd_check_launch();
}

extern "C" {

// bytes of workspace dlpd_rotate_trilinear_rgrad needs: the blocks' float64 partial sums; 0 for an unsupported shape
size_t dlpd_rotate_trilinear_rgrad_ws_bytes(int B, int L) {
  if (B <= 0 || L < 2 || L > DLPD_LOCAL_MAXL) return 0;
  return (size_t)B * rot_rgrad_nblk(L) * 9 * sizeof(double);
}

// gout (B, C, L^3) the gradient of dlpd_rotate_trilinear's output; vol, R, vol_bstride and center as that call took them.
// gR (B, 9): the gradient of the nine entries of every R_b, laid out as R.  Every element is written.
int dlpd_rotate_trilinear_rgrad(const float* gout, const float* vol, const float* R, float* gR, void* ws, int B, int C, int L,
                                long long vol_bstride, float center, void* stream) {
  if (!gout || !vol || !R || !gR || !ws || B <= 0 || C <= 0 || vol_bstride < 0) return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL) return DLPD_ERR_UNSUPPORTED;
  return rot_rgrad_run<false>(gout, vol, R, nullptr, gR, nullptr, ws, B, C, L, vol_bstride, center, stream);
}

}  // extern "C"

// Local docking, backward: the adjoint of dlpd_local_correlate (dlpd_local.h) -- what lets the reference's LocalTrainer
// (src/Training/LocalTrainer.py:81-144) push a gradient through MultiplyVolumes (src/Models/MultiplyVolumes.py:13-60).
//
//   corr[p,c,d]  = sum_x rec[c, x + tau_p + d] lig'_p[c, x]                        (the forward; tau_p = coarse(T_p))
//   grec[p,c,X]  = sum_d g[p,c,d] lig'_p[c, X - tau_p - d]                          (terms that leave the box are 0)
//   glig[p,c,x]  = sum_d g[p,c,d] rec[c, x + tau_p + d]
//
// Both are ONE stencil, out[q] = sum_e g[s e] src[q + s tau + e], e in [-r, r]^3: s = +1 with src = rec for glig, s = -1 with
// src = lig' for grec.  k_local_corr_grad computes one of them per launch, in the family of k_local_corr: 256 threads = XT
// x-planes x L lanes along z (the contiguous axis), a thread owns an (x, z) column and walks y in chunks of YC rows whose sums
// it keeps in registers.  For a column of the window (e_x, e_z) it reads the YC + 2r source rows once; every value loaded
// feeds the W = 2r + 1 outputs along y it belongs to.  The W^3 coefficients of (pose, channel) are block-uniform: they sit in
// LDS and are read at one address by all lanes.  With R the source is the trilinear_fetch sample of the forward, recomputed:
// no rotated volume is stored.
//
// A per-pose stride of 0 on the volume whose gradient is asked for means ONE volume for all poses: its gradient is (C, L^3),
// the sum over the poses, added in pose order inside the block (one block per (channel, slab), looping over p for every chunk
// of rows).  No float atomics, no workspace: every output voxel is written exactly once (zeros included), and the order of
// the additions is fixed -- poses ascending; within a pose e_x, then e_z, then e_y ascending -- so results are the same bits
// run to run.  At r = 0 the kernel is a scaled, shifted copy: one volume read, one written per gradient.
#pragma once
#include "dlpd_local.h"

#define DLPD_LOCAL_GRAD_YC 16        // output rows a thread holds in registers at a time

// grid (NO * C * nxb), NO = P (out_pstride != 0: a gradient per pose) or 1 (one gradient, summed over the P poses); block 256.
// off (P, 3) or null (ROT only): the per-pose offset of the sample position, as k_local_corr takes it.
// g (P, C, W^3); sgn = +1: out[q] = sum_d g[d] src[q + tau + d]; sgn = -1: out[q] = sum_d g[d] src[q - tau - d].
template <int R, bool ROT> __global__ void __launch_bounds__(256)
k_local_corr_grad(const float* __restrict__ src, const float* __restrict__ Rm, const float* __restrict__ off,
                  const int* __restrict__ T,
                  const float* __restrict__ g, float* __restrict__ out, int P, int C, int L, int XT, int nxb,
                  long long src_pstride, long long out_pstride, float c0, int scale, int mode, int sgn) {
  constexpr int W = 2 * R + 1, W3 = W * W * W, YC = DLPD_LOCAL_GRAD_YC, NJ = YC + 2 * R;
  __shared__ float sg[W3];
  const int tid = threadIdx.x;
  const int xb = blockIdx.x % nxb, oc = blockIdx.x / nxb, c = oc % C, po = oc / C;
  const int xl = tid / L, z = tid - xl * L, x = xb * XT + xl;
  const bool active = (xl < XT) & (x < L);
  const int p_beg = out_pstride ? po : 0, p_end = out_pstride ? po + 1 : P;
  const bool many = p_end - p_beg > 1;
  const size_t L3 = (size_t)L * L * L;
  float* outv = out + (size_t)po * out_pstride + (size_t)c * L3;
  for (int y0 = 0; y0 < L; y0 += YC) {
    float acc[YC];
#pragma unroll
    for (int o = 0; o < YC; o++) acc[o] = 0.f;
    for (int p = p_beg; p < p_end; p++) {
      if (many || y0 == 0) {                       // (block-uniform) this pose's coefficients; one pose: loaded once
        __syncthreads();
        for (int a = tid; a < W3; a += 256) sg[a] = g[((size_t)p * C + c) * W3 + a];
        __syncthreads();
      }
      if (!active) continue;
      const int tx = sgn * local_coarse(T[3 * p + 0], scale, mode), ty = sgn * local_coarse(T[3 * p + 1], scale, mode),
                tz = sgn * local_coarse(T[3 * p + 2], scale, mode);
      const float* srcv = src + (size_t)p * src_pstride + (size_t)c * L3;
      float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
      if (ROT)
        for (int i = 0; i < 9; i++) m[i] = Rm[(size_t)p * 9 + i];
      const float cx = (ROT && off) ? c0 + off[(size_t)p * 3 + 0] : c0, cy = (ROT && off) ? c0 + off[(size_t)p * 3 + 1] : c0,
                  cz = (ROT && off) ? c0 + off[(size_t)p * 3 + 2] : c0;
      const int ys0 = y0 + ty - R;                 // source row of j = 0; row j feeds the outputs o = j - i, i = e_y + R
      if (ys0 >= L || ys0 + NJ <= 0) continue;     // (block-uniform) no source row of this chunk is in the box
#pragma unroll 1
      for (int ex = -R; ex <= R; ex++) {
        const int X = x + tx + ex;
        if (X < 0 || X >= L) continue;
#pragma unroll 1
        for (int ez = -R; ez <= R; ez++) {
          const int Z = z + tz + ez;
          if (Z < 0 || Z >= L) continue;
          float gy[W];
#pragma unroll
          for (int i = 0; i < W; i++) gy[i] = sg[((sgn * ex + R) * W + (sgn * (i - R) + R)) * W + (sgn * ez + R)];
          const float dx = X - c0, dz = Z - c0;
#pragma unroll
          for (int j = 0; j < NJ; j++) {
            const int ys = ys0 + j;
            if (ys < 0 || ys >= L) continue;       // (block-uniform)
            float v;
            if (ROT) {
              const float dy = ys - c0;
              const float px = cx + (m[0] * dx + m[3] * dy + m[6] * dz);
              const float py = cy + (m[1] * dx + m[4] * dy + m[7] * dz);
              const float pz = cz + (m[2] * dx + m[5] * dy + m[8] * dz);
              v = trilinear_fetch(srcv, L, px, py, pz);
            } else {
              v = srcv[((size_t)X * L + ys) * L + Z];
            }
#pragma unroll
            for (int i = 0; i < W; i++)
              if (j - i >= 0 && j - i < YC) acc[j - i] = fmaf(gy[i], v, acc[j - i]);
          }
        }
      }
    }
    if (active) {
#pragma unroll
      for (int o = 0; o < YC; o++)
        if (y0 + o < L) outv[((size_t)x * L + y0 + o) * L + z] = acc[o];
    }
  }
}

template <int R>
static void local_grad_launch(const float* src, const float* Rm, const float* off, const int* T, const float* g, float* out, int P, int C, int L,
                              long long src_pstride, long long out_pstride, float c0, int scale, int mode, int sgn,
                              hipStream_t st) {
  const int XT = local_xt(L), nxb = local_nxb(L);
  const dim3 grid((unsigned)((size_t)(out_pstride ? P : 1) * C * nxb));
  if (Rm) {
    DLPD_LAUNCH((k_local_corr_grad<R, true>), grid, dim3(256), 0, st, src, Rm, off, T, g, out, P, C, L, XT, nxb, src_pstride,
                out_pstride, c0, scale, mode, sgn);
  } else {
    DLPD_LAUNCH((k_local_corr_grad<R, false>), grid, dim3(256), 0, st, src, Rm, off, T, g, out, P, C, L, XT, nxb, src_pstride,
                out_pstride, c0, scale, mode, sgn);
  }
}

static void local_grad_dispatch(int r, const float* src, const float* Rm, const float* off, const int* T, const float* g, float* out, int P, int C,
                                int L, long long src_pstride, long long out_pstride, float c0, int scale, int mode, int sgn,
                                hipStream_t st) {
  switch (r) {
    case 0: local_grad_launch<0>(src, Rm, off, T, g, out, P, C, L, src_pstride, out_pstride, c0, scale, mode, sgn, st); break;
    case 1: local_grad_launch<1>(src, Rm, off, T, g, out, P, C, L, src_pstride, out_pstride, c0, scale, mode, sgn, st); break;
    case 2: local_grad_launch<2>(src, Rm, off, T, g, out, P, C, L, src_pstride, out_pstride, c0, scale, mode, sgn, st); break;
    default: local_grad_launch<3>(src, Rm, off, T, g, out, P, C, L, src_pstride, out_pstride, c0, scale, mode, sgn, st); break;
  }
}

// the body of dlpd_local_correlate_grad and, with `off`, of dlpd_local_correlate_shift_grad (dlpd_rotate_shift.h)
static int local_correlate_grad_run(const float* rec, const float* lig, const float* R, const float* off, const int* T,
                                    const float* gcorr, float* grec, float* glig, int P, int C, int L, int r, int scale,
                                    int coarse_mode, float center, long long rec_pstride, long long lig_pstride, void* stream) {
  if (off && !R) return DLPD_ERR_ARG;
  if (!rec || !lig || !T || !gcorr || (!grec && !glig) || P <= 0 || C <= 0 || scale < 1 || rec_pstride < 0 || lig_pstride < 0 ||
      (coarse_mode != 0 && coarse_mode != 1))
    return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL || r < 0 || r > DLPD_LOCAL_MAXR) return DLPD_ERR_UNSUPPORTED;
  // the ligand's gradient through the rotation is the scatter adjoint of the trilinear gather: not built
  if (glig && R) return DLPD_ERR_UNSUPPORTED;
  // a gradient per pose is one block per (pose, channel, slab), as the forward: the same limit of a launch
  if (((grec && rec_pstride) || (glig && lig_pstride)) && P > dlpd_local_max_poses(C, L)) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  if (grec) local_grad_dispatch(r, lig, R, off, T, gcorr, grec, P, C, L, lig_pstride, rec_pstride, center, scale, coarse_mode, -1, st);
  if (glig) local_grad_dispatch(r, rec, nullptr, nullptr, T, gcorr, glig, P, C, L, rec_pstride, lig_pstride, center, scale, coarse_mode, 1, st);
  return dlpd_check_launch();
}

extern "C" {

// rec, lig, R, T, strides, scale, coarse_mode, center: as dlpd_local_correlate took them; gcorr (P, C, W^3) the incoming
// gradient.  grec / glig: the gradients, laid out as rec / lig are -- (P, C, L^3) with the volume's own per-pose stride, or
// (C, L^3), the sum over the poses, for stride 0; either may be null (not wanted).  Every element is written.
int dlpd_local_correlate_grad(const float* rec, const float* lig, const float* R, const int* T, const float* gcorr, float* grec,
                              float* glig, int P, int C, int L, int r, int scale, int coarse_mode, float center,
                              long long rec_pstride, long long lig_pstride, void* stream) {
  return local_correlate_grad_run(rec, lig, R, nullptr, T, gcorr, grec, glig, P, C, L, r, scale, coarse_mode, center, rec_pstride,
                                  lig_pstride, stream);
}

}  // extern "C"

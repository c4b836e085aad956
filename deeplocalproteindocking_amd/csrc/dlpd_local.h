// Local docking: the per-channel correlation of the receptor with a ligand under an ARBITRARY rotation at a HANDFUL of
// translations, by direct summation (no transform) -- what scores given poses and refines the search's top list.
//
// Reference path (file:line in the reference tree):
//   src/Models/MultiplyVolumes.py:13-60    MultiplyVolumes.multiply / forward: the slices and the int() of the translation
//   src/Models/DockingModels.py:102-120    LocalDockingModel.forward: per-resolution rescale of T, concat, filter
//   src/Training/LocalTrainer.py:146-177   LocalTrainer.score, the caller
//   src/Docker/Docker.py:218,225-232       rotation, clash mask and mask multiply of the search these scores must agree with
//
//   lig'         = trilinear rotation of lig by the pose's matrix (dlpd_rotate_trilinear's definition; R null: lig itself)
//   corr[p,c,d]  = sum_x rec[c, x + tau] lig'[c, x],  tau = coarse(T_p) + d,  d in [-r, r]^3, 0 where x + tau leaves the box
//   coarse(t)    = floor(t / scale) (mode 0: the global search's index // scale on the wrapped grid) or trunc(t / scale)
//                  (mode 1: Python's int(), MultiplyVolumes.py:56-58)
//
// k_local_corr: one block per (pose, channel, slab of XT x-planes), 256 threads = XT planes x L lanes along z (the contiguous
// axis: the receptor rows are read coalesced).  A thread walks its (x, z) column along y; the rotated ligand sample is
// gathered from the NATURAL layout straight into a register window of W = 2r + 1 values (never to memory, not even LDS: the
// only consumer of a sample is the thread that gathered it), and every receptor value loaded feeds W multiply-adds
// (acc[dx][dy][dz] += rec(x + tx + dx, yr, z + tz + dz) * lig'(x, yr - ty - dy, z)).  Natural layout and not the
// channels-last copy of K1: the accumulators are per channel (W^3 of them per thread), a thread that took 16 channels of a
// sample at once would need 16 W^3.  r = 3 (343 accumulators) is split over dx: one dx per block (grid.y), 49 accumulators.
// Block partials go to a workspace; k_local_reduce adds them in slab order: no float atomics, the results are the same bits
// run to run.
#pragma once
#include <dlpd_platform.h>
#include "dlpd_internal.h"
#include "dlpd_trilinear.h"

#define DLPD_LOCAL_MAXR 3
#define DLPD_LOCAL_MAXL 128

extern "C" int dlpd_hidden_pad(int H);

DLPD_HD int local_coarse(int t, int s, int mode) {
  if (s <= 1) return t;
  if (mode == 0) return t >= 0 ? t / s : -((-t + s - 1) / s);
  return t / s;                                   // C division truncates, as int() does
}
static inline int local_xt(int L) { return L >= 256 ? 1 : (256 / L < L ? 256 / L : L); }   // x-planes per block
static inline int local_nxb(int L) { const int xt = local_xt(L); return (L + xt - 1) / xt; }

// grid (P * C * nxb, W / NDX), block 256.  part (P, C, nxb, W^3).  off (P, 3) or null: the per-pose offset of the ligand's
// sample position (dlpd_rotate_shift.h), added to the pivot before the rotated term -- null or zeros: the plain position's bits.
template <int R, int NDX> __global__ void __launch_bounds__(256)
k_local_corr(const float* __restrict__ rec, const float* __restrict__ lig, const float* __restrict__ Rm,
             const float* __restrict__ off, const int* __restrict__ T, float* __restrict__ part, int C, int L, int XT, int nxb, long long rec_pstride,
             long long lig_pstride, float c0, int scale, int mode) {
  constexpr int W = 2 * R + 1, NACC = NDX * W * W, W3 = W * W * W;
  __shared__ float sm[4 * NACC];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int xb = blockIdx.x % nxb, pc = blockIdx.x / nxb, c = pc % C, p = pc / C;
  const int xl = tid / L, z = tid - xl * L, x = xb * XT + xl;
  const bool active = (xl < XT) & (x < L);
  const int tx = local_coarse(T[3 * p + 0], scale, mode), ty = local_coarse(T[3 * p + 1], scale, mode),
            tz = local_coarse(T[3 * p + 2], scale, mode);
  const size_t L3 = (size_t)L * L * L;
  const float* recv = rec + (size_t)p * rec_pstride + (size_t)c * L3;
  const float* ligv = lig + (size_t)p * lig_pstride + (size_t)c * L3;
  const int j0 = blockIdx.y * NDX;                 // first dx of this block, as an index into the window
  float acc[NACC];
#pragma unroll
  for (int a = 0; a < NACC; a++) acc[a] = 0.f;
  if (active) {
    int rowx[NDX], colz[W];
    bool xok[NDX], zok[W];
#pragma unroll
    for (int j = 0; j < NDX; j++) {
      const int X = x + tx + j0 + j - R;
      xok[j] = (X >= 0) & (X < L);
      rowx[j] = min(max(X, 0), L - 1) * L;
    }
#pragma unroll
    for (int k = 0; k < W; k++) {
      const int Z = z + tz + k - R;
      zok[k] = (Z >= 0) & (Z < L);
      colz[k] = min(max(Z, 0), L - 1);
    }
    float m[9] = {1.f, 0.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f, 1.f};
    if (Rm)
      for (int i = 0; i < 9; i++) m[i] = Rm[(size_t)p * 9 + i];
    const float dx = x - c0, dz = z - c0;
    const float cx = (Rm && off) ? c0 + off[(size_t)p * 3 + 0] : c0, cy = (Rm && off) ? c0 + off[(size_t)p * 3 + 1] : c0,
                cz = (Rm && off) ? c0 + off[(size_t)p * 3 + 2] : c0;
    float win[W];
#pragma unroll
    for (int i = 0; i < W; i++) win[i] = 0.f;
    // s = receptor row - ty: the ligand rows s + r .. s - r pair with it
    const int s_lo = max(-R, -ty), s_hi = min(L + R, L - ty);     // rows of the receptor inside the box
    for (int s = max(s_lo - 2 * R, -R); s < s_hi; s++) {
#pragma unroll
      for (int i = W - 1; i > 0; i--) win[i] = win[i - 1];
      const int yl = s + R;
      float v = 0.f;
      if (yl < L) {
        if (Rm) {
          const float dy = yl - c0;
          const float px = cx + (m[0] * dx + m[3] * dy + m[6] * dz);
          const float py = cy + (m[1] * dx + m[4] * dy + m[7] * dz);
          const float pz = cz + (m[2] * dx + m[5] * dy + m[8] * dz);
          v = trilinear_fetch(ligv, L, px, py, pz);
        } else {
          v = ligv[((size_t)x * L + yl) * L + z];
        }
      }
      win[0] = v;
      const int yr = s + ty;
      if (yr < 0 || yr >= L) continue;             // (block-uniform) the window keeps sliding
#pragma unroll
      for (int j = 0; j < NDX; j++) {
#pragma unroll
        for (int k = 0; k < W; k++) {
          const float rv = (xok[j] & zok[k]) ? recv[(size_t)(rowx[j] + yr) * L + colz[k]] : 0.f;
#pragma unroll
          for (int i = 0; i < W; i++) acc[(j * W + i) * W + k] = fmaf(rv, win[i], acc[(j * W + i) * W + k]);
        }
      }
    }
  }
  // block sum in a fixed order: lanes by halving, then the four waves one after the other
#pragma unroll
  for (int a = 0; a < NACC; a++) {
    float v = acc[a];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off);
    if (lane == 0) sm[wave * NACC + a] = v;
  }
  __syncthreads();
  float* dst = part + ((size_t)pc * nxb + xb) * W3 + (size_t)j0 * W * W;
  for (int a = tid; a < NACC; a += 256) dst[a] = ((sm[a] + sm[NACC + a]) + sm[2 * NACC + a]) + sm[3 * NACC + a];
}

// corr (P * C, W^3) = the slabs' partial sums added in slab order
__global__ void __launch_bounds__(256) k_local_reduce(const float* __restrict__ part, float* __restrict__ corr, size_t npc,
                                                      int nxb, int W3) {
  const size_t total = npc * W3;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const size_t pc = i / W3;
    const int w = (int)(i - pc * W3);
    const float* src = part + pc * nxb * W3 + w;
    float v = 0.f;
    for (int b = 0; b < nxb; b++) v += src[(size_t)b * W3];
    corr[i] = v;
  }
}

// One wave per pose: clamp, coarse index by the chosen convention, MLP, clash mask -> score (P, W^3); per pose the minimum
// and its flat window index (lowest index wins a tie, as torch.min does in Docker.update_top).
//   corr0 (P, C0, W^3) fine grid; corr1 (P, C1, Wc^3), Wc = 2 rc + 1, rc = (r + 1) / 2 (scale 2) or r (scale 1), centred at
//   coarse(T_p), or null
//   clash (P, W^3) correlation of the forbidden volumes, or null
__global__ void __launch_bounds__(64)
k_local_filter(const float* __restrict__ corr0, int C0, const float* __restrict__ corr1, int C1, const float* __restrict__ clash,
               const int* __restrict__ T, int r, int scale, int mode, const float* __restrict__ W1t,
               const float* __restrict__ b1, const float* __restrict__ W2, float b2, int HP, int has_clip, float clip, float thr,
               float* __restrict__ score, float* __restrict__ best_score, int* __restrict__ best_index) {
  const int p = blockIdx.x, lane = threadIdx.x;
  const int W = 2 * r + 1, W3 = W * W * W, rc = scale == 1 ? r : (r + 1) / 2, Wc = 2 * rc + 1, Wc3 = Wc * Wc * Wc;
  const int t0 = T[3 * p], t1 = T[3 * p + 1], t2 = T[3 * p + 2];
  float bv = 0.f;
  int bi = 0x7fffffff;
  for (int d0 = 0; d0 < W3; d0 += 64) {
    const int d = d0 + lane;
    if (d < W3) {
      float hid[32];
#pragma unroll
      for (int j = 0; j < 32; j++) hid[j] = j < HP ? b1[j] : 0.f;
      for (int c = 0; c < C0; c++) {
        float v = corr0[((size_t)p * C0 + c) * W3 + d];
        if (has_clip) v = DLPD_CLAMP(v, clip);
#pragma unroll
        for (int j = 0; j < 32; j++)
          if (j < HP) hid[j] = fmaf(W1t[(size_t)c * HP + j], v, hid[j]);
      }
      if (C1 > 0) {
        const int dz = d % W - r, dy = (d / W) % W - r, dx = d / (W * W) - r;
        // 0 <= k < Wc for either convention (scale 1 or 2); clamped all the same: an index never leaves the pose's window
        const int k0 = min(max(local_coarse(t0 + dx, scale, mode) - local_coarse(t0, scale, mode) + rc, 0), Wc - 1);
        const int k1 = min(max(local_coarse(t1 + dy, scale, mode) - local_coarse(t1, scale, mode) + rc, 0), Wc - 1);
        const int k2 = min(max(local_coarse(t2 + dz, scale, mode) - local_coarse(t2, scale, mode) + rc, 0), Wc - 1);
        const int d1 = (k0 * Wc + k1) * Wc + k2;
        for (int c = 0; c < C1; c++) {
          float v = corr1[((size_t)p * C1 + c) * Wc3 + d1];
          if (has_clip) v = DLPD_CLAMP(v, clip);
#pragma unroll
          for (int j = 0; j < 32; j++)
            if (j < HP) hid[j] = fmaf(W1t[(size_t)(C0 + c) * HP + j], v, hid[j]);
        }
      }
      float a = b2;
#pragma unroll
      for (int j = 0; j < 32; j++)
        if (j < HP) a = fmaf(W2[j], fmaxf(hid[j], 0.f), a);
      if (clash) a = a * ((clash[(size_t)p * W3 + d] < thr) ? 1.0f : 0.0f);
      score[(size_t)p * W3 + d] = a;
      if (bi == 0x7fffffff || a < bv) { bv = a; bi = d; }
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    const float ov = __shfl_down(bv, off);
    const int oi = __shfl_down(bi, off);
    if (oi != 0x7fffffff && (bi == 0x7fffffff || ov < bv || (ov == bv && oi < bi))) { bv = ov; bi = oi; }
  }
  if (lane == 0) {
    if (best_score) best_score[p] = bv;
    if (best_index) best_index[p] = bi;
  }
}

template <int R, int NDX>
static int local_corr_launch(const float* rec, const float* lig, const float* Rm, const float* off, const int* T, float* part, int P, int C, int L,
                             long long rec_pstride, long long lig_pstride, float c0, int scale, int mode, hipStream_t st) {
  const int XT = local_xt(L), nxb = local_nxb(L);
  DLPD_LAUNCH((k_local_corr<R, NDX>), dim3((unsigned)((size_t)P * C * nxb), (unsigned)((2 * R + 1) / NDX)), dim3(256), 0, st, rec,
              lig, Rm, off, T, part, C, L, XT, nxb, rec_pstride, lig_pstride, c0, scale, mode);
  return DLPD_OK;
}

extern "C" int dlpd_local_max_poses(int C, int L);

// the body of dlpd_local_correlate and, with `off`, of dlpd_local_correlate_shift (dlpd_rotate_shift.h)
static int local_correlate_run(const float* rec, const float* lig, const float* R, const float* off, const int* T, float* corr,
                               void* ws, int P, int C, int L, int r, int scale, int coarse_mode, float center,
                               long long rec_pstride, long long lig_pstride, void* stream) {
  if (off && !R) return DLPD_ERR_ARG;              // an offset belongs to a rotated sample
  if (!rec || !lig || !T || !corr || !ws || P <= 0 || C <= 0 || scale < 1 || rec_pstride < 0 || lig_pstride < 0 ||
      (coarse_mode != 0 && coarse_mode != 1))
    return DLPD_ERR_ARG;
  if (L < 2 || L > DLPD_LOCAL_MAXL || r < 0 || r > DLPD_LOCAL_MAXR) return DLPD_ERR_UNSUPPORTED;
  // a launch may not exceed 2^32 - 1 threads: 256 per block -> 2^24 - 1 blocks (dlpd_local_max_poses; the caller batches)
  if (P > dlpd_local_max_poses(C, L)) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  float* part = (float*)ws;
  switch (r) {
    case 0: local_corr_launch<0, 1>(rec, lig, R, off, T, part, P, C, L, rec_pstride, lig_pstride, center, scale, coarse_mode, st); break;
    case 1: local_corr_launch<1, 3>(rec, lig, R, off, T, part, P, C, L, rec_pstride, lig_pstride, center, scale, coarse_mode, st); break;
    case 2: local_corr_launch<2, 5>(rec, lig, R, off, T, part, P, C, L, rec_pstride, lig_pstride, center, scale, coarse_mode, st); break;
    default: local_corr_launch<3, 1>(rec, lig, R, off, T, part, P, C, L, rec_pstride, lig_pstride, center, scale, coarse_mode, st); break;
  }
  const int W = 2 * r + 1, W3 = W * W * W;
  const size_t total = (size_t)P * C * W3;
  size_t nblk = (total + 255) / 256;
  if (nblk > 65536) nblk = 65536;
  DLPD_LAUNCH(k_local_reduce, dim3((unsigned)nblk), dim3(256), 0, st, (const float*)part, corr, (size_t)P * C, local_nxb(L), W3);
  return dlpd_check_launch();
}

extern "C" {

// bytes of workspace dlpd_local_correlate needs: the slabs' partial sums
size_t dlpd_local_ws_bytes(int P, int C, int L, int r) {
  if (P <= 0 || C <= 0 || L < 2 || L > DLPD_LOCAL_MAXL || r < 0 || r > DLPD_LOCAL_MAXR) return 0;
  const size_t W = 2 * (size_t)r + 1;
  return (size_t)P * C * local_nxb(L) * W * W * W * sizeof(float);
}

// poses one dlpd_local_correlate call takes at most for C volumes of edge L (the grid limit of a launch); 0: unsupported shape
int dlpd_local_max_poses(int C, int L) {
  if (C <= 0 || L < 2 || L > DLPD_LOCAL_MAXL) return 0;
  const size_t per = (size_t)C * local_nxb(L), most = (0xffffffffull / 256) / per;
  return (int)(most > 0x7fffffffull ? 0x7fffffffull : most);
}

// rec, lig (C, L^3) f32 with per-pose strides rec_pstride / lig_pstride floats (0: one volume set for every pose);
// R (P, 9) matrices as dlpd_rotate_trilinear takes them, or null (the ligand as it is); T (P, 3) int32 signed translations
// on the grid of `scale` x L voxels; corr (P, C, W^3), W = 2r + 1, window centred at coarse(T_p)
int dlpd_local_correlate(const float* rec, const float* lig, const float* R, const int* T, float* corr, void* ws, int P, int C,
                         int L, int r, int scale, int coarse_mode, float center, long long rec_pstride, long long lig_pstride,
                         void* stream) {
  return local_correlate_run(rec, lig, R, nullptr, T, corr, ws, P, C, L, r, scale, coarse_mode, center, rec_pstride, lig_pstride,
                             stream);
}

// score (P, W^3) [+ best_score (P), best_index (P) int32, either may be null]; T (P, 3) on the FINE grid, scale = fine edge /
// coarse edge (1 or 2; ignored without corr1).  Hidden widths as dlpd_hidden_pad allows; wider: DLPD_ERR_UNSUPPORTED.
int dlpd_local_filter(const float* corr0, int C0, const float* corr1, int C1, const float* clash, const int* T, int P, int r,
                      int scale, int coarse_mode, const float* W1t, const float* b1, const float* W2, float b2, int HP,
                      int has_clip, float clip, float thr, float* score, float* best_score, int* best_index, void* stream) {
  if (!corr0 || !T || !W1t || !b1 || !W2 || !score || P <= 0 || C0 <= 0 || C1 < 0 || (C1 > 0 && !corr1) ||
      (coarse_mode != 0 && coarse_mode != 1))
    return DLPD_ERR_ARG;
  if (r < 0 || r > DLPD_LOCAL_MAXR || HP <= 0 || HP > 32 || dlpd_hidden_pad(HP) != HP || (C1 > 0 && scale != 1 && scale != 2))
    return DLPD_ERR_UNSUPPORTED;
  DLPD_LAUNCH(k_local_filter, dim3((unsigned)P), dim3(64), 0, (hipStream_t)stream, corr0, C0, corr1, C1, clash, T, r, scale,
              coarse_mode, W1t, b1, W2, b2, HP, has_clip, clip, thr, score, best_score, best_index);
  return dlpd_check_launch();
}

}  // extern "C"

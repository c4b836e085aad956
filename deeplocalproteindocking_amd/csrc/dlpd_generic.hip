// Circular cross-correlation on the 2L zero-padded grid for ANY box size L (the reference's `box_size` is a free
// constructor argument, /root/reference/src/Docker/Docker.py:18,22-24,31): the stand-alone VolumeConvolution op
// (Docker.py:32,225; DockingModels.py:48,71) where the fused pipeline has no compiled plan (L other than 32 / 40 / 64 / 80).
//
//     out[v][t mod N] = sum_r v1[v][r + t] v2[v][r],  N = 2L        (semantics: src/Models/MultiplyVolumes.py:13-47)
//     = IDFT3( DFT3(pad v1) . conj(DFT3(pad v2)) ) / N^3
//
// A correctness path, not a tuned one: every 1-D transform is a direct O(n N) sum from an LDS-resident tile (any length,
// no radix plan), pruned to the L non-zero inputs on the way in.  3 N^4 complex multiply-adds per volume for the inverse
// (~5e9 at box 100): tens of milliseconds per rotation of a 48-channel pair, against ~0.4 ms on the compiled plans.
#include <dlpd_platform.h>
#include "dlpd_fft.h"
#include "dlpd_internal.h"
#include "dlpd_local.h"                 // local docking: direct correlation at given poses (any box size, no plan)
#include "dlpd_local_grad.h"            // ... and its adjoint (the receptor's and the ligand's gradient)
#include "dlpd_rotate_grad.h"           // ... and the adjoint of the rotation (the ligand's gradient through the poses)
#include "dlpd_rotate_rgrad.h"          // ... and the rotation's gradient with respect to its matrix (the poses' own gradient)
#include "dlpd_rotate_shift.h"          // ... and all of them with a per-pose offset of the sample position (sub-voxel translations)
#include "dlpd_corr_grad.h"             // the adjoint of VolumeConvolution itself (compiled boxes; the plan-free one is below)
#include "dlpd_filter_grad.h"           // the adjoint of the per-voxel filter over the correlations (global training)

#define GEN_MAXN 256                      // box sizes up to 128 (tile: n_in x 64 complex <= 128 KB)
#define GEN_NACC 4                        // partial sums per output of a direct transform (the final adds are written for 4)

// transform along a MIDDLE axis: in (outer, n_in, inner) -> out (outer, N, inner), inner contiguous;
// out[o][k][i] = sum_j in[o][j][i] exp(dir 2 pi i j k / N).  grid (ceil(inner / 64), outer), block 256 = 64 columns x 4
// groups of output rows; each thread takes its column for four consecutive k at a time.
__global__ void __launch_bounds__(256) k_gdft_mid(const cplx* __restrict__ in, cplx* __restrict__ out, int n_in, int N,
                                                  long long inner, int dir) {
  DLPD_DYN_SHARED(cplx, S);
  cplx* tile = S;                         // [n_in][64]
  cplx* tw = S + (size_t)n_in * 64;       // exp(dir 2 pi i k / N)
  const int tid = threadIdx.x, c = tid & 63, g = tid >> 6;
  const long long i0 = (long long)blockIdx.x * 64, o = blockIdx.y;
  for (int k = tid; k < N; k += 256) {
    double s, co;
    sincospi(2.0 * (double)k / (double)N, &s, &co);
    tw[k] = c_make((float)co, (float)(dir * s));
  }
  const cplx* src = in + (size_t)o * n_in * inner;
  for (int e = tid; e < n_in * 64; e += 256) {
    const int j = e >> 6, cc = e & 63;
    tile[e] = (i0 + cc < inner) ? src[(size_t)j * inner + i0 + cc] : c_make(0.f, 0.f);
  }
  __syncthreads();
  if (i0 + c >= inner) return;
  cplx* dst = out + (size_t)o * N * inner + i0 + c;
  for (int k0 = 4 * g; k0 < N; k0 += 16) {
    // GEN_NACC partial sums per output, term j into sum j mod GEN_NACC, added pairwise at the end: where the terms are in
    // phase (the peak of an impulse's correlation) a single running sum grows like j and its rounding error like n^1.5 eps;
    // split, each sum is a quarter as long and the error of the total a quarter as large (half, for terms of random phase)
    float ar[GEN_NACC][4], ai[GEN_NACC][4];
#pragma unroll
    for (int a = 0; a < GEN_NACC; a++)
#pragma unroll
      for (int u = 0; u < 4; u++) ar[a][u] = ai[a][u] = 0.f;
    int idx[4] = {0, 0, 0, 0};
    for (int j0 = 0; j0 < n_in; j0 += GEN_NACC) {
#pragma unroll
      for (int a = 0; a < GEN_NACC; a++) {
        if (j0 + a >= n_in) break;
        const cplx v = tile[(j0 + a) * 64 + c];
#pragma unroll
        for (int u = 0; u < 4; u++) {
          const cplx w = tw[idx[u]];
          ar[a][u] = fmaf(v.x, w.x, fmaf(-v.y, w.y, ar[a][u]));
          ai[a][u] = fmaf(v.x, w.y, fmaf(v.y, w.x, ai[a][u]));
          // (j k) mod N, incrementally.  The step is reduced mod N first: for an odd box N = 2L is not a multiple of 4
          // and the lanes k0 + u >= N of the last round (their results are discarded below) would otherwise walk idx past
          // the table -- a read beyond the LDS allocation (harmless zeros on the GPU, a heap over-read in the emulator)
          idx[u] += (k0 + u < N) ? (k0 + u) : (k0 + u - N);
          if (idx[u] >= N) idx[u] -= N;
        }
      }
    }
#pragma unroll
    for (int u = 0; u < 4; u++)
      if (k0 + u < N)
        dst[(size_t)(k0 + u) * inner] = c_make((ar[0][u] + ar[1][u]) + (ar[2][u] + ar[3][u]), (ai[0][u] + ai[1][u]) + (ai[2][u] + ai[3][u]));
  }
}

// transform along the LAST (contiguous) axis of P pencils: in (P, n_in) real or complex -> out (P, N) complex, or real
// (the real part times `scale`, clamped to +-clip if has_clip).  grid ceil(P / 16), block 256 = 16 pencils x 16 lanes.
__global__ void __launch_bounds__(256) k_gdft_last(const void* __restrict__ in, void* __restrict__ out, long long P,
                                                   int n_in, int N, int dir, int in_real, int out_real, float scale,
                                                   int has_clip, float clip) {
  DLPD_DYN_SHARED(cplx, S);
  const int RSL = n_in + 1;
  cplx* tile = S;                         // [16][n_in + 1]
  cplx* tw = S + 16 * RSL;
  const int tid = threadIdx.x, p = tid >> 4, kl = tid & 15;
  const long long p0 = (long long)blockIdx.x * 16;
  for (int k = tid; k < N; k += 256) {
    double s, co;
    sincospi(2.0 * (double)k / (double)N, &s, &co);
    tw[k] = c_make((float)co, (float)(dir * s));
  }
  for (int e = tid; e < 16 * n_in; e += 256) {
    const int pp = e / n_in, j = e % n_in;
    cplx v = c_make(0.f, 0.f);
    if (p0 + pp < P) {
      if (in_real) v.x = reinterpret_cast<const float*>(in)[(size_t)(p0 + pp) * n_in + j];
      else v = reinterpret_cast<const cplx*>(in)[(size_t)(p0 + pp) * n_in + j];
    }
    tile[pp * RSL + j] = v;
  }
  __syncthreads();
  if (p0 + p >= P) return;
  for (int k = kl; k < N; k += 16) {
    float pr[GEN_NACC], pi[GEN_NACC];              // partial sums, as in k_gdft_mid
#pragma unroll
    for (int a = 0; a < GEN_NACC; a++) pr[a] = pi[a] = 0.f;
    int idx = 0;
    for (int j0 = 0; j0 < n_in; j0 += GEN_NACC) {
#pragma unroll
      for (int a = 0; a < GEN_NACC; a++) {
        if (j0 + a >= n_in) break;
        const cplx v = tile[p * RSL + j0 + a], w = tw[idx];
        pr[a] = fmaf(v.x, w.x, fmaf(-v.y, w.y, pr[a]));
        pi[a] = fmaf(v.x, w.y, fmaf(v.y, w.x, pi[a]));
        idx += k;
        if (idx >= N) idx -= N;
      }
    }
    const float ar = (pr[0] + pr[1]) + (pr[2] + pr[3]), ai = (pi[0] + pi[1]) + (pi[2] + pi[3]);
    if (out_real) {
      float r = ar * scale;
      if (has_clip) r = DLPD_CLAMP(r, clip);
      reinterpret_cast<float*>(out)[(size_t)(p0 + p) * N + k] = r;
    } else {
      reinterpret_cast<cplx*>(out)[(size_t)(p0 + p) * N + k] = c_make(ar, ai);
    }
  }
}

// a <- a * conj(b)
__global__ void __launch_bounds__(256) k_gmul_conj(cplx* __restrict__ a, const cplx* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] = c_mulc(a[i], b[i]);
}

static int gen_mid(const cplx* in, cplx* out, long long outer, int n_in, int N, long long inner, int dir, hipStream_t st) {
  const size_t shmem = ((size_t)n_in * 64 + N) * sizeof(cplx);
  int rc = dlpd_set_max_dyn_shared((const void*)k_gdft_mid, shmem);
  if (rc) return rc;
  DLPD_LAUNCH(k_gdft_mid, dim3((unsigned)((inner + 63) / 64), (unsigned)outer), dim3(256), shmem, st, in, out, n_in, N, inner, dir);
  return DLPD_OK;
}
static int gen_last(const void* in, void* out, long long P, int n_in, int N, int dir, int in_real, int out_real, float scale,
                    int has_clip, float clip, hipStream_t st) {
  const size_t shmem = ((size_t)16 * (n_in + 1) + N) * sizeof(cplx);
  int rc = dlpd_set_max_dyn_shared((const void*)k_gdft_last, shmem);
  if (rc) return rc;
  DLPD_LAUNCH(k_gdft_last, dim3((unsigned)((P + 15) / 16)), dim3(256), shmem, st, in, out, P, n_in, N, dir, in_real, out_real, scale,
              has_clip, clip);
  return DLPD_OK;
}

extern "C" {

// bytes of workspace dlpd_correlate_generic needs for nvol volume pairs of box L
size_t dlpd_correlate_generic_ws_bytes(int nvol, int L) {
  if (nvol <= 0 || L <= 0) return 0;
  const size_t N = 2 * (size_t)L;
  return (size_t)nvol * (2 * N * N * N + (size_t)L * L * N + (size_t)L * N * N) * sizeof(cplx);
}

int dlpd_generic_box_supported(int L) { return (L >= 1 && 2 * L <= GEN_MAXN) ? 1 : 0; }

// v1, v2 (nvol, L^3) f32 -> out (nvol, N^3) f32, N = 2L, optional clamp to +-clip (VolumeConvolution(clip),
// DockingModels.py:48); ws: dlpd_correlate_generic_ws_bytes(nvol, L) bytes of device scratch.
int dlpd_correlate_generic(const float* v1, const float* v2, float* out, int nvol, int L, int has_clip, float clip, void* ws,
                           void* stream) {
  if (!v1 || !v2 || !out || !ws || nvol <= 0) return DLPD_ERR_ARG;
  if (!dlpd_generic_box_supported(L)) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = 2 * L;
  const size_t N3 = (size_t)N * N * N;
  cplx* P = (cplx*)ws;                    // (nvol, N, N, N)
  cplx* Q = P + (size_t)nvol * N3;
  cplx* T1 = Q + (size_t)nvol * N3;       // (nvol, L, L, N)
  cplx* T2 = T1 + (size_t)nvol * L * L * N;   // (nvol, L, N, N)
  int rc = 0;
  for (int which = 0; which < 2 && !rc; which++) {
    const float* v = which ? v2 : v1;
    cplx* F = which ? Q : P;
    // forward, pruned to the L non-zero inputs: z (real -> complex), y, x
    rc = gen_last(v, T1, (long long)nvol * L * L, L, N, -1, 1, 0, 1.f, 0, 0.f, st);
    if (!rc) rc = gen_mid(T1, T2, (long long)nvol * L, L, N, N, -1, st);
    if (!rc) rc = gen_mid(T2, F, nvol, L, N, (long long)N * N, -1, st);
  }
  if (rc) return rc;
  {
    size_t nblk = ((size_t)nvol * N3 + 255) / 256;
    if (nblk > 65536) nblk = 65536;
    DLPD_LAUNCH(k_gmul_conj, dim3((unsigned)nblk), dim3(256), 0, st, P, (const cplx*)Q, (size_t)nvol * N3);
  }
  // inverse: x, y, z (real part, 1 / N^3, clamp)
  rc = gen_mid(P, Q, nvol, N, N, (long long)N * N, +1, st);
  if (!rc) rc = gen_mid(Q, P, (long long)nvol * N, N, N, N, +1, st);
  if (!rc) rc = gen_last(P, out, (long long)nvol * N * N, N, N, +1, 0, 1, 1.0f / ((float)N * (float)N * (float)N), has_clip, clip, st);
  if (rc) return rc;
  return dlpd_check_launch();
}

// bytes of workspace dlpd_correlate_generic_grad needs for nvol volume pairs of box L
size_t dlpd_correlate_generic_grad_ws_bytes(int nvol, int L) {
  if (nvol <= 0 || !dlpd_generic_box_supported(L)) return 0;
  const size_t N = 2 * (size_t)L;
  return (size_t)nvol * (3 * N * N * N + (size_t)L * L * N + (size_t)L * N * N) * sizeof(cplx);
}

// The adjoint of dlpd_correlate_generic (the backward of VolumeConvolution, DockingModels.py:48,71, on a box without a
// compiled plan): gout (nvol, N^3) f32, v1, v2 (nvol, L^3) f32 -> g1, g2 (nvol, L^3) f32 (csrc/dlpd_corr_grad.h for the
// formulas); a null g1 / g2 skips that gradient.  The same direct transforms: the FULL forward of gout (n_in = N), the
// pruned forward of the other volume, the product (without the conjugate for g1), the full inverse, the L^3 corner.
int dlpd_correlate_generic_grad(const float* gout, const float* v1, const float* v2, float* g1, float* g2, int nvol, int L,
                                void* ws, void* stream) {
  if (!gout || !ws || nvol <= 0 || (!g1 && !g2) || (g1 && !v2) || (g2 && !v1)) return DLPD_ERR_ARG;
  if (!dlpd_generic_box_supported(L)) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int N = 2 * L;
  const size_t N3 = (size_t)N * N * N;
  cplx* A = (cplx*)ws;                    // (nvol, N, N, N): the spectrum of gout
  cplx* B = A + (size_t)nvol * N3;
  cplx* C = B + (size_t)nvol * N3;
  cplx* T1 = C + (size_t)nvol * N3;       // (nvol, L, L, N)
  cplx* T2 = T1 + (size_t)nvol * L * L * N;   // (nvol, L, N, N)
  size_t nblk = ((size_t)nvol * N3 + 255) / 256;
  if (nblk > 65536) nblk = 65536;
  int rc = gen_last(gout, B, (long long)nvol * N * N, N, N, -1, 1, 0, 1.f, 0, 0.f, st);
  if (!rc) rc = gen_mid(B, C, (long long)nvol * N, N, N, N, -1, st);
  if (!rc) rc = gen_mid(C, A, nvol, N, N, (long long)N * N, -1, st);
  for (int which = 0; which < 2 && !rc; which++) {
    float* out = which ? g2 : g1;
    if (!out) continue;
    rc = gen_last(which ? v1 : v2, T1, (long long)nvol * L * L, L, N, -1, 1, 0, 1.f, 0, 0.f, st);
    if (!rc) rc = gen_mid(T1, T2, (long long)nvol * L, L, N, N, -1, st);
    if (!rc) rc = gen_mid(T2, B, nvol, L, N, (long long)N * N, -1, st);
    if (rc) break;
    if (which) DLPD_LAUNCH(k_gmul_conj, dim3((unsigned)nblk), dim3(256), 0, st, B, (const cplx*)A, (size_t)nvol * N3);   // V1 conj(G)
    else DLPD_LAUNCH(k_gmul, dim3((unsigned)nblk), dim3(256), 0, st, B, (const cplx*)A, (size_t)nvol * N3);              // G V2
    rc = gen_mid(B, C, nvol, N, N, (long long)N * N, +1, st);
    if (!rc) rc = gen_mid(C, B, (long long)nvol * N, N, N, N, +1, st);
    float* full = (float*)C;                // (nvol, N, N, N) real: C is free again
    if (!rc) rc = gen_last(B, full, (long long)nvol * N * N, N, N, +1, 0, 1, 1.0f / ((float)N * (float)N * (float)N), 0, 0.f, st);
    if (rc) break;
    const size_t n = (size_t)nvol * L * L * L;
    size_t cblk = (n + 255) / 256;
    if (cblk > 65536) cblk = 65536;
    DLPD_LAUNCH(k_gcorner, dim3((unsigned)cblk), dim3(256), 0, st, (const float*)full, out, L, n);
  }
  if (rc) return rc;
  return dlpd_check_launch();
}

}  // extern "C"

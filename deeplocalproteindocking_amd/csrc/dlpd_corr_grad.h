// Adjoint of VolumeConvolution (DockingModels.py:48,71): the two input gradients of
//
//     out[t mod N] = sum_r v1[r + t] v2[r]  =  IDFT3( V1 . conj(V2) ) / N^3,        N = 2L, v1, v2 zero outside [0, L)^3
//
// for an incoming gradient g over the WHOLE (N, N, N) grid (real, not zero padded), G its R2C spectrum:
//
//     grad_v1[s] = sum_r g[(s - r) mod N] v2[r]  =  IDFT3( G . V2 ) / N^3          kept for s in [0, L)^3
//     grad_v2[r] = sum_s g[(s - r) mod N] v1[s]  =  IDFT3( V1 . conj(G) ) / N^3    kept for r in [0, L)^3
//
// The transpose of the forward pipeline: where K1 / K2 prune their INPUTS to the L non-zero samples and the z inverse writes
// all N, here the forward transform of g is full and the inverses prune their OUTPUTS to the L^3 corner.  Five separable
// passes over LDS tiles of 16 pencils, one code path for N = 64 / 80 / 128 / 160 (the radix plans of dlpd_fft.h), the
// layouts of the forward: volumes [x][y][z], spectra (nvol, NZ = L + 1, N, N) as [kz][kx][ky]:
//
//   (a) k_cg_z_r2c   g (nvol, N, N, N) real          -> G  (nvol, NZ, N, N)   z transform, transposed through LDS
//   (b) k_cg_rows    G                               -> G                     forward along y, in place
//   (c) k_cg_x       G, V2 and / or V1               -> H1, H2 (nvol, NZ, L, N)   forward along x, product, inverse along x, x < L
//   (d) k_cg_rows    H                               -> D  (nvol, NZ, L, L)   inverse along y, y < L
//   (e) k_cg_z_c2r   D                               -> grad (nvol, L, L, L)  Hermitian extension, inverse along z, z < L, 1 / N^3
//
// Every output element is written by exactly one thread from one fixed-order sum: no atomics, the same bits run to run.
// (A slab-resident fusion of (b)-(d) fits the LDS at N <= 128 only; DESIGN.md, "VolumeConvolution backward".)
#pragma once
#include <dlpd_platform.h>
#include "dlpd_fft.h"
#include "dlpd_internal.h"

#define CG_P 16                           // pencils per tile: 16 complex = one 128-byte line across the tile

// both passes of the length-N plan on the tile's CG_P pencils, in place; pencil p of this thread at S + p * ps, element
// stride es, t its index among the T threads of the pencil.  EVERY thread of the block calls it (block = CG_P * T).
template <int N, int DIR> DLPD_D void cg_fft_tile(cplx* P, int es, int t, const cplx* tw) {
  constexpr int T = FftPlan<N>::T, R1 = FftPlan<N>::R1, R2 = FftPlan<N>::R2;
  {
    FftPass<N, R1, 1, DIR, T> ps;
    ps.load(P, es, t, tw);
    __syncthreads();
    ps.store(P, es, t);
    __syncthreads();
  }
  {
    FftPass<N, R2, R1, DIR, T> ps;
    ps.load(P, es, t, tw);
    __syncthreads();
    ps.store(P, es, t);
    __syncthreads();
  }
}

// (a) pencils q = (v, x, y) of N reals, z contiguous -> G[(v NZ + kz) N^2 + x N + y], kz <= L.  grid nvol N^2 / 16.
template <int N> __global__ void __launch_bounds__(CG_P * FftPlan<N>::T)
k_cg_z_r2c(const float* __restrict__ g, cplx* __restrict__ G) {
  constexpr int L = N / 2, NZ = L + 1, RS = N + 1, T = FftPlan<N>::T, NT = CG_P * T;
  __shared__ cplx S[CG_P * RS + N];
  cplx* tw = S + CG_P * RS;
  const int tid = threadIdx.x;
  init_twiddles<N>(tw, tid, NT);
  const size_t q0 = (size_t)blockIdx.x * CG_P;               // N^2 is a multiple of 16: a tile lies in one volume
  const float* src = g + q0 * N;                              // 16 pencils = 16 N consecutive floats
  for (int e = tid; e < CG_P * N; e += NT) S[(e / N) * RS + e % N] = c_make(src[e], 0.f);
  __syncthreads();
  cg_fft_tile<N, -1>(S + (tid / T) * RS, 1, tid % T, tw);
  const size_t v = q0 / ((size_t)N * N), r = q0 % ((size_t)N * N);
  cplx* dst = G + v * NZ * N * N + r;
  for (int e = tid; e < CG_P * NZ; e += NT) {
    const int p = e % CG_P, k = e / CG_P;
    dst[(size_t)k * N * N + p] = S[p * RS + k];
  }
}

// (b), (d) rows of N complex, contiguous: in (rows, N) -> out (rows, n_out), the first n_out outputs of the transform.
// grid ceil(rows / 16); in place when n_out = N (a block reads its 16 rows before it writes them).
template <int N, int DIR> __global__ void __launch_bounds__(CG_P * FftPlan<N>::T)
k_cg_rows(const cplx* in, cplx* out, long long rows, int n_out) {
  constexpr int RS = N + 1, T = FftPlan<N>::T, NT = CG_P * T;
  __shared__ cplx S[CG_P * RS + N];
  cplx* tw = S + CG_P * RS;
  const int tid = threadIdx.x;
  init_twiddles<N>(tw, tid, NT);
  const long long r0 = (long long)blockIdx.x * CG_P;
  const cplx* src = in + (size_t)r0 * N;
  for (int e = tid; e < CG_P * N; e += NT) {
    const int p = e / N;
    S[p * RS + e % N] = (r0 + p < rows) ? src[e] : c_make(0.f, 0.f);
  }
  __syncthreads();
  cg_fft_tile<N, DIR>(S + (tid / T) * RS, 1, tid % T, tw);
  cplx* dst = out + (size_t)r0 * n_out;
  for (int e = tid; e < CG_P * n_out; e += NT) {
    const int p = e / n_out;
    if (r0 + p < rows) dst[e] = S[p * RS + e % n_out];
  }
}

// (c) block = (v, kz, 16 columns ky): forward along x of G; per requested gradient the product with the other volume's
// spectrum, the inverse along x and the rows x < L.  H1 = x-inverse of G . V2 (grad_v1), H2 = of V1 . conj(G) (grad_v2);
// a null H skips that gradient (its spectrum is then not read).  grid nvol NZ N / 16.
// ONE tile: after the forward transform every thread takes its N / T elements of the tile (column p, rows t + k T) into
// registers, and the tile is rewritten with the product of each gradient in turn.
template <int N> __global__ void __launch_bounds__(CG_P * FftPlan<N>::T)
k_cg_x(const cplx* __restrict__ G, const cplx* __restrict__ V1, const cplx* __restrict__ V2, cplx* __restrict__ H1,
       cplx* __restrict__ H2) {
  constexpr int L = N / 2, ES = CG_P + 1, T = FftPlan<N>::T, NT = CG_P * T, PERT = N / T;
  static_assert(PERT * T == N, "every thread owns N / T elements of the tile");
  __shared__ cplx S[N * ES + N];          // [x][17]
  cplx* tw = S + N * ES;
  const int tid = threadIdx.x;
  init_twiddles<N>(tw, tid, NT);
  const size_t slab = blockIdx.x / (N / CG_P);               // v NZ + kz
  const int c0 = (int)(blockIdx.x % (N / CG_P)) * CG_P;
  const size_t base = slab * N * N + c0;
  const int p = tid % CG_P, t = tid / CG_P;                   // neighbouring lanes: neighbouring columns
#pragma unroll
  for (int k = 0; k < PERT; k++) S[(t + k * T) * ES + p] = G[base + (size_t)(t + k * T) * N + p];
  __syncthreads();
  cg_fft_tile<N, -1>(S + p, ES, t, tw);
  cplx a[PERT];                                               // the transform of g
#pragma unroll
  for (int k = 0; k < PERT; k++) a[k] = S[(t + k * T) * ES + p];
  __syncthreads();
  for (int w = 0; w < 2; w++) {
    const cplx* V = w ? V1 : V2;
    cplx* H = w ? H2 : H1;
    if (!H) continue;                                         // (block-uniform)
#pragma unroll
    for (int k = 0; k < PERT; k++) {
      const cplx s = V[base + (size_t)(t + k * T) * N + p];
      S[(t + k * T) * ES + p] = w ? c_mulc(s, a[k]) : c_mul(a[k], s);
    }
    __syncthreads();
    cg_fft_tile<N, +1>(S + p, ES, t, tw);
    cplx* dst = H + slab * L * N + c0;
    for (int e = tid; e < L * CG_P; e += NT) dst[(size_t)(e / CG_P) * N + e % CG_P] = S[(e / CG_P) * ES + e % CG_P];
    __syncthreads();
  }
}

// (e) pencils q = (v, x, y), x, y < L, of NZ complex at D[(v NZ + kz) L^2 + q] -> out[(v L^2 + q) L + z], z < L: the
// Hermitian half extended to N, inverse along z, real part times scale.  grid nvol L^2 / 16 (L^2 is a multiple of 16).
template <int N> __global__ void __launch_bounds__(CG_P * FftPlan<N>::T)
k_cg_z_c2r(const cplx* __restrict__ D, float* __restrict__ out, float scale) {
  constexpr int L = N / 2, NZ = L + 1, RS = N + 1, T = FftPlan<N>::T, NT = CG_P * T;
  __shared__ cplx S[CG_P * RS + N];
  cplx* tw = S + CG_P * RS;
  const int tid = threadIdx.x;
  init_twiddles<N>(tw, tid, NT);
  const size_t q0 = (size_t)blockIdx.x * CG_P;
  const size_t v = q0 / ((size_t)L * L), r = q0 % ((size_t)L * L);
  const cplx* src = D + v * NZ * L * L + r;
  for (int e = tid; e < CG_P * NZ; e += NT) {
    const int p = e % CG_P, k = e / CG_P;
    const cplx a = src[(size_t)k * L * L + p];
    S[p * RS + k] = a;
    if (k > 0 && k < L) S[p * RS + N - k] = c_conj(a);
  }
  __syncthreads();
  cg_fft_tile<N, +1>(S + (tid / T) * RS, 1, tid % T, tw);
  float* dst = out + q0 * L;                                  // 16 pencils = 16 L consecutive floats
  for (int e = tid; e < CG_P * L; e += NT) dst[e] = S[(e / L) * RS + e % L].x * scale;
}

template <int N> static int cg_run(const float* gout, const cplx* V1, const cplx* V2, float* g1, float* g2, cplx* ws, int nvol,
                                   hipStream_t st) {
  constexpr int L = N / 2, NZ = L + 1, NT = CG_P * FftPlan<N>::T;
  static_assert(N % CG_P == 0 && (L * L) % CG_P == 0, "whole tiles");
  const size_t slabs = (size_t)nvol * NZ;
  cplx* G = ws;
  cplx* H1 = G + slabs * N * N;
  cplx* H2 = H1 + slabs * L * N;
  cplx* D = H2 + slabs * L * N;
  DLPD_LAUNCH((k_cg_z_r2c<N>), dim3((unsigned)((size_t)nvol * N * N / CG_P)), dim3(NT), 0, st, gout, G);
  DLPD_LAUNCH((k_cg_rows<N, -1>), dim3((unsigned)(slabs * N / CG_P)), dim3(NT), 0, st, (const cplx*)G, G, (long long)(slabs * N), N);
  DLPD_LAUNCH((k_cg_x<N>), dim3((unsigned)(slabs * (N / CG_P))), dim3(NT), 0, st, (const cplx*)G, V1, V2, g1 ? H1 : (cplx*)nullptr,
              g2 ? H2 : (cplx*)nullptr);
  const float scale = 1.0f / ((float)N * (float)N * (float)N);
  for (int w = 0; w < 2; w++) {
    float* out = w ? g2 : g1;
    if (!out) continue;
    const long long rows = (long long)(slabs * L);
    DLPD_LAUNCH((k_cg_rows<N, +1>), dim3((unsigned)((rows + CG_P - 1) / CG_P)), dim3(NT), 0, st, (const cplx*)(w ? H2 : H1), D, rows, L);
    DLPD_LAUNCH((k_cg_z_c2r<N>), dim3((unsigned)((size_t)nvol * L * L / CG_P)), dim3(NT), 0, st, (const cplx*)D, out, scale);
  }
  return dlpd_check_launch();
}

// a <- a * b
__global__ void __launch_bounds__(256) k_gmul(cplx* __restrict__ a, const cplx* __restrict__ b, size_t n) {
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) a[i] = c_mul(a[i], b[i]);
}
// the L^3 corner of (nvol, N, N, N)
__global__ void __launch_bounds__(256) k_gcorner(const float* __restrict__ full, float* __restrict__ out, int L, size_t n) {
  const size_t N = 2 * (size_t)L;
  for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    const size_t z = i % L, y = (i / L) % L, x = (i / ((size_t)L * L)) % L, v = i / ((size_t)L * L * L);
    out[i] = full[((v * N + x) * N + y) * N + z];
  }
}

extern "C" {

int dlpd_correlate_grad_supported(int L) { return dlpd_listed<DLPD_BOXES>(L) ? 1 : 0; }

// bytes of workspace dlpd_correlate_grad needs: G (NZ, N, N), H1, H2 (NZ, L, N), D (NZ, L, L) complex per volume
size_t dlpd_correlate_grad_ws_bytes(int nvol, int L) {
  if (nvol <= 0 || !dlpd_correlate_grad_supported(L)) return 0;
  const size_t N = 2 * (size_t)L, NZ = (size_t)L + 1;
  return (size_t)nvol * NZ * (N * N + 2 * L * N + (size_t)L * L) * sizeof(cplx);
}

// gout (nvol, N^3) f32; spec1, spec2 (nvol, NZ, N, N): dlpd_rfft3d_padded(scale = 1) of v1, v2; g1, g2 (nvol, L^3) f32.
// A null g1 / g2 skips that gradient, and the spectrum only it reads (spec2 / spec1) may then be null too.
int dlpd_correlate_grad(const float* gout, const void* spec1, const void* spec2, float* g1, float* g2, void* ws, int nvol, int L,
                        void* stream) {
  if (!gout || !ws || nvol <= 0 || (!g1 && !g2) || (g1 && !spec2) || (g2 && !spec1)) return DLPD_ERR_ARG;
  return dlpd_dispatch<DLPD_BOXES>(L, [&](auto l) {
    return cg_run<2 * l()>(gout, (const cplx*)spec1, (const cplx*)spec2, g1, g2, (cplx*)ws, nvol, (hipStream_t)stream);
  });
}

}  // extern "C"

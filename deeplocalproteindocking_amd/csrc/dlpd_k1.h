// Shared pieces of the channels-last K1 (trilinear rotation + forward z transform, Docker.py:218 + the z pass of the
// correlation of DockingModels.py:70-71): the block shapes and THE sample -- both formulations of the kernel
// (k_rotate_zfft_cl in dlpd_corr.hip: every wave gathers, transforms and stores in turn; k_rotate_zfft_cl_rs in
// dlpd_k1r.hip: gather waves and transform / store waves) call the same function, so their samples are the same bits.
#pragma once
#include <dlpd_platform.h>
#include "dlpd_fft.h"

#define DLPD_K1CL_CC 16                   // channel padding of the channels-last copy
// rows x channels per block (64 two-row pencils either way).  8 x 16: 64-byte gathers, 64-byte output pieces;
// 16 x 8: 32-byte gathers, full 128-byte output lines.  Measured: N = 128 (48 channels) 0.83 / 0.75 ms,
// N = 160 (16 channels) 0.61 / 0.66 ms.  32 x 4 (16-byte gathers, 256-byte pieces), round 3: 1.24 ms at N = 128.
// Also measured in round 3 (all bit-identical or equal to rounding, none kept):
//  * a lane fetching TWO adjacent channel quads of a corner itself (position, weights and offsets computed once per voxel
//    instead of once per lane: a third fewer vector instructions): 1.56 ms at N = 128, 0.66 against 0.60 at N = 160 (four
//    quads per lane 0.90) -- what the gather costs is the number of (lane, instruction) line requests, and two lanes
//    reading 32 adjacent bytes in ONE instruction are one request where one lane reading them in two instructions is two;
//  * the z transform as two half-length transforms (Z[2j] = FFT_L(z), Z[2j+1] = FFT_L(z w_N^n); samples kept in registers,
//    34 KB of LDS and 63 registers: four blocks per CU instead of two): 0.90-0.93 ms against 0.77 with 2, 3 or 4 resident
//    blocks alike -- the kernel is not waiting for a free block slot, and the second set of passes and barriers costs.
//  * 16 rows x 16 channels = 128 pencils per block (64-byte gathers AND 128-byte pieces; 145 KB, one block per CU, 1024
//    threads): 0.77-0.80 ms against 0.76-0.77.
//  * round 4, N = 160 (one 89 KB block per CU): 32 pencils per block -- 44 KB, three blocks per CU -- as 8 rows x 8 channels
//    0.686 ms (32-byte gathers), as 4 rows x 16 channels 1.67 ms (32-byte OUTPUT runs: 2.7 x), 16 rows x 8 channels
//    re-measured 0.675, against 0.61 for 8 x 16; 48 ch x 80^3: 1.93 / 3.65 / 2.12 against 1.71.  Occupancy is not what this
//    kernel lacks; the run lengths of its gathers and stores are what it pays for.
// The SOURCE layout (EXPERIMENTS.md, K1 chunk-major): k_rotate_zfft_cl addresses the copy as chunk * cstride + voxel * vstride + q,
// so the same kernel reads cl[x][y][z][Cp] and the chunk-major [chunk][x][y][z][CC] (dlpd_make_channel_chunks; CC = this
// struct's CC, so the copy follows the block shape).  At N = 128 (48 channels, launches of 32 rotations) a 16 x 8 block used 32
// bytes of every 128-byte line of the channels-last records; chunk-major, TCP -> TCC read requests per launch fall 2.35e8 ->
// 0.92e8 (2.55 x), tag accesses 4.37e8 -> 3.98e8, and the launch 1.60 -> 1.37 ms: line fills were about a seventh of the
// kernel, the rest is its (lane, instruction) request count, which the layout does not change.  Re-measured under the new
// layout (ms per launch / per step of 32 rotations, same session): 16 x 8 1.35 / 9.57, 8 x 16 1.40 / 9.63, 32 x 4 (4-channel
// chunks, eight z-neighbours per line) 2.23 / 10.59; blocks of one chunk adjacent (row group inside chunk, -DDLPD_K1_CHUNK_OUTER)
// 1.40 / 9.63 against chunk inside row group 1.35 / 9.57.  Shape and order stay as they were.
// A/B switches of this file (scripts/build_variant.py --corr=-D...): DLPD_K1_YG128 / DLPD_K1_YG160 / DLPD_K1_CC160 (block shape),
// DLPD_K1_ZPAIR (0: the two-lane gather at N = 128 from the chunk-major copy too, i.e. the kernel before ZPAIR) and
// DLPD_K1_ZPAIR_DEPTH (1: one four-lane task in flight per lane), both described at k1cl_zpair_issue below.
#ifndef DLPD_K1_YG160
#define DLPD_K1_YG160 8
#endif
#ifndef DLPD_K1_CC160
#define DLPD_K1_CC160 16
#endif
#ifndef DLPD_K1_YG128
#define DLPD_K1_YG128 16
#endif
template <int N> struct K1ClCfg {
  static constexpr int YG = (N == 128) ? DLPD_K1_YG128 : (N == 160 ? DLPD_K1_YG160 : 8), CC = (N == 160) ? DLPD_K1_CC160 : 128 / YG;
  static constexpr int NP = CC * (YG / 2);             // two-row pencils per block
};
struct K1ClRot { float r0, r1, r2, r3, r4, r5, r6, r7, r8; };
DLPD_D K1ClRot k1cl_load_rotation(const float* r) {
  K1ClRot o = {r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]};
  return o;
}

// Rows yrow and yrow + 1 of output plane x at depth z, four channels (one float4 of the channels-last copy `src`, which
// already points at the lane's channel quad): same corner weights, products and summation order as trilinear_fetch.
DLPD_D void k1cl_sample_rows(const float4* __restrict__ src, int Cq, int L, int ext, float c0, const K1ClRot& r, int x, int yrow,
                             int z, float4 (&acc)[2]) {
  const float dx = x - c0, dz = z - c0;
  const int hi = L - 1;
#pragma unroll
      for (int u = 0; u < 2; u++) {
        // outside the embedded box (ext < L) the sample is cropped: all eight weights zero (no branch: the loads of both
        // rows stay batched; a branch here cost 0.06 ms at N = 128)
        const bool live = max(x, max(yrow + u, z)) < ext;
        const float dy = (yrow + u) - c0;
        const float px = c0 + (r.r0 * dx + r.r3 * dy + r.r6 * dz);
        const float py = c0 + (r.r1 * dx + r.r4 * dy + r.r7 * dz);
        const float pz = c0 + (r.r2 * dx + r.r5 * dy + r.r8 * dz);
        const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
        const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
        const float ax = px - fx, ay = py - fy, az = pz - fz;
        const bool x0 = live & (ix >= 0) & (ix <= hi), x1 = live & (ix + 1 >= 0) & (ix + 1 <= hi);
        const bool y0 = (iy >= 0) & (iy <= hi), y1 = (iy + 1 >= 0) & (iy + 1 <= hi);
        const bool z0 = (iz >= 0) & (iz <= hi), z1 = (iz + 1 >= 0) & (iz + 1 <= hi);
        const float wx0 = x0 ? 1.f - ax : 0.f, wx1 = x1 ? ax : 0.f;
        const float wy0 = y0 ? 1.f - ay : 0.f, wy1 = y1 ? ay : 0.f;
        const float wz0 = z0 ? 1.f - az : 0.f, wz1 = z1 ? az : 0.f;
        const int cx0 = min(max(ix, 0), hi), cx1 = min(max(ix + 1, 0), hi);
        const int cy0 = min(max(iy, 0), hi), cy1 = min(max(iy + 1, 0), hi);
        const int cz0 = min(max(iz, 0), hi), cz1 = min(max(iz + 1, 0), hi);
        const float4 v000 = src[(size_t)((cx0 * L + cy0) * L + cz0) * Cq], v001 = src[(size_t)((cx0 * L + cy0) * L + cz1) * Cq];
        const float4 v010 = src[(size_t)((cx0 * L + cy1) * L + cz0) * Cq], v011 = src[(size_t)((cx0 * L + cy1) * L + cz1) * Cq];
        const float4 v100 = src[(size_t)((cx1 * L + cy0) * L + cz0) * Cq], v101 = src[(size_t)((cx1 * L + cy0) * L + cz1) * Cq];
        const float4 v110 = src[(size_t)((cx1 * L + cy1) * L + cz0) * Cq], v111 = src[(size_t)((cx1 * L + cy1) * L + cz1) * Cq];
        const float w000 = wx0 * wy0 * wz0, w001 = wx0 * wy0 * wz1, w010 = wx0 * wy1 * wz0, w011 = wx0 * wy1 * wz1;
        const float w100 = wx1 * wy0 * wz0, w101 = wx1 * wy0 * wz1, w110 = wx1 * wy1 * wz0, w111 = wx1 * wy1 * wz1;
#define DLPD_TRI(f)                                                                                               \
  {                                                                                                               \
    float a = v000.f * w000;                                                                                      \
    a += v001.f * w001;                                                                                           \
    a += v010.f * w010;                                                                                           \
    a += v011.f * w011;                                                                                           \
    a += v100.f * w100;                                                                                           \
    a += v101.f * w101;                                                                                           \
    a += v110.f * w110;                                                                                           \
    a += v111.f * w111;                                                                                           \
    acc[u].f = a;                                                                                                 \
  }
        DLPD_TRI(x) DLPD_TRI(y) DLPD_TRI(z) DLPD_TRI(w)
#undef DLPD_TRI
      }
}

// ------------------------------------------------------------------------------------------
// ZPAIR (EXPERIMENTS.md K1-ZPAIR; chunk-major source at N = 128 only: CC = 8, two channel quads): the two z corners of a
// sample, (cx, cy, zb) and (cx, cy, zb + 1), are 64 contiguous bytes of [chunk][x][y][z][8], so the FOUR lanes
// lane = 4 voxel + 2 zc + q of a (row pair, z) task fetch that run with one instruction: lane (zc, q) loads channel quad q of
// voxel zb + zc, zb = clamp(iz, 0, L - 2), for the four (x, y) corner columns of BOTH rows -- eight loads per lane over
// twice as many lanes instead of sixteen.  Lane zc keeps row yrow + zc: it loads that row first and the partner's row
// second, and one dlpd_quad_swap2 per register of the second set hands each lane the other z corner of its own row.
// Same bits as k1cl_sample_rows: with d = iz - zb the element cz0 = clamp(iz) is voxel zb + (d > 0) and cz1 = clamp(iz + 1)
// is voxel zb + (d >= 0), so every term takes the value, weight and place in the sum it always had -- also outside the
// box, where all weights are 0 and the sign of the zero sum depends on the values.
// `gather` = false (an empty occupancy cell, uniform over the four lanes): no loads, +0.0; the exchange still runs, so
// that every lane of the wave reaches it.  Both instantiations (dense and OCC) are dealt this way.
// Measured (EXPERIMENTS.md K1-ZPAIR; config 2, 48 channels, ms per launch / per step of 32 rotations, three alternating runs):
// two-lane gather 1.31-1.33 / 9.59-9.62, this gather with two tasks in flight (DEPTH 2: 16 loads per lane before the first
// wait, as the two-lane gather has; 124 registers, no scratch) 1.23-1.26 / 9.48-9.50, with one (63 registers) 1.27-1.29 /
// 9.52-9.53.  Kept: K1 -5.8 %, step -1.1 %.  NOT for the reason it was built for: TCP_TOTAL_CACHE_ACCESSES per launch went
// 3.98e8 -> 4.18e8, not to 0.6 of it -- four lanes reading 64 adjacent bytes in one instruction count as two tag accesses
// exactly as two lanes reading 32 bytes each in two instructions did; TCP -> TCC read requests 0.92e8 -> 0.89e8, TA busy
// cycles 1.70e6 -> 1.64e6.  Where the gain comes from is not established by these counters.
// ------------------------------------------------------------------------------------------
#ifndef DLPD_K1_ZPAIR
#define DLPD_K1_ZPAIR 1                  // 0: the parent's gather (two lanes per voxel, sixteen loads) from the chunk-major copy too
#endif
#ifndef DLPD_K1_ZPAIR_DEPTH
#define DLPD_K1_ZPAIR_DEPTH 2            // tasks whose loads a lane issues before it consumes the first (1 or 2)
#endif
#if !defined(DLPD_HAS_QUAD_SWAP2)        // the emulator: lanes are fibers, the exchange a wave shuffle (8 bytes at a time)
DLPD_D float4 dlpd_quad_swap2(float4 v) {
  const float2 a = __shfl_xor(make_float2(v.x, v.y), 2), b = __shfl_xor(make_float2(v.z, v.w), 2);
  return make_float4(a.x, a.y, b.x, b.y);
}
#endif
template <int N> struct K1ClZpair {
  static constexpr bool ON = DLPD_K1_ZPAIR && N == 128 && K1ClCfg<N>::CC == 8;
};
struct K1ClPos { float ax, ay, az; int ix, iy, iz; };
DLPD_D K1ClPos k1cl_position(float c0, const K1ClRot& r, float dx, float dy, float dz) {
  const float px = c0 + (r.r0 * dx + r.r3 * dy + r.r6 * dz);
  const float py = c0 + (r.r1 * dx + r.r4 * dy + r.r7 * dz);
  const float pz = c0 + (r.r2 * dx + r.r5 * dy + r.r8 * dz);
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  K1ClPos o = {px - fx, py - fy, pz - fz, (int)fx, (int)fy, (int)fz};
  return o;
}
// Row yrow + zc of output plane x at depth z, four channels, in two steps, so that the caller can have the loads of several
// tasks in flight: k1cl_zpair_issue (position, weights, the eight loads) and k1cl_zpair_finish (exchange, sum).  src points
// at the lane's channel quad of the chunk, Cq = the voxel stride in float4 (2).  All four lanes of a task call both together.
struct K1ClZpairTask {
  float4 keep[4], send[4];               // corner columns (x0,y0) (x0,y1) (x1,y0) (x1,y1) of the kept row / of the partner's
  float wx0, wx1, wy0, wy1, wz0, wz1;
  bool own0, own1, gather;
};
DLPD_D void k1cl_zpair_issue(K1ClZpairTask& t, const float4* __restrict__ src, int Cq, int L, int ext, float c0, const K1ClRot& r,
                             int x, int yrow, int z, int zc, bool gather) {
  const float4 zero = make_float4(0.f, 0.f, 0.f, 0.f);
  const int hi = L - 1;
  float4 (&keep)[4] = t.keep, (&send)[4] = t.send;
  float &wx0 = t.wx0, &wx1 = t.wx1, &wy0 = t.wy0, &wy1 = t.wy1, &wz0 = t.wz0, &wz1 = t.wz1;
  bool &own0 = t.own0, &own1 = t.own1;
#pragma unroll
  for (int j = 0; j < 4; j++) keep[j] = send[j] = zero;
  wx0 = wx1 = wy0 = wy1 = wz0 = wz1 = 0.f;
  own0 = own1 = false;
  t.gather = gather;
  if (gather) {
    const float dx = x - c0, dz = z - c0;
    // the row this lane keeps: weights as k1cl_sample_rows (cropped outside the embedded box, no branch)
    const bool live = max(x, max(yrow + zc, z)) < ext;
    const K1ClPos k = k1cl_position(c0, r, dx, (yrow + zc) - c0, dz);
    const bool x0 = live & (k.ix >= 0) & (k.ix <= hi), x1 = live & (k.ix + 1 >= 0) & (k.ix + 1 <= hi);
    const bool y0 = (k.iy >= 0) & (k.iy <= hi), y1 = (k.iy + 1 >= 0) & (k.iy + 1 <= hi);
    const bool z0 = (k.iz >= 0) & (k.iz <= hi), z1 = (k.iz + 1 >= 0) & (k.iz + 1 <= hi);
    wx0 = x0 ? 1.f - k.ax : 0.f, wx1 = x1 ? k.ax : 0.f;
    wy0 = y0 ? 1.f - k.ay : 0.f, wy1 = y1 ? k.ay : 0.f;
    wz0 = z0 ? 1.f - k.az : 0.f, wz1 = z1 ? k.az : 0.f;
    const int zb = min(max(k.iz, 0), hi - 1), d = k.iz - zb;
    own0 = (zc != 0) == (d > 0);                     // this lane's own load is the element of the z0 term ...
    own1 = (zc != 0) == (d >= 0);                    // ... of the z1 term (else the partner's)
    // the partner's row: addresses only
    const K1ClPos s = k1cl_position(c0, r, dx, (yrow + (zc ^ 1)) - c0, dz);
    const int sb = min(max(s.iz, 0), hi - 1);
    const int kx0 = min(max(k.ix, 0), hi) * L, kx1 = min(max(k.ix + 1, 0), hi) * L;
    const int ky0 = min(max(k.iy, 0), hi), ky1 = min(max(k.iy + 1, 0), hi);
    const int sx0 = min(max(s.ix, 0), hi) * L, sx1 = min(max(s.ix + 1, 0), hi) * L;
    const int sy0 = min(max(s.iy, 0), hi), sy1 = min(max(s.iy + 1, 0), hi);
    const int kz = zb + zc, sz = sb + zc;            // <= L - 1: inside the chunk
    keep[0] = src[(size_t)((kx0 + ky0) * L + kz) * Cq], keep[1] = src[(size_t)((kx0 + ky1) * L + kz) * Cq];
    keep[2] = src[(size_t)((kx1 + ky0) * L + kz) * Cq], keep[3] = src[(size_t)((kx1 + ky1) * L + kz) * Cq];
    send[0] = src[(size_t)((sx0 + sy0) * L + sz) * Cq], send[1] = src[(size_t)((sx0 + sy1) * L + sz) * Cq];
    send[2] = src[(size_t)((sx1 + sy0) * L + sz) * Cq], send[3] = src[(size_t)((sx1 + sy1) * L + sz) * Cq];
  }
}
DLPD_D float4 k1cl_zpair_finish(const K1ClZpairTask& t) {
  const float4 (&keep)[4] = t.keep;
  const float wx0 = t.wx0, wx1 = t.wx1, wy0 = t.wy0, wy1 = t.wy1, wz0 = t.wz0, wz1 = t.wz1;
  const bool own0 = t.own0, own1 = t.own1;
  float4 recv[4];
#pragma unroll
  for (int j = 0; j < 4; j++) recv[j] = dlpd_quad_swap2(t.send[j]);
  if (!t.gather) return make_float4(0.f, 0.f, 0.f, 0.f);
  const float w000 = wx0 * wy0 * wz0, w001 = wx0 * wy0 * wz1, w010 = wx0 * wy1 * wz0, w011 = wx0 * wy1 * wz1;
  const float w100 = wx1 * wy0 * wz0, w101 = wx1 * wy0 * wz1, w110 = wx1 * wy1 * wz0, w111 = wx1 * wy1 * wz1;
  float4 acc;
  // The sum as k1cl_sample_rows COMPILES (-ffp-contract=fast): of `a = v000 w000; a += v001 w001` the compiler fuses the
  // FIRST product, fma(v000, w000, v001 * w001), and every later term is one fma onto the sum.  Said here in so many words
  // (contract(on): one fma per expression that has a product and a sum, none across statements), because left to its own
  // choice the compiler paired these products (v_pk_mul_f32) and added them unfused in the OCC instantiation: other bits.
  // (The emulator's compiler fuses nothing in either function: (v000 w000) + (v001 w001) both times.)
#define DLPD_TRI(f)                                                                                               \
  {                                                                                                               \
    _Pragma("clang fp contract(on)")                                                                              \
    const float p1 = (own1 ? keep[0].f : recv[0].f) * w001;                                                       \
    float a = (own0 ? keep[0].f : recv[0].f) * w000 + p1;                                                         \
    a += (own0 ? keep[1].f : recv[1].f) * w010;                                                                   \
    a += (own1 ? keep[1].f : recv[1].f) * w011;                                                                   \
    a += (own0 ? keep[2].f : recv[2].f) * w100;                                                                   \
    a += (own1 ? keep[2].f : recv[2].f) * w101;                                                                   \
    a += (own0 ? keep[3].f : recv[3].f) * w110;                                                                   \
    a += (own1 ? keep[3].f : recv[3].f) * w111;                                                                   \
    acc.f = a;                                                                                                    \
  }
  DLPD_TRI(x) DLPD_TRI(y) DLPD_TRI(z) DLPD_TRI(w)
#undef DLPD_TRI
  return acc;
}

// dlpd_k1r.hip: the role-split formulation behind dlpd_zfft_channels_last_form(form = 2); boxes 64 and 80
int dlpd_k1_role_split(const float4* cl, const float* R, cplx* A, int C, int nb, float c0, hipStream_t st, int CT_out, int c_base,
                       int ext, int L);

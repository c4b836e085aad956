// The trilinear sample every rotation kernel of the library takes (dlpd_corr.hip: k_rotate, K1; dlpd_local.h: the local
// correlation): ONE definition, so that a pose scored by direct correlation samples the ligand exactly as the search does.
#pragma once
#include <dlpd_platform.h>

// ------------------------------------------------------------------------------------------
// trilinear sample of a (L,L,L) volume at position (px,py,pz), zeros outside
// ------------------------------------------------------------------------------------------
DLPD_D float trilinear_fetch(const float* __restrict__ v, int L, float px, float py, float pz) {
  // branch-free: out-of-box corners get weight 0 and a clamped (valid) address, so all loads are
  // unconditional and in flight together; the two z-neighbours come from ONE 8-byte load
  // (half the address-unit work of eight scalar gathers)
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
  const float ax = px - fx, ay = py - fy, az = pz - fz;
  const int hi = L - 1;
  const bool x0 = (ix >= 0) & (ix <= hi), x1 = (ix + 1 >= 0) & (ix + 1 <= hi);
  const bool y0 = (iy >= 0) & (iy <= hi), y1 = (iy + 1 >= 0) & (iy + 1 <= hi);
  const bool z0 = (iz >= 0) & (iz <= hi), z1 = (iz + 1 >= 0) & (iz + 1 <= hi);
  const float wx0 = x0 ? 1.f - ax : 0.f, wx1 = x1 ? ax : 0.f;
  const float wy0 = y0 ? 1.f - ay : 0.f, wy1 = y1 ? ay : 0.f;
  const float wz0 = z0 ? 1.f - az : 0.f, wz1 = z1 ? az : 0.f;
  const int cx0 = min(max(ix, 0), hi), cx1 = min(max(ix + 1, 0), hi);
  const int cy0 = min(max(iy, 0), hi), cy1 = min(max(iy + 1, 0), hi);
  const int zb = min(max(iz, 0), hi - 1);          // pair (zb, zb+1) always inside the row
  const int d = iz - zb;                           // 0 inside; -1 / +1 at the two faces
  DLPD_PAIR p00 = dlpd_load_pair(v + (cx0 * L + cy0) * L + zb);
  DLPD_PAIR p01 = dlpd_load_pair(v + (cx0 * L + cy1) * L + zb);
  DLPD_PAIR p10 = dlpd_load_pair(v + (cx1 * L + cy0) * L + zb);
  DLPD_PAIR p11 = dlpd_load_pair(v + (cx1 * L + cy1) * L + zb);
  // value at z0 = iz is .x unless iz = zb+1 ; value at z1 = iz+1 is .y unless iz+1 = zb
  const float v000 = d > 0 ? p00.y : p00.x, v001 = d < 0 ? p00.x : p00.y;
  const float v010 = d > 0 ? p01.y : p01.x, v011 = d < 0 ? p01.x : p01.y;
  const float v100 = d > 0 ? p10.y : p10.x, v101 = d < 0 ? p10.x : p10.y;
  const float v110 = d > 0 ? p11.y : p11.x, v111 = d < 0 ? p11.x : p11.y;
  float acc = v000 * (wx0 * wy0 * wz0);
  acc += v001 * (wx0 * wy0 * wz1);
  acc += v010 * (wx0 * wy1 * wz0);
  acc += v011 * (wx0 * wy1 * wz1);
  acc += v100 * (wx1 * wy0 * wz0);
  acc += v101 * (wx1 * wy0 * wz1);
  acc += v110 * (wx1 * wy1 * wz0);
  acc += v111 * (wx1 * wy1 * wz1);
  return acc;
}

// The weight trilinear_fetch gives the corner with index q (inside the box) along ONE axis for a sample at p -- the same
// floorf and fraction; the sample's weight of voxel (qx, qy, qz) is wx * wy * wz, in that order.  For the adjoint of the
// rotation (dlpd_rotate_grad.h).
DLPD_D float trilinear_axis_weight(float p, int q) {
  const float f = floorf(p);
  const int i = (int)f;
  const float a = p - f;
  return i == q ? 1.f - a : (i + 1 == q ? a : 0.f);
}

// The partial derivatives of the value trilinear_fetch returns, with respect to the sample position: the same floorf,
// fractions, in-box masks, clamped addresses and four pair loads.  Along x
//   d/dpx = sum over the (y, z) corners of wy wz ([x1] v1yz - [x0] v0yz),
// wy, wz the forward's masked weights and [x0], [x1] its in-box masks; likewise along y and z.  The value is piecewise
// trilinear: at an exactly integer coordinate this is the derivative of the cell floorf picks, the one on the right.
// For the rotation's gradient with respect to its matrix (dlpd_rotate_rgrad.h).
DLPD_D void trilinear_fetch_grad(const float* __restrict__ v, int L, float px, float py, float pz, float* dx, float* dy,
                                 float* dz) {
  const float fx = floorf(px), fy = floorf(py), fz = floorf(pz);
  const int ix = (int)fx, iy = (int)fy, iz = (int)fz;
  const float ax = px - fx, ay = py - fy, az = pz - fz;
  const int hi = L - 1;
  const bool x0 = (ix >= 0) & (ix <= hi), x1 = (ix + 1 >= 0) & (ix + 1 <= hi);
  const bool y0 = (iy >= 0) & (iy <= hi), y1 = (iy + 1 >= 0) & (iy + 1 <= hi);
  const bool z0 = (iz >= 0) & (iz <= hi), z1 = (iz + 1 >= 0) & (iz + 1 <= hi);
  const float wx0 = x0 ? 1.f - ax : 0.f, wx1 = x1 ? ax : 0.f;
  const float wy0 = y0 ? 1.f - ay : 0.f, wy1 = y1 ? ay : 0.f;
  const float wz0 = z0 ? 1.f - az : 0.f, wz1 = z1 ? az : 0.f;
  const int cx0 = min(max(ix, 0), hi), cx1 = min(max(ix + 1, 0), hi);
  const int cy0 = min(max(iy, 0), hi), cy1 = min(max(iy + 1, 0), hi);
  const int zb = min(max(iz, 0), hi - 1);
  const int d = iz - zb;
  DLPD_PAIR p00 = dlpd_load_pair(v + (cx0 * L + cy0) * L + zb);
  DLPD_PAIR p01 = dlpd_load_pair(v + (cx0 * L + cy1) * L + zb);
  DLPD_PAIR p10 = dlpd_load_pair(v + (cx1 * L + cy0) * L + zb);
  DLPD_PAIR p11 = dlpd_load_pair(v + (cx1 * L + cy1) * L + zb);
  // the corner values with their in-box masks applied (a corner outside the box is the zero the forward gives it)
  const float v000 = (x0 & y0 & z0) ? (d > 0 ? p00.y : p00.x) : 0.f, v001 = (x0 & y0 & z1) ? (d < 0 ? p00.x : p00.y) : 0.f;
  const float v010 = (x0 & y1 & z0) ? (d > 0 ? p01.y : p01.x) : 0.f, v011 = (x0 & y1 & z1) ? (d < 0 ? p01.x : p01.y) : 0.f;
  const float v100 = (x1 & y0 & z0) ? (d > 0 ? p10.y : p10.x) : 0.f, v101 = (x1 & y0 & z1) ? (d < 0 ? p10.x : p10.y) : 0.f;
  const float v110 = (x1 & y1 & z0) ? (d > 0 ? p11.y : p11.x) : 0.f, v111 = (x1 & y1 & z1) ? (d < 0 ? p11.x : p11.y) : 0.f;
  float gx = (wy0 * wz0) * (v100 - v000);
  gx += (wy0 * wz1) * (v101 - v001);
  gx += (wy1 * wz0) * (v110 - v010);
  gx += (wy1 * wz1) * (v111 - v011);
  float gy = (wx0 * wz0) * (v010 - v000);
  gy += (wx0 * wz1) * (v011 - v001);
  gy += (wx1 * wz0) * (v110 - v100);
  gy += (wx1 * wz1) * (v111 - v101);
  float gz = (wx0 * wy0) * (v001 - v000);
  gz += (wx0 * wy1) * (v011 - v010);
  gz += (wx1 * wy0) * (v101 - v100);
  gz += (wx1 * wy1) * (v111 - v110);
  *dx = gx;
  *dy = gy;
  *dz = gz;
}

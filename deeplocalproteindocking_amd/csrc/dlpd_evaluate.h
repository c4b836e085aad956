// Pose evaluation against a native complex: interface RMSD, ligand RMSD, native contacts and the CAPRI class of every pose
// of a list.  Included by dlpd_topk.hip, the list stage.  What the reference computes pose by pose on the
// host -- scripts/Results/Benchmark/EvaluateBenchmark.py:95-113 (the superposed RMSD of every interface pair, the minimum
// kept) and scripts/Dataset/processing_utils.py:183-236 (contacts, fnat, the class cascade) -- restated in closed forms.
//
// A pose is 12 doubles, R row-major then t: it carries the ligand point y to R y + t.
//
// I-RMSD.  An interface pair is nr receptor points a, nl ligand points y and n = nr + nl static points q (receptor rows
// first).  The host (ops.native_moments) takes a about its centroid ca, y about its centroid cy, q about its mean, and packs
//   A = sum_rec a q^T   Y = sum_lig y q^T   s = sum_lig q   sa = sum a   sy = sum y   Saa = sum |a|^2   Cyy = sum y y^T
//   Gq = sum |q|^2
// A common shift of the mobile set changes no superposed RMSD, so with u = t + R cy - ca in place of t
//   H  = A + R Y + u s^T                                        (P^T Q of the centred sets)
//   w  = sa + R sy                                              (zero up to rounding for centred moments)
//   Syy(R) = sum |R y|^2 = sum_i r_i^T Cyy r_i over the rows r_i of R       (= tr Cyy for a rotation; the matrices of a .dat
//                                                                             file are rotations to six decimals only)
//   Gp = Saa + Syy(R) + 2 u.(R sy - (nl/n) w) - |w|^2 / n + (nl nr / n) |u|^2
//   rmsd^2 = max(0, Gp + Gq - 2 lambda) / n,   lambda = the largest eigenvalue of Horn's 4x4 matrix of H
//          = sigma1 + sigma2 + sign(det H) sigma3.
// Gp is sum |p|^2 - |sum p|^2 / n of the mobile set with the two |u|^2 terms combined: they cancel completely when nr = 0.
// lambda comes from cyclic Jacobi sweeps over the six off-diagonal entries, the ten matrix entries in registers, at most
// EVAL_SWEEPS sweeps: every rotation is well defined whatever the matrix (H = 0, rank 1 or 2, det H < 0 included), the work
// is bounded, and a sweep that finds nothing to rotate ends the loop.
//
// L-RMSD.  z are the bound ligand's points in the docking frame (about their centroid cz), M = sum z y^T, u = t + R cy - cz:
//   lrmsd^2 = max(0, Syy(R) + Szz + nl |u|^2 + 2 u.(R sy - sz) - 2 sum_ab R_ab M_ab) / nl     (no superposition per pose)
//
// The moment block: nI records of EVAL_REC doubles, then the L-RMSD record.
//   interface record: A[9] Y[9] s[3] sa[3] sy[3] Saa Syy Gq ca[3] cy[3] Cyy[6]     (42 used; Cyy as xx xy xz yy yz zz)
//   L-RMSD record:    M[9] sy[3] sz[3] Syy Szz cy[3] cz[3] Cyy[6]                  (29 used)
// (Syy = tr Cyy is carried for the reader of a block; the kernel takes Syy(R).)
// The point counts are integers the host knows: they travel as kernel arguments, not in the block.
//
// Contacts.  The ligand's interface atoms are posed once per pose into LDS in float32 (R and t rounded once, a coordinate is
// the chain t -> fma(R0, x, .) -> fma(R1, y, .) -> fma(R2, z, .)); the receptor's atoms are the same for every pose and are
// read through the cache.  A contact (r0, r1, l0, l1) holds iff some atom pair of the two ranges has d^2 <= r^2 in float32,
// d^2 one fma chain over the three differences as cluster_d2 forms it.  Contacts are dealt to the lanes of the pose's
// threads; the count is a butterfly sum per wave, one plain LDS word per wave and a barrier (no LDS atomic).
// One pose per block of EVAL_CONTACT_NT threads: a wave (DESIGN.md 4j has the measurement).
#pragma once

#define EVAL_MAXI 16                  // interface pairs per target
#define EVAL_REC 48                   // doubles per record of the moment block
#define EVAL_NT 256                   // threads per block: k_pose_native_rmsd, k_pose_capri
#define EVAL_SWEEPS 12                // cap on the Jacobi sweeps
#define EVAL_MAXLIG 2048              // ligand interface atoms (24 KB of LDS)
#define EVAL_SMALLLIG 512             // ... and the instance typical interfaces take (6 KB: four times the blocks per CU)
#define EVAL_MAXREC 65536             // receptor interface atoms
#define EVAL_MAXC 65536               // native contacts
#ifndef EVAL_CONTACT_NT
#define EVAL_CONTACT_NT 64            // threads per pose of k_pose_native_contacts (a multiple of 64)
#endif

struct eval_counts {
  int nr[EVAL_MAXI + 1], nl[EVAL_MAXI + 1];       // entry nI: the L-RMSD record (nr unused)
};

// one Jacobi rotation in the (p, q) plane of a symmetric 4x4 matrix; (r, s) are the other two indices
DLPD_D void eval_rotate(double& app, double& aqq, double& apq, double& arp, double& arq, double& asp, double& asq) {
  if (apq == 0.0) return;
  const double theta = 0.5 * (aqq - app) / apq;                   // (overflows to +-inf for a tiny apq: t = 0 below)
  double t = 1.0 / (fabs(theta) + sqrt(fma(theta, theta, 1.0)));  // the smaller root: |angle| <= pi / 4
  if (theta < 0.0) t = -t;
  const double c = 1.0 / sqrt(fma(t, t, 1.0)), s = t * c, tau = s / (1.0 + c);
  const double h = t * apq;
  app -= h;
  aqq += h;
  apq = 0.0;
  const double g0 = arp, h0 = arq, g1 = asp, h1 = asq;
  arp = fma(-s, fma(g0, tau, h0), g0);
  arq = fma(s, fma(-h0, tau, g0), h0);
  asp = fma(-s, fma(g1, tau, h1), g1);
  asq = fma(s, fma(-h1, tau, g1), h1);
}

// the largest eigenvalue of Horn's quaternion matrix of H (row-major 3x3)
DLPD_D double eval_lambda(const double* H) {
  double a00 = H[0] + H[4] + H[8], a11 = H[0] - H[4] - H[8], a22 = -H[0] + H[4] - H[8], a33 = -H[0] - H[4] + H[8];
  double a01 = H[5] - H[7], a02 = H[6] - H[2], a03 = H[1] - H[3];
  double a12 = H[1] + H[3], a13 = H[6] + H[2], a23 = H[5] + H[7];
  for (int sweep = 0; sweep < EVAL_SWEEPS; sweep++) {
    const double off = fabs(a01) + fabs(a02) + fabs(a03) + fabs(a12) + fabs(a13) + fabs(a23);
    const double dia = fabs(a00) + fabs(a11) + fabs(a22) + fabs(a33);
    if (off <= 0x1p-70 * dia) break;                              // (also H = 0; an eigenvalue moves by at most 2 off)
    eval_rotate(a00, a11, a01, a02, a12, a03, a13);
    eval_rotate(a00, a22, a02, a01, a12, a03, a23);
    eval_rotate(a00, a33, a03, a01, a13, a02, a23);
    eval_rotate(a11, a22, a12, a01, a02, a13, a23);
    eval_rotate(a11, a33, a13, a01, a03, a12, a23);
    eval_rotate(a22, a33, a23, a02, a03, a12, a13);
  }
  double l = a00;
  l = a11 > l ? a11 : l;
  l = a22 > l ? a22 : l;
  l = a33 > l ? a33 : l;
  return l;
}

DLPD_D double eval_norm2(const double* v) { return fma(v[2], v[2], fma(v[1], v[1], v[0] * v[0])); }
DLPD_D double eval_dot(const double* a, const double* b) { return fma(a[2], b[2], fma(a[1], b[1], a[0] * b[0])); }
// sum_i r_i^T C r_i: sum |R y|^2 from the second moments C (xx xy xz yy yz zz) of y
DLPD_D double eval_energy(const double* R, const double* C) {
  double e = 0.0;
#pragma unroll
  for (int i = 0; i < 3; i++) {
    const double x = R[3 * i], y = R[3 * i + 1], z = R[3 * i + 2];
    e += fma(x, fma(x, C[0], 2.0 * fma(y, C[1], z * C[2])), fma(y, fma(y, C[3], 2.0 * z * C[4]), z * z * C[5]));
  }
  return e;
}
// u = t + R c - o
DLPD_D void eval_offset(const double* R, const double* t, const double* c, const double* o, double* u) {
#pragma unroll
  for (int i = 0; i < 3; i++) u[i] = fma(R[3 * i + 2], c[2], fma(R[3 * i + 1], c[1], fma(R[3 * i], c[0], t[i]))) - o[i];
}

// one pose per thread; the moment block in LDS: every lane reads the same address (a broadcast)
__global__ void __launch_bounds__(EVAL_NT) k_pose_native_rmsd(const double* __restrict__ poses, const double* __restrict__ moments,
                                                              eval_counts cnt, int nI, int K, double* __restrict__ irmsd,
                                                              double* __restrict__ lrmsd) {
  __shared__ double mom[(EVAL_MAXI + 1) * EVAL_REC];
  const int tid = threadIdx.x, k = blockIdx.x * EVAL_NT + tid;
  for (int q = tid; q < (nI + 1) * EVAL_REC; q += EVAL_NT) mom[q] = moments[q];
  __syncthreads();
  if (k >= K) return;
  double R[9], t[3];
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = poses[(size_t)k * 12 + i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = poses[(size_t)k * 12 + 9 + i];
  double best = 0.0;
  for (int p = 0; p < nI; p++) {
    const double* m = mom + p * EVAL_REC;
    const double* A = m, *Y = m + 9, *s = m + 18, *sa = m + 21, *sy = m + 24;
    const double nl = (double)cnt.nl[p], nr = (double)cnt.nr[p], n = nl + nr;
    double u[3], H[9], Rsy[3], w[3], v[3];
    eval_offset(R, t, m + 33, m + 30, u);
#pragma unroll
    for (int i = 0; i < 3; i++) {
#pragma unroll
      for (int j = 0; j < 3; j++)
        H[3 * i + j] = fma(u[i], s[j], fma(R[3 * i + 2], Y[6 + j], fma(R[3 * i + 1], Y[3 + j], fma(R[3 * i], Y[j], A[3 * i + j]))));
      Rsy[i] = eval_dot(R + 3 * i, sy);
      w[i] = sa[i] + Rsy[i];
      v[i] = fma(-nl / n, w[i], Rsy[i]);
    }
    const double Gp = m[27] + eval_energy(R, m + 36) + 2.0 * eval_dot(u, v) - eval_norm2(w) / n + (nl * nr / n) * eval_norm2(u);
    const double e = Gp + m[29] - 2.0 * eval_lambda(H);
    const double r2 = (e < 0.0 ? 0.0 : e) / n;                    // (not fmax: a pose that is not a number stays one)
    if (p == 0 || !(r2 >= best)) best = r2;
  }
  irmsd[k] = sqrt(best);
  {
    const double* m = mom + nI * EVAL_REC;
    const double nl = (double)cnt.nl[nI];
    double u[3], v[3], rm = 0.0;
    eval_offset(R, t, m + 17, m + 20, u);
#pragma unroll
    for (int i = 0; i < 3; i++) v[i] = eval_dot(R + 3 * i, m + 9) - m[12 + i];
#pragma unroll
    for (int i = 0; i < 9; i++) rm = fma(R[i], m[i], rm);
    const double e = eval_energy(R, m + 23) + m[16] + nl * eval_norm2(u) + 2.0 * eval_dot(u, v) - 2.0 * rm;
    lrmsd[k] = sqrt((e < 0.0 ? 0.0 : e) / nl);
  }
}

// The contact predicate, shared with k_pose_contacts_all (dlpd_contacts.h): the pose rounded to float32 once, a posed atom by
// one fma chain per coordinate, d^2 by one fma chain over the three differences, d2 <= r2.
DLPD_D void eval_pose32(const double* __restrict__ P, float* R, float* t) {
#pragma unroll
  for (int i = 0; i < 9; i++) R[i] = (float)P[i];
#pragma unroll
  for (int i = 0; i < 3; i++) t[i] = (float)P[9 + i];
}
// p = R y + t: the chain t -> fma(R0, x, .) -> fma(R1, y, .) -> fma(R2, z, .) per coordinate
DLPD_D void eval_pose_point(const float* R, const float* t, const float* __restrict__ y, float* p) {
  const float x = y[0], yy = y[1], z = y[2];
#pragma unroll
  for (int i = 0; i < 3; i++) p[i] = __fmaf_rn(R[3 * i + 2], z, __fmaf_rn(R[3 * i + 1], yy, __fmaf_rn(R[3 * i], x, t[i])));
}
// some atom pair of rec [r0, r1) x posed [l0, l1) has d^2 <= r2
DLPD_D bool eval_ranges_touch(const float* __restrict__ rec, int r0, int r1, const float* posed, int l0, int l1, float r2) {
  for (int i = r0; i < r1; i++) {
    const float a[3] = {rec[3 * i], rec[3 * i + 1], rec[3 * i + 2]};
    for (int j = l0; j < l1; j++) {
      float d2 = 0.f;
#pragma unroll
      for (int q = 0; q < 3; q++) {
        const float d = a[q] - posed[3 * j + q];
        d2 = __fmaf_rn(d, d, d2);
      }
      if (d2 <= r2) return true;
    }
  }
  return false;
}

// one pose per block; CAP: the posed ligand's room in LDS
template <int CAP>
__global__ void __launch_bounds__(EVAL_CONTACT_NT) k_pose_native_contacts(const double* __restrict__ poses, const float* __restrict__ rec,
                                                                          const float* __restrict__ lig, const int* __restrict__ ranges,
                                                                          int NRa, int NLa, int C, float r2, int* __restrict__ count) {
  __shared__ float posed[CAP * 3];
  __shared__ int s_cnt[EVAL_CONTACT_NT / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float R[9], t[3];
  eval_pose32(poses + (size_t)blockIdx.x * 12, R, t);
  for (int j = tid; j < NLa; j += EVAL_CONTACT_NT) eval_pose_point(R, t, lig + 3 * j, posed + 3 * j);
  __syncthreads();
  int n = 0;
  for (int c = tid; c < C; c += EVAL_CONTACT_NT) {
    const int r0 = max(ranges[4 * c], 0), r1 = min(ranges[4 * c + 1], NRa);       // (clamped: never outside the arrays)
    const int l0 = max(ranges[4 * c + 2], 0), l1 = min(ranges[4 * c + 3], NLa);
    n += eval_ranges_touch(rec, r0, r1, posed, l0, l1, r2) ? 1 : 0;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) n += __shfl_xor(n, m);
  if (lane == 0) s_cnt[wave] = n;
  __syncthreads();
  if (tid == 0) {
    int total = s_cnt[0];
#pragma unroll
    for (int q = 1; q < EVAL_CONTACT_NT / 64; q++) total += s_cnt[q];
    count[blockIdx.x] = total;
  }
}

// fnat = count / (C + 0.001) (processing_utils.py:222) and the class cascade (:226-236): three successive, independent ifs
__global__ void __launch_bounds__(EVAL_NT) k_pose_capri(const int* __restrict__ count, const double* __restrict__ irmsd,
                                                        const double* __restrict__ lrmsd, int C, int K, double* __restrict__ fnat,
                                                        int* __restrict__ capri) {
  const int k = blockIdx.x * EVAL_NT + threadIdx.x;
  if (k >= K) return;
  const double f = (double)count[k] / ((double)C + 0.001), l = lrmsd[k], i = irmsd[k];
  int cls = 0;
  if ((f >= 0.1 && l <= 10.0) || i <= 4.0) cls = 1;
  if ((f >= 0.3 && l <= 5.0) || i <= 2.0) cls = 2;
  if ((f >= 0.5 && l <= 1.0) || i <= 1.0) cls = 3;
  fnat[k] = f;
  capri[k] = cls;
}

extern "C" {

/* irmsd, lrmsd (K) of K poses against the moment block; counts: HOST array of (nI + 1) x (nr, nl) */
int dlpd_pose_native_rmsd(const double* poses, int K, const double* moments, const int* counts, int nI, double* irmsd, double* lrmsd,
                          void* stream) {
  if (!poses || !moments || !counts || !irmsd || !lrmsd || K <= 0 || nI <= 0) return DLPD_ERR_ARG;
  if (nI > EVAL_MAXI || K > CLUSTER_MAXK) return DLPD_ERR_UNSUPPORTED;
  eval_counts cnt;
  for (int p = 0; p <= EVAL_MAXI; p++) cnt.nr[p] = cnt.nl[p] = 0;
  for (int p = 0; p <= nI; p++) {
    cnt.nr[p] = p < nI ? counts[2 * p] : 0;
    cnt.nl[p] = counts[2 * p + 1];
    if (cnt.nr[p] < 0 || cnt.nl[p] < 1) return DLPD_ERR_ARG;
  }
  DLPD_LAUNCH(k_pose_native_rmsd, dim3((K + EVAL_NT - 1) / EVAL_NT), dim3(EVAL_NT), 0, (hipStream_t)stream, poses, moments, cnt, nI, K,
              irmsd, lrmsd);
  return dlpd_check_launch();
}

/* count (K) = the native contacts that hold under each pose; ranges: (C, 4) int32 on the device, ranges_host: the same in
 * host memory (what is checked here) */
int dlpd_pose_native_contacts(const double* poses, int K, const float* rec_atoms, int NRa, const float* lig_atoms, int NLa,
                              const int* ranges, const int* ranges_host, int C, float cutoff, int* count, void* stream) {
  if (!poses || !count || K <= 0 || C < 0 || NRa < 0 || NLa < 0 || !(cutoff >= 0.f)) return DLPD_ERR_ARG;   // (NaN fails too)
  if (C > 0 && (!rec_atoms || !lig_atoms || !ranges || !ranges_host)) return DLPD_ERR_ARG;
  if (K > CLUSTER_MAXK || C > EVAL_MAXC || NRa > EVAL_MAXREC || NLa > EVAL_MAXLIG) return DLPD_ERR_UNSUPPORTED;
  for (int c = 0; c < C; c++) {
    const int* r = ranges_host + 4 * c;
    if (r[0] < 0 || r[0] >= r[1] || r[1] > NRa || r[2] < 0 || r[2] >= r[3] || r[3] > NLa) return DLPD_ERR_ARG;
  }
  if (NLa <= EVAL_SMALLLIG)
    DLPD_LAUNCH((k_pose_native_contacts<EVAL_SMALLLIG>), dim3(K), dim3(EVAL_CONTACT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                lig_atoms, ranges, NRa, NLa, C, cutoff * cutoff, count);
  else
    DLPD_LAUNCH((k_pose_native_contacts<EVAL_MAXLIG>), dim3(K), dim3(EVAL_CONTACT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                lig_atoms, ranges, NRa, NLa, C, cutoff * cutoff, count);
  return dlpd_check_launch();
}

/* fnat (K) float64 and capri (K) int32 from the counts of C native contacts and the two RMSDs */
int dlpd_pose_capri(const int* count, const double* irmsd, const double* lrmsd, int C, int K, double* fnat, int* capri, void* stream) {
  if (!count || !irmsd || !lrmsd || !fnat || !capri || K <= 0 || C < 0) return DLPD_ERR_ARG;
  if (K > CLUSTER_MAXK || C > EVAL_MAXC) return DLPD_ERR_UNSUPPORTED;
  DLPD_LAUNCH(k_pose_capri, dim3((K + EVAL_NT - 1) / EVAL_NT), dim3(EVAL_NT), 0, (hipStream_t)stream, count, irmsd, lrmsd, C, K, fnat,
              capri);
  return dlpd_check_launch();
}

}  // extern "C"

// All residue contacts of a posed complex, for every pose of a list: what scripts/Dataset/processing_utils.py:
// 183-216 finds per decoy with a neighbour search over every atom of both proteins, and what its fnonnat (:219-224) is made of.
// Included by dlpd_topk.hip after dlpd_evaluate.h, whose contact predicate (eval_pose32, eval_pose_point, eval_ranges_touch)
// it shares bit for bit with k_pose_native_contacts.
//
// For a pose, dec = the residue pairs (rho of the receptor, lambda of the ligand) with some atom pair at d^2 <= r^2 in float32,
// nat = the native pairs, handed over as a bitmap over (lambda, rho): bit (rho & 31) of bits[lambda * W + (rho >> 5)],
// W = ceil(NRres / 32) -- a set, a pair named twice is one bit.  Per pose: n_dec = |dec|, n_corr = |dec & nat|.
//
// One pose per block of CONT_NT threads.  The ligand's atoms and the centres of its residues' bounding spheres are posed once
// into LDS.  Wave w takes the receptor residues w, w + CONT_NT / 64, ...; a residue whose sphere misses the sphere of the whole
// ligand is left at once (a wave-uniform branch); otherwise the lanes take the ligand's residues, test the two spheres, and
// the survivors run the atom loop with its early exit.  A hit looks up the bitmap.  Counts: a butterfly per wave, one plain LDS
// word per wave and a barrier (no LDS atomic).
//
// THE SPHERE TEST never rejects a pair the predicate accepts.  u = 2^-24.  The host packs, per residue, a centre c (float32)
// and a radius rounded UP to float32 that covers every float32 atom of the residue about that centre; for the whole ligand
// likewise (row NLres of lig_sph), and ``lig_extent`` >= |y|_2 of every ligand atom and centre.  The pose's matrix R (float32)
// need not be a rotation: s = 1 + delta / 2 + 2^-18 (1 + |R|_F^2), delta = |R^T R - I|_F in float32, bounds |R|_2
// (|R|_2^2 <= 1 + |R^T R - I|_2; the last term covers the rounding of delta itself).  With Mk = |t|_inf + s lig_extent:
//   a posed atom p and a posed centre pc are each three fma away from R y + t: at most sqrt(3) 3 u Mk each, so
//   |p - pc| <= s Rl + 10.4 u Mk;
//   the predicate's d^2 carries the rounding of the differences and of its chain: d^2_32 >= d^2 (1 - u)^5, and r = sqrtf(r2)
//   one more: a pair it accepts has d <= r (1 + 4 u);
//   so an accepted pair has |a - p| <= r (1 + 4 u) and its centres lie within r (1 + 4 u) + Rr + s Rl + 10.4 u Mk.
// The test rejects iff dc^2_32 > B^2 with B = (r + Rr + s Rl) (1 + 2^-19) + 2^-19 Mk: 32 u of relative slack against the 4 u
// above, the 3 u of dc_32 and the five roundings of B, and 32 u Mk against 10.4 u Mk.  It is written as a comparison that is
// false for a NaN: a pose that is not a number reaches the predicate, which decides.  At Mk = 100 A the padding is 2e-4 A.
#pragma once

#define CONT_NT 256                   // threads per pose
#define CONT_MAXLIG 8192              // ligand atoms (96 KB of LDS) ...
#define CONT_MAXLRES 1024             // ... and residues (16 + 4 KB)
#define CONT_SMALLLIG 2048            // the instance typical ligands take (24 + 8 + 2 KB: four blocks per CU)
#define CONT_SMALLLRES 512
#define CONT_MAXREC 65536             // receptor atoms
#define CONT_MAXRRES 8192             // receptor residues

DLPD_D float cont_norm_bound(const float* R) {
  float delta2 = 0.f, f2 = 0.f;
#pragma unroll
  for (int i = 0; i < 3; i++) {
#pragma unroll
    for (int j = 0; j < 3; j++) {
      const float g = __fmaf_rn(R[6 + i], R[6 + j], __fmaf_rn(R[3 + i], R[3 + j], R[i] * R[j])) - (i == j ? 1.f : 0.f);
      delta2 = __fmaf_rn(g, g, delta2);
      f2 = __fmaf_rn(R[3 * i + j], R[3 * i + j], f2);
    }
  }
  return 1.f + 0.5f * sqrtf(delta2) + 0x1p-18f * (1.f + f2);
}

// NOT (centre distance^2 > B^2): false only where the two spheres are certainly further apart than the cutoff
DLPD_D bool cont_spheres_near(const float* a, const float* b, float B) {
  float d2 = 0.f;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const float d = a[q] - b[q];
    d2 = __fmaf_rn(d, d, d2);
  }
  return !(d2 > B * B);
}

template <int CAPA, int CAPR>
__global__ void __launch_bounds__(CONT_NT) k_pose_contacts_all(const double* __restrict__ poses, const float* __restrict__ rec,
                                                               const int* __restrict__ rec_off, const float* __restrict__ rec_sph,
                                                               int NRa, int NRres, const float* __restrict__ lig,
                                                               const int* __restrict__ lig_off, const float* __restrict__ lig_sph,
                                                               int NLa, int NLres, const unsigned* __restrict__ bits, float lig_extent,
                                                               float r2, int* __restrict__ n_dec, int* __restrict__ n_corr) {
  __shared__ float posed[CAPA * 3];
  __shared__ float centre[CAPR * 4];                                 // posed centre, then s Rl
  __shared__ int s_off[CAPR + 1];
  __shared__ int s_cnt[2 * (CONT_NT / 64)];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  float R[9], t[3];
  eval_pose32(poses + (size_t)blockIdx.x * 12, R, t);
  const float s = cont_norm_bound(R);
  const float Mk = fmaxf(fabsf(t[0]), fmaxf(fabsf(t[1]), fabsf(t[2]))) + s * lig_extent;
  const float r = sqrtf(r2), pad = 0x1p-19f * Mk, grow = 1.f + 0x1p-19f;
  for (int j = tid; j < NLa; j += CONT_NT) eval_pose_point(R, t, lig + 3 * j, posed + 3 * j);
  for (int l = tid; l < NLres; l += CONT_NT) {
    eval_pose_point(R, t, lig_sph + 4 * l, centre + 4 * l);
    centre[4 * l + 3] = s * lig_sph[4 * l + 3];
  }
  for (int l = tid; l <= NLres; l += CONT_NT) s_off[l] = min(max(lig_off[l], 0), NLa);      // (clamped: never outside the arrays)
  float whole[3];
  eval_pose_point(R, t, lig_sph + 4 * NLres, whole);
  const float whole_r = s * lig_sph[4 * NLres + 3];
  __syncthreads();
  const int W = (NRres + 31) >> 5;
  int dec = 0, corr = 0;
  for (int rho = wave; rho < NRres; rho += CONT_NT / 64) {
    const float c[3] = {rec_sph[4 * rho], rec_sph[4 * rho + 1], rec_sph[4 * rho + 2]};
    const float Rr = rec_sph[4 * rho + 3];
    if (!cont_spheres_near(c, whole, (r + Rr + whole_r) * grow + pad)) continue;
    const int r0 = min(max(rec_off[rho], 0), NRa), r1 = min(max(rec_off[rho + 1], 0), NRa);
    for (int l = lane; l < NLres; l += 64) {
      if (!cont_spheres_near(c, centre + 4 * l, (r + Rr + centre[4 * l + 3]) * grow + pad)) continue;
      if (!eval_ranges_touch(rec, r0, r1, posed, s_off[l], s_off[l + 1], r2)) continue;
      dec++;
      corr += (int)((bits[(size_t)l * W + (rho >> 5)] >> (rho & 31)) & 1u);
    }
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    dec += __shfl_xor(dec, m);
    corr += __shfl_xor(corr, m);
  }
  if (lane == 0) {
    s_cnt[2 * wave] = dec;
    s_cnt[2 * wave + 1] = corr;
  }
  __syncthreads();
  if (tid == 0) {
    int d = 0, c = 0;
#pragma unroll
    for (int q = 0; q < CONT_NT / 64; q++) {
      d += s_cnt[2 * q];
      c += s_cnt[2 * q + 1];
    }
    n_dec[blockIdx.x] = d;
    n_corr[blockIdx.x] = c;
  }
}

static bool cont_offsets_ok(const int* off, int nres, int natoms) {
  if (off[0] < 0 || off[nres] > natoms) return false;
  for (int i = 0; i < nres; i++)
    if (off[i] > off[i + 1]) return false;
  return true;
}

extern "C" {

/* n_dec, n_corr (K) int32: the residue pairs in contact under each pose, and those of them the native bitmap names */
int dlpd_pose_contacts_all(const double* poses, int K, const float* rec_atoms, const int* rec_off, const float* rec_sph, int NRa,
                           int NRres, const float* lig_atoms, const int* lig_off, const float* lig_sph, int NLa, int NLres,
                           const int* rec_off_host, const int* lig_off_host, const unsigned* native_bits, float lig_extent,
                           float cutoff, int* n_dec, int* n_corr, void* stream) {
  if (K < 0 || NRa < 1 || NRres < 1 || NLa < 1 || NLres < 1 || !(cutoff >= 0.f) || !(lig_extent >= 0.f)) return DLPD_ERR_ARG;
  if (K > CLUSTER_MAXK || NRa > CONT_MAXREC || NRres > CONT_MAXRRES || NLa > CONT_MAXLIG || NLres > CONT_MAXLRES)
    return DLPD_ERR_UNSUPPORTED;
  if (!poses || !rec_atoms || !rec_off || !rec_sph || !lig_atoms || !lig_off || !lig_sph || !rec_off_host || !lig_off_host ||
      !native_bits || !n_dec || !n_corr)
    return DLPD_ERR_ARG;
  if (!cont_offsets_ok(rec_off_host, NRres, NRa) || !cont_offsets_ok(lig_off_host, NLres, NLa)) return DLPD_ERR_ARG;
  if (K == 0) return DLPD_OK;
  if (NLa <= CONT_SMALLLIG && NLres <= CONT_SMALLLRES)
    DLPD_LAUNCH((k_pose_contacts_all<CONT_SMALLLIG, CONT_SMALLLRES>), dim3(K), dim3(CONT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                rec_off, rec_sph, NRa, NRres, lig_atoms, lig_off, lig_sph, NLa, NLres, native_bits, lig_extent, cutoff * cutoff, n_dec,
                n_corr);
  else
    DLPD_LAUNCH((k_pose_contacts_all<CONT_MAXLIG, CONT_MAXLRES>), dim3(K), dim3(CONT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                rec_off, rec_sph, NRa, NRres, lig_atoms, lig_off, lig_sph, NLa, NLres, native_bits, lig_extent, cutoff * cutoff, n_dec,
                n_corr);
  return dlpd_check_launch();
}

}  // extern "C"

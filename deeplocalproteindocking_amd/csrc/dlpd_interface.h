// The interface of every pose of a list as a device object (BUILD-DEFINED: the reference has no counterpart): which
// residues of each protein a pose puts within the cutoff of the partner, and two consumers of those residue sets -- weighted
// residue frequencies over the list, and the neighbour bitmap of interface similarity that k_pose_scan (dlpd_cluster.h) clusters.
// Included by dlpd_topk.hip after dlpd_contacts.h, whose predicate (eval_pose32, eval_pose_point, eval_ranges_touch) and sphere
// pre-tests (cont_spheres_near with cont_norm_bound: they never drop a pair the predicate accepts) it uses unchanged.
//
//   k_pose_residue_bits   one pose per block -> rec_bits (K, Wr), lig_bits (K, Wl) uint32, Wr = ceil(NRres / 32), Wl = ceil(NLres / 32):
//                         bit (i & 31) of word i >> 5 is set iff residue i has an atom with d^2 <= r^2 (float32) to some atom of the
//                         partner.  Every word of every pose is written, the bits at and above NRres / NLres as zero.
//   k_interface_profile   count[j] = the poses that mark residue j (int32), freq[j] = sum_k weights[k] bit(k, j) (float64), the sum in
//                         an order that depends on K alone (below)
//   k_interface_within    the K x K bitmap of |F_i & F_j| 1024 >= q |F_i | F_j| over the fingerprints F = (rec words, lig words), in
//                         the layout of k_pose_within
//
// k_pose_residue_bits.  The work of k_pose_contacts_all, pair for pair, dealt the same way (wave w takes the receptor residues
// w, w + 4, ...; the lanes take the ligand's residues lane + 64 j), so the two cost the same; only what a hit does differs, and
// it needs no atomic.  RECEPTOR: whether residue rho is marked is one OR butterfly over the wave; lane 0 then sets the bit in a row
// of LDS words that belongs to its wave alone (a plain read-modify-write by one lane).  After the barrier the four rows are ORed and
// stored, a word per thread.  LIGAND: a lane keeps a register mask, bit j for residue lane + 64 j (16 bits at 1,024 residues);
// each lane writes its mask to a word of its own, and after the barrier wave 0 ORs the four and re-lays them into residue order:
// the ballot of bit j over the 64 lanes IS the words 2 j and 2 j + 1.  Padding bits are never set: no lane tests a residue past
// the end.  (Skipping a pair whose two residues are both marked already is not built: a lane knows the receptor residue's mark
// only after the wave's butterfly, and a collective inside the inner loop costs more than the rare skip saves.)
//
// k_interface_profile.  A thread owns a residue, a block row a chunk of IFACE_CHUNK = 1,024 poses: s = +0; for k ascending in the
// chunk: if bit(k, j) then s = s + weights[k] (an addition, never a product); the partial goes to the workspace.  A second
// launch adds the partials of a residue in ascending chunk order, starting from the first partial.  No atomics; a host loop in
// that order reproduces freq bit for bit, for any weights.
//
// k_interface_within.  Integer work only.  |F_i | F_j| = |F_i| + |F_j| - |F_i & F_j|, so the loop is one AND and one population
// count per word pair.  Block (256 rows, 8 words = 512 columns) as k_pose_within: a thread owns a row; per output word the 64
// columns' fingerprints are staged in LDS IFACE_C words at a time (every lane reads the same address: a broadcast), the thread's
// own words of that chunk sit in registers, 64 counters in registers.  Two empty fingerprints are neighbours (0 >= q 0), the
// diagonal is set (|F| 1024 >= q |F| for q <= 1024), the test is symmetric in i and j: no special case.  The eight words of a row are
// transposed through LDS and stored as k_pose_within stores them.
#pragma once

#define IFACE_MAXWR (CONT_MAXRRES / 32)   // words of a receptor bitmap row (256)
#define IFACE_MAXWL (CONT_MAXLRES / 32)   // ... of a ligand row (32)
#define IFACE_CHUNK 1024                  // poses per partial sum of the profile
#define IFACE_C 8                         // fingerprint words staged per step of k_interface_within
#define IFACE_QONE 1024                   // the similarity threshold is q / 1024

// (the CPU harness has no __popc; the builtin is what __popc is made of)
DLPD_D int iface_popc(unsigned v) { return __builtin_popcount(v); }

template <int CAPA, int CAPR>
__global__ void __launch_bounds__(CONT_NT) k_pose_residue_bits(const double* __restrict__ poses, const float* __restrict__ rec,
                                                               const int* __restrict__ rec_off, const float* __restrict__ rec_sph,
                                                               int NRa, int NRres, const float* __restrict__ lig,
                                                               const int* __restrict__ lig_off, const float* __restrict__ lig_sph,
                                                               int NLa, int NLres, float lig_extent, float r2,
                                                               unsigned* __restrict__ rec_bits, unsigned* __restrict__ lig_bits) {
  __shared__ float posed[CAPA * 3];
  __shared__ float centre[CAPR * 4];                                 // posed centre, then s Rl
  __shared__ int s_off[CAPR + 1];
  __shared__ unsigned s_rec[(CONT_NT / 64) * IFACE_MAXWR];           // a row of receptor words per wave
  __shared__ unsigned s_lig[CONT_NT];                                // a ligand mask per lane
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
  const int Wr = (NRres + 31) >> 5, Wl = (NLres + 31) >> 5;
  for (int w = tid; w < Wr; w += CONT_NT) {
#pragma unroll
    for (int q = 0; q < CONT_NT / 64; q++) s_rec[q * IFACE_MAXWR + w] = 0u;
  }
  float whole[3];
  eval_pose_point(R, t, lig_sph + 4 * NLres, whole);
  const float whole_r = s * lig_sph[4 * NLres + 3];
  __syncthreads();
  unsigned lmask = 0u;
  for (int rho = wave; rho < NRres; rho += CONT_NT / 64) {
    const float c[3] = {rec_sph[4 * rho], rec_sph[4 * rho + 1], rec_sph[4 * rho + 2]};
    const float Rr = rec_sph[4 * rho + 3];
    if (!cont_spheres_near(c, whole, (r + Rr + whole_r) * grow + pad)) continue;          // (the same for the whole wave)
    const int r0 = min(max(rec_off[rho], 0), NRa), r1 = min(max(rec_off[rho + 1], 0), NRa);
    int hit = 0;
    for (int j = 0; j < CAPR / 64; j++) {
      const int l = lane + 64 * j;
      if (l >= NLres) break;
      if (!cont_spheres_near(c, centre + 4 * l, (r + Rr + centre[4 * l + 3]) * grow + pad)) continue;
      if (!eval_ranges_touch(rec, r0, r1, posed, s_off[l], s_off[l + 1], r2)) continue;
      hit = 1;
      lmask |= 1u << j;
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) hit |= __shfl_xor(hit, m);
    if (hit && lane == 0) s_rec[wave * IFACE_MAXWR + (rho >> 5)] |= 1u << (rho & 31);
  }
  s_lig[tid] = lmask;
  __syncthreads();
  for (int w = tid; w < Wr; w += CONT_NT) {
    unsigned v = 0u;
#pragma unroll
    for (int q = 0; q < CONT_NT / 64; q++) v |= s_rec[q * IFACE_MAXWR + w];
    rec_bits[(size_t)blockIdx.x * Wr + w] = v;
  }
  if (wave == 0) {
    unsigned m = 0u;
#pragma unroll
    for (int q = 0; q < CONT_NT / 64; q++) m |= s_lig[64 * q + lane];
    for (int j = 0; 64 * j < NLres; j++) {                          // residues 64 j .. 64 j + 63: the words 2 j and 2 j + 1
      const unsigned long long b = __ballot((int)((m >> j) & 1u));
      if (lane < 2 && 2 * j + lane < Wl) lig_bits[(size_t)blockIdx.x * Wl + 2 * j + lane] = (unsigned)(b >> (32 * lane));
    }
  }
}

// grid (ceil(max(NRres, NLres) / 256), chunks, 2 sides); part_freq / part_count: (chunks, NRres + NLres), the receptor's columns first
__global__ void __launch_bounds__(CLUSTER_NT) k_interface_profile(const unsigned* __restrict__ rec_bits, const unsigned* __restrict__ lig_bits,
                                                                  int K, int NRres, int NLres, const double* __restrict__ weights,
                                                                  double* __restrict__ part_freq, int* __restrict__ part_count) {
  const int side = blockIdx.z, n = side ? NLres : NRres, j = blockIdx.x * CLUSTER_NT + threadIdx.x;
  if (j >= n) return;
  const int W = (n + 31) >> 5, sh = j & 31;
  const int k0 = blockIdx.y * IFACE_CHUNK, k1 = min(K, k0 + IFACE_CHUNK);
  const unsigned* p = (side ? lig_bits : rec_bits) + (size_t)k0 * W + (j >> 5);
  double sum = 0.0;
  int cnt = 0;
  for (int k = k0; k < k1; k++, p += W) {
    const bool set = (*p >> sh) & 1u;
    const double w = weights[k];
    sum = set ? sum + w : sum;
    cnt += set ? 1 : 0;
  }
  const size_t at = (size_t)blockIdx.y * (NRres + NLres) + (side ? NRres : 0) + j;
  part_freq[at] = sum;
  part_count[at] = cnt;
}

// the partials of a residue, chunks ascending
__global__ void __launch_bounds__(CLUSTER_NT) k_interface_profile_sum(const double* __restrict__ part_freq, const int* __restrict__ part_count,
                                                                      int chunks, int NRres, int NLres, double* __restrict__ rec_freq,
                                                                      double* __restrict__ lig_freq, int* __restrict__ rec_count,
                                                                      int* __restrict__ lig_count) {
  const int n = NRres + NLres, col = blockIdx.x * CLUSTER_NT + threadIdx.x;
  if (col >= n) return;
  double sum = part_freq[col];
  int cnt = part_count[col];
  for (int c = 1; c < chunks; c++) {
    sum += part_freq[(size_t)c * n + col];
    cnt += part_count[(size_t)c * n + col];
  }
  if (col < NRres) {
    rec_freq[col] = sum;
    rec_count[col] = cnt;
  } else {
    lig_freq[col - NRres] = sum;
    lig_count[col - NRres] = cnt;
  }
}

// word f of pose p's fingerprint: the receptor's words, then the ligand's; zero past the end
DLPD_D unsigned iface_word(const unsigned* __restrict__ rec_bits, const unsigned* __restrict__ lig_bits, int Wr, int Wl, int p, int f) {
  if (f < Wr) return rec_bits[(size_t)p * Wr + f];
  f -= Wr;
  return f < Wl ? lig_bits[(size_t)p * Wl + f] : 0u;
}

__global__ void __launch_bounds__(CLUSTER_NT) k_interface_within(const unsigned* __restrict__ rec_bits, const unsigned* __restrict__ lig_bits,
                                                                 int K, int Wr, int Wl, int q, cl_u64* __restrict__ mask, int W) {
  __shared__ __attribute__((aligned(16))) unsigned cols[64 * IFACE_C];
  __shared__ int colpop[CLUSTER_CW * 64];
  __shared__ cl_u64 words[CLUSTER_NT * (CLUSTER_CW + 1)];          // (+1: rows on different banks)
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * CLUSTER_CW, i0 = blockIdx.y * CLUSTER_NT, i = i0 + tid;
  const int F = Wr + Wl;
  for (int c = tid; c < CLUSTER_CW * 64; c += CLUSTER_NT) {         // |F_j| of the block's columns (read after the loop's barriers)
    const int j = w0 * 64 + c;
    int n = 0;
    if (j < K)
      for (int f = 0; f < F; f++) n += iface_popc(iface_word(rec_bits, lig_bits, Wr, Wl, j, f));
    colpop[c] = n;
  }
  for (int w = 0; w < CLUSTER_CW; w++) {
    const int j0 = (w0 + w) * 64;
    const int nb = min(64, K - j0);                                // valid columns of this word (<= 0: none); the same for the block
    cl_u64 word = 0;
    if (nb > 0) {
      int acc[64];
#pragma unroll
      for (int b = 0; b < 64; b++) acc[b] = 0;
      int pa = 0;
      for (int f0 = 0; f0 < F; f0 += IFACE_C) {
        __syncthreads();                                           // the last tile has been read
        for (int x = tid; x < 64 * IFACE_C; x += CLUSTER_NT) {
          const int b = x / IFACE_C, c = x % IFACE_C;
          cols[x] = (b < nb) ? iface_word(rec_bits, lig_bits, Wr, Wl, j0 + b, f0 + c) : 0u;
        }
        unsigned a[IFACE_C];
#pragma unroll
        for (int c = 0; c < IFACE_C; c++) {
          a[c] = (i < K) ? iface_word(rec_bits, lig_bits, Wr, Wl, i, f0 + c) : 0u;
          pa += iface_popc(a[c]);
        }
        __syncthreads();
#pragma unroll
        for (int b = 0; b < 64; b++) {
#pragma unroll
          for (int c = 0; c < IFACE_C; c++) acc[b] += iface_popc(a[c] & cols[b * IFACE_C + c]);
        }
      }
#pragma unroll
      for (int b = 0; b < 64; b++) {
        const int uni = pa + colpop[w * 64 + b] - acc[b];
        word |= (cl_u64)(b < nb && acc[b] * IFACE_QONE >= q * uni) << b;
      }
    }
    words[tid * (CLUSTER_CW + 1) + w] = word;
  }
  __syncthreads();
  for (int x = tid; x < CLUSTER_NT * CLUSTER_CW; x += CLUSTER_NT) {
    const int r = x / CLUSTER_CW, w = x % CLUSTER_CW;
    if (i0 + r < K && w0 + w < W) mask[(size_t)(i0 + r) * W + w0 + w] = words[r * (CLUSTER_CW + 1) + w];
  }
}

static int iface_check(int K, int Wr, int Wl, int q) {
  if (K < 0 || Wr < 0 || Wl < 0 || Wr + Wl < 1 || q < 0 || q > IFACE_QONE) return DLPD_ERR_ARG;
  return (K > CLUSTER_MAXK || Wr > IFACE_MAXWR || Wl > IFACE_MAXWL) ? DLPD_ERR_UNSUPPORTED : DLPD_OK;
}

static void iface_within(const unsigned* rec_bits, const unsigned* lig_bits, int K, int Wr, int Wl, int q, cl_u64* mask, hipStream_t st) {
  const int W = cluster_words(K);
  DLPD_LAUNCH(k_interface_within, dim3((W + CLUSTER_CW - 1) / CLUSTER_CW, (K + CLUSTER_NT - 1) / CLUSTER_NT), dim3(CLUSTER_NT), 0, st,
              rec_bits, lig_bits, K, Wr, Wl, q, mask, W);
}

extern "C" {

/* rec_bits (K, ceil(NRres / 32)), lig_bits (K, ceil(NLres / 32)) uint32: the residues of each side in contact under each pose */
int dlpd_pose_residue_bits(const double* poses, int K, const float* rec_atoms, const int* rec_off, const float* rec_sph, int NRa,
                           int NRres, const float* lig_atoms, const int* lig_off, const float* lig_sph, int NLa, int NLres,
                           const int* rec_off_host, const int* lig_off_host, float lig_extent, float cutoff, unsigned* rec_bits,
                           unsigned* lig_bits, void* stream) {
  if (K < 0 || NRa < 1 || NRres < 1 || NLa < 1 || NLres < 1 || !(cutoff >= 0.f) || !(lig_extent >= 0.f)) return DLPD_ERR_ARG;
  if (K > CLUSTER_MAXK || NRa > CONT_MAXREC || NRres > CONT_MAXRRES || NLa > CONT_MAXLIG || NLres > CONT_MAXLRES)
    return DLPD_ERR_UNSUPPORTED;
  if (!poses || !rec_atoms || !rec_off || !rec_sph || !lig_atoms || !lig_off || !lig_sph || !rec_off_host || !lig_off_host ||
      !rec_bits || !lig_bits)
    return DLPD_ERR_ARG;
  if (!cont_offsets_ok(rec_off_host, NRres, NRa) || !cont_offsets_ok(lig_off_host, NLres, NLa)) return DLPD_ERR_ARG;
  if (K == 0) return DLPD_OK;
  if (NLa <= CONT_SMALLLIG && NLres <= CONT_SMALLLRES)
    DLPD_LAUNCH((k_pose_residue_bits<CONT_SMALLLIG, CONT_SMALLLRES>), dim3(K), dim3(CONT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                rec_off, rec_sph, NRa, NRres, lig_atoms, lig_off, lig_sph, NLa, NLres, lig_extent, cutoff * cutoff, rec_bits, lig_bits);
  else
    DLPD_LAUNCH((k_pose_residue_bits<CONT_MAXLIG, CONT_MAXLRES>), dim3(K), dim3(CONT_NT), 0, (hipStream_t)stream, poses, rec_atoms,
                rec_off, rec_sph, NRa, NRres, lig_atoms, lig_off, lig_sph, NLa, NLres, lig_extent, cutoff * cutoff, rec_bits, lig_bits);
  return dlpd_check_launch();
}

size_t dlpd_interface_profile_ws(int K, int NRres, int NLres) {
  if (K <= 0 || K > CLUSTER_MAXK || NRres < 1 || NLres < 1 || NRres > CONT_MAXRRES || NLres > CONT_MAXLRES) return 0;
  return (size_t)((K + IFACE_CHUNK - 1) / IFACE_CHUNK) * (size_t)(NRres + NLres) * (sizeof(double) + sizeof(int));
}

/* count = the poses that mark each residue, freq = the sum of their weights, in chunks of 1,024 poses */
int dlpd_interface_profile(const unsigned* rec_bits, const unsigned* lig_bits, int K, int NRres, int NLres, const double* weights,
                           double* rec_freq, double* lig_freq, int* rec_count, int* lig_count, void* ws, size_t ws_bytes, void* stream) {
  if (K < 0 || NRres < 1 || NLres < 1) return DLPD_ERR_ARG;
  if (K > CLUSTER_MAXK || NRres > CONT_MAXRRES || NLres > CONT_MAXLRES) return DLPD_ERR_UNSUPPORTED;
  if (!rec_bits || !lig_bits || !weights || !rec_freq || !lig_freq || !rec_count || !lig_count) return DLPD_ERR_ARG;
  if (K == 0) return DLPD_OK;
  if (!ws || ws_bytes < dlpd_interface_profile_ws(K, NRres, NLres)) return DLPD_ERR_ARG;
  const int chunks = (K + IFACE_CHUNK - 1) / IFACE_CHUNK, n = NRres + NLres;
  double* part_freq = (double*)ws;
  int* part_count = (int*)(part_freq + (size_t)chunks * n);
  DLPD_LAUNCH(k_interface_profile, dim3(((NRres > NLres ? NRres : NLres) + CLUSTER_NT - 1) / CLUSTER_NT, chunks, 2), dim3(CLUSTER_NT), 0,
              (hipStream_t)stream, rec_bits, lig_bits, K, NRres, NLres, weights, part_freq, part_count);
  DLPD_LAUNCH(k_interface_profile_sum, dim3((n + CLUSTER_NT - 1) / CLUSTER_NT), dim3(CLUSTER_NT), 0, (hipStream_t)stream,
              (const double*)part_freq, (const int*)part_count, chunks, NRres, NLres, rec_freq, lig_freq, rec_count, lig_count);
  return dlpd_check_launch();
}

/* the neighbour bitmap of interface similarity alone: mask = K * ceil(K / 64) 64-bit words, row-major */
int dlpd_interface_within(const unsigned* rec_bits, const unsigned* lig_bits, int K, int Wr, int Wl, int q, void* mask, void* stream) {
  const int rc = iface_check(K, Wr, Wl, q);
  if (rc) return rc;
  if ((Wr > 0 && !rec_bits) || (Wl > 0 && !lig_bits) || !mask) return DLPD_ERR_ARG;
  if (K == 0) return DLPD_OK;
  iface_within(rec_bits, lig_bits, K, Wr, Wl, q, (cl_u64*)mask, (hipStream_t)stream);
  return dlpd_check_launch();
}

/* bitmap + the greedy scan of dlpd_pose_cluster; max_clusters <= 0 or > K: no limit */
int dlpd_interface_cluster(const unsigned* rec_bits, const unsigned* lig_bits, int K, int Wr, int Wl, int q, int max_clusters,
                           int* centres, int* sizes, int* labels, int* count, void* ws, size_t ws_bytes, void* stream) {
  const int rc = iface_check(K, Wr, Wl, q);
  if (rc) return rc;
  if ((Wr > 0 && !rec_bits) || (Wl > 0 && !lig_bits) || !centres || !sizes || !labels || !count) return DLPD_ERR_ARG;
  if (K == 0) return DLPD_OK;
  if (!ws || ws_bytes < dlpd_pose_cluster_ws(K)) return DLPD_ERR_ARG;
  if (max_clusters <= 0 || max_clusters > K) max_clusters = K;
  iface_within(rec_bits, lig_bits, K, Wr, Wl, q, (cl_u64*)ws, (hipStream_t)stream);
  DLPD_LAUNCH(k_pose_scan, dim3(1), dim3(CLUSTER_NT), 0, (hipStream_t)stream, (const cl_u64*)ws, K, cluster_words(K), max_clusters,
              centres, sizes, labels, count);
  return dlpd_check_launch();
}

}  // extern "C"

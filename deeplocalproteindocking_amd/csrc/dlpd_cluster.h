// Pose clustering (BUILD-DEFINED: the reference has no counterpart and no call site): pairwise RMSD of rigid poses of one
// ligand and the greedy clustering of a score-sorted list by it.  Included by dlpd_topk.hip, the list stage.
//
// A pose p = (R_p, t_p) of the atoms x_k (weights w_k, sum 1) is embedded on the host as the 12-vector
//   e_p = (R_p c + t_p, vec(R_p B)),   c = sum w_k x_k,   B = V L^(1/2) of S = sum w_k (x_k - c)(x_k - c)^T = V L V^T,
// and d(i, j)^2 = sum_k w_k |(R_i x_k + t_i) - (R_j x_k + t_j)|^2 = |e_i - e_j|^2 (ops.pose_embedding).  The kernels only
// see embeddings.  Every squared distance is ONE chain, in one order:
//   s = 0;  for k = 0..11:  d = a[k] - b[k];  s = fma(d, d, s)
// so d2(i, j) and d2(j, i) have the same bits (a - b and b - a differ in sign only) and equal poses give exactly 0.
//
//   k_pose_rmsd    (Ea (Ka,12), Eb (Kb,12)) -> D (Ka,Kb) = sqrt(d2)
//   k_pose_within  (E (K,12), r2) -> mask, K rows of W = ceil(K/64) 64-bit words, ROW-MAJOR: bit (j & 63) of word
//                  mask[i * W + (j >> 6)] is set iff d2(i, j) <= r2; bits of columns >= K are zero
//   k_pose_scan    one block: the greedy scan over the mask, the `removed` bitmap in LDS
//
// Layout of the mask (pose clustering): the scan is the serial part -- one row per centre, and nothing else of it
// can start before that row has arrived -- so the ROW is contiguous: the scan's threads read consecutive words, W * 8 bytes
// in whole cache lines.  The build, which has all the parallelism, pays for it: a thread owns a row and eight words of it
// (512 columns), the block transposes them through LDS and every wave store writes eight rows x 64 contiguous bytes.
// Plain C++ in the subset both platform headers offer; vector stores only.
#pragma once

#define CLUSTER_MAXK 65536            // = TOPK_MAXK: the longest list the list stage keeps
#define CLUSTER_E 12                  // floats per embedded pose
#define CLUSTER_ROWS 64               // k_pose_rmsd: rows of Ea per block (staged in LDS)
#define CLUSTER_NT 256                // threads per block, all three kernels
#define CLUSTER_CW 8                  // k_pose_within: words (of 64 columns) per block
#define CLUSTER_WMAX (CLUSTER_MAXK / 64)

typedef unsigned long long cl_u64;

DLPD_D float cluster_d2(const float* a, const float* b) {
  float s = 0.f;
#pragma unroll
  for (int k = 0; k < CLUSTER_E; k++) {
    const float d = a[k] - b[k];
    s = __fmaf_rn(d, d, s);
  }
  return s;
}

// block (256 columns of Eb, 64 rows of Ea): the rows in LDS (every lane reads the same address: a broadcast), a thread's
// column in registers, D written along j
__global__ void __launch_bounds__(CLUSTER_NT) k_pose_rmsd(const float* __restrict__ Ea, const float* __restrict__ Eb,
                                                          float* __restrict__ D, int Ka, int Kb) {
  __shared__ __attribute__((aligned(16))) float rows[CLUSTER_ROWS * CLUSTER_E];
  const int tid = threadIdx.x;
  const int i0 = blockIdx.y * CLUSTER_ROWS, j = blockIdx.x * CLUSTER_NT + tid;
  const int nrow = min(CLUSTER_ROWS, Ka - i0);
  for (int q = tid; q < nrow * CLUSTER_E; q += CLUSTER_NT) rows[q] = Ea[(size_t)i0 * CLUSTER_E + q];
  __syncthreads();
  if (j >= Kb) return;
  float b[CLUSTER_E];
#pragma unroll
  for (int k = 0; k < CLUSTER_E; k++) b[k] = Eb[(size_t)j * CLUSTER_E + k];
  for (int r = 0; r < nrow; r++) D[(size_t)(i0 + r) * Kb + j] = sqrtf(cluster_d2(rows + r * CLUSTER_E, b));
}

// block (8 words = 512 columns, 256 rows): the columns in LDS (broadcast reads), a thread's row in registers, its eight
// words formed by a shift loop, transposed through LDS and stored as 64-byte pieces of eight rows per wave instruction
__global__ void __launch_bounds__(CLUSTER_NT) k_pose_within(const float* __restrict__ E, cl_u64* __restrict__ mask, int K, int W,
                                                            float r2) {
  __shared__ __attribute__((aligned(16))) float cols[CLUSTER_CW * 64 * CLUSTER_E];
  __shared__ cl_u64 words[CLUSTER_NT * (CLUSTER_CW + 1)];          // (+1: rows on different banks)
  const int tid = threadIdx.x;
  const int w0 = blockIdx.x * CLUSTER_CW, i0 = blockIdx.y * CLUSTER_NT, i = i0 + tid;
  const int j0 = w0 * 64;
  const int ncol = min(CLUSTER_CW * 64, K - j0);                 // > 0: the grid covers W words
  for (int q = tid; q < CLUSTER_CW * 64 * CLUSTER_E; q += CLUSTER_NT)
    cols[q] = (q < ncol * CLUSTER_E) ? E[(size_t)j0 * CLUSTER_E + q] : 0.f;
  float a[CLUSTER_E];
#pragma unroll
  for (int k = 0; k < CLUSTER_E; k++) a[k] = (i < K) ? E[(size_t)i * CLUSTER_E + k] : 0.f;
  __syncthreads();
  for (int w = 0; w < CLUSTER_CW; w++) {
    const int nb = min(64, ncol - w * 64);                       // valid columns of this word (<= 0: none)
    cl_u64 word = 0;
    for (int b = 0; b < nb; b++)
      word |= (cl_u64)(cluster_d2(a, cols + (w * 64 + b) * CLUSTER_E) <= r2) << b;
    words[tid * (CLUSTER_CW + 1) + w] = word;
  }
  __syncthreads();
  for (int q = tid; q < CLUSTER_NT * CLUSTER_CW; q += CLUSTER_NT) {
    const int r = q / CLUSTER_CW, w = q % CLUSTER_CW;
    if (i0 + r < K && w0 + w < W) mask[(size_t)(i0 + r) * W + w0 + w] = words[r * (CLUSTER_CW + 1) + w];
  }
}

// The greedy scan, one block.  Pose c is a centre iff it is not yet removed; its row then labels and removes what it still
// covers.  A thread owns the words tid, tid + 256, ... of `removed` and, inside the loop, the labels of their bits: no word
// is ever touched by two threads, and a label is written at most once after its -1.  The next centre is the block's minimum
// over every thread's first clear bit, the size a sum of population counts: a butterfly inside each wave, one plain LDS word
// per wave, a barrier (no LDS atomic: the library carries none).  Each of those words is written by one lane, on one side of
// a barrier, and read on the other.  Integer work only: the same mask gives the same bytes.  (A centre's own bit is set here
// whatever the mask says, so a pose whose embedding is not a number is a cluster of one and the loop always ends.)
__global__ void __launch_bounds__(CLUSTER_NT) k_pose_scan(const cl_u64* __restrict__ mask, int K, int W, int max_clusters,
                                                          int* __restrict__ centres, int* __restrict__ sizes,
                                                          int* __restrict__ labels, int* __restrict__ count) {
  __shared__ cl_u64 removed[CLUSTER_WMAX];
  __shared__ int s_next[CLUSTER_NT / 64], s_size[CLUSTER_NT / 64];
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  const int none = 0x7fffffff;
  for (int w = tid; w < W; w += CLUSTER_NT) {
    const int nb = min(64, K - w * 64);
    removed[w] = (nb < 64) ? ~(cl_u64)0 << nb : (cl_u64)0;       // columns >= K can never be centres
  }
  for (int j = tid; j < K; j += CLUSTER_NT) labels[j] = -1;      // (ordered before the loop's writes by the barrier)
  __syncthreads();
  int n = 0;
  for (; n < max_clusters; n++) {
    int cand = none;
    for (int w = tid; w < W; w += CLUSTER_NT) {
      const cl_u64 clear = ~removed[w];
      if (clear) { cand = w * 64 + __builtin_ctzll(clear); break; }      // (ascending words: this thread's first)
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) cand = min(cand, __shfl_xor(cand, m));
    if (lane == 0) s_next[wave] = cand;
    __syncthreads();
    int c = s_next[0];
#pragma unroll
    for (int q = 1; q < CLUSTER_NT / 64; q++) c = min(c, s_next[q]);
    if (c == none) break;                                        // (the same for every thread)
    int sz = 0;
    for (int w = tid; w < W; w += CLUSTER_NT) {
      cl_u64 row = mask[(size_t)c * W + w];
      if (w == (c >> 6)) row |= (cl_u64)1 << (c & 63);
      const cl_u64 rem = removed[w];
      cl_u64 fresh = row & ~rem;
      removed[w] = rem | row;
      sz += __popcll(fresh);
      while (fresh) {
        labels[w * 64 + __builtin_ctzll(fresh)] = n;
        fresh &= fresh - 1;
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) sz += __shfl_xor(sz, m);
    if (lane == 0) s_size[wave] = sz;
    __syncthreads();
    if (tid == 0) {
      int total = s_size[0];
#pragma unroll
      for (int q = 1; q < CLUSTER_NT / 64; q++) total += s_size[q];
      centres[n] = c;
      sizes[n] = total;
    }
  }
  if (tid == 0) *count = n;
}

extern "C" {

static int cluster_words(int K) { return (K + 63) / 64; }

/* D (Ka, Kb) = the RMSD between the poses of two embedded sets */
int dlpd_pose_rmsd(const float* Ea, const float* Eb, float* D, int Ka, int Kb, void* stream) {
  if (!Ea || !Eb || !D || Ka <= 0 || Kb <= 0) return DLPD_ERR_ARG;
  if (Ka > CLUSTER_MAXK || Kb > CLUSTER_MAXK) return DLPD_ERR_UNSUPPORTED;
  DLPD_LAUNCH(k_pose_rmsd, dim3((Kb + CLUSTER_NT - 1) / CLUSTER_NT, (Ka + CLUSTER_ROWS - 1) / CLUSTER_ROWS), dim3(CLUSTER_NT), 0,
              (hipStream_t)stream, Ea, Eb, D, Ka, Kb);
  return dlpd_check_launch();
}

static int cluster_check(const void* E, int K, float radius) {
  if (!E || K <= 0 || !(radius >= 0.f)) return DLPD_ERR_ARG;     // (a NaN radius fails the comparison too)
  return K > CLUSTER_MAXK ? DLPD_ERR_UNSUPPORTED : DLPD_OK;
}

static void cluster_within(const float* E, int K, float radius, cl_u64* mask, hipStream_t st) {
  const int W = cluster_words(K);
  DLPD_LAUNCH(k_pose_within, dim3((W + CLUSTER_CW - 1) / CLUSTER_CW, (K + CLUSTER_NT - 1) / CLUSTER_NT), dim3(CLUSTER_NT), 0, st, E,
              mask, K, W, radius * radius);
}

/* the neighbour bitmap alone: mask = K * ceil(K / 64) 64-bit words, row-major */
int dlpd_pose_within(const float* E, int K, float radius, void* mask, void* stream) {
  const int rc = cluster_check(E, K, radius);
  if (rc) return rc;
  if (!mask) return DLPD_ERR_ARG;
  cluster_within(E, K, radius, (cl_u64*)mask, (hipStream_t)stream);
  return dlpd_check_launch();
}

size_t dlpd_pose_cluster_ws(int K) {
  if (K <= 0 || K > CLUSTER_MAXK) return 0;
  return (size_t)K * (size_t)cluster_words(K) * sizeof(cl_u64);
}

/* bitmap + greedy scan; max_clusters <= 0 or > K: no limit */
int dlpd_pose_cluster(const float* E, int K, float radius, int max_clusters, int* centres, int* sizes, int* labels, int* count,
                      void* ws, size_t ws_bytes, void* stream) {
  const int rc = cluster_check(E, K, radius);
  if (rc) return rc;
  if (!centres || !sizes || !labels || !count || !ws || ws_bytes < dlpd_pose_cluster_ws(K)) return DLPD_ERR_ARG;
  if (max_clusters <= 0 || max_clusters > K) max_clusters = K;
  cluster_within(E, K, radius, (cl_u64*)ws, (hipStream_t)stream);
  DLPD_LAUNCH(k_pose_scan, dim3(1), dim3(CLUSTER_NT), 0, (hipStream_t)stream, (const cl_u64*)ws, K, cluster_words(K), max_clusters,
              centres, sizes, labels, count);
  return dlpd_check_launch();
}

}  // extern "C"

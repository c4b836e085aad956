// Search under distance restraints (included at the end of dlpd_topk.hip).  BUILD-DEFINED: the reference has no
// counterpart; no restraints -- none of this -- is the reference.
//
// Definition (include/dlpd.h): restraint j of rotation rot is a centre c = (cx, cy, cz) in 1/256 voxel (int32, |c| <= 2^20) and
// two squared bounds lo^2 <= hi^2 (int64, hi <= 2^21).  Voxel v of the cubic grid of even side n has the signed index
// t = v - n if v >= n / 2 else v per axis; d^2 = sum over the axes of (256 t - c)^2 in int64; the restraint is satisfied iff
// lo^2 <= d^2 <= hi^2.  A voxel is ALLOWED iff it satisfies at least `need` of the J restraints.  restrain(V)[v] = V[v] where
// V[v] < 0 is false (zeros, -0.0 and positives keep their bits) and where V[v] < 0 and v is allowed; +0.0 everywhere else.
// Integers throughout: the kernels compare, they compute nothing that rounds.
//
// k_restrain_volume   V -> Vs (or in place) for the rotations that go through the radix select.  A tile is 8 x 8 rows of 32
//                     voxels; x and y are uniform along a row, so every (row, restraint) is reduced ONCE to the interval
//                     za <= |256 tz - cz| <= zb of 32-bit integers (two exact integer square roots of 64-bit numbers), and a
//                     voxel costs J subtractions and compares, no 64-bit multiply.  A tile that fewer than `need` bounding
//                     cubes touch skips all of that and only clears its negatives.
// k_restrain_cand     one block per rotation.  THIN: a complete candidate list of K3 loses the candidates that are not allowed,
//                     in list order (the scheme of k_suppress_cand).  REBUILD: a list that overflowed the cap -- under a
//                     restraint tau is shallow and most do -- is written again from the bounding cubes of the balls: every
//                     allowed voxel with key <= *tau, once (at the lowest restraint it satisfies).  At most cap of them: the
//                     list is complete, and neither the volume kernel nor the radix select runs for the rotation.
// No atomics of any kind; plain LDS words and the block-wide count of dlpd_topk.hip.
#pragma once

#define RST_TX 8
#define RST_TY 8
#define RST_TZ 32                // z is the contiguous axis: a tile row is 128 bytes
#define RST_ROWS (RST_TX * RST_TY)
#define RST_THREADS 256
#define RST_CAND_THREADS 512
#define RST_MAXJ 32
#define RST_MAXC (1 << 20)       // |c|, in 1/256 voxel
#define RST_MAXHI (1ll << 42)    // hi^2

DLPD_D int rst_signed(int v, int n) { return v >= (n >> 1) ? v - n : v; }

// floor(sqrt(v)) for 0 <= v < 2^52: the double root is within one of it, two integer steps make it exact
DLPD_D int rst_isqrt(long long v) {
  long long s = (long long)sqrt((double)v);
  while (s * s > v) s--;
  while ((s + 1) * (s + 1) <= v) s++;
  return (int)s;
}

// the restraints of one rotation in LDS: centres, then squared bounds
struct RstSet {
  int c[RST_MAXJ][3];
  long long lo2[RST_MAXJ], hi2[RST_MAXJ];
};

DLPD_D void rst_load(RstSet& s, const int* __restrict__ centres, const long long* __restrict__ bounds, int rot, int J, int tid) {
  if (tid < 3 * J) (&s.c[0][0])[tid] = centres[(size_t)rot * J * 3 + tid];
  if (tid < J) { s.lo2[tid] = bounds[tid]; s.hi2[tid] = bounds[J + tid]; }
}

// bit j: the voxel at signed index (tx, ty, tz) satisfies restraint j -- the definition, three 64-bit products per restraint
// (the candidate kernel's test: a few thousand voxels per rotation, not a volume)
DLPD_D unsigned rst_satisfied(const RstSet& s, int J, int tx, int ty, int tz) {
  unsigned m = 0;
  for (int j = 0; j < J; j++) {
    const long long dx = 256 * tx - s.c[j][0], dy = 256 * ty - s.c[j][1], dz = 256 * tz - s.c[j][2];
    const long long d2 = dx * dx + dy * dy + dz * dz;
    m |= (d2 >= s.lo2[j] && d2 <= s.hi2[j]) ? (1u << j) : 0u;
  }
  return m;
}

// grid (tiles, nb).  V == Vs is allowed (element-wise).  ccount (null: every rotation): [0, nb) candidate counts, [nb, 2 nb)
// need-full flags -- a rotation whose list is complete is served from that list, and its row of Vs is not written.
__global__ void __launch_bounds__(RST_THREADS)
k_restrain_volume(const float* V, float* Vs, int n, int vec, const int* __restrict__ rot_ids, const int* __restrict__ centres,
                  const long long* __restrict__ bounds, int J, int need, const unsigned* __restrict__ ccount, int nb, int cap) {
  __shared__ RstSet set;
  __shared__ int touch[RST_MAXJ];
  __shared__ int zlo[RST_MAXJ][RST_ROWS], zhi[RST_MAXJ][RST_ROWS];      // [restraint][row]: the lanes of a wave read neighbours
  const int b = blockIdx.y, tid = threadIdx.x;
  if (ccount && ccount[nb + b] == 0 && ccount[b] <= (unsigned)cap) return;
  const int ntz = (n + RST_TZ - 1) / RST_TZ, nty = (n + RST_TY - 1) / RST_TY;
  const int tz = blockIdx.x % ntz, ty = (blockIdx.x / ntz) % nty, tx = blockIdx.x / (ntz * nty);
  const int x0 = tx * RST_TX, y0 = ty * RST_TY, z0 = tz * RST_TZ;
  rst_load(set, centres, bounds, rot_ids[b], J, tid);
  __syncthreads();
  // does the bounding cube of ball j reach the tile?  Per axis: some index of the tile within hi of the centre (the tile may
  // lie across the seam n / 2, so the indices are tested one by one: 48 steps for J threads, once per block)
  if (tid < J) {
    const int h = rst_isqrt(set.hi2[tid]);
    bool ax = false, ay = false, az = false;
    for (int i = 0; i < RST_TX; i++) { const int d = 256 * rst_signed(x0 + i, n) - set.c[tid][0]; ax = ax || (x0 + i < n && (d < 0 ? -d : d) <= h); }
    for (int i = 0; i < RST_TY; i++) { const int d = 256 * rst_signed(y0 + i, n) - set.c[tid][1]; ay = ay || (y0 + i < n && (d < 0 ? -d : d) <= h); }
    for (int i = 0; i < RST_TZ; i++) { const int d = 256 * rst_signed(z0 + i, n) - set.c[tid][2]; az = az || (z0 + i < n && (d < 0 ? -d : d) <= h); }
    touch[tid] = (ax && ay && az) ? 1 : 0;
  }
  __syncthreads();
  int touched = 0;
  for (int j = 0; j < J; j++) touched += touch[j];
  const bool live = touched >= need;                                   // (block-uniform)
  if (live) {
    // every (restraint, row): lo^2 - Sxy <= dz^2 <= hi^2 - Sxy as za <= |dz| <= zb; an empty interval is za > zb
    for (int it = tid; it < J * RST_ROWS; it += RST_THREADS) {
      const int j = it / RST_ROWS, row = it - j * RST_ROWS;
      const long long dx = 256 * rst_signed(x0 + (row >> 3), n) - set.c[j][0], dy = 256 * rst_signed(y0 + (row & 7), n) - set.c[j][1];
      const long long sxy = dx * dx + dy * dy, A = set.lo2[j] - sxy, B = set.hi2[j] - sxy;
      int za = 0, zb = -1;
      if (touch[j] && B >= 0) {
        zb = rst_isqrt(B);
        if (A > 0) { za = rst_isqrt(A); za += (long long)za * za < A ? 1 : 0; }
      }
      zlo[j][row] = za;
      zhi[j][row] = zb;
    }
    __syncthreads();
  }
  const size_t n3 = (size_t)n * n * n;
  const float* v = V + (size_t)b * n3;
  float* vs = Vs + (size_t)b * n3;
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int it = tid + h * RST_THREADS;
    const int c = it & 7, row = it >> 3;
    const int gx = x0 + (row >> 3), gy = y0 + (row & 7), gz = z0 + 4 * c;
    if (gx >= n || gy >= n || gz >= n) continue;
    const size_t at = ((size_t)gx * n + gy) * n + gz;
    const bool wide = vec && gz + 3 < n;
    float q[4] = {0.f, 0.f, 0.f, 0.f};
    if (wide) {
      const float4 f = *reinterpret_cast<const float4*>(v + at);
      q[0] = f.x; q[1] = f.y; q[2] = f.z; q[3] = f.w;
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) if (gz + e < n) q[e] = v[at + e];
    }
    int cnt[4] = {0, 0, 0, 0};
    if (live && (q[0] < 0.f || q[1] < 0.f || q[2] < 0.f || q[3] < 0.f)) {
      int t256[4];
#pragma unroll
      for (int e = 0; e < 4; e++) t256[e] = 256 * rst_signed(gz + e < n ? gz + e : gz, n);
      for (int j = 0; j < J; j++) {
        const int za = zlo[j][row], zb = zhi[j][row], cz = set.c[j][2];
#pragma unroll
        for (int e = 0; e < 4; e++) {
          int d = t256[e] - cz;
          d = d < 0 ? -d : d;
          cnt[e] += (d >= za && d <= zb) ? 1 : 0;
        }
      }
    }
#pragma unroll
    for (int e = 0; e < 4; e++) q[e] = (q[e] < 0.f && cnt[e] < need) ? 0.0f : q[e];
    if (wide) {
      *reinterpret_cast<float4*>(vs + at) = make_float4(q[0], q[1], q[2], q[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) if (gz + e < n) vs[at + e] = q[e];
    }
  }
}

// one block per rotation; LDS (dynamic): cap u64 keys.  cbuf (nb, cap): score key << 32 | flat index, as K3 appends them.
// tau (null: no rebuild): the u32 key of the running list's K-th score, 0 while there is none.
__global__ void __launch_bounds__(RST_CAND_THREADS)
k_restrain_cand(const float* __restrict__ V, int n, const int* __restrict__ rot_ids, const int* __restrict__ centres,
                const long long* __restrict__ bounds, int J, int need, const unsigned* __restrict__ tau, u64* __restrict__ cbuf,
                unsigned* __restrict__ ccount, int nb, int cap) {
  DLPD_DYN_SHARED(u64, keys);
  __shared__ RstSet set;
  __shared__ int scr[32];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const unsigned nc = ccount[b];
  if (ccount[nb + b]) return;                                        // K3 saw no filter: the radix select's, left alone
  const unsigned tk = (nc > (unsigned)cap && tau) ? *tau : 0u;
  if (nc == 0 || (nc > (unsigned)cap && tk == 0u)) return;           // empty; overflowed and no rebuild: left alone
  rst_load(set, centres, bounds, rot_ids[b], J, tid);
  u64* list = cbuf + (size_t)b * cap;
  const int half = n >> 1;
  if (nc <= (unsigned)cap) {                                         // ---- thin a complete list
    for (int i = tid; i < (int)nc; i += nt) keys[i] = list[i];
    __syncthreads();
    int kept = 0;                                                    // survivors written so far (uniform)
    for (int i0 = 0; i0 < (int)nc; i0 += nt) {                       // (every thread runs every round: block_rank has barriers)
      const int i = i0 + tid;
      bool keep = i < (int)nc;
      u64 key = 0;
      if (keep) {
        key = keys[i];
        const int flat = (int)(key & 0xffffffffu);
        const int gz = flat % n, gy = (flat / n) % n, gx = flat / (n * n);
        keep = __popcll((u64)rst_satisfied(set, J, rst_signed(gx, n), rst_signed(gy, n), rst_signed(gz, n))) >= need;
      }
      int added;
      const int slot = kept + block_rank(keep, scr, tid, nt, added);
      if (keep) list[slot] = key;                                    // slot <= i, and every key was read into LDS first
      kept += added;
    }
    if (tid == 0) ccount[b] = (unsigned)kept;
    return;
  }
  // ---- rebuild an overflowed list from the balls' bounding cubes, clipped to the grid's signed range [-n/2, n/2)
  __syncthreads();
  const float* v = V + (size_t)b * n * n * n;
  int emitted = 0;                                                   // (uniform)
  for (int j = 0; j < J; j++) {
    const int h = rst_isqrt(set.hi2[j]);
    int lo3[3], len[3];
#pragma unroll
    for (int a = 0; a < 3; a++) {
      // ceil((c - h) / 256) and floor((c + h) / 256): the arithmetic shift is the floor for either sign
      int first = -((h - set.c[j][a]) >> 8), last = (set.c[j][a] + h) >> 8;
      first = first < -half ? -half : first;
      last = last > half - 1 ? half - 1 : last;
      lo3[a] = first;
      len[a] = last >= first ? last - first + 1 : 0;
    }
    const int vol = len[0] * len[1] * len[2];                        // (uniform; the host bounds the sum over j)
    for (int i0 = 0; i0 < vol; i0 += nt) {
      const int i = i0 + tid;
      bool emit = i < vol;
      u64 key = 0;
      if (emit) {
        const int iz = i % len[2], iy = (i / len[2]) % len[1], ix = i / (len[2] * len[1]);
        const int tx = lo3[0] + ix, ty = lo3[1] + iy, tz = lo3[2] + iz;
        const unsigned m = rst_satisfied(set, J, tx, ty, tz);
        // the lowest restraint the voxel satisfies is j: no voxel is listed twice, however the cubes overlap
        emit = (m & ((1u << j) - 1u)) == 0u && ((m >> j) & 1u) != 0u && __popcll((u64)m) >= need;
        if (emit) {
          const int flat = (((tx < 0 ? tx + n : tx) * n) + (ty < 0 ? ty + n : ty)) * n + (tz < 0 ? tz + n : tz);
          const unsigned k = f2key(v[flat]);
          emit = k <= tk;
          key = ((u64)k << 32) | (u64)(unsigned)flat;
        }
      }
      int added;
      const int slot = emitted + block_rank(emit, scr, tid, nt, added);
      if (emit && slot < cap) list[slot] = key;
      emitted += added;
    }
  }
  if (tid == 0 && emitted <= cap) ccount[b] = (unsigned)emitted;     // complete now; else the count stays above the cap
}

extern "C" {

static int rst_check(const void* V, int nb, int n, const int* rot_ids, const int* centres, const long long* bounds, int J, int need) {
  if (!V || !rot_ids || !centres || !bounds || nb <= 0 || n < 2 || (n & 1) || J < 1 || J > RST_MAXJ || need < 1 || need > J)
    return DLPD_ERR_ARG;
  if (n > 1290 || (long long)n * n * n >= (1ll << 31)) return DLPD_ERR_UNSUPPORTED;
  return DLPD_OK;
}

// V (nb, n^3) -> Vs (nb, n^3) = restrain(V); Vs == V is allowed.  rot_ids (nb) device int32 index centres (nrot, J, 3);
// bounds: lo^2 of the J restraints, then hi^2.  cand_count (null: every rotation): 2 nb u32 as K3 / dlpd_topk_restrain_cand
// left them; the rows of rotations with a complete list are not written.
int dlpd_topk_restrain(const float* V, float* Vs, int nb, int n, const int* rot_ids, const int* centres, const long long* bounds,
                       int J, int need, const void* cand_count, int cap, void* stream) {
  if (!Vs) return DLPD_ERR_ARG;
  if (int rc = rst_check(V, nb, n, rot_ids, centres, bounds, J, need)) return rc;
  const int vec = (n & 3) == 0 && ((size_t)V & 15) == 0 && ((size_t)Vs & 15) == 0;
  const int tiles = ((n + RST_TX - 1) / RST_TX) * ((n + RST_TY - 1) / RST_TY) * ((n + RST_TZ - 1) / RST_TZ);
  DLPD_LAUNCH(k_restrain_volume, dim3(tiles, nb), dim3(RST_THREADS), 0, (hipStream_t)stream, V, Vs, n, vec, rot_ids, centres,
              bounds, J, need, (const unsigned*)cand_count, nb, cap);
  return dlpd_check_launch();
}

// The complete candidate lists of the batch (flag clear, count <= cap) lose every candidate that is not allowed; survivors
// keep their order and cand_count[b] is lowered.  With tau (non-null, *tau != 0) the overflowed lists (flag clear, count > cap)
// are rebuilt from the allowed region: complete and their count set if at most cap allowed voxels have a key <= *tau.
// Flagged lists and the flags are left alone.
int dlpd_topk_restrain_cand(const float* V, int nb, int n, const int* rot_ids, const int* centres, const long long* bounds,
                            int J, int need, const void* tau, void* cand_keys, void* cand_count, int cap, void* stream) {
  if (!cand_keys || !cand_count || cap < 64 || cap > 8192) return DLPD_ERR_ARG;
  if (int rc = rst_check(V, nb, n, rot_ids, centres, bounds, J, need)) return rc;
  const size_t shmem = (size_t)cap * sizeof(u64);
  if (int rc = dlpd_set_max_dyn_shared((const void*)k_restrain_cand, shmem)) return rc;
  DLPD_LAUNCH(k_restrain_cand, dim3(nb), dim3(RST_CAND_THREADS), shmem, (hipStream_t)stream, V, n, rot_ids, centres, bounds, J, need,
              (const unsigned*)tau, (u64*)cand_keys, (unsigned*)cand_count, nb, cap);
  return dlpd_check_launch();
}

}  // extern "C"

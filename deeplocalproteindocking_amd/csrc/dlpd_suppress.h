// Exclusion radius of the search (included at the end of dlpd_topk.hip).  BUILD-DEFINED: the reference clears
// one voxel per pick (Docker.py:98) and has no counterpart; r = 0 -- none of this -- is the reference.
//
// Definition (include/dlpd.h): on the cubic grid of side n, u BEATS v iff V[u] < V[v], or V[u] == V[v] and flat(u) < flat(v);
// B_r(v) is the cyclic Chebyshev ball {(v + d) mod n : d in [-r, r]^3}.  suppress_r(V)[v] = V[v] where V[v] < 0 is false
// (zeros, -0.0 and positives keep their bits) and where V[v] < 0 and no other voxel of B_r(v) beats v; +0.0 -- what a pick
// of the reference leaves behind -- everywhere else.  The list of a search with exclusion r is update_top on suppress_r(V).
//
// k_suppress_volume   V -> Vs for the rotations that go through the radix select: a tile plus a halo of r as u32 keys in LDS,
//                     three separable minimum passes (z, y, x), a voxel survives iff it is negative and IS the minimum of its
//                     ball; two equal keys in one ball (rare) are told apart by a scan of the staged ball for the lower flat
//                     index, one candidate at a time with the 64 lanes of a wave.
// k_suppress_cand     the steady state: a rotation whose K3 candidate list is complete keeps its list, and every candidate is
//                     tested against its ball in V directly -- whatever beats a candidate scores below it, so V is all the
//                     test needs, and what can still enter the running list (score <= tau) is among the candidates as before.
// No LDS atomics, no global float atomics, no workspace beyond Vs; plain LDS words and the block-wide count of dlpd_topk.hip.
#pragma once

#define SUP_TX 8
#define SUP_TY 8
#define SUP_TZ 32                // z is the contiguous axis: a tile row is 128 bytes
#define SUP_THREADS 256
#define SUP_MAXR 4

// Order-preserving key WITHOUT the -0.0 -> +0.0 fold of f2key, so that a key gives back the float's own bits.  For V < 0 it
// is f2key; -0.0 (0x7fffffff) sorts below +0.0 here, which no comparison below can see: only strictly negative voxels
// (key < 0x7fffffff) are ever suppressed, and what beats one is strictly negative itself.
DLPD_HD unsigned sup_key(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
#define SUP_KEY_NEGZERO 0x7fffffffu      // keys below it: V < 0
#define SUP_KEY_ZERO 0x80000000u         // +0.0

struct __attribute__((aligned(16))) sup_u4 { unsigned x, y, z, w; };

// c mod n for c >= -r > -n, without a division: one step for every grid that is not tiny
DLPD_D int sup_wrap(int c, int n) {
  c = c < 0 ? c + n : c;
  while (c >= n) c -= n;
  return c;
}
// q / d by a multiplication, inv = 65536 / d + 1: exact while q * d < 65536 (the overshoot of inv stays below one step of 1 / d)
DLPD_D int sup_div(int q, int inv) { return (q * inv) >> 16; }

// grid (tiles, nb).  LDS (dynamic): K (TX+2r)(TY+2r)(TZ+2r) keys, M1 (TX+2r)(TY+2r) TZ z-minima, M2 (TX+2r) TY TZ yz-minima.
// ccount (null: every rotation): [0, nb) candidate counts, [nb, 2 nb) need-full flags -- a rotation whose list is complete
// (k_topk_from_cand's own conditions) is served from that list, and its row of Vs is not written.
__global__ void __launch_bounds__(SUP_THREADS)
k_suppress_volume(const float* __restrict__ V, float* __restrict__ Vs, int n, int r, int vec, const unsigned* __restrict__ ccount,
                  int nb, int cap) {
  DLPD_DYN_SHARED(unsigned, K);
  const int b = blockIdx.y, tid = threadIdx.x;
  if (ccount && ccount[nb + b] == 0 && ccount[b] <= (unsigned)cap) return;
  const int PX = SUP_TX + 2 * r, PY = SUP_TY + 2 * r, PZ = SUP_TZ + 2 * r, rows = PX * PY;
  unsigned* M1 = K + rows * PZ;
  unsigned* M2 = M1 + rows * SUP_TZ;
  const int ntz = (n + SUP_TZ - 1) / SUP_TZ, nty = (n + SUP_TY - 1) / SUP_TY;
  const int tz = blockIdx.x % ntz, ty = (blockIdx.x / ntz) % nty, tx = blockIdx.x / (ntz * nty);
  const int x0 = tx * SUP_TX, y0 = ty * SUP_TY, z0 = tz * SUP_TZ;
  const size_t n3 = (size_t)n * n * n;
  const float* v = V + (size_t)b * n3;
  // the rows' 32 centre voxels, four per thread; then the 2r halo voxels of every row.  All addresses wrap.
  const int inv_py = 65536 / PY + 1, inv_2r = 65536 / (2 * r) + 1;
  for (int it = tid; it < rows * (SUP_TZ / 4); it += SUP_THREADS) {
    const int row = it >> 3, c = it & 7;
    const int i = sup_div(row, inv_py), j = row - i * PY;
    const float* p = v + ((size_t)sup_wrap(x0 - r + i, n) * n + sup_wrap(y0 - r + j, n)) * n;
    const int z = z0 + 4 * c;
    unsigned* dst = K + row * PZ + r + 4 * c;
    if (vec && z + 3 < n) {
      const float4 q = *reinterpret_cast<const float4*>(p + z);
      dst[0] = sup_key(q.x); dst[1] = sup_key(q.y); dst[2] = sup_key(q.z); dst[3] = sup_key(q.w);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) dst[e] = sup_key(p[sup_wrap(z + e, n)]);
    }
  }
  for (int it = tid; it < rows * 2 * r; it += SUP_THREADS) {
    const int row = sup_div(it, inv_2r), h = it - row * 2 * r;
    const int i = sup_div(row, inv_py), j = row - i * PY;
    const float* p = v + ((size_t)sup_wrap(x0 - r + i, n) * n + sup_wrap(y0 - r + j, n)) * n;
    const int pz = h < r ? h : SUP_TZ + h;
    K[row * PZ + pz] = sup_key(p[sup_wrap(z0 - r + pz, n)]);
  }
  __syncthreads();
  for (int it = tid; it < rows * SUP_TZ; it += SUP_THREADS) {                      // z
    const unsigned* src = K + (it >> 5) * PZ + (it & 31);
    unsigned m = src[0];
    for (int d = 1; d <= 2 * r; d++) { const unsigned o = src[d]; m = o < m ? o : m; }
    M1[it] = m;
  }
  __syncthreads();
  for (int it = tid; it < PX * SUP_TY * SUP_TZ; it += SUP_THREADS) {               // y
    const int z = it & 31, y = (it >> 5) & 7, i = it >> 8;
    const unsigned* src = M1 + (i * PY + y) * SUP_TZ + z;
    unsigned m = src[0];
    for (int d = 1; d <= 2 * r; d++) { const unsigned o = src[d * SUP_TZ]; m = o < m ? o : m; }
    M2[it] = m;
  }
  __syncthreads();
  // x and the verdict: a thread owns four voxels of a row in each half of the tile.  A negative voxel survives iff it equals
  // the minimum of its ball -- and, where the ball holds that key twice, has the lower flat index.  That second test is rare
  // but its candidates are not (every local minimum is one), so it is not run lane by lane: the wave lists its candidates'
  // positions in LDS (M1 is free by now; 512 words per wave) and then scans the ball of one candidate at a time with all 64
  // lanes, an offset per lane.  A loser's list entry is overwritten (several lanes may store the same word).
  float* vs = Vs + (size_t)b * n3;
  const int lane = tid & 63, side = 2 * r + 1, ball = side * side * side, inv_s = 65536 / side + 1, inv_ss = 65536 / (side * side) + 1;
  unsigned* wl = M1 + (tid >> 6) * (SUP_TX * SUP_TY * SUP_TZ / (SUP_THREADS / 64));
  unsigned res[2][4], slot[2][4];
  int nlist = 0;                                                                   // (wave-uniform)
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int it = tid + h * SUP_THREADS;
    const int c = it & 7, y = (it >> 3) & 7, x = it >> 6;
    const bool inside = x0 + x < n && y0 + y < n;
    const sup_u4* src = reinterpret_cast<const sup_u4*>(M2 + (x * SUP_TY + y) * SUP_TZ + 4 * c);   // (16-byte aligned: one LDS read)
    sup_u4 q = src[0];
    unsigned m[4] = {q.x, q.y, q.z, q.w};
    for (int d = 1; d <= 2 * r; d++) {
      q = src[d * (SUP_TY * SUP_TZ / 4)];
      m[0] = q.x < m[0] ? q.x : m[0]; m[1] = q.y < m[1] ? q.y : m[1];
      m[2] = q.z < m[2] ? q.z : m[2]; m[3] = q.w < m[3] ? q.w : m[3];
    }
    const int kpos = ((x + r) * PY + (y + r)) * PZ + (4 * c + r);
    bool cand[4];
    int mine = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const unsigned kc = K[kpos + e];
      cand[e] = inside && z0 + 4 * c + e < n && kc < SUP_KEY_NEGZERO && m[e] == kc;
      res[h][e] = (kc < SUP_KEY_NEGZERO && !cand[e]) ? SUP_KEY_ZERO : kc;
      mine += cand[e] ? 1 : 0;
    }
    int upto = mine;                                                               // inclusive count over the lanes of the wave
    for (int d = 1; d < 64; d <<= 1) { const int o = __shfl(upto, lane - d); upto += lane >= d ? o : 0; }
    int at = nlist + upto - mine;
    nlist += __shfl(upto, 63);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      slot[h][e] = cand[e] ? (unsigned)at : 0xffffffffu;
      if (cand[e]) wl[at++] = (unsigned)(kpos + e);
    }
  }
  DLPD_WAVE_SYNC();
  for (int i = 0; i < nlist; i++) {
    const int kpos = (int)wl[i];                                                   // (every lane reads the same word)
    const int row = kpos / PZ, pz = kpos - row * PZ, px = row / PY, py = row - px * PY;
    const int gx = x0 + px - r, gy = y0 + py - r, gz = z0 + pz - r, flat = (gx * n + gy) * n + gz;
    const unsigned kc = K[kpos];
    bool lost = false;
    for (int o = lane; o < ball; o += 64) {
      const int ox = sup_div(o, inv_ss), oyz = o - ox * side * side, oy = sup_div(oyz, inv_s), oz = oyz - oy * side;
      const int dx = ox - r, dy = oy - r, dz = oz - r;
      if ((dx | dy | dz) != 0 && K[kpos + (dx * PY + dy) * PZ + dz] == kc)
        lost = lost || (sup_wrap(gx + dx, n) * n + sup_wrap(gy + dy, n)) * n + sup_wrap(gz + dz, n) < flat;
    }
    DLPD_WAVE_SYNC();                                                              // every lane has read entry i
    if (lost) wl[i] = 0xffffffffu;
  }
  DLPD_WAVE_SYNC();
#pragma unroll
  for (int h = 0; h < 2; h++) {
    const int it = tid + h * SUP_THREADS;
    const int c = it & 7, y = (it >> 3) & 7, x = it >> 6;
    const int gx = x0 + x, gy = y0 + y, gz = z0 + 4 * c;
    if (gx >= n || gy >= n || gz >= n) continue;
    float out[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      unsigned k = res[h][e];
      if (slot[h][e] != 0xffffffffu && wl[slot[h][e]] == 0xffffffffu) k = SUP_KEY_ZERO;
      out[e] = __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
    }
    float* dst = vs + ((size_t)gx * n + gy) * n + gz;
    if (vec && gz + 3 < n) {
      *reinterpret_cast<float4*>(dst) = make_float4(out[0], out[1], out[2], out[3]);
    } else {
#pragma unroll
      for (int e = 0; e < 4; e++) if (gz + e < n) dst[e] = out[e];
    }
  }
}

// one block per rotation; LDS (dynamic): cap u64 keys.  cbuf (nb, cap): score key << 32 | flat index, as K3 appends them.
__global__ void __launch_bounds__(SUP_THREADS)
k_suppress_cand(const float* __restrict__ V, int n, int r, u64* __restrict__ cbuf, unsigned* __restrict__ ccount, int nb, int cap) {
  DLPD_DYN_SHARED(u64, keys);
  __shared__ int scr[32];
  const int b = blockIdx.x, tid = threadIdx.x, nt = blockDim.x;
  const unsigned nc = ccount[b];
  if (ccount[nb + b] || nc > (unsigned)cap || nc == 0) return;       // incomplete (the radix select's) or empty: left alone
  u64* list = cbuf + (size_t)b * cap;
  for (int i = tid; i < (int)nc; i += nt) keys[i] = list[i];
  __syncthreads();
  const float* v = V + (size_t)b * n * n * n;
  int kept = 0;                                                      // survivors written so far (uniform)
  for (int i0 = 0; i0 < (int)nc; i0 += nt) {                         // (every thread runs every round: block_rank has barriers)
    const int i = i0 + tid;
    bool keep = i < (int)nc;
    u64 key = 0;
    if (keep) {
      key = keys[i];
      const unsigned kc = (unsigned)(key >> 32);
      const int flat = (int)(key & 0xffffffffu);
      const int gz = flat % n, gy = (flat / n) % n, gx = flat / (n * n);
      for (int dx = -r; dx <= r && keep; dx++) {
        const int ux = sup_wrap(gx + dx, n);
        for (int dy = -r; dy <= r && keep; dy++) {
          const int uy = sup_wrap(gy + dy, n);
          for (int dz = -r; dz <= r; dz++) {
            if ((dx | dy | dz) == 0) continue;
            const int fu = (ux * n + uy) * n + sup_wrap(gz + dz, n);
            const unsigned ku = f2key(v[fu]);
            if (ku < kc || (ku == kc && fu < flat)) { keep = false; break; }
          }
        }
      }
    }
    int added;
    const int slot = kept + block_rank(keep, scr, tid, nt, added);
    if (keep) list[slot] = key;                                      // slot <= i, and every key was read into LDS first
    kept += added;
  }
  if (tid == 0) ccount[b] = (unsigned)kept;
}

extern "C" {

static int sup_check(const void* V, int nb, int n, int r) {
  if (!V || nb <= 0 || r < 1 || r > SUP_MAXR || 2 * r + 1 > n) return DLPD_ERR_ARG;
  if (n > 1290 || (long long)n * n * n >= (1ll << 31)) return DLPD_ERR_UNSUPPORTED;
  return DLPD_OK;
}

// V (nb, n^3) -> Vs (nb, n^3) = suppress_r(V), never in place.  cand_count (null: every rotation): 2 nb u32 as K3 left them
// (counters, then need-full flags); the rows of rotations with a complete list are not written.
int dlpd_topk_suppress(const float* V, float* Vs, int nb, int n, int r, const void* cand_count, int cap, void* stream) {
  if (!Vs || (const float*)Vs == V) return DLPD_ERR_ARG;
  if (int rc = sup_check(V, nb, n, r)) return rc;
  const size_t shmem = ((size_t)(SUP_TX + 2 * r) * (SUP_TY + 2 * r) * (SUP_TZ + 2 * r + SUP_TZ) +
                        (size_t)(SUP_TX + 2 * r) * SUP_TY * SUP_TZ) * sizeof(unsigned);
  if (int rc = dlpd_set_max_dyn_shared((const void*)k_suppress_volume, shmem)) return rc;
  const int vec = (n & 3) == 0 && ((size_t)V & 15) == 0 && ((size_t)Vs & 15) == 0;
  const int tiles = ((n + SUP_TX - 1) / SUP_TX) * ((n + SUP_TY - 1) / SUP_TY) * ((n + SUP_TZ - 1) / SUP_TZ);
  DLPD_LAUNCH(k_suppress_volume, dim3(tiles, nb), dim3(SUP_THREADS), shmem, (hipStream_t)stream, V, Vs, n, r, vec,
              (const unsigned*)cand_count, nb, cap);
  return dlpd_check_launch();
}

// The complete candidate lists of the batch (flag clear, count <= cap) lose every candidate that a voxel of its ball beats
// in V; survivors keep their order and cand_count[b] is lowered.  Incomplete lists and the flags are left alone.
int dlpd_topk_suppress_cand(const float* V, int nb, int n, int r, void* cand_keys, void* cand_count, int cap, void* stream) {
  if (!cand_keys || !cand_count || cap < 64 || cap > 8192) return DLPD_ERR_ARG;
  if (int rc = sup_check(V, nb, n, r)) return rc;
  const size_t shmem = (size_t)cap * sizeof(u64);
  if (int rc = dlpd_set_max_dyn_shared((const void*)k_suppress_cand, shmem)) return rc;
  DLPD_LAUNCH(k_suppress_cand, dim3(nb), dim3(SUP_THREADS), shmem, (hipStream_t)stream, V, n, r, (u64*)cand_keys,
              (unsigned*)cand_count, nb, cap);
  return dlpd_check_launch();
}

}  // extern "C"

// The BACKWARD of the per-voxel filter (k_filter_vec / k_filter_generic, dlpd_corr.hip; DockingModels.py:74-83) -- what
// GlobalDockingModel(differentiable=True, fused_filter_grad=True) trains the filter and, through the correlations, the
// representation with.  Per fine voxel v
//
//   x     = [conv0 channels at v | conv1 channels at the coarse parent of v]            (C = C0 + C1)
//   pre_j = b1_j + sum_c W1[j,c] x_c          (the forward's fmaf chain: b1 first, then the channels in order, conv0 first)
//   out   = b2 + sum_j W2_j relu(pre_j)
//
// and for the incoming gradient g (nb, N^3), with delta_j = g W2_j [pre_j > 0] (pre is RECOMPUTED, nothing but the inputs is
// kept between forward and backward):
//
//   gconv0[c] = sum_j W1[j,c] delta_j                 gconv1[c] = sum_j W1[j,C0+c] Delta_j,  Delta_j = sum over the s^3 fine
//   gW1[j,c]  = sum_v delta_j x_c                                 children of the coarse voxel of delta_j, in a fixed order
//   gb1_j = sum_v delta_j      gW2_j = sum_v g relu(pre_j)      gb2 = sum_v g
//
// All three products are small GEMMs on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact f32 products, k-ordered
// fmaf chain -- so `pre` carries the forward's bits).  One block = 4 waves walks TILES of 128 fine voxels: the 2 x 2 (x, y)
// rows of 32 z over one coarse (x, y) -- whole coarse voxels, 16 of them, so Delta needs no atomics and no second pass:
//
//   stage   X (fine channels x 128 voxels), Xc (coarse channels x 16 coarse voxels), g                   -> LDS
//   pre     (16 hidden x 16 voxel) tiles, K = the channels; wave w owns voxel tiles 2w, 2w + 1 = row w of the tile; from the
//           accumulators: delta -> LDS, and the lane's running sums for gb1 and gW2
//   Delta   (hidden x 16 coarse voxels) in LDS: the eight children added in ascending (row, z)
//   gconv0  (16 voxel x 16 channel) tiles, K = hidden: a lane ends with 4 z-consecutive voxels of one channel, one 16-byte
//           store;  gconv1 the same from Delta, one tile of 16 coarse voxels per 16 channels
//   gW1     (16 hidden x 16 channel) tiles, K = the 128 voxels (coarse channels: Delta x Xc, K = 16); the tiles are dealt to
//           the waves (at most FG_NT each) and live in registers for the whole launch: a tile's sum starts from zero and
//           joins the lane's running total, so an element is a sum of short sums (the remedy of dlpd_conv_grad.h)
//
// With N1 = N0 the conv1 channels are fine channels like conv0's (another source and destination pointer, nothing else).
// Voxels of a tile outside the box (N not a multiple of 32, odd N) enter with x = 0 and g = 0 and are not stored.
// DETERMINISTIC SPLIT: the launch has nparts = min(tiles, FG_MAX_PARTS) blocks -- a function of the shape alone --, block p
// walks tiles p, p + nparts, ... and writes its partial [gW1t | gb1 | gW2 | gb2] to ws; k_filter_grad_reduce adds the partials
// in a fixed order in float64 and writes every element once.  No float atomics: the same bits run to run and machine to machine.
//
// LDS strides (ds_read_b32: bank = dword address mod 32 within each half of the wave = two k rows x 16 columns): the voxel
// tiles X and delta have row stride 130 and the coarse ones 18 (== 2 mod 32 and 16: sixteen rows fall on the even banks, the
// k neighbour on the odd ones), which makes the long K loops (gW1) conflict-free and leaves a two-way conflict on the reads
// of `pre`, whose K is the channel count; the weights (row = channel, stride HP + 2) the same way round.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): the table at k_filter_grad.
#pragma once

#define FG_TV 128                         // fine voxels per tile: 4 rows x 32 z
#define FG_XS 130                         // row stride of the voxel tiles in LDS
#define FG_CS 18                          // ... and of the coarse tiles (16 coarse voxels)
#define FG_NT 9                           // gW1 tiles per wave: 4 hidden tiles x 9 channel tiles (128 channels, both kinds padded) / 4 waves
#define FG_MAX_PARTS 1024                 // partial parameter gradients (blocks) of a launch
#define FG_MAX_CHANNELS 128

struct FgLayout {
  int CF, CC, CFp, CCp, HP, HS;           // fine / coarse channels and both padded to 16; hidden width padded to 16, weight row stride
  int oW, oX, oD, oXc, oDc, oG, oW2, oB1, oRed, total;   // LDS offsets (floats)
};

static inline FgLayout fg_layout(int C0, int N0, int C1, int N1, int H) {
  FgLayout L;
  const bool coarse = C1 > 0 && N1 != N0;
  L.CF = C0 + (coarse ? 0 : C1);
  L.CC = coarse ? C1 : 0;
  L.CFp = (L.CF + 15) / 16 * 16;
  L.CCp = (L.CC + 15) / 16 * 16;
  L.HP = (H + 15) / 16 * 16;
  L.HS = L.HP + 2;
  int o = 0;
  L.oW = o;   o += (L.CFp + L.CCp) * L.HS;   // W1t rows: the fine channels, then the coarse ones; zeros in the padding
  L.oX = o;   o += L.CFp * FG_XS;
  L.oD = o;   o += L.HP * FG_XS;             // delta
  L.oXc = o;  o += L.CCp * FG_CS;
  L.oDc = o;  o += L.HP * FG_CS;             // Delta
  L.oG = o;   o += FG_TV;
  L.oW2 = o;  o += DLPD_MAX_HIDDEN;
  L.oB1 = o;  o += DLPD_MAX_HIDDEN;
  L.oRed = o; o += 4 * DLPD_MAX_HIDDEN * 2;  // per wave: the gb1 and gW2 sums of its lanes
  L.total = o;
  return L;
}

static inline long long fg_tiles(int N0, int nb) {
  const long long nxy = (N0 + 1) / 2, nz = (N0 + 31) / 32;
  return (long long)nb * nxy * nxy * nz;
}

static DLPD_D dlpd_acc4 fg_add(dlpd_acc4 a, dlpd_acc4 b) {
  return dlpd_acc4_make(dlpd_acc4_get(a, 0) + dlpd_acc4_get(b, 0), dlpd_acc4_get(a, 1) + dlpd_acc4_get(b, 1),
                        dlpd_acc4_get(a, 2) + dlpd_acc4_get(b, 2), dlpd_acc4_get(a, 3) + dlpd_acc4_get(b, 3));
}

// grid nparts, block 256, dynamic LDS L.total floats.  g (nb, N^3); conv0 (nb, C0, N^3); conv1 (nb, C1, N1^3); W1t (C, H);
// gconv0 / gconv1 as the inputs or null; WS (nparts, C H + 2 H + 1) or null (no parameter gradients).
// NT: gW1 tiles a wave owns (4 NT >= hidden tiles x channel tiles), HTM: hidden tiles of 16 (HTM >= ceil(H / 16)) -- they size
// the register arrays; <2, 2> serves H <= 32 with at most four channel tiles (the reference's shapes), <FG_NT, 4> everything.
//   <NT, HTM>   VGPRs   AGPRs   scratch   waves / SIMD by registers   LDS (bytes, dynamic)
//   <2, 2>       114       8        0        4                         39,168 at [16 @ N + 32 @ N/2], H = 24; 53,504 at 48 @ N, H = 24
//   <9, 4>       228       8        0        2                         up to 146,688 (128 channels, H = 64)
// (One kernel for every shape, <9, 4> alone, would run the reference's shapes at 2 waves / SIMD; held to 128 registers by
// its launch bounds it spills 416 bytes per lane.  Hence the two.)
template <int NT, int HTM> __global__ void __launch_bounds__(256)
k_filter_grad(const float* __restrict__ g, const float* __restrict__ conv0, int C0, int N, const float* __restrict__ conv1,
              int C1, int N1, const float* __restrict__ W1t, const float* __restrict__ b1, const float* __restrict__ W2, int H,
              float* __restrict__ gconv0, float* __restrict__ gconv1, float* __restrict__ WS, int ntiles, FgLayout L) {
  DLPD_DYN_SHARED(float, S);
  float* Ws = S + L.oW;
  float* Xs = S + L.oX;
  float* Ds = S + L.oD;
  float* Xc = S + L.oXc;
  float* Dc = S + L.oDc;
  float* gs = S + L.oG;
  float* W2s = S + L.oW2;
  float* b1s = S + L.oB1;
  float* red = S + L.oRed;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, n = lane & 15;                     // fragment coordinates of this lane
  const int CF = L.CF, CC = L.CC, CFp = L.CFp, HS = L.HS, HP = L.HP;
  const int HT = HP / 16, CFT = CFp / 16, CCT = L.CCp / 16, NTILE = HT * (CFT + CCT), KH = (H + 3) / 4;   // (K steps over the hidden units: the padding rows of delta are zero)
  const int CF4 = (CF + 3) / 4, CC4 = (CC + 3) / 4;
  const bool params = WS != nullptr;
  const bool vec0 = (N % 4 == 0), vec1 = (N1 % 4 == 0);
  const size_t N3 = (size_t)N * N * N, N13 = (size_t)N1 * N1 * N1;

  // ---- once per block: the weights (row = channel as the tiles hold them, zeros in every padding), zeros in the tiles' padding rows
  for (int i = tid; i < (CFp + L.CCp) * HS; i += 256) {
    const int row = i / HS, h = i % HS;
    const int src = row < CFp ? (row < CF ? row : -1) : (row - CFp < CC ? C0 + row - CFp : -1);
    Ws[i] = (src >= 0 && h < H) ? W1t[(size_t)src * H + h] : 0.f;
  }
  for (int i = tid; i < DLPD_MAX_HIDDEN; i += 256) {
    W2s[i] = i < H ? W2[i] : 0.f;
    b1s[i] = i < H ? b1[i] : 0.f;
  }
  for (int i = tid; i < CFp * FG_XS; i += 256) Xs[i] = 0.f;
  for (int i = tid; i < L.CCp * FG_CS; i += 256) Xc[i] = 0.f;

  dlpd_acc4 tot[NT];                                        // this lane's elements of gW1, summed over the block's tiles
#pragma unroll
  for (int t = 0; t < NT; t++) tot[t] = dlpd_acc4_zero();
  float dsum[HTM][4], rsum[HTM][4], gsum = 0.f;                    // gb1, gW2 (hidden 16 ht + 4 kq + j, this lane's voxels), gb2
#pragma unroll
  for (int ht = 0; ht < HTM; ht++)
#pragma unroll
    for (int j = 0; j < 4; j++) dsum[ht][j] = rsum[ht][j] = 0.f;
  __syncthreads();

  const int nxy = (N + 1) / 2, nz = (N + 31) / 32;
  for (int tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int tz = tile % nz, ty = (tile / nz) % nxy, tx = (tile / (nz * nxy)) % nxy, b = tile / (nz * nxy * nxy);
    const int z0 = tz * 32;
    // ---- stage g, X, Xc.  Voxel v of the tile: row r = v / 32 -> (x, y) = (2 tx + r / 2, 2 ty + r % 2), z = z0 + v % 32
    if (tid < FG_TV) {
      const int r = tid >> 5, x = 2 * tx + (r >> 1), y = 2 * ty + (r & 1), z = z0 + (tid & 31);
      const float v = (x < N && y < N && z < N) ? g[(size_t)b * N3 + ((size_t)x * N + y) * N + z] : 0.f;
      gs[tid] = v;
      gsum += v;
    }
    if (vec0) {
      // float4 along z: 32 quads per channel, eight channels per pass of the block; a group of loads is issued before it is stored
      const int qd = tid & 31, cg = tid >> 5, r = qd >> 3, zq = 4 * (qd & 7);
      const int x = 2 * tx + (r >> 1), y = 2 * ty + (r & 1), z = z0 + zq;
      const bool ok = x < N && y < N && z < N;
      const size_t off = ok ? ((size_t)x * N + y) * N + z : 0;
      constexpr int CH = 4;
      for (int cb = cg; cb < CF; cb += 8 * CH) {
        float4 v[CH];
#pragma unroll
        for (int u = 0; u < CH; u++) {
          const int c = cb + 8 * u;
          if (c < CF) {
            const float* src = c < C0 ? conv0 + ((size_t)b * C0 + c) * N3 : conv1 + ((size_t)b * C1 + (c - C0)) * N3;
            v[u] = ok ? DLPD_LOAD_STREAM(reinterpret_cast<const float4*>(src + off)) : make_float4(0.f, 0.f, 0.f, 0.f);
          }
        }
#pragma unroll
        for (int u = 0; u < CH; u++) {
          const int c = cb + 8 * u;
          if (c < CF) {
            float* dst = Xs + c * FG_XS + r * 32 + zq;
            dst[0] = v[u].x; dst[1] = v[u].y; dst[2] = v[u].z; dst[3] = v[u].w;
          }
        }
      }
    } else {
      const int v = tid & 127, r = v >> 5, x = 2 * tx + (r >> 1), y = 2 * ty + (r & 1), z = z0 + (v & 31);
      const bool ok = x < N && y < N && z < N;
      const size_t off = ok ? ((size_t)x * N + y) * N + z : 0;
      for (int c = tid >> 7; c < CF; c += 2) {
        const float* src = c < C0 ? conv0 + ((size_t)b * C0 + c) * N3 : conv1 + ((size_t)b * C1 + (c - C0)) * N3;
        Xs[c * FG_XS + v] = ok ? src[off] : 0.f;
      }
    }
    for (int i = tid; i < CC * 16; i += 256) {                 // the coarse voxels (tx, ty, 16 tz + cv)
      const int cc = i >> 4, cv = i & 15, cz = tz * 16 + cv;
      Xc[cc * FG_CS + cv] = cz < N1 ? conv1[((size_t)b * C1 + cc) * N13 + ((size_t)tx * N1 + ty) * N1 + cz] : 0.f;
    }
    __syncthreads();

    // ---- pre = b1 + W1 x on voxel tiles 2 wave, 2 wave + 1 (row `wave` of the tile, z halves 0 and 1), then delta
    {
      const float* xb = Xs + kq * FG_XS + wave * 32 + n;       // B[k = channel 4 ks + kq][n = voxel]
      const float* xcb = Xc + kq * FG_CS + (n >> 1);           // ... of a coarse channel: the parent, z half 1 is 8 further
      const float g0 = gs[wave * 32 + n], g1 = gs[wave * 32 + 16 + n];
#pragma unroll
      for (int ht = 0; ht < HTM; ht++) {
        if (ht >= HT) break;                                   // (block-uniform)
        const int hb = ht * 16 + 4 * kq;                       // the accumulator holds hidden hb + j of voxel n
        dlpd_acc4 a0 = dlpd_acc4_make(b1s[hb], b1s[hb + 1], b1s[hb + 2], b1s[hb + 3]), a1 = a0;
        const float* wa = Ws + kq * HS + ht * 16 + n;          // A[m = hidden 16 ht + n][k = channel 4 ks + kq]
        for (int ks = 0; ks < CF4; ks++) {
          const float a = wa[4 * ks * HS], b0 = xb[4 * ks * FG_XS], b1v = xb[4 * ks * FG_XS + 16];
          a0 = DLPD_MFMA_16x16x4(a, b0, a0);
          a1 = DLPD_MFMA_16x16x4(a, b1v, a1);
        }
        const float* wc = wa + CFp * HS;
        for (int ks = 0; ks < CC4; ks++) {
          const float a = wc[4 * ks * HS], b0 = xcb[4 * ks * FG_CS], b1v = xcb[4 * ks * FG_CS + 8];
          a0 = DLPD_MFMA_16x16x4(a, b0, a0);
          a1 = DLPD_MFMA_16x16x4(a, b1v, a1);
        }
#pragma unroll
        for (int j = 0; j < 4; j++) {
          const float w2 = W2s[hb + j], p0 = dlpd_acc4_get(a0, j), p1 = dlpd_acc4_get(a1, j);
          const float d0 = p0 > 0.f ? g0 * w2 : 0.f, d1 = p1 > 0.f ? g1 * w2 : 0.f;
          Ds[(hb + j) * FG_XS + wave * 32 + n] = d0;
          Ds[(hb + j) * FG_XS + wave * 32 + 16 + n] = d1;
          if (params) {
            dsum[ht][j] += d0 + d1;
            rsum[ht][j] += (p0 > 0.f ? g0 * p0 : 0.f) + (p1 > 0.f ? g1 * p1 : 0.f);
          }
        }
      }
    }
    __syncthreads();
    // ---- Delta: the eight children of a coarse voxel in ascending (row, z)
    if (CC > 0) {
      for (int i = tid; i < HP * 16; i += 256) {
        const int h = i >> 4, cv = i & 15;
        const float* d = Ds + h * FG_XS + 2 * cv;
        float s = 0.f;
#pragma unroll
        for (int r = 0; r < 4; r++) s += d[r * 32] + d[r * 32 + 1];
        Dc[h * FG_CS + cv] = s;
      }
      __syncthreads();
    }

    // ---- gconv (fine channels): D[m = voxel][n = channel], K = hidden; the lane ends with voxels 4 kq + j of channel 16 ct + n
    if (gconv0 || (gconv1 && CF > C0)) {
      const int x = 2 * tx + (wave >> 1), y = 2 * ty + (wave & 1);
      const float* da = Ds + kq * FG_XS + wave * 32 + n;       // A[m = voxel n][k = hidden 4 ks + kq]
      for (int ct = 0; ct < CFT; ct++) {
        const float* wb = Ws + (ct * 16 + n) * HS + kq;        // B[k = hidden 4 ks + kq][n = channel 16 ct + n]
        dlpd_acc4 a0 = dlpd_acc4_zero(), a1 = a0;
        for (int ks = 0; ks < KH; ks++) {
          const float w = wb[4 * ks], d0 = da[4 * ks * FG_XS], d1 = da[4 * ks * FG_XS + 16];
          a0 = DLPD_MFMA_16x16x4(d0, w, a0);
          a1 = DLPD_MFMA_16x16x4(d1, w, a1);
        }
        const int c = ct * 16 + n;
        float* dst = c < C0 ? (gconv0 ? gconv0 + ((size_t)b * C0 + c) * N3 : nullptr)
                            : (gconv1 && c < CF ? gconv1 + ((size_t)b * C1 + (c - C0)) * N3 : nullptr);
        if (dst && x < N && y < N) {
          dst += ((size_t)x * N + y) * N;
#pragma unroll
          for (int half = 0; half < 2; half++) {
            const dlpd_acc4 a = half ? a1 : a0;
            const int z = z0 + half * 16 + 4 * kq;
            if (vec0) {
              if (z < N)
                *reinterpret_cast<float4*>(dst + z) = make_float4(dlpd_acc4_get(a, 0), dlpd_acc4_get(a, 1), dlpd_acc4_get(a, 2), dlpd_acc4_get(a, 3));
            } else {
#pragma unroll
              for (int j = 0; j < 4; j++)
                if (z + j < N) dst[z + j] = dlpd_acc4_get(a, j);
            }
          }
        }
      }
    }
    // ---- gconv1 (coarse channels): D[m = coarse voxel][n = channel] from Delta, one tile per 16 channels
    if (gconv1 && CC > 0) {
      for (int ct = wave; ct < CCT; ct += 4) {
        const float* wb = Ws + (CFp + ct * 16 + n) * HS + kq;
        const float* da = Dc + kq * FG_CS + n;
        dlpd_acc4 a = dlpd_acc4_zero();
        for (int ks = 0; ks < KH; ks++) a = DLPD_MFMA_16x16x4(da[4 * ks * FG_CS], wb[4 * ks], a);
        const int cc = ct * 16 + n, cz = tz * 16 + 4 * kq;
        if (cc < CC) {
          float* dst = gconv1 + ((size_t)b * C1 + cc) * N13 + ((size_t)tx * N1 + ty) * N1;
          if (vec1) {
            if (cz < N1)
              *reinterpret_cast<float4*>(dst + cz) = make_float4(dlpd_acc4_get(a, 0), dlpd_acc4_get(a, 1), dlpd_acc4_get(a, 2), dlpd_acc4_get(a, 3));
          } else {
#pragma unroll
            for (int j = 0; j < 4; j++)
              if (cz + j < N1) dst[cz + j] = dlpd_acc4_get(a, j);
          }
        }
      }
    }
    // ---- gW1: D[m = hidden][n = channel], K = the tile's voxels; tile q = wave + 4 t -> (ht, ct) = (q % HT, q / HT)
    if (params) {
#pragma unroll
      for (int t = 0; t < NT; t++) {
        const int q = wave + 4 * t;
        if (q >= NTILE) break;                                 // (wave-uniform)
        const int ht = q % HT, ct = q / HT;
        dlpd_acc4 a = dlpd_acc4_zero();
        if (ct < CFT) {
          const float* da = Ds + (ht * 16 + n) * FG_XS + kq;   // A[m = hidden][k = voxel 4 ks + kq]
          const float* xb = Xs + (ct * 16 + n) * FG_XS + kq;   // B[k = voxel][n = channel]
          for (int ks = 0; ks < FG_TV / 4; ks++) a = DLPD_MFMA_16x16x4(da[4 * ks], xb[4 * ks], a);
        } else {
          const float* da = Dc + (ht * 16 + n) * FG_CS + kq;
          const float* xb = Xc + ((ct - CFT) * 16 + n) * FG_CS + kq;
#pragma unroll
          for (int ks = 0; ks < 4; ks++) a = DLPD_MFMA_16x16x4(da[4 * ks], xb[4 * ks], a);
        }
        tot[t] = fg_add(tot[t], a);
      }
    }
    __syncthreads();                                           // the tiles are consumed
  }
  if (!params) return;

  // ---- this block's partial [gW1t (C, H) | gb1 | gW2 | gb2]
  const int P = (C0 + C1) * H + 2 * H + 1;
  float* Wp = WS + (size_t)blockIdx.x * P;
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int q = wave + 4 * t;
    if (q >= NTILE) break;
    const int ht = q % HT, ct = q / HT;
    const int cl = (ct < CFT ? ct : ct - CFT) * 16 + n;
    const int row = ct < CFT ? (cl < CF ? cl : -1) : (cl < CC ? C0 + cl : -1);
    if (row < 0) continue;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      const int h = ht * 16 + 4 * kq + j;
      if (h < H) Wp[(size_t)row * H + h] = dlpd_acc4_get(tot[t], j);
    }
  }
  // gb1, gW2: the 16 voxel columns of a wave by a fixed butterfly, then the four waves in order
#pragma unroll
  for (int ht = 0; ht < HTM; ht++) {
    if (ht >= HT) break;
#pragma unroll
    for (int j = 0; j < 4; j++) {
      float d = dsum[ht][j], r = rsum[ht][j];
#pragma unroll
      for (int m = 1; m < 16; m <<= 1) {
        d += __shfl_xor(d, m);
        r += __shfl_xor(r, m);
      }
      if (n == 0) {
        red[(wave * 2 + 0) * DLPD_MAX_HIDDEN + ht * 16 + 4 * kq + j] = d;
        red[(wave * 2 + 1) * DLPD_MAX_HIDDEN + ht * 16 + 4 * kq + j] = r;
      }
    }
  }
  if (tid < FG_TV) gs[tid] = gsum;
  __syncthreads();
  if (tid < H) {
    double d = 0.0, r = 0.0;
    for (int w = 0; w < 4; w++) {
      d += (double)red[(w * 2 + 0) * DLPD_MAX_HIDDEN + tid];
      r += (double)red[(w * 2 + 1) * DLPD_MAX_HIDDEN + tid];
    }
    Wp[(size_t)(C0 + C1) * H + tid] = (float)d;
    Wp[(size_t)(C0 + C1) * H + H + tid] = (float)r;
  }
  if (tid == 64) {                                             // (a lane of another wave than the hidden units' for H <= 64)
    double s = 0.0;
    for (int i = 0; i < FG_TV; i++) s += (double)gs[i];
    Wp[P - 1] = (float)s;
  }
}

// gparams[e] = the sum of ws[p][e] over the parts, in a fixed order, carried in float64 and rounded once; every element
// written once.  Block = 16 elements x 16 groups: group q adds parts q, q + 16, ... in ascending order, then the sixteen group
// sums are added in ascending q (one thread walking a thousand partials alone took 48 us, a tenth of the backward).
#define FG_RG 16
__global__ void __launch_bounds__(256) k_filter_grad_reduce(const float* __restrict__ ws, float* __restrict__ gp, int total,
                                                            int nparts) {
  __shared__ double part[FG_RG][16];
  const int el = threadIdx.x & 15, q = threadIdx.x >> 4, e = blockIdx.x * 16 + el;
  double s = 0.0;
  if (e < total)
    for (int p = q; p < nparts; p += FG_RG) s += (double)ws[(size_t)p * total + e];
  part[q][el] = s;
  __syncthreads();
  if (q == 0 && e < total) {
    double r = 0.0;
#pragma unroll
    for (int k = 0; k < FG_RG; k++) r += part[k][el];
    gp[e] = (float)r;
  }
}

template <int NT, int HTM> static int fg_launch(const float* g, const float* conv0, int C0, int N0, const float* conv1, int C1, int N1,
                                                const float* W1t, const float* b1, const float* W2, int H, float* gconv0,
                                                float* gconv1, float* ws, int ntiles, int nparts, FgLayout L, hipStream_t st) {
  const size_t shmem = (size_t)L.total * sizeof(float);
  int rc = dlpd_set_max_dyn_shared((const void*)k_filter_grad<NT, HTM>, shmem);
  if (rc) return rc;
  DLPD_LAUNCH((k_filter_grad<NT, HTM>), dim3((unsigned)nparts), dim3(256), shmem, st, g, conv0, C0, N0, conv1, C1, N1, W1t, b1, W2, H,
              gconv0, gconv1, ws, ntiles, L);
  return DLPD_OK;
}
#define FG_ARGS g, conv0, C0, N0, conv1, C1, C1 > 0 ? N1 : N0, W1t, b1, W2, H, gconv0, gconv1, gparams ? (float*)ws : (float*)nullptr, \
                (int)tiles, nparts, L, st

extern "C" {

int dlpd_filter_grad_supported(int C0, int N0, int C1, int N1, int H) {
  if (H < 1 || H > DLPD_MAX_HIDDEN || C0 < 1 || C1 < 0 || N0 < 2 || C0 + C1 > FG_MAX_CHANNELS) return 0;
  if (C1 > 0 && !(N1 == N0 || (N0 % 2 == 0 && N1 == N0 / 2))) return 0;
  return 1;
}

static inline int fg_nparts(int N0, int nb) {
  const long long tiles = fg_tiles(N0, nb);
  return (int)(tiles < FG_MAX_PARTS ? tiles : FG_MAX_PARTS);
}

size_t dlpd_filter_grad_ws_bytes(int C0, int N0, int C1, int N1, int H, int nb) {
  if (nb <= 0 || !dlpd_filter_grad_supported(C0, N0, C1, N1, H)) return 0;
  return (size_t)fg_nparts(N0, nb) * ((size_t)(C0 + C1) * H + 2 * H + 1) * sizeof(float);
}

int dlpd_filter_grad(const float* g, const float* conv0, int C0, int N0, const float* conv1, int C1, int N1, const float* W1t,
                     const float* b1, const float* W2, int H, float* gconv0, float* gconv1, float* gparams, void* ws, int nb,
                     void* stream) {
  if (!g || !conv0 || !W1t || !b1 || !W2 || nb <= 0 || C0 <= 0 || C1 < 0 || N0 <= 0 || H <= 0) return DLPD_ERR_ARG;
  if ((C1 > 0 && (!conv1 || N1 <= 0)) || (gconv1 && C1 == 0) || (!gconv0 && !gconv1 && !gparams) || (gparams && !ws))
    return DLPD_ERR_ARG;
  if (!dlpd_filter_grad_supported(C0, N0, C1, N1, H)) return DLPD_ERR_UNSUPPORTED;
  const long long tiles = fg_tiles(N0, nb);
  if (tiles > 0x7fffffffLL) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const FgLayout L = fg_layout(C0, N0, C1, N1, H);
  const int nparts = fg_nparts(N0, nb);
  const int HT = L.HP / 16, ntile = HT * (L.CFp + L.CCp) / 16;       // gW1 tiles: at most 4 NT; hidden tiles: at most HTM
  int rc;
  if (HT <= 2 && ntile <= 8) rc = fg_launch<2, 2>(FG_ARGS);
  else rc = fg_launch<FG_NT, 4>(FG_ARGS);
  if (rc) return rc;
  if (gparams) {
    const int total = (C0 + C1) * H + 2 * H + 1;
    DLPD_LAUNCH(k_filter_grad_reduce, dim3((unsigned)((total + 15) / 16)), dim3(256), 0, st, (const float*)ws, gparams, total,
                nparts);
  }
  return dlpd_check_launch();
}

}  // extern "C"

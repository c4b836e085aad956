// Representation-plugin convolution, backward with respect to the WEIGHTS -- what LocalTrainer.optimize's L.backward()
// (src/Training/LocalTrainer.py) asks of the nine Conv3d layers per protein (stride 1, padding k/2, no bias):
//
//   gW[co][ci][dx,dy,dz] = sum_b sum_v  gY[b][co][v] * X[b][ci][v + (dx,dy,dz) - k/2]          (zeros outside the box)
//
// as an implicit GEMM on the f32-input matrix cores (v_mfma_f32_16x16x4_f32: exact f32 products, k-ordered fmaf chain):
//   M = 16 output channels, K = 4 z-consecutive voxels, N = 16 COLUMNS; a column is a (input channel of the chunk, tap) pair.
// (The gradient with respect to the INPUT needs no kernel of its own: it is the forward kernel on gY with the flipped,
// transposed weights -- ops.conv3d_input_grad.)
//
// One block = 8 waves walks a list of (volume, 4 x 4 (x, y) patch of full-z rows) items.  Per item and chunk of four input
// channels the halo tile of X goes to LDS as in the forward kernel (ConvCfg's patch and halo); the gY rows of the patch sit
// next to it, one x of the patch (four rows x all output channels of the block) at a time.  The 4 k^3 columns of a chunk are
// dealt to the waves in tiles of 16 (k = 3: 7 tiles, one per wave, the eighth wave only stages; k = 5: 32 tiles, 4 per wave);
// every lane computes the LDS address of ITS column once (channel plane + tap offset), so a B fragment is one ds_read_b32
// at base + lane offset; an A fragment (gY) is one ds_read_b32 shared by all the wave's column tiles.  The f32 matrix
// instruction takes 32 cycles: per instruction the kernel needs (MT + NT) / (MT NT) LDS reads (MT output-channel tiles, NT
// column tiles: 2 at worst, k = 3 with 16 output channels), half of what the LDS delivers in that time.
// LDS strides (ds_read_b32: bank = dword address mod 32 within each half of the wave = two k rows x 16 columns; equal
// addresses broadcast): the z row stride of the X tile is 16 NZT + 6 for both kernel sizes, the channel plane stride is
// == 8 (mod 32) for k = 5 with the channel the fastest column index, and unpadded for k = 3 with the tap the fastest -- every
// B read of every column tile is conflict-free (enumerated over all tiles when the strides were chosen); the gY row stride
// 16 NZT + 2 is twice an odd number, so the 16 channels x 2 k rows of an A read fall on 32 different banks.
//
// A wave holds NT x MT accumulator tiles.  They are SHORT sums: after every (item, chunk) -- at most 16 rows x D voxels --
// each lane adds them to the elements of the part's partial gW it owns (a lane owns the same elements for the whole launch:
// a plain read-add-write, no other thread touches them) and starts again from zero.  A running f32 sum over all voxels of
// a part would carry the rounding error of its length; this way an output is a sum of sums, the remedy the plan-free
// transforms use (GEN_NACC, dlpd_generic.hip).  Input channels beyond sixteen and output channels beyond 16 MT are other
// blocks (grid y and z).  DETERMINISTIC SPLIT over the voxels: the launch has `nparts` blocks along x, block p walks items
// p, p + nparts, ... in ascending order and writes its full partial gW to ws (nparts, cout, cin, k^3) -- zeros if it has no
// item --, and k_conv3d_wgrad_reduce adds the partials in ascending p, carried in float64, and writes every element of gW
// once.  No float atomics; nparts is the caller's constant, not a device property: the same bits run to run and machine to
// machine.
//
// Compiler report (-Rpass-analysis=kernel-resource-usage, gfx950): the table at k_conv3d_wgrad.
#pragma once

template <int KS, int NZT> struct ConvGradCfg {
  typedef ConvCfg<KS, 16, NZT> F;                              // the forward kernel's patch and halo
  static constexpr int TX = F::TX, TY = F::TY, NW = F::NW, H = F::H, XS = F::XS, YS = F::YS;
  static constexpr int ZS = NZT * 16 + 6;                      // X row stride (floats): >= 16 NZT + KS - 1, see the banks above
  static constexpr int PLANE = XS * YS * ZS + (KS == 5 ? 8 : 0);
  static constexpr bool CI_FASTEST = (KS == 5);                // column j -> (channel, tap): j % 4, j / 4  |  j / NTAP, j % NTAP
  static constexpr int GZS = NZT * 16 + 2;                     // gY row stride
  static constexpr int NTAP = KS * KS * KS, NCOL = 4 * NTAP, NTILE = (NCOL + 15) / 16, NT = (NTILE + NW - 1) / NW;
  static constexpr int CPG = 4;                                // chunks (of four input channels) a block walks: 16 channels per grid y
  static constexpr int GROWS = TY;                             // gY rows in LDS at a time: one x of the patch
  template <int MT> static constexpr size_t lds_bytes() { return (size_t)(4 * PLANE + GROWS * 16 * MT * GZS) * sizeof(float); }
  static_assert(ZS >= NZT * 16 + KS - 1, "the halo must fit the row");
};

// grid (nparts, ceil(cin / 16), cout / (16 MT)), block 512.  X (B, CIN, D^3), GY (B, COUT, D^3), WS (nparts, COUT, CIN, KS^3).
//   <KS, MT, NZT>   VGPRs   AGPRs   scratch   LDS (bytes, dynamic)   waves / SIMD by registers
//   <3, 1, 3>         36       0        0         43,904                 8
//   <3, 1, 5>         37       0        0         70,528                 7
//   <3, 2, 3>         48       0        0         56,704                 8
//   <3, 2, 5>         49       0        0         91,520                 7
//   <5, 1, 3>         71       0        0         68,224                 7
//   <5, 1, 5>         63       0        0        109,184                 8
//   <5, 2, 3>         87       0        0         81,024                 5
//   <5, 2, 5>         83       0        0        130,176                 5
template <int KS, int MT, int NZT> __global__ void __launch_bounds__(512)
k_conv3d_wgrad(const float* __restrict__ X, const float* __restrict__ GY, float* __restrict__ WS, int B, int CIN, int COUT,
               int D) {
  typedef ConvGradCfg<KS, NZT> C;
  constexpr int H = C::H, NT = C::NT, CPG = C::CPG, NTAP = C::NTAP, GCH = 16 * MT;
  DLPD_DYN_SHARED(float, S);
  float* Xs = S;                         // [4][XS][YS][ZS] (+ plane padding)
  float* Gs = S + 4 * C::PLANE;          // [GROWS][16 MT][GZS]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int kq = lane >> 4, n = lane & 15;                     // fragment coordinates of this lane
  const int part = blockIdx.x, nparts = gridDim.x, ci0 = blockIdx.y * 4 * CPG, co0 = blockIdx.z * GCH;
  const int npx = (D + C::TX - 1) / C::TX, npy = (D + C::TY - 1) / C::TY, nitem = B * npx * npy;
  const int nch = min(CPG, (CIN - ci0 + 3) / 4);               // chunks of this block that hold a channel
  const size_t D3 = (size_t)D * D * D;
  const bool computes = wave * NT < C::NTILE;                  // (k = 3: seven column tiles for eight waves)
  // this lane's column of each of the wave's tiles: (channel of the chunk, tap) and where its B operand starts in the tile
  int bcol[NT], boff[NT];
#pragma unroll
  for (int t = 0; t < NT; t++) {
    const int j = (wave * NT + t) * 16 + n;
    bcol[t] = j < C::NCOL ? j : -1;                            // (padding columns read column 0 and are not written)
    const int jj = j < C::NCOL ? j : 0;
    const int k = C::CI_FASTEST ? jj % 4 : jj / NTAP, tap = C::CI_FASTEST ? jj / 4 : jj % NTAP;
    const int dz = tap % KS, dy = (tap / KS) % KS, dx = tap / (KS * KS);
    boff[t] = k * C::PLANE + (dx * C::YS + dy) * C::ZS + dz + kq;
  }
  // This part's partial gW: a lane holds rows (output channels) 4 kq + j, column n of each of its tiles -- for a given chunk
  // the SAME elements of ws from the first item to the last, so the sums of (item, chunk) go to their elements by a plain
  // read-add-write of the one lane that owns them (first item: a store; a part without items stores the zeros), and one set
  // of NT x MT accumulators serves every chunk.
  float* Wp = WS + (size_t)part * COUT * CIN * NTAP;
  dlpd_acc4 acc[NT][MT];
  auto restart = [&]() {
#pragma unroll
    for (int t = 0; t < NT; t++)
#pragma unroll
      for (int mt = 0; mt < MT; mt++) acc[t][mt] = dlpd_acc4_zero();
  };
  auto flush = [&](int c, bool first) {
#pragma unroll
    for (int t = 0; t < NT; t++) {
      if (bcol[t] < 0 || !computes) continue;
      const int k = C::CI_FASTEST ? bcol[t] % 4 : bcol[t] / NTAP, tap = C::CI_FASTEST ? bcol[t] / 4 : bcol[t] % NTAP;
      const int ci = ci0 + 4 * c + k;
      if (ci >= CIN) continue;
#pragma unroll
      for (int mt = 0; mt < MT; mt++)
#pragma unroll
        for (int j = 0; j < 4; j++) {
          float* w = Wp + ((size_t)(co0 + mt * 16 + 4 * kq + j) * CIN + ci) * NTAP + tap;
          const float v = dlpd_acc4_get(acc[t][mt], j);
          *w = first ? v : *w + v;
        }
    }
  };
  restart();
  constexpr int NROW = 4 * C::XS * C::YS, ZL = (C::ZS + 63) / 64, NGROW = C::GROWS * GCH, GL = (C::GZS + 63) / 64;
  if (part >= nitem)                                           // (block-uniform) more parts than items: this one is zero
    for (int c = 0; c < nch; c++) flush(c, true);
  for (int item = part; item < nitem; item += nparts) {
    const int b = item / (npx * npy), x0 = ((item / npy) % npx) * C::TX, y0 = (item % npy) * C::TY;
    const float* Xb = X + (size_t)b * CIN * D3;
    const float* Gb = GY + ((size_t)b * COUT + co0) * D3;
    for (int c = 0; c < nch; c++) {
      __syncthreads();                                         // the previous tile and gY rows are consumed
      // ---- the chunk's halo tile: one z row per wave and step (the forward kernel's staging)
      for (int row = wave; row < NROW; row += C::NW) {
        const int yy = row % C::YS, xx = (row / C::YS) % C::XS, k = row / (C::YS * C::XS);
        const int gx = x0 + xx - H, gy = y0 + yy - H, ci = ci0 + 4 * c + k;
        const bool ok = ci < CIN && gx >= 0 && gx < D && gy >= 0 && gy < D;
        const float* src = Xb + (size_t)(ok ? ci : 0) * D3 + ((size_t)(ok ? gx : 0) * D + (ok ? gy : 0)) * D;
        float* dst = Xs + k * C::PLANE + (xx * C::YS + yy) * C::ZS;
#pragma unroll
        for (int q = 0; q < ZL; q++) {
          const int zz = q * 64 + lane;
          if (zz < C::ZS) dst[zz] = (ok && zz >= H && zz < D + H) ? src[zz - H] : 0.f;
        }
      }
      for (int rx = 0; rx < C::TX; rx++) {
        const int gx = x0 + rx;
        if (gx >= D) break;                                    // (block-uniform) the patch hangs over the box
        if (rx > 0) __syncthreads();                           // the previous x's gY rows are consumed
        // ---- the gY rows of this x: [ry][co][z], zeros behind the box (the K = 4 steps run to a multiple of four)
        for (int row = wave; row < NGROW; row += C::NW) {
          const int ry = row / GCH, co = row % GCH, gy = y0 + ry;
          const bool ok = gy < D;
          const float* src = Gb + (size_t)co * D3 + ((size_t)gx * D + (ok ? gy : 0)) * D;
          float* dst = Gs + row * C::GZS;
#pragma unroll
          for (int q = 0; q < GL; q++) {
            const int z = q * 64 + lane;
            if (z < C::GZS) dst[z] = (ok && z < D) ? src[z] : 0.f;
          }
        }
        __syncthreads();
        if (!computes) continue;                               // (wave-uniform)
        for (int ry = 0; ry < C::TY; ry++) {
          if (y0 + ry >= D) break;                             // (block-uniform)
          const float* ga = Gs + (ry * GCH + n) * C::GZS + kq;
          const float* xb = Xs + (rx * C::YS + ry) * C::ZS;
          for (int z0 = 0; z0 < D; z0 += 4) {
            float a[MT], bv[NT];
#pragma unroll
            for (int mt = 0; mt < MT; mt++) a[mt] = ga[mt * 16 * C::GZS + z0];
#pragma unroll
            for (int t = 0; t < NT; t++) bv[t] = xb[boff[t] + z0];
#pragma unroll
            for (int t = 0; t < NT; t++)
#pragma unroll
              for (int mt = 0; mt < MT; mt++) acc[t][mt] = DLPD_MFMA_16x16x4(a[mt], bv[t], acc[t][mt]);
          }
        }
      }
      flush(c, item == part);                                  // the sums of (item, chunk) join the part's; the accumulators restart
      restart();
    }
  }
}

// gw[e] = ws[0][e] + ws[1][e] + ... in ascending part order, carried in float64 and rounded once; every element written once
__global__ void __launch_bounds__(256) k_conv3d_wgrad_reduce(const float* __restrict__ ws, float* __restrict__ gw, int total,
                                                             int nparts) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= total) return;
  double s = 0.0;
  for (int p = 0; p < nparts; p++) s += (double)ws[(size_t)p * total + e];
  gw[e] = (float)s;
}

template <int KS, int MT, int NZT> static int launch_conv_wgrad(const float* X, const float* GY, float* WS, int B, int CIN,
                                                                int COUT, int D, int nparts, hipStream_t st) {
  typedef ConvGradCfg<KS, NZT> C;
  dim3 grid(nparts, (CIN + 4 * C::CPG - 1) / (4 * C::CPG), COUT / (16 * MT)), block(512);
  int rc = dlpd_set_max_dyn_shared((const void*)k_conv3d_wgrad<KS, MT, NZT>, C::template lds_bytes<MT>());
  if (rc) return rc;
  DLPD_LAUNCH((k_conv3d_wgrad<KS, MT, NZT>), grid, block, C::template lds_bytes<MT>(), st, X, GY, WS, B, CIN, COUT, D);
  return dlpd_check_launch();
}

extern "C" {

size_t dlpd_conv3d_wgrad_ws_floats(int cin, int cout, int ks, int nparts) {
  if (cin <= 0 || cout <= 0 || ks <= 0 || nparts <= 0) return 0;
  return (size_t)nparts * cout * cin * ks * ks * ks;
}

int dlpd_conv3d_wgrad(const float* x, const float* gy, float* gw, float* ws, int B, int cin, int cout, int D, int ks,
                      int nparts, void* stream) {
  // (nparts bounds the workspace, nparts partial gW: 65535 is far beyond any use, not a limit of the grid)
  if (!x || !gy || !gw || !ws || B <= 0 || nparts <= 0 || nparts > 65535) return DLPD_ERR_ARG;
  if (!dlpd_conv3d_supported(cin, cout, ks, D)) return DLPD_ERR_UNSUPPORTED;
  const size_t total = (size_t)cout * cin * ks * ks * ks;
  if (total > 0x7fffffffu || (size_t)B * ((D + 3) / 4) * ((D + 3) / 4) > 0x7fffffffu) return DLPD_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int mt = cout % 32 == 0 ? 2 : 1, nzt = D <= 48 ? 3 : 5;
  int rc = DLPD_ERR_UNSUPPORTED;
#define DLPD_WGRAD(KS, MT, NZ) if (ks == KS && mt == MT && nzt == NZ) \
  rc = launch_conv_wgrad<KS, MT, NZ>(x, gy, ws, B, cin, cout, D, nparts, st)
  DLPD_WGRAD(3, 1, 3); DLPD_WGRAD(3, 1, 5); DLPD_WGRAD(3, 2, 3); DLPD_WGRAD(3, 2, 5);
  DLPD_WGRAD(5, 1, 3); DLPD_WGRAD(5, 1, 5); DLPD_WGRAD(5, 2, 3); DLPD_WGRAD(5, 2, 5);
#undef DLPD_WGRAD
  if (rc) return rc;
  DLPD_LAUNCH(k_conv3d_wgrad_reduce, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, st, ws, gw, (int)total, nparts);
  return dlpd_check_launch();
}

}  // extern "C"

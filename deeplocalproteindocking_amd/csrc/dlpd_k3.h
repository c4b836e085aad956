// Declarations shared by the K3 kernels (z-axis C2R + filter MLP + clash mask): dlpd_corr.hip (channel-owning waves,
// barrier-separated phases) and dlpd_k3r.hip (role-split waves).
#pragma once
#include <dlpd_platform.h>
#include "dlpd_fft.h"

// LDS geometry of a K3 block, read by the kernel AND its launcher.  A tile is TY y-rows = NPAIR two-row complex pencils of
// RS elements; a transform wave holds 8 pencils = CPW channels; a 64-lane DMA instruction fetches LPK kz rows of a channel
// into its raw staging area of RAWC float4 slots.
template <int N, int TY> struct K3Tile {
  static constexpr int NZ = N / 2 + 1, RS = N + 8, NPAIR = TY / 2;
  static constexpr int CPW = 8 / NPAIR, LPK = 64 / NPAIR;
};
// channel-owning waves (dlpd_corr.hip), Cfg = K3Cfg: WC x 8 pencils | twiddles | raw[WC][CPW][RAWC], RAWC in whole waves
template <int N, class Cfg> struct K3Lds : K3Tile<N, Cfg::TY> {
  typedef K3Tile<N, Cfg::TY> T;
  static constexpr int RAWC = ((T::NZ * T::NPAIR + 63) / 64) * 64;
  static constexpr size_t BYTES = (size_t)(Cfg::WC * 8 * T::RS + N) * sizeof(cplx) + (size_t)Cfg::WC * T::CPW * RAWC * 16;
};
// role-split waves (dlpd_k3r.hip), Cfg = K3rCfg: PBUF x F x 8 pencils | twiddles | raw[RAWBUF][F][CPW][RAWC]; RAWC in whole
// waves, or -- where two pencil buffers leave no room -- exactly the channel, the last DMA instruction then running on NPAIR
// lanes only
template <int N, class Cfg> struct K3rLds : K3Tile<N, Cfg::TY> {
  typedef K3Tile<N, Cfg::TY> T;
  static constexpr int RAWC = (Cfg::PBUF == 2) ? T::NZ * T::NPAIR : ((T::NZ * T::NPAIR + 63) / 64) * 64;
  static constexpr size_t BYTES = (size_t)(Cfg::PBUF * Cfg::F * 8 * T::RS + N) * sizeof(cplx) +
                                  (size_t)Cfg::RAWBUF * Cfg::F * T::CPW * RAWC * 16;
};

// channels per group.  One channel per wave (16-row tiles, N <= 128): as many as there are channel-owning waves -- 49
// channels on 8 waves are six full groups and one with the clash channel alone, 1 % faster than seven groups of seven,
// which leave a wave idle in every transform phase.  Two channels per wave (8-row tiles, N = 160): balanced groups
// (17 channels on 10 slots: 9 + 8 is 3 % faster than 10 + 7).  The role-split kernel always balances.
static inline int k3_group(int CT, int maxg, bool balanced) {
  if (!balanced) return CT < maxg ? CT : maxg;
  const int ng = (CT + maxg - 1) / maxg;
  return (CT + ng - 1) / ng;
}

// Extra first-layer inputs that are already real volumes on the coarser (N/2) grid, nearest-upsampled by
// index (DockingModels.py:74-76): either the Caux clipped correlations of that resolution (W1t rows
// C..C+Caux-1 are applied here), or -- is_preact -- the HP first-layer pre-activations k_filter_preact
// computed from them once per COARSE voxel (bias included; the first layer is linear): 8x fewer multiply-adds.
struct K3Aux {
  const float* p;   // (nb, Caux or HP, Naux^3), Naux = N/2
  int C, N, is_preact;
};
// Candidate emission for the top-K stage (dlpd_topk.hip, candidate path): every score whose order-preserving key is
// <= *tau is appended to the rotation's list; *tau == 0 means "no valid filter yet" and flags the rotation for the
// full radix select.  tau is written by the merge kernel of earlier batches on another stream: a stale (larger) value
// only lengthens the list.  count: [0, nb) counters, [nb, 2 nb) need-full flags.
struct K3Cand {
  const unsigned* tau;
  unsigned long long* keys;   // (nb, cap)
  unsigned* count;
  int cap, nb;
};
DLPD_D unsigned k3_score_key(float v) {           // == f2key of dlpd_topk.hip
  v = v + 0.0f;
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
DLPD_D void k3_emit(const K3Cand& cd, unsigned tau, int b, unsigned flat, float score) {
  const unsigned key = k3_score_key(score);
  if (key <= tau) {
    const unsigned slot = atomicAdd(&cd.count[b], 1u);
    if (slot < (unsigned)cd.cap) cd.keys[(size_t)b * cd.cap + slot] = ((unsigned long long)key << 32) | flat;
  }
}

// In-register mixed-radix Stockham FFT passes for LDS-resident pencils (gfx950).
//
// A length-N transform is a short list of passes (N=64: 8x8, N=128: 16x8, N=80: 8x10,
// N=160: 16x10).  T threads cooperate on one pencil; in a pass of radix R each thread
// loads R strided elements per butterfly into registers, applies the Stockham twiddle,
// does the radix-R DFT in registers (load()), and after a barrier scatters the results back
// to the SAME pencil storage at the autosort positions (store()).  Because every read of a
// pass happens before the barrier and every write after it, the transform is in place.
//
// Built-in zero-padding pruning: NNZ < N declares that only the first NNZ inputs of the first
// pass are non-zero (the docking grids are 2L-padded L-boxes), so those loads are skipped.
#pragma once
#include <dlpd_platform.h>

typedef float2 cplx;

DLPD_HD cplx c_make(float a, float b) { cplx r; r.x = a; r.y = b; return r; }
DLPD_HD cplx c_conj(cplx a) { return c_make(a.x, -a.y); }
#if defined(DLPD_PK) && DLPD_PK && defined(__HIP_DEVICE_COMPILE__)
// packed forms (dlpd_platform.h): one VOP3P instruction per complex add, two per multiply
DLPD_D cplx c_add(cplx a, cplx b) { return dlpd_c_add(a, b); }
DLPD_D cplx c_sub(cplx a, cplx b) { return dlpd_c_sub(a, b); }
DLPD_D cplx c_mul(cplx a, cplx b) { return dlpd_c_mul(a, b); }
DLPD_D cplx c_mulc(cplx a, cplx b) { return dlpd_c_mulc(a, b); }
DLPD_D cplx c_scale(cplx a, float s) { return dlpd_c_scale(a, s); }
DLPD_D cplx c_axpy(cplx a, float s, cplx b) { return dlpd_c_axpy(a, s, b); }
// a + exp(DIR*i*pi/2) * b   and   a - exp(DIR*i*pi/2) * b
template <int DIR> DLPD_D cplx c_add_rot(cplx a, cplx b) { return DIR < 0 ? dlpd_c_add_mi(a, b) : dlpd_c_add_pi(a, b); }
template <int DIR> DLPD_D cplx c_sub_rot(cplx a, cplx b) { return DIR < 0 ? dlpd_c_add_pi(a, b) : dlpd_c_add_mi(a, b); }
template <int DIR> DLPD_D cplx c_rot90(cplx a) { return c_add_rot<DIR>(c_make(0.f, 0.f), a); }
// multiply by (c + DIR*i*s): c*a + s * (DIR*i*a)
template <int DIR> DLPD_D cplx c_rotcs(cplx a, float c, float s) {
  return DIR < 0 ? dlpd_c_rotcs_m(a, c, s) : dlpd_c_rotcs_p(a, c, s);
}
#else
DLPD_HD cplx c_add(cplx a, cplx b) { return c_make(a.x + b.x, a.y + b.y); }
DLPD_HD cplx c_sub(cplx a, cplx b) { return c_make(a.x - b.x, a.y - b.y); }
DLPD_HD cplx c_mul(cplx a, cplx b) { return c_make(a.x * b.x - a.y * b.y, a.x * b.y + a.y * b.x); }
// a * conj(b)
DLPD_HD cplx c_mulc(cplx a, cplx b) { return c_make(a.x * b.x + a.y * b.y, a.y * b.x - a.x * b.y); }
DLPD_HD cplx c_scale(cplx a, float s) { return c_make(a.x * s, a.y * s); }
DLPD_HD cplx c_axpy(cplx a, float s, cplx b) { return c_make(a.x + s * b.x, a.y + s * b.y); }

// multiply by exp(DIR * i * pi/2):  DIR=-1 (forward) -> -i*a ; DIR=+1 (inverse) -> +i*a
template <int DIR> DLPD_HD cplx c_rot90(cplx a) {
  return DIR < 0 ? c_make(a.y, -a.x) : c_make(-a.y, a.x);
}
template <int DIR> DLPD_HD cplx c_add_rot(cplx a, cplx b) { return c_add(a, c_rot90<DIR>(b)); }
template <int DIR> DLPD_HD cplx c_sub_rot(cplx a, cplx b) { return c_sub(a, c_rot90<DIR>(b)); }
// multiply by (c + DIR*i*s) i.e. exp(DIR*i*phi) with c=cos(phi), s=sin(phi)
template <int DIR> DLPD_HD cplx c_rotcs(cplx a, float c, float s) {
  return DIR < 0 ? c_make(a.x * c + a.y * s, a.y * c - a.x * s)
                 : c_make(a.x * c - a.y * s, a.y * c + a.x * s);
}
#endif

// tw[k] = exp(-2 pi i k / N), k < N, made by the block's nthreads threads (every kernel's twiddle table in LDS)
template <int N> DLPD_D void init_twiddles(cplx* tw, int tid, int nthreads) {
  for (int k = tid; k < N; k += nthreads) {
    double s, c;
    sincospi(-2.0 * (double)k / (double)N, &s, &c);
    tw[k] = c_make((float)c, (float)s);
  }
}

#define DLPD_SQRT1_2 0.70710678118654752440f
#define DLPD_COS_PI_8 0.92387953251128675613f
#define DLPD_SIN_PI_8 0.38268343236508977173f
#define DLPD_COS_2PI_5 0.30901699437494742410f
#define DLPD_COS_4PI_5 (-0.80901699437494742410f)
#define DLPD_SIN_2PI_5 0.95105651629515357212f
#define DLPD_SIN_4PI_5 0.58778525229247312917f
#define DLPD_COS_PI_5 0.80901699437494742410f
#define DLPD_SIN_PI_5 0.58778525229247312917f

// ---- small DFTs in registers: v[k] <- sum_n v[n] exp(DIR*2*pi*i*n*k/R), natural order ----
template <int DIR> DLPD_HD void dft2(cplx& a, cplx& b) {
  cplx t = c_sub(a, b);
  a = c_add(a, b);
  b = t;
}
template <int DIR> DLPD_HD void dft4(cplx& a0, cplx& a1, cplx& a2, cplx& a3) {
  cplx t0 = c_add(a0, a2), t1 = c_sub(a0, a2);
  cplx t2 = c_add(a1, a3), t3 = c_sub(a1, a3);
  a0 = c_add(t0, t2);
  a1 = c_add_rot<DIR>(t1, t3);
  a2 = c_sub(t0, t2);
  a3 = c_sub_rot<DIR>(t1, t3);
}
template <int DIR> DLPD_HD void dft5(cplx& a0, cplx& a1, cplx& a2, cplx& a3, cplx& a4) {
  cplx s1 = c_add(a1, a4), d1 = c_sub(a1, a4);
  cplx s2 = c_add(a2, a3), d2 = c_sub(a2, a3);
  cplx x0 = c_add(a0, c_add(s1, s2));
  cplx p1 = c_axpy(c_axpy(a0, DLPD_COS_2PI_5, s1), DLPD_COS_4PI_5, s2);
  cplx p2 = c_axpy(c_axpy(a0, DLPD_COS_4PI_5, s1), DLPD_COS_2PI_5, s2);
  // q1 = i*DIR*(s1*d1 + s2*d2), q2 = i*DIR*(s2*d1 - s1*d2) with s1=sin(2pi/5), s2=sin(4pi/5)
  cplx u1 = c_axpy(c_scale(d1, DLPD_SIN_2PI_5), DLPD_SIN_4PI_5, d2);
  cplx u2 = c_axpy(c_scale(d1, DLPD_SIN_4PI_5), -DLPD_SIN_2PI_5, d2);
  a0 = x0;
  a1 = c_add_rot<DIR>(p1, u1);
  a4 = c_sub_rot<DIR>(p1, u1);
  a2 = c_add_rot<DIR>(p2, u2);
  a3 = c_sub_rot<DIR>(p2, u2);
}

template <int R, int DIR> struct SmallDft;
template <int DIR> struct SmallDft<2, DIR> {
  DLPD_HD static void run(cplx* v) { dft2<DIR>(v[0], v[1]); }
};
template <int DIR> struct SmallDft<4, DIR> {
  DLPD_HD static void run(cplx* v) { dft4<DIR>(v[0], v[1], v[2], v[3]); }
};
template <int DIR> struct SmallDft<5, DIR> {
  DLPD_HD static void run(cplx* v) { dft5<DIR>(v[0], v[1], v[2], v[3], v[4]); }
};
template <int DIR> struct SmallDft<8, DIR> {
  DLPD_HD static void run(cplx* v) {
    // even / odd split
    cplx e0 = v[0], e1 = v[2], e2 = v[4], e3 = v[6];
    cplx o0 = v[1], o1 = v[3], o2 = v[5], o3 = v[7];
    dft4<DIR>(e0, e1, e2, e3);
    dft4<DIR>(o0, o1, o2, o3);
    o1 = c_rotcs<DIR>(o1, DLPD_SQRT1_2, DLPD_SQRT1_2);
    o3 = c_rotcs<DIR>(o3, -DLPD_SQRT1_2, DLPD_SQRT1_2);
    v[0] = c_add(e0, o0); v[4] = c_sub(e0, o0);
    v[1] = c_add(e1, o1); v[5] = c_sub(e1, o1);
    v[2] = c_add_rot<DIR>(e2, o2); v[6] = c_sub_rot<DIR>(e2, o2);
    v[3] = c_add(e3, o3); v[7] = c_sub(e3, o3);
  }
};
template <int DIR> struct SmallDft<16, DIR> {
  DLPD_HD static void run(cplx* v) {
    // n = 4*n1 + n2 ; k = k1 + 4*k2.  Step 1: DFT4 over n1 for each n2.
    cplx y[4][4];
#pragma unroll
    for (int n2 = 0; n2 < 4; n2++) {
      y[n2][0] = v[n2]; y[n2][1] = v[n2 + 4]; y[n2][2] = v[n2 + 8]; y[n2][3] = v[n2 + 12];
      dft4<DIR>(y[n2][0], y[n2][1], y[n2][2], y[n2][3]);
    }
    // twiddle W16^(n2*k1)
    const float c1 = DLPD_COS_PI_8, s1 = DLPD_SIN_PI_8, h = DLPD_SQRT1_2;
    y[1][1] = c_rotcs<DIR>(y[1][1], c1, s1);
    y[1][2] = c_rotcs<DIR>(y[1][2], h, h);
    y[1][3] = c_rotcs<DIR>(y[1][3], s1, c1);
    y[2][1] = c_rotcs<DIR>(y[2][1], h, h);
    y[2][2] = c_rot90<DIR>(y[2][2]);
    y[2][3] = c_rotcs<DIR>(y[2][3], -h, h);
    y[3][1] = c_rotcs<DIR>(y[3][1], s1, c1);
    y[3][2] = c_rotcs<DIR>(y[3][2], -h, h);
    y[3][3] = c_rotcs<DIR>(y[3][3], -c1, -s1);
    // Step 2: DFT4 over n2 for each k1 -> X[k1 + 4*k2]
#pragma unroll
    for (int k1 = 0; k1 < 4; k1++) {
      dft4<DIR>(y[0][k1], y[1][k1], y[2][k1], y[3][k1]);
      v[k1] = y[0][k1]; v[k1 + 4] = y[1][k1]; v[k1 + 8] = y[2][k1]; v[k1 + 12] = y[3][k1];
    }
  }
};
template <int DIR> struct SmallDft<10, DIR> {
  DLPD_HD static void run(cplx* v) {
    // n = 2*n1 + n2 (n1<5, n2<2) ; k = k1 + 5*k2
    cplx e[5] = {v[0], v[2], v[4], v[6], v[8]};
    cplx o[5] = {v[1], v[3], v[5], v[7], v[9]};
    dft5<DIR>(e[0], e[1], e[2], e[3], e[4]);
    dft5<DIR>(o[0], o[1], o[2], o[3], o[4]);
    // W10^k1 on odd branch: angle k1*pi/5
    o[1] = c_rotcs<DIR>(o[1], DLPD_COS_PI_5, DLPD_SIN_PI_5);
    o[2] = c_rotcs<DIR>(o[2], DLPD_COS_2PI_5, DLPD_SIN_2PI_5);
    o[3] = c_rotcs<DIR>(o[3], -DLPD_COS_2PI_5, DLPD_SIN_2PI_5);
    o[4] = c_rotcs<DIR>(o[4], -DLPD_COS_PI_5, DLPD_SIN_PI_5);
#pragma unroll
    for (int k1 = 0; k1 < 5; k1++) {
      v[k1] = c_add(e[k1], o[k1]);
      v[k1 + 5] = c_sub(e[k1], o[k1]);
    }
  }
};

template <int DIR> struct SmallDft<20, DIR> {
  DLPD_HD static void run(cplx* v) {
    // prime-factor (Good-Thomas) 4 x 5: n = (5 n1 + 4 n2) mod 20, k = (5 k1 + 16 k2) mod 20 -- then
    // n k = 5 n1 k1 + 4 n2 k2 (mod 20): a 5-point transform over n2 and a 4-point one over n1, NO twiddles between
    cplx y[4][5];
#pragma unroll
    for (int n1 = 0; n1 < 4; n1++) {
#pragma unroll
      for (int n2 = 0; n2 < 5; n2++) y[n1][n2] = v[(5 * n1 + 4 * n2) % 20];
      dft5<DIR>(y[n1][0], y[n1][1], y[n1][2], y[n1][3], y[n1][4]);
    }
#pragma unroll
    for (int k2 = 0; k2 < 5; k2++) {
      dft4<DIR>(y[0][k2], y[1][k2], y[2][k2], y[3][k2]);
#pragma unroll
      for (int k1 = 0; k1 < 4; k1++) v[(5 * k1 + 16 * k2) % 20] = y[k1][k2];
    }
  }
};

// ---- one Stockham pass over one pencil, register-resident between load() and store() ----
//  N   transform length            R   radix of this pass
//  NS  product of earlier radices  DIR -1 forward / +1 inverse (unnormalised)
//  T   threads cooperating on the pencil
//  NNZ only inputs [0,NNZ) are non-zero (pruned loads); NNZ % (N/R) == 0
template <int N, int R, int NS, int DIR, int T, int NNZ = N> struct FftPass {
  static constexpr int NBF = N / R;
  static constexpr int PER = (NBF + T - 1) / T;
  static constexpr int RNZ = NNZ / NBF;   // radix inputs r < RNZ are non-zero
  static_assert(N % R == 0, "radix must divide N");
  static_assert(NNZ % NBF == 0, "NNZ must be a multiple of N/R");
  cplx v[PER][R];

  // P: pencil base, es: element stride (in cplx), t: thread index within the pencil [0,T),
  // tw: table of exp(-2*pi*i*k/N), k in [0,N)
  DLPD_HD void load(const cplx* P, int es, int t, const cplx* tw) {
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int j = t + i * T;
      if ((NBF % T == 0) || j < NBF) {
#pragma unroll
        for (int r = 0; r < R; r++) v[i][r] = (r < RNZ) ? P[(j + r * NBF) * es] : c_make(0.f, 0.f);
        if (NS > 1) {
          const int k = (j % NS) * (N / (NS * R));
#pragma unroll
          for (int r = 1; r < R; r++) {
            if (r < RNZ) {
              cplx w = tw[k * r];
              v[i][r] = DIR < 0 ? c_mul(v[i][r], w) : c_mulc(v[i][r], w);
            }
          }
        }
        SmallDft<R, DIR>::run(v[i]);
      }
    }
  }
  DLPD_HD int out_index(int i, int r, int t) const {
    const int j = t + i * T;
    return (j / NS) * NS * R + (j % NS) + r * NS;
  }
  DLPD_HD bool active(int i, int t) const { return (NBF % T == 0) || (t + i * T) < NBF; }
  DLPD_HD void store(cplx* P, int es, int t) const {
#pragma unroll
    for (int i = 0; i < PER; i++) {
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) P[out_index(i, r, t) * es] = v[i][r];
      }
    }
  }
};

// Pass plans: radices R1 (first, NS=1) and R2 (second, NS=R1); T threads per pencil.
template <int N> struct FftPlan;
template <> struct FftPlan<64> { static constexpr int R1 = 8, R2 = 8, T = 8; };
template <> struct FftPlan<128> { static constexpr int R1 = 16, R2 = 8, T = 8; };
template <> struct FftPlan<80> { static constexpr int R1 = 8, R2 = 10, T = 10; };
template <> struct FftPlan<160> { static constexpr int R1 = 16, R2 = 10, T = 10; };

// ------------------------------------------------------------------------------------------
// Wave-local variant: the T (= 8) threads of a pencil are lanes of ONE wave and a wave owns 8
// pencils, so the load -> store hand-over of a pass needs only wave-level ordering
// (DLPD_WAVE_SYNC: LDS instructions of a wave execute in issue order) and the waves of a block
// drift apart, overlapping one wave's LDS traffic with another's butterflies.  Addressing goes
// through a functor (swizzled slabs).
// ------------------------------------------------------------------------------------------
// slab addressing: element (row, col) of an N x N complex slab with row stride RS (RS % 32 == 8)
// lives at row*RS + swz(col), swz(c) = c ^ ((c >> 4) & 15): both the contiguous (row pencil) and
// the strided (column pencil) Stockham accesses of 8 pencils x 8 threads are LDS-bank-conflict free.
DLPD_HD int slab_swz(int c) { return c ^ ((c >> 4) & 15); }
// Elements (col, col + 1), col even, of one slab row as ONE 16-byte LDS access: the swizzle XORs both with the
// same value, so they stay an aligned pair, exchanged when that value is odd.  (Two 8-byte accesses at a 16-byte
// lane stride are 2-way bank conflicts; the row base must be 16-byte aligned: RS even.)
DLPD_D float4 slab_load_pair(const cplx* row, int col) {
  const int s = slab_swz(col);
  const float4 v = *reinterpret_cast<const float4*>(row + (s & ~1));
  return (s & 1) ? make_float4(v.z, v.w, v.x, v.y) : v;
}
DLPD_D void slab_store_pair(cplx* row, int col, float4 v) {
  const int s = slab_swz(col);
  *reinterpret_cast<float4*>(row + (s & ~1)) = (s & 1) ? make_float4(v.z, v.w, v.x, v.y) : v;
}
// One 8-byte LDS access per element.  Plain loads / stores of neighbouring offsets get merged by the compiler into
// ds_read2_b64 / ds_write2_b64, which cost 8 / 13 LDS cycles against 2 x 2 / 2 x 6 for the separate instructions
// (MI355X_MICROARCH.md, LDS table); volatile accesses are left alone (the emulator build has no such pass).
#ifndef DLPD_LDS_NOMERGE
#define DLPD_LDS_NOMERGE 1
#endif
#if DLPD_LDS_NOMERGE && defined(DLPD_HAS_LDS_ADDRESS_SPACE)
typedef float dlpd_v2f __attribute__((ext_vector_type(2)));
DLPD_D cplx lds_ld(const cplx* p) {
  const dlpd_v2f v = *(const volatile __attribute__((address_space(3))) dlpd_v2f*)(p);
  return c_make(v.x, v.y);
}
DLPD_D void lds_st(cplx* p, cplx v) {
  dlpd_v2f w;
  w.x = v.x;
  w.y = v.y;
  *(volatile __attribute__((address_space(3))) dlpd_v2f*)(p) = w;
}
#else
DLPD_D cplx lds_ld(const cplx* p) { return *p; }
DLPD_D void lds_st(cplx* p, cplx v) { *p = v; }
#endif
// ADJ: thread t takes the butterflies PER*t .. PER*t+PER-1 instead of t, t+T, ..: with PER = 2 in a last pass
// (outputs j + r*NBF) it ends up holding ADJACENT element pairs -- 16 bytes per lane, 8 lanes a full 128-byte line.
template <int N, int R, int NS, int DIR, int T, int NNZ = N, int ADJ = 0> struct FftPassW {
  static constexpr int NBF = N / R;
  static constexpr int PER = (NBF + T - 1) / T;
  static constexpr int RNZ = NNZ / NBF;
  static_assert(N % R == 0 && NNZ % NBF == 0, "unsupported wave-local pass shape");
  static constexpr bool FULL = (NBF % T == 0);     // otherwise the last round is partly idle
  cplx v[PER][R];

  DLPD_HD static int bf(int i, int t) { return ADJ ? t * PER + i : t + i * T; }
  DLPD_HD bool active(int i, int t) const { return FULL || bf(i, t) < NBF; }
  DLPD_D void twiddle_and_run(int i, int j, const cplx* tw) {
    if (NS > 1) {
      const int k = (j % NS) * (N / (NS * R));
#pragma unroll
      for (int r = 1; r < R; r++)
        if (r < RNZ) {
          const cplx w = tw[k * r];
          v[i][r] = DIR < 0 ? c_mul(v[i][r], w) : c_mulc(v[i][r], w);
        }
    }
    SmallDft<R, DIR>::run(v[i]);
  }
  // ADJ, PER == 2: the two butterflies' inputs (2t + r*NBF, 2t + 1 + r*NBF) as one 16-byte access of a slab row
  DLPD_D void load_pairs(const cplx* row, int t, const cplx* tw) {
    static_assert(!ADJ || (PER == 2 && FULL && NNZ == N), "pair loads: two whole butterflies per thread");
#pragma unroll
    for (int r = 0; r < R; r++) {
      const float4 p = slab_load_pair(row, 2 * t + r * NBF);
      v[0][r] = c_make(p.x, p.y);
      v[1][r] = c_make(p.z, p.w);
    }
    twiddle_and_run(0, 2 * t, tw);
    twiddle_and_run(1, 2 * t + 1, tw);
  }
  // tw: LDS table of exp(-2 pi i k / N)
  template <class Addr> DLPD_D void load(const cplx* S, const Addr& ad, int t, const cplx* tw) {
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int j = bf(i, t);
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) v[i][r] = (r < RNZ) ? lds_ld(S + ad(j + r * NBF)) : c_make(0.f, 0.f);
        if (NS > 1) {
          const int k = (j % NS) * (N / (NS * R));
#pragma unroll
          for (int r = 1; r < R; r++)
            if (r < RNZ) {
              const cplx w = tw[k * r];
              v[i][r] = DIR < 0 ? c_mul(v[i][r], w) : c_mulc(v[i][r], w);
            }
        }
        SmallDft<R, DIR>::run(v[i]);
      }
    }
  }
  // the same with this thread's twiddles handed in (twr[i][r - 1] = tw[k_i r]: they do not change between calls, so a caller
  // that loops can keep them in registers -- fetch_twiddles -- instead of re-reading the LDS table every time)
  DLPD_D void fetch_twiddles(int t, const cplx* tw, cplx (&twr)[PER][R - 1]) const {
    static_assert(NS > 1 && NNZ == N, "second or later pass of an unpruned plan");
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int k = (bf(i, t) % NS) * (N / (NS * R));
#pragma unroll
      for (int r = 1; r < R; r++) twr[i][r - 1] = active(i, t) ? tw[k * r] : c_make(1.f, 0.f);
    }
  }
  // ... in two halves, so that a caller can put other work behind the LDS reads while they are in flight
  template <class Addr> DLPD_D void load_only(const cplx* S, const Addr& ad, int t) {
#pragma unroll
    for (int i = 0; i < PER; i++)
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) v[i][r] = lds_ld(S + ad(bf(i, t) + r * NBF));
      }
  }
  DLPD_D void run_twr(int t, const cplx (&twr)[PER][R - 1]) {
#pragma unroll
    for (int i = 0; i < PER; i++)
      if (active(i, t)) {
#pragma unroll
        for (int r = 1; r < R; r++) v[i][r] = DIR < 0 ? c_mul(v[i][r], twr[i][r - 1]) : c_mulc(v[i][r], twr[i][r - 1]);
        SmallDft<R, DIR>::run(v[i]);
      }
  }
  template <class Addr> DLPD_D void load_twr(const cplx* S, const Addr& ad, int t, const cplx (&twr)[PER][R - 1]) {
#pragma unroll
    for (int i = 0; i < PER; i++) {
      const int j = bf(i, t);
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) v[i][r] = lds_ld(S + ad(j + r * NBF));
#pragma unroll
        for (int r = 1; r < R; r++) v[i][r] = DIR < 0 ? c_mul(v[i][r], twr[i][r - 1]) : c_mulc(v[i][r], twr[i][r - 1]);
        SmallDft<R, DIR>::run(v[i]);
      }
    }
  }
  DLPD_HD int out_index(int i, int r, int t) const {
    const int j = bf(i, t);
    return (j / NS) * NS * R + (j % NS) + r * NS;
  }
  template <class Addr> DLPD_D void store(cplx* S, const Addr& ad, int t) const {
#pragma unroll
    for (int i = 0; i < PER; i++)
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) lds_st(S + ad(out_index(i, r, t)), v[i][r]);
      }
  }
  // INTERMEDIATE layout of a two-pass plan (R1 x R2): the first pass (NS == 1) leaves the R outputs of butterfly j as
  // block j, the second pass (NS == R1) reads offset j of the blocks r = 0..R-1.  With the blocks R1 + 1 elements apart
  // instead of R1 (natural order) the 8 threads' stores of one r land on different banks: the first-pass stores of the
  // 10 x 8 plan cost 104 (rows) / 80 (columns) LDS-array cycles per pencil set in natural order, those of the column
  // 16 x 8 plan 128; 40 / 40 / 64 this way (model of the ds_write_b64 lane groups).  8 (R1 + 1) = N + 8 elements / rows.
  template <class Mid> DLPD_D void store_blk(cplx* S, const Mid& md, int t) const {
    static_assert(NS == 1, "first pass of a two-pass plan");
#pragma unroll
    for (int i = 0; i < PER; i++)
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) lds_st(S + md(bf(i, t), r), v[i][r]);
      }
  }
  template <class Mid> DLPD_D void load_blk(const cplx* S, const Mid& md, int t, const cplx* tw) {
    static_assert(NS == NBF && NNZ == N, "second pass of a two-pass plan");
#pragma unroll
    for (int i = 0; i < PER; i++)
      if (active(i, t)) {
#pragma unroll
        for (int r = 0; r < R; r++) v[i][r] = lds_ld(S + md(r, bf(i, t)));
        twiddle_and_run(i, bf(i, t), tw);
      }
  }
};
// intermediate positions: block `blk`, offset `off`, blocks B = R1 + 1 apart, along a slab row / down a slab column
template <int B> struct RowMid {
  int base;   // row * RS
  DLPD_HD int operator()(int blk, int off) const { return base + blk * B + off; }
};
template <int RS, int B> struct ColMid {
  int base;   // swz(col)
  DLPD_HD int operator()(int blk, int off) const { return (blk * B + off) * RS + base; }
};

// wave-local two-pass plans R1 (pruned) x R2: 8 threads per pencil.  (N = 160, used by K3 only: 20 x 8 with its own
// pencil layout, fft_wave_pencils below; the three-pass 8 x 4 x 5 plan of round 1 cost one LDS exchange more.)
template <int N> struct FftPlanW;
template <> struct FftPlanW<64> { static constexpr int R1 = 8, R2 = 8; };
template <> struct FftPlanW<128> { static constexpr int R1 = 16, R2 = 8; };
template <> struct FftPlanW<80> { static constexpr int R1 = 10, R2 = 8; };

template <int RS> struct RowAddr {
  static constexpr bool IS_ROW = true;
  int base;   // row * RS
  DLPD_HD int operator()(int e) const { return base + slab_swz(e); }
};
template <int RS> struct ColAddr {
  static constexpr bool IS_ROW = false;
  int base;   // swz(col)
  DLPD_HD int operator()(int e) const { return e * RS + base; }
};

// all passes of a wave-local transform of one pencil set, in place (ends without a trailing sync)
template <int N, int DIR, int NNZ, class Addr, class P = FftPlanW<N>>
DLPD_D void fft_wave(cplx* S, const Addr& ad, int t, const cplx* tw) {
  if constexpr (N == 80 && Addr::IS_ROW) {
    // the 10 x 8 plan along a row: blocked intermediate (see store_blk; at N = 128 / 64 the natural order is
    // conflict-free already and measured 1 % faster)
    const RowMid<P::R1 + 1> md = {ad.base};
    {
      FftPassW<N, P::R1, 1, DIR, 8, NNZ> ps;
      ps.load(S, ad, t, tw);
      DLPD_WAVE_SYNC();
      ps.store_blk(S, md, t);
      DLPD_WAVE_SYNC();
    }
    FftPassW<N, P::R2, P::R1, DIR, 8> ps;
    ps.load_blk(S, md, t, tw);
    DLPD_WAVE_SYNC();
    ps.store(S, ad, t);
    return;
  }
  {
    FftPassW<N, P::R1, 1, DIR, 8, NNZ> ps;
    ps.load(S, ad, t, tw);
    DLPD_WAVE_SYNC();
    ps.store(S, ad, t);
    DLPD_WAVE_SYNC();
  }
  {
    FftPassW<N, P::R2, P::R1, DIR, 8> ps;
    ps.load(S, ad, t, tw);
    DLPD_WAVE_SYNC();
    ps.store(S, ad, t);
  }
}

// ------------------------------------------------------------------------------------------
// Pencil layouts of the wave-local z transforms (K3).  N != 160: element e of a pencil lives at slab_swz(e) before,
// between and after the passes.  N = 160 runs TWO passes (20 x 8, one LDS exchange; the three-pass 8 x 4 x 5 plan
// of rounds 1-2 needed two) and keeps its pencils in "blocks of 21": the input is stored in natural order, the
// first pass writes its 20 outputs of butterfly t at 21 t + r and the second pass reads / writes j + 21 r -- the
// stride 21 (42 dwords) puts the 8 threads' 8-byte stores of one r on 8 distinct bank pairs, which stride 20 does not
// (model of the ds_write_b64 lane groups: 208 -> 80 LDS-array cycles per pencil set).  8 x 21 = 168 = the row stride.
// ------------------------------------------------------------------------------------------
template <int N> DLPD_HD int pencil_in_pos(int k) { return N == 160 ? k : slab_swz(k); }
template <int N> DLPD_HD int pencil_out_pos(int z) { return N == 160 ? z + z / 20 : slab_swz(z); }

// all passes of the wave-local length-N transform of 8 pencils (rows rowbase + 8 more, lane = 8 * pencil + thread),
// input at pencil_in_pos, output at pencil_out_pos
template <int N, int DIR> DLPD_D void fft_wave_pencils(cplx* S, int rowbase, int RS, int q, int t, const cplx* tw) {
  if constexpr (N == 160) {
    cplx* P = S + (rowbase + q) * RS;
    {
      FftPassW<N, 20, 1, DIR, 8> ps;                   // 8 butterflies of radix 20: one per thread
#pragma unroll
      for (int r = 0; r < 20; r++) ps.v[0][r] = lds_ld(P + t + 8 * r);
      ps.twiddle_and_run(0, t, tw);
      DLPD_WAVE_SYNC();
#pragma unroll
      for (int r = 0; r < 20; r++) lds_st(P + 21 * t + r, ps.v[0][r]);
      DLPD_WAVE_SYNC();
    }
    {
      FftPassW<N, 8, 20, DIR, 8> ps;                   // 20 butterflies of radix 8: three rounds, the last half full
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (t + 8 * i < 20) {
#pragma unroll
          for (int r = 0; r < 8; r++) ps.v[i][r] = lds_ld(P + t + 8 * i + 21 * r);
          ps.twiddle_and_run(i, t + 8 * i, tw);
        }
      DLPD_WAVE_SYNC();
#pragma unroll
      for (int i = 0; i < 3; i++)
        if (t + 8 * i < 20) {
#pragma unroll
          for (int r = 0; r < 8; r++) lds_st(P + t + 8 * i + 21 * r, ps.v[i][r]);
        }
    }
  } else {
    const RowAddr<0> ad = {(rowbase + q) * RS};
    fft_wave<N, DIR, N>(S, ad, t, tw);
  }
}

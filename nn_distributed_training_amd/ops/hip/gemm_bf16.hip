// Mixed-precision stacked linear kernels (CDNA4 gfx950): fp32 storage,
// bf16 MFMA operands, fp32 accumulation.
//
// Same [L, n] fp32 parameter stack, fp32 activation buffers and
// arguments as the float instantiations of gmfma::mfma_fwd_k /
// mfma_dx_k / mfma_dw_k; only the operands of the contraction are
// rounded (RNE) to bf16 on their way to v_mfma_f32_16x16x32_bf16,
// which contracts 8 k-values per lane per instruction where the
// 16x16x4 f32 shape contracts one. Bias, activation, masks, db and
// every result stay fp32. The fwd and dx kernels end in the SAME
// epilogues as the float kernels (EPI_FWD_EPILOGUE, EPI_DX_EPILOGUE
// in linear_epilogue.h, with the f32 lane map).
//
// Geometry (all three kernels): 256-thread blocks = 4 waves in a 2x2
// grid over a 64x64 output tile, each wave a 32x32 sub-tile as 2x2
// 16x16 fragments; K advances KS = 64 bf16 per LDS stage (2 MFMA
// k-steps), so the 64-wide density layers contract in ONE stage and
// the 256->64 layer in four, pipelined like mfma_fwd_k: one register
// set holds the fp32 values of stage s+1 while the MFMAs run on the
// LDS image of stage s (write-after-barrier).
//
// Fragment map of 16x16x32_bf16 (the numerics tests in
// tests/test_gemm_bf16_gpu.py are its confirmation on hardware):
//   A operand: lane l holds A[l&15][8*(l>>4) .. +7]   (8 bf16, 16 B)
//   B operand: lane l holds B[8*(l>>4) .. +7][l&15]
//   C/D:       the f32 16x16 map, row (l>>4)*4 + r, col l&15
//              (epi::acc_map<float>)
// Both operands want 8 CONSECUTIVE k per lane, so both LDS images are
// k-contiguous: As[row][k], Bs[col][k], and a fragment is one 16-byte
// LDS read.
//
// LDS row stride LDK = 72 bf16 = 144 B = 36 dwords. A fragment read
// has lanes 0-15 on 16 consecutive rows at one k offset: 36*r mod 64 =
// {0,36,8,44,16,52,24,60,32,4,40,12,48,20,56,28}, 16 distinct
// multiples of 4, so the 16 four-dword reads cover all 64 banks once
// (on a 32-bank reading 8 rows cover 32 banks once). An unpadded
// 128-byte stride would put all 16 rows on the same four banks.
// 2 x 64 x 72 x 2 B = 18 KB of LDS per block.
//
// Conversion happens once, at staging: fp32 global loads into
// registers, v_cvt_pk_bf16_f32 (from plain C++ vector conversion) as
// the registers are written to LDS, 16 bytes per LDS write. Two
// staging patterns, by where k lies in memory:
//   rows (k contiguous in memory: X and W in fwd, dZ in dx): a thread
//     loads 8 consecutive k of one row as two 16-byte loads when the
//     row starts are 16-byte aligned (leading dimension % 4 == 0 and
//     an aligned slice base - w_off, l*n and I are not guaranteed to
//     give that, e.g. the odd n of the FourierNet stack), else as 8
//     scalar loads; either way guard-free on full tiles;
//   cols (k strided: W in dx, dZ and X in dw): a thread owns one
//     column and loads 8 consecutive k-rows with scalar loads (a wave
//     reads 256 contiguous bytes per k-row, no alignment needed) and
//     the 8 values transpose into one 16-byte LDS write for free.
// Ragged M/I/O/K edges take a guarded scalar path that stages zeros,
// so the MFMA loop itself never tests an element (a K or M tail that
// is no multiple of 32 contracts against zeros).
//
// dW contracts over M, chunked across blocks like mfma_dw_k; chunk
// lengths are multiples of KS so only the last chunk has a tail. Each
// block writes its [64, 64] partial tile to a per-chunk SLAB and its
// db partial (column sums of the UNROUNDED fp32 dZ it staged, VALU
// adds + a 4-way LDS fold) to a db slab; gmfma::dw_reduce_parts_k
// folds both. No atomics: the result overwrites the grad slice and is
// bit-reproducible.
//
// The kernels are compiled without packed fp32 VALU ops.

#include "common.h"
#include "linear_epilogue.h"

namespace gbf16 {

typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
using epi::f32x4;

#if defined(__HIP_DEVICE_COMPILE__)
#define GBF16_KERNEL \
  __attribute__((target("no-packed-fp32-ops"))) __global__
#else
#define GBF16_KERNEL __global__
#endif

constexpr int TM = 64;    // block tile rows
constexpr int TN = 64;    // block tile cols
constexpr int KS = 64;    // bf16 k per LDS stage
constexpr int LDK = 72;   // LDS row stride in bf16 (see header)

DEV_INLINE bf16x8 pack8(f32x4 a, f32x4 b) {
  const bf16x4 lo = __builtin_convertvector(a, bf16x4);
  const bf16x4 hi = __builtin_convertvector(b, bf16x4);
  return __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
}

DEV_INLINE bool aligned16(const void* p) {
  return (reinterpret_cast<unsigned long long>(p) & 15ull) == 0;
}

// ---- rows staging: tile[row][k] = base[(row0 + row) * ld + k0 + k] ---
// thread -> row (tid>>3) + 32q, k octet (tid&7): 8 threads stream 256
// contiguous bytes of a row
DEV_INLINE void load_rows(const float* __restrict__ base, long ld,
                          int row0, int nrows, int k0, int K, bool vec,
                          int tid, f32x4 (&r)[2][2]) {
  const int sr = tid >> 3, sk = (tid & 7) * 8;
  const bool full = row0 + TM <= nrows && k0 + KS <= K;
  if (full && vec) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float* p = base + (long)(row0 + sr + 32 * q) * ld + k0 + sk;
      r[q][0] = *reinterpret_cast<const f32x4*>(p);
      r[q][1] = *reinterpret_cast<const f32x4*>(p + 4);
    }
  } else if (full) {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const float* p = base + (long)(row0 + sr + 32 * q) * ld + k0 + sk;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        r[q][0][j] = p[j];
        r[q][1][j] = p[4 + j];
      }
    }
  } else {
#pragma unroll
    for (int q = 0; q < 2; ++q) {
      const int row = row0 + sr + 32 * q;
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + sk + 4 * h + j;
          r[q][h][j] =
              (row < nrows && k < K) ? base[(long)row * ld + k] : 0.f;
        }
      }
    }
  }
}

DEV_INLINE void store_rows(__bf16* S, int tid, const f32x4 (&r)[2][2]) {
  const int sr = tid >> 3, sk = (tid & 7) * 8;
#pragma unroll
  for (int q = 0; q < 2; ++q) {
    *reinterpret_cast<bf16x8*>(&S[(sr + 32 * q) * LDK + sk]) =
        pack8(r[q][0], r[q][1]);
  }
}

// ---- cols staging: tile[col][k] = base[(k0 + k) * ld + col0 + col] ---
// thread -> col tid&63, k octets (tid>>6) and (tid>>6) + 4
DEV_INLINE void load_cols(const float* __restrict__ base, long ld,
                          int k0, int K, int col0, int ncols, int tid,
                          f32x4 (&v)[2][2]) {
  const int sc = tid & 63, sg = tid >> 6;
  if (k0 + KS <= K && col0 + TN <= ncols) {
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const float* p =
          base + (long)(k0 + 8 * (sg + 4 * h)) * ld + col0 + sc;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        v[h][0][j] = p[(long)j * ld];
        v[h][1][j] = p[(long)(4 + j) * ld];
      }
    }
  } else {
    const int col = col0 + sc;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int e = 0; e < 2; ++e) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = k0 + 8 * (sg + 4 * h) + 4 * e + j;
          v[h][e][j] =
              (k < K && col < ncols) ? base[(long)k * ld + col] : 0.f;
        }
      }
    }
  }
}

DEV_INLINE void store_cols(__bf16* S, int tid, const f32x4 (&v)[2][2]) {
  const int sc = tid & 63, sg = tid >> 6;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    *reinterpret_cast<bf16x8*>(&S[sc * LDK + 8 * (sg + 4 * h)]) =
        pack8(v[h][0], v[h][1]);
  }
}

// one LDS stage: 2 k-steps of 32, 4 MFMAs each; klim = valid k in the
// stage (a whole k-step of staged zeros is skipped, wave-uniformly)
DEV_INLINE void mma_stage(const __bf16* As, const __bf16* Bs, int wm,
                          int wn, int lane, int klim,
                          f32x4 (&acc)[2][2]) {
#pragma unroll
  for (int kk = 0; kk < KS; kk += 32) {
    if (kk < klim) {
      const int ko = kk + 8 * (lane >> 4);
      bf16x8 a[2], b[2];
#pragma unroll
      for (int f = 0; f < 2; ++f) {
        a[f] = *reinterpret_cast<const bf16x8*>(
            &As[(wm + f * 16 + (lane & 15)) * LDK + ko]);
        b[f] = *reinterpret_cast<const bf16x8*>(
            &Bs[(wn + f * 16 + (lane & 15)) * LDK + ko]);
      }
#pragma unroll
      for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
        for (int fn = 0; fn < 2; ++fn) {
          acc[fm][fn] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[fm], b[fn], acc[fm][fn], 0, 0, 0);
        }
      }
    }
  }
}

// ---------------------------------------------------------------------
// NT: Y[M,O] = act(bf(X[M,I]) @ bf(W_l[O,I])^T + b_l)  [+ optional Z]
GBF16_KERNEL __launch_bounds__(256) void bf16_fwd_k(
    const float* __restrict__ X, const float* __restrict__ theta,
    float* __restrict__ Y, float* __restrict__ Z,
    long n, long w_off, long b_off, int M, int I, int O,
    int act, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 As[TM * LDK];  // [m][k]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[TN * LDK];  // [o][k]

  const long l = blockIdx.z;
  const float* Xl = X + l * (long)M * I;
  const float* W = theta + l * n + w_off;
  const float* bias = theta + l * n + b_off;

  const int m0 = blockIdx.y * TM;
  const int o0 = blockIdx.x * TN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = (wid >> 1) * 32;
  const int wn = (wid & 1) * 32;

  const bool vec_a = (I & 3) == 0 && aligned16(Xl);
  const bool vec_b = (I & 3) == 0 && aligned16(W);
  f32x4 acc[2][2] = {};
  f32x4 ra[2][2], rb[2][2];

  const int nstages = (I + KS - 1) / KS;
  load_rows(Xl, I, m0, M, 0, I, vec_a, tid, ra);
  load_rows(W, I, o0, O, 0, I, vec_b, tid, rb);
  for (int s = 0; s < nstages; ++s) {
    __syncthreads();  // previous compute done: LDS free
    store_rows(As, tid, ra);
    store_rows(Bs, tid, rb);
    if (s + 1 < nstages) {  // next stage's fetch overlaps the MFMAs
      load_rows(Xl, I, m0, M, (s + 1) * KS, I, vec_a, tid, ra);
      load_rows(W, I, o0, O, (s + 1) * KS, I, vec_b, tid, rb);
    }
    __syncthreads();  // LDS image of stage s visible
    mma_stage(As, Bs, wm, wn, lane, I - s * KS, acc);
  }

  const bool full_mo = (m0 + TM) <= M && (o0 + TN) <= O;
  EPI_FWD_EPILOGUE(float, epi::acc_map<float>, acc, bias, Y, Z, l, M, O,
                   m0, o0, wm, wn, lane, act, scale, full_mo);
}

// ---------------------------------------------------------------------
// NN: dX[M,I] = bf(dZ[M,O]) @ bf(W_l[O,I])  (contraction over O), with
// the BELOW layer's activation backward in the epilogue from the fp32
// Yb / Zb, or from z recomputed out of the below layer's tiny input
// (Xb2, Ib <= 4): EPI_DX_EPILOGUE, shared with mfma_dx_k.
GBF16_KERNEL __launch_bounds__(256) void bf16_dx_k(
    const float* __restrict__ dZ, const float* __restrict__ theta,
    float* __restrict__ dX,
    const float* __restrict__ Yb, const float* __restrict__ Zb,
    int act_below, float scale_below,
    long n, long w_off, int M, int I, int O,
    const float* __restrict__ Xb2, long wb_off, long bb_off, int Ib) {
  __shared__ __attribute__((aligned(16))) __bf16 As[TM * LDK];  // [m][o]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[TN * LDK];  // [i][o]

  const long l = blockIdx.z;
  const float* Gl = dZ + l * (long)M * O;
  const float* W = theta + l * n + w_off;

  const int m0 = blockIdx.y * TM;
  const int i0 = blockIdx.x * TN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = (wid >> 1) * 32;
  const int wn = (wid & 1) * 32;

  const bool vec_a = (O & 3) == 0 && aligned16(Gl);
  f32x4 acc[2][2] = {};
  f32x4 ra[2][2], vb[2][2];

  const int nstages = (O + KS - 1) / KS;
  load_rows(Gl, O, m0, M, 0, O, vec_a, tid, ra);
  load_cols(W, I, 0, O, i0, I, tid, vb);
  for (int s = 0; s < nstages; ++s) {
    __syncthreads();
    store_rows(As, tid, ra);
    store_cols(Bs, tid, vb);
    if (s + 1 < nstages) {
      load_rows(Gl, O, m0, M, (s + 1) * KS, O, vec_a, tid, ra);
      load_cols(W, I, (s + 1) * KS, O, i0, I, tid, vb);
    }
    __syncthreads();
    mma_stage(As, Bs, wm, wn, lane, O - s * KS, acc);
  }

  const bool full_mi = (m0 + TM) <= M && (i0 + TN) <= I;
  const float* Wb = theta + l * n + wb_off;
  const float* bb = theta + l * n + bb_off;
  EPI_DX_EPILOGUE(float, epi::acc_map<float>, acc, dX, Yb, Zb, act_below,
                  scale_below, Wb, bb, Xb2, Ib, l, M, I, m0, i0, wm, wn,
                  lane, full_mi);
}

// ---------------------------------------------------------------------
// TN: chunk's dW[O,I] partial = bf(dZ[mlo:mhi, O])^T @ bf(X[mlo:mhi, I])
// and db partial = column sums of the fp32 dZ chunk, stored to
//   parts  [(l*nchunk + chunk) * pstride + o*I + i]
//   dbparts[(l*nchunk + chunk) * dbstride + o]     (i-tile 0 blocks)
// The host interleaves the two ([dW | db] per chunk, pstride =
// dbstride = O*I + O) where the layer's bias follows its weights in
// the stack, so ONE dw_reduce_parts_k launch folds both (a second
// launch for the 64 db columns measured 21 us of serial chunk chain,
// as much as the dW kernel itself).
// Grid (I tiles, O tiles, L * nchunk); mc = rows per chunk, a multiple
// of KS with (nchunk - 1) * mc < M, so every chunk has rows and every
// slab element is written.
GBF16_KERNEL __launch_bounds__(256) void bf16_dw_k(
    const float* __restrict__ dZ, const float* __restrict__ X,
    float* __restrict__ parts, float* __restrict__ dbparts,
    long pstride, long dbstride, int M, int I, int O, int mc,
    int nchunk) {
  __shared__ __attribute__((aligned(16))) __bf16 As[TM * LDK];  // [o][m]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[TN * LDK];  // [i][m]
  __shared__ float dbs[4][TM];

  const int chunk = blockIdx.z % nchunk;
  const long l = blockIdx.z / nchunk;
  const float* Gl = dZ + l * (long)M * O;
  const float* Xl = X + l * (long)M * I;
  const int mlo = chunk * mc;
  const int mhi = min(M, mlo + mc);

  const int o0 = blockIdx.y * TM;
  const int i0 = blockIdx.x * TN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;
  const int wm = (wid >> 1) * 32;   // o-direction
  const int wn = (wid & 1) * 32;    // i-direction

  f32x4 acc[2][2] = {};
  f32x4 va[2][2], vb[2][2];
  float db_acc = 0.f;  // column o0 + (tid&63), this thread's k octets

  load_cols(Gl, O, mlo, mhi, o0, O, tid, va);
  load_cols(Xl, I, mlo, mhi, i0, I, tid, vb);
  for (int k0 = mlo; k0 < mhi; k0 += KS) {
    __syncthreads();
    store_cols(As, tid, va);
    store_cols(Bs, tid, vb);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) db_acc += va[h][0][j] + va[h][1][j];
    }
    if (k0 + KS < mhi) {
      load_cols(Gl, O, k0 + KS, mhi, o0, O, tid, va);
      load_cols(Xl, I, k0 + KS, mhi, i0, I, tid, vb);
    }
    __syncthreads();
    mma_stage(As, Bs, wm, wn, lane, mhi - k0, acc);
  }

  if (blockIdx.x == 0) {
    dbs[wid][tid & 63] = db_acc;
    __syncthreads();
    if (tid < TM && o0 + tid < O) {
      dbparts[(long)blockIdx.z * dbstride + o0 + tid] =
          (dbs[0][tid] + dbs[1][tid]) + (dbs[2][tid] + dbs[3][tid]);
    }
  }

  float* slab = parts + (long)blockIdx.z * pstride;
  const bool full_oi = (o0 + TM) <= O && (i0 + TN) <= I;
#pragma unroll
  for (int fm = 0; fm < 2; ++fm) {
#pragma unroll
    for (int fn = 0; fn < 2; ++fn) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int o =
            o0 + wm + fm * 16 + epi::acc_map<float>::acc_row(lane, r);
        const int i = i0 + wn + fn * 16 + (lane & 15);
        if (full_oi || (o < O && i < I)) {
          slab[(long)o * I + i] = acc[fm][fn][r];
        }
      }
    }
  }
}

}  // namespace gbf16

// bf16 ACTIVATION STORAGE for the bf16-operand stacked linear kernels
// (CDNA4 gfx950).
//
// gemm_bf16.hip keeps every activation fp32 in memory and rounds it RNE
// to bf16 each time it is staged for v_mfma_f32_16x16x32_bf16. A hidden
// activation whose every consumer rounds it that way (the next layer's
// forward and dW operands, and the relu sign mask of its dX) can be
// stored as those bf16 bits by its producer instead: the operands are
// the same bits, the mask is the same (RNE keeps sign and zero-ness of
// every normal fp32), and the buffer is half as many bytes each time it
// is written or read. The kernels here are the ones that write or read
// such a buffer; dZ, dX, the parameter and gradient stacks, bias,
// activation and db stay fp32 exactly as in gemm_bf16.hip.
//
//   act_fwd_k<XB, YB>  Y = act(X W^T + b), X and Y each fp32 or bf16
//   encode_bf16_k<IK>  gemm::encode_fwd_k<float, IK> with a bf16 Y
//   act_dx_k           dX = (dZ W) * act_below', relu mask from a bf16 Yb
//   act_dw_k           dW = dZ^T X, db, with a bf16 X
//
// Transposed product (act_fwd_k, act_dx_k), as in mlp_fused.hip: the A
// operand is the WEIGHT image and the B operand the activation, so with
// the fragment maps of gemm_bf16.hip
//   A: lane l holds W[o = l&15][8*(l>>4) .. +7]
//   B: lane l holds X[m = l&15][8*(l>>4) .. +7]
//   D: lane l holds D[o = 4*(l>>4) + r][m = l&15], r = 0..3
// a lane ends with 4 CONSECUTIVE outputs of ONE row: one 8-byte packed
// bf16 store (or one 16-byte fp32 store) per fragment, where the plain
// product would scatter four 2-byte stores over four rows. It also makes
// the B fragment 8 consecutive k of one row of X (or dZ): 16 contiguous
// bytes of bf16 (32 of fp32) in GLOBAL memory, loaded straight into the
// fragment register. Only the weights go through LDS; the activation
// needs no LDS image, no staging pass and no barrier in the K loop.
//
// Work split (act_fwd_k, act_dx_k): a 256-thread block owns 64 rows x 64
// outputs; wave w owns rows 16w .. 16w+15 and all four 16-wide output
// fragments, so each activation byte is fetched once per output tile and
// a k-step is 1 global fragment + 4 LDS fragments + 4 MFMAs.
//
// act_dw_k keeps the geometry of gbf16::bf16_dw_k (both operands are
// contracted down their columns and go through LDS, 2x2 waves of 2x2
// fragments, per-chunk [dW | db] slabs for gmfma::dw_reduce_parts_k);
// what changes is how the bf16 X reaches its [i][m] image, see there.
//
// Alignment: a bf16 buffer is a torch allocation of [L*M, W] with
// W % 8 == 0, so every row starts on a 16-byte boundary; the host checks
// it. fp32 rows take 16-byte loads where K % 8 == 0 and the base is
// aligned, else guarded scalar loads.
//
// The kernels are compiled without packed fp32 VALU ops.

#include "common.h"

namespace gbf16a {

using gbf16::bf16x4;
using gbf16::bf16x8;
using gbf16::f32x4;
using gbf16::KS;
using gbf16::LDK;
using gbf16::TM;
using gbf16::TN;

typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));

constexpr int KC = 256;       // K per weight image of act_fwd_k
constexpr int LDW = KC + 8;   // its largest row stride (bf16)

DEV_INLINE int r32(int v) { return (v + 31) & ~31; }

// 8 consecutive k of one fp32 row as a bf16 fragment; zeros from K on.
// vec: K % 8 == 0 and 16-byte aligned rows, so an octet is whole or
// absent; the address is clamped and the value selected, which keeps the
// loads unconditional.
DEV_INLINE bf16x8 frag_f32(const float* __restrict__ row, int k, int K,
                           bool vec) {
  f32x4 a, b;
  if (vec) {
    const float* p = row + min(k, K - 8);
    a = *reinterpret_cast<const f32x4*>(p);
    b = *reinterpret_cast<const f32x4*>(p + 4);
    if (k >= K) {
      a = f32x4{0.f, 0.f, 0.f, 0.f};
      b = a;
    }
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      a[j] = k + j < K ? row[k + j] : 0.f;
      b[j] = k + 4 + j < K ? row[k + 4 + j] : 0.f;
    }
  }
  return gbf16::pack8(a, b);
}

// the same octet of a bf16 row (K % 8 == 0, 16-byte aligned rows)
DEV_INLINE bf16x8 frag_bf16(const __bf16* __restrict__ row, int k, int K) {
  bf16x8 v = *reinterpret_cast<const bf16x8*>(row + min(k, K - 8));
  if (k >= K) v = __builtin_bit_cast(bf16x8, u32x4{0u, 0u, 0u, 0u});
  return v;
}

// ---------------------------------------------------------------------
// Y[M,O] = act(bf(X[M,I]) @ bf(W_l[O,I])^T + b_l), D[o][m] = W X^T.
// Grid (O tiles, M tiles, L). K runs in chunks of <= KC: the chunk's X
// fragments (<= 8 per lane) are all requested first, then the chunk's
// weights are staged ([o][k] rows of stride r32(kl) + 8 bf16 = 4 * odd
// dwords: the 16 rows of a fragment read cover all 64 banks once; K and
// O tails are zeros), one barrier, then the MFMAs run from registers
// and LDS alone. Rows past M load row M - 1 and are not stored.
template <bool XB, bool YB>
GBF16_KERNEL __launch_bounds__(256) void act_fwd_k(
    const void* __restrict__ Xv, const float* __restrict__ theta,
    void* __restrict__ Yv, long n, long w_off, long b_off, int M, int I,
    int O, int act, float scale) {
  __shared__ __attribute__((aligned(16))) __bf16 Ws[TN * LDW];  // [o][k]

  const long l = blockIdx.z;
  const float* W = theta + l * n + w_off;
  const float* bias = theta + l * n + b_off;
  const int m0 = blockIdx.y * TM;
  const int o0 = blockIdx.x * TN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  const int mrow = m0 + wid * 16 + (lane & 15);
  const long grow = l * (long)M + min(mrow, M - 1);
  const __bf16* xrow_b = reinterpret_cast<const __bf16*>(Xv) + grow * I;
  const float* xrow_f = reinterpret_cast<const float*>(Xv) + grow * I;
  const bool vec_x = (I & 7) == 0 && gbf16::aligned16(Xv);

  f32x4 acc[4] = {};  // [fo]: 4 consecutive o of row mrow
  for (int kb = 0; kb < I; kb += KC) {
    const int kl = min(KC, I - kb);
    const int kp = r32(kl), sw = kp + 8, noct = kp >> 3;

    bf16x8 xf[KC / 32];
#pragma unroll
    for (int s = 0; s < KC / 32; ++s) {
      if (s * 32 < kl) {
        const int k = kb + s * 32 + 8 * (lane >> 4);
        xf[s] = XB ? frag_bf16(xrow_b, k, I) : frag_f32(xrow_f, k, I, vec_x);
      }
    }

    if (kb > 0) __syncthreads();  // the previous chunk's reads are done
    for (int t = tid; t < TN * noct; t += 256) {
      const int o = t / noct, k0 = (t - o * noct) * 8;
      const int og = o0 + o;
      f32x4 v[2];
#pragma unroll
      for (int h = 0; h < 2; ++h) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int k = kb + k0 + 4 * h + j;
          v[h][j] = (og < O && k < I) ? W[(long)og * I + k] : 0.f;
        }
      }
      *reinterpret_cast<bf16x8*>(&Ws[o * sw + k0]) =
          gbf16::pack8(v[0], v[1]);
    }
    __syncthreads();

#pragma unroll
    for (int s = 0; s < KC / 32; ++s) {
      if (s * 32 < kl) {
        const int ko = s * 32 + 8 * (lane >> 4);
        bf16x8 w[4];
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
          w[fo] = *reinterpret_cast<const bf16x8*>(
              &Ws[(fo * 16 + (lane & 15)) * sw + ko]);
        }
#pragma unroll
        for (int fo = 0; fo < 4; ++fo) {
          acc[fo] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              w[fo], xf[s], acc[fo], 0, 0, 0);
        }
      }
    }
  }

  // epilogue: bias and activation in fp32, then ONE RNE convert. A quad
  // of outputs is whole or absent where O % 4 == 0.
  const bool full = m0 + TM <= M && o0 + TN <= O;
  const bool vec_y = YB || ((O & 3) == 0 && gbf16::aligned16(Yv));
  const long yoff = (l * (long)M + mrow) * O;
#pragma unroll
  for (int fo = 0; fo < 4; ++fo) {
    const int o4 = o0 + fo * 16 + (lane >> 4) * 4;
    f32x4 v;
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const float b = (full || o4 + r < O) ? bias[o4 + r] : 0.f;
      v[r] = act_fwd(act, acc[fo][r] + b, scale);
    }
    if (full || (mrow < M && o4 + 4 <= O && vec_y)) {
      if (YB) {
        *reinterpret_cast<bf16x4*>(
            reinterpret_cast<__bf16*>(Yv) + yoff + o4) =
            __builtin_convertvector(v, bf16x4);
      } else if (vec_y) {
        *reinterpret_cast<f32x4*>(
            reinterpret_cast<float*>(Yv) + yoff + o4) = v;
      } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          reinterpret_cast<float*>(Yv)[yoff + o4 + r] = v[r];
        }
      }
    } else if (!YB && mrow < M) {
      // fp32 Y whose O is no multiple of 4, or whose base is unaligned
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        if (o4 + r < O) reinterpret_cast<float*>(Yv)[yoff + o4 + r] = v[r];
      }
    }
  }
}

// ---------------------------------------------------------------------
// gemm::encode_fwd_k<float, IK> with a bf16 Y and no Z: one thread per
// output column (blockDim == O), its W row and bias in registers for
// the whole kernel, block-uniform X row loads. Each thread stores ONE
// bf16 per row, so a wave writes 128 contiguous bytes.
template <int IK>
GBF16_KERNEL void encode_bf16_k(
    const float* __restrict__ X, const float* __restrict__ theta,
    __bf16* __restrict__ Y, long n, long w_off, long b_off, int M, int O,
    int act, float scale) {
  const long l = blockIdx.z;
  const int o = threadIdx.x;
  const float* W = theta + l * n + w_off;
  float w[IK];
#pragma unroll
  for (int i = 0; i < IK; ++i) w[i] = W[(long)o * IK + i];
  const float bo = theta[l * n + b_off + o];
  const float* Xl = X + l * (long)M * IK;
  __bf16* Yl = Y + l * (long)M * O;
  for (long m = blockIdx.x; m < M; m += gridDim.x) {
    float acc = bo;
#pragma unroll
    for (int i = 0; i < IK; ++i) acc += Xl[m * IK + i] * w[i];
    Yl[m * O + o] = (__bf16)act_fwd(act, acc, scale);
  }
}

// ---------------------------------------------------------------------
// dX[M,I] = (bf(dZ[M,O]) @ bf(W_l[O,I])) * act_below', D[i][m] = W^T dZ^T.
// A = W^T image [i][o], staged by columns like gbf16::bf16_dx_k's
// (load_cols / store_cols, 64 o per stage, next stage's registers in
// flight during the MFMAs); B fragment = 8 consecutive o of a dZ row,
// fp32 from global, converted in registers, the next stage's two
// requested before this stage's MFMAs. Below-layer activation:
//   relu      mask from the bf16 Yb, one 8-byte load per fragment,
//             requested before the stage loop;
//   sin_relu  z recomputed from the below layer's input (Ib <= 4) as
//             bb + x0*w0 + x1*w1 ..., EPI_DX_EPILOGUE's operand order;
//   none      plain copy.
// I % 8 == 0 (the width of the bf16 buffer), so a quad of i is whole or
// absent and every dX / Yb access is 16 / 8-byte aligned.
GBF16_KERNEL __launch_bounds__(256) void act_dx_k(
    const float* __restrict__ dZ, const float* __restrict__ theta,
    float* __restrict__ dX, const __bf16* __restrict__ Yb, int act_below,
    float scale_below, long n, long w_off, int M, int I, int O,
    const float* __restrict__ Xb2, long wb_off, long bb_off, int Ib) {
  __shared__ __attribute__((aligned(16))) __bf16 Ws[TN * LDK];  // [i][o]

  const long l = blockIdx.z;
  const float* W = theta + l * n + w_off;
  const int m0 = blockIdx.y * TM;
  const int i0 = blockIdx.x * TN;
  const int tid = threadIdx.x;
  const int lane = tid & 63;
  const int wid = tid >> 6;

  const int mrow = m0 + wid * 16 + (lane & 15);
  const long grow = l * (long)M + min(mrow, M - 1);
  const float* grow_p = dZ + grow * O;
  const bool vec_g = (O & 7) == 0 && gbf16::aligned16(dZ);
  const int kq = 8 * (lane >> 4);

  // relu mask: bits of 4 consecutive bf16 per fragment
  bf16x4 yb[4];
  if (act_below == ACT_RELU) {
#pragma unroll
    for (int fi = 0; fi < 4; ++fi) {
      const int i4 = min(i0 + fi * 16 + (lane >> 4) * 4, I - 4);
      yb[fi] = *reinterpret_cast<const bf16x4*>(Yb + grow * I + i4);
    }
  }

  f32x4 acc[4] = {};  // [fi]: 4 consecutive i of row mrow
  f32x4 vw[2][2];
  bf16x8 g[2];
  const int nstages = (O + KS - 1) / KS;
  gbf16::load_cols(W, I, 0, O, i0, I, tid, vw);
  g[0] = frag_f32(grow_p, kq, O, vec_g);
  g[1] = frag_f32(grow_p, 32 + kq, O, vec_g);
  for (int s = 0; s < nstages; ++s) {
    __syncthreads();  // previous compute done: LDS free
    gbf16::store_cols(Ws, tid, vw);
    const bf16x8 b0 = g[0], b1 = g[1];
    if (s + 1 < nstages) {
      gbf16::load_cols(W, I, (s + 1) * KS, O, i0, I, tid, vw);
      g[0] = frag_f32(grow_p, (s + 1) * KS + kq, O, vec_g);
      g[1] = frag_f32(grow_p, (s + 1) * KS + 32 + kq, O, vec_g);
    }
    __syncthreads();  // LDS image of stage s visible
    const int klim = O - s * KS;
#pragma unroll
    for (int kk = 0; kk < KS; kk += 32) {
      if (kk < klim) {
        bf16x8 a[4];
#pragma unroll
        for (int fi = 0; fi < 4; ++fi) {
          a[fi] = *reinterpret_cast<const bf16x8*>(
              &Ws[(fi * 16 + (lane & 15)) * LDK + kk + kq]);
        }
#pragma unroll
        for (int fi = 0; fi < 4; ++fi) {
          acc[fi] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(
              a[fi], kk == 0 ? b0 : b1, acc[fi], 0, 0, 0);
        }
      }
    }
  }

  const bool full = m0 + TM <= M && i0 + TN <= I;
  const float* Wb = theta + l * n + wb_off;
  const float* bb = theta + l * n + bb_off;
  float xv[4] = {0.f, 0.f, 0.f, 0.f};
  if (act_below == ACT_SIN_RELU) {
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      if (j < Ib) xv[j] = Xb2[grow * Ib + j];
    }
  }
#pragma unroll
  for (int fi = 0; fi < 4; ++fi) {
    const int i4 = i0 + fi * 16 + (lane >> 4) * 4;
    if (full || (mrow < M && i4 < I)) {
      f32x4 v = acc[fi];
      if (act_below == ACT_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          v[r] = (float)yb[fi][r] > 0.f ? v[r] : 0.f;
        }
      } else if (act_below == ACT_SIN_RELU) {
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          float z = bb[i4 + r];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (j < Ib) z += xv[j] * Wb[(long)(i4 + r) * Ib + j];
          }
          v[r] *= act_bwd(ACT_SIN_RELU, z, 0.f, scale_below);
        }
      }
      *reinterpret_cast<f32x4*>(dX + (l * (long)M + mrow) * I + i4) = v;
    }
  }
}

// ---------------------------------------------------------------------
// chunk's dW[O,I] partial = bf(dZ[mlo:mhi, O])^T @ X[mlo:mhi, I] with a
// bf16 X, and the db partial from the UNROUNDED fp32 dZ: the slabs,
// grid and chunking of gbf16::bf16_dw_k (see there), folded by the same
// gmfma::dw_reduce_parts_k launch. dZ is staged with load_cols /
// store_cols and feeds db from the same registers. For X a thread owns
// a column PAIR (tid & 31) and a k-octet (tid >> 5): it loads 8 dwords,
// two bf16 of 8 consecutive rows, so a wave reads 128 contiguous bytes
// of each of its 16 rows, and shuffles their low and high halves into
// the two 16-byte writes of the [i][m] image. I % 8 == 0.
DEV_INLINE void load_pairs(const __bf16* __restrict__ Xl, int I, int k0,
                           int K, int i0, int tid, unsigned (&d)[8]) {
  const int c = i0 + 2 * (tid & 31);
  const int kr = k0 + 8 * (tid >> 5);
  if (k0 + KS <= K && i0 + TN <= I) {
    const __bf16* p = Xl + (long)kr * I + c;
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      d[j] = *reinterpret_cast<const unsigned*>(p + (long)j * I);
    }
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) {
      d[j] = (kr + j < K && c < I)
                 ? *reinterpret_cast<const unsigned*>(
                       Xl + (long)(kr + j) * I + c)
                 : 0u;
    }
  }
}

DEV_INLINE void store_pairs(__bf16* S, int tid, const unsigned (&d)[8]) {
  u32x4 lo, hi;
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    lo[j] = (d[2 * j] & 0xffffu) | (d[2 * j + 1] << 16);
    hi[j] = (d[2 * j] >> 16) | (d[2 * j + 1] & 0xffff0000u);
  }
  __bf16* p = &S[2 * (tid & 31) * LDK + 8 * (tid >> 5)];
  *reinterpret_cast<u32x4*>(p) = lo;
  *reinterpret_cast<u32x4*>(p + LDK) = hi;
}

GBF16_KERNEL __launch_bounds__(256) void act_dw_k(
    const float* __restrict__ dZ, const __bf16* __restrict__ X,
    float* __restrict__ parts, float* __restrict__ dbparts,
    long pstride, long dbstride, int M, int I, int O, int mc,
    int nchunk) {
  __shared__ __attribute__((aligned(16))) __bf16 As[TM * LDK];  // [o][m]
  __shared__ __attribute__((aligned(16))) __bf16 Bs[TN * LDK];  // [i][m]
  __shared__ float dbs[4][TM];

  const int chunk = blockIdx.z % nchunk;
  const long l = blockIdx.z / nchunk;
  const float* Gl = dZ + l * (long)M * O;
  const __bf16* Xl = X + l * (long)M * I;
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
  f32x4 va[2][2];
  unsigned xd[8];
  float db_acc = 0.f;  // column o0 + (tid&63), this thread's k octets

  gbf16::load_cols(Gl, O, mlo, mhi, o0, O, tid, va);
  load_pairs(Xl, I, mlo, mhi, i0, tid, xd);
  for (int k0 = mlo; k0 < mhi; k0 += KS) {
    __syncthreads();
    gbf16::store_cols(As, tid, va);
    store_pairs(Bs, tid, xd);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
#pragma unroll
      for (int j = 0; j < 4; ++j) db_acc += va[h][0][j] + va[h][1][j];
    }
    if (k0 + KS < mhi) {
      gbf16::load_cols(Gl, O, k0 + KS, mhi, o0, O, tid, va);
      load_pairs(Xl, I, k0 + KS, mhi, i0, tid, xd);
    }
    __syncthreads();
    gbf16::mma_stage(As, Bs, wm, wn, lane, mhi - k0, acc);
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

}  // namespace gbf16a

// Epilogues of the MFMA stacked linear kernels, written once.
//
// gmfma::mfma_fwd_k / mfma_dx_k (f32 and f64 operands, 16x16x4) and
// gbf16::bf16_fwd_k / bf16_dx_k (bf16 operands, 16x16x32, f32
// accumulators) share one block geometry: a 64x64 output tile, 4 waves
// in a 2x2 grid, each wave a 32x32 sub-tile held as acc[2][2] 16x16
// accumulator fragments. What differs is the element type T and, by
// accumulator dtype, the row a lane's r-th accumulator element belongs
// to (acc_map). Everything after the stage loop is here:
//   EPI_FWD_EPILOGUE      Y = act(acc + bias)  [+ Z stash]
//   EPI_DX_EPILOGUE       dX = acc * act_below'(z_below, y_below)
//   EPI_BELOW_ACT_FACTOR  that multiplier for one element, also used by
//                         the kernels without a tiled fast path
//                         (gmfma::mfma_dx16_k, gemm::linear_bwd_dx_k)
//
// They are statement MACROS, not inline functions, for a measured
// reason. An inline function is optimised on its own (its fragment
// loops unrolled) BEFORE it is inlined into the kernel. The kernel the
// optimiser then sees differs from one with the epilogue written in
// place: the f32/f64 kernels' stage loops came out with another
// register assignment and MFMA/LDS interleaving (0.3-0.4 % of a density
// round), and in the bf16 kernels the accumulator array, now indexed by
// constants everywhere, was promoted to ONE 16-wide vector that the
// epilogue copies to VGPRs whole (+16 VGPRs: 4 waves/SIMD, not 5). The
// macros expand in the kernel, so each kernel compiles to the code it
// had with its own copy of the epilogue. Arguments are evaluated where
// they appear: pass names and side-effect-free expressions only.
#pragma once

#include "common.h"

namespace epi {

typedef double f64x4 __attribute__((ext_vector_type(4)));
typedef float f32x4 __attribute__((ext_vector_type(4)));

// C/D fragment of the 16x16 MFMA shapes: 4 elements per lane, column
// lane & 15; the row differs BY ACCUMULATOR DTYPE (measured on gfx950,
// tools/mfma_probe.hip). 16x16x32_bf16 accumulates in f32 and has the
// f32 map.
template <typename T>
struct acc_map;

template <>
struct acc_map<float> {
  using acc_t = f32x4;
  static DEV_INLINE int acc_row(int lane, int r) {
    return (lane >> 4) * 4 + r;
  }
};

template <>
struct acc_map<double> {
  using acc_t = f64x4;
  // f64 acc rows interleave as 4*reg + (lane>>4)
  static DEV_INLINE int acc_row(int lane, int r) {
    return 4 * r + (lane >> 4);
  }
};

}  // namespace epi

// v *= act_below'(z_below, y_below) for element (m, i) of node l's dX,
// flat offset `off`. z_below comes from Zb, or with Xb2 != null is
// RECOMPUTED from the below layer's tiny input,
// Xb2[l*M + m, :Ib] @ Wb[i, :Ib] + bb[i] (Ib <= 4): a few flops on
// L1-resident reads instead of a full [M, I] Zb tensor back from HBM
// (328 MB/call at the FourierNet encode of the density config).
// Callers skip it where act_below == ACT_NONE.
#define EPI_BELOW_ACT_FACTOR(T, v, act_below, scale_below, Yb, Zb, off,  \
                             Xb2, Wb, bb, l, M, m, i, Ib)                \
  do {                                                                   \
    T z = T(0);                                                          \
    if ((Xb2) != nullptr) {                                              \
      z = (bb)[i];                                                       \
      _Pragma("unroll") for (int j = 0; j < 4; ++j) {                    \
        if (j < (Ib)) {                                                  \
          z += (Xb2)[(long)((l) * (long)(M) + (m)) * (Ib) + j]           \
               * (Wb)[(long)(i) * (Ib) + j];                             \
        }                                                                \
      }                                                                  \
    } else if ((Zb) != nullptr) {                                        \
      z = (Zb)[off];                                                     \
    }                                                                    \
    (v) *= act_bwd(act_below, z, (Yb) ? (Yb)[off] : T(0), scale_below);  \
  } while (0)

// Y[l, m, o] = act(acc + bias[o]), Z[l, m, o] = acc + bias[o] where Z
// is asked for. MAP is the accumulator's acc_map, (m0, o0) the block's
// tile, (wm, wn) the wave's sub-tile in it, full_mo whether the tile
// lies inside [M, O]. Full tiles without a Z stash store guard-free
// with the bias preloaded: per-element bounds guards serialize the
// store chain (trap 4c).
#define EPI_FWD_EPILOGUE(T, MAP, acc, bias, Y, Z, l, M, O, m0, o0, wm,   \
                         wn, lane, act, scale, full_mo)                  \
  do {                                                                   \
    if ((full_mo) && (Z) == nullptr) {                                   \
      T bv[2];                                                           \
      _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {                 \
        bv[fn] = (bias)[(o0) + (wn) + fn * 16 + ((lane) & 15)];          \
      }                                                                  \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int o = (o0) + (wn) + fn * 16 + ((lane) & 15);         \
            const long off = (l) * (long)(M) * (O) + (long)m * (O) + o;  \
            (Y)[off] = act_fwd(act, (acc)[fm][fn][r] + bv[fn], scale);   \
          }                                                              \
        }                                                                \
      }                                                                  \
    } else {                                                             \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int o = (o0) + (wn) + fn * 16 + ((lane) & 15);         \
            if (m < (M) && o < (O)) {                                    \
              const T z = (acc)[fm][fn][r] + (bias)[o];                  \
              const long off =                                           \
                  (l) * (long)(M) * (O) + (long)m * (O) + o;             \
              if ((Z) != nullptr) (Z)[off] = z;                          \
              (Y)[off] = act_fwd(act, z, scale);                         \
            }                                                            \
          }                                                              \
        }                                                                \
      }                                                                  \
    }                                                                    \
  } while (0)

// dX[l, m, i] = acc * act_below'(z_below, y_below); Wb / bb are the
// below layer's weights and bias in node l's parameter row (recompute
// mode only), full_mi whether the tile lies inside [M, I]. Two
// guard-free fast paths for full tiles, each with ALL its loads issued
// before the first store (per-element bounds guards serialized this
// epilogue - trap 4c): relu below (the 16 Yb mask values), and the
// sin_relu encode below with z recomputed from its 2-wide input,
// written bv + x0*w0 + x1*w1 so that it contracts as it always has.
// Every other tile and activation takes the guarded per-element path.
#define EPI_DX_EPILOGUE(T, MAP, acc, dX, Yb, Zb, act_below, scale_below, \
                        Wb, bb, Xb2, Ib, l, M, I, m0, i0, wm, wn, lane,  \
                        full_mi)                                         \
  do {                                                                   \
    if ((full_mi) && (act_below) == ACT_RELU) {                          \
      T yv[2][2][4];                                                     \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int i = (i0) + (wn) + fn * 16 + ((lane) & 15);         \
            yv[fm][fn][r] =                                              \
                (Yb)[(l) * (long)(M) * (I) + (long)m * (I) + i];         \
          }                                                              \
        }                                                                \
      }                                                                  \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int i = (i0) + (wn) + fn * 16 + ((lane) & 15);         \
            const long off = (l) * (long)(M) * (I) + (long)m * (I) + i;  \
            (dX)[off] = yv[fm][fn][r] > T(0) ? (acc)[fm][fn][r] : T(0);  \
          }                                                              \
        }                                                                \
      }                                                                  \
    } else if ((full_mi) && (act_below) == ACT_SIN_RELU                  \
               && (Xb2) != nullptr && (Ib) == 2) {                       \
      T x0v[2][4], x1v[2][4];                                            \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int r = 0; r < 4; ++r) {                  \
          const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r);   \
          const long xoff = (long)((l) * (long)(M) + m) * 2;             \
          x0v[fm][r] = (Xb2)[xoff];                                      \
          x1v[fm][r] = (Xb2)[xoff + 1];                                  \
        }                                                                \
      }                                                                  \
      T w0v[2], w1v[2], bv[2];                                           \
      _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {                 \
        const int i = (i0) + (wn) + fn * 16 + ((lane) & 15);             \
        w0v[fn] = (Wb)[(long)i * 2];                                     \
        w1v[fn] = (Wb)[(long)i * 2 + 1];                                 \
        bv[fn] = (bb)[i];                                                \
      }                                                                  \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int i = (i0) + (wn) + fn * 16 + ((lane) & 15);         \
            const long off = (l) * (long)(M) * (I) + (long)m * (I) + i;  \
            const T z = bv[fn] + x0v[fm][r] * w0v[fn]                    \
                        + x1v[fm][r] * w1v[fn];                          \
            (dX)[off] = (acc)[fm][fn][r]                                 \
                        * act_bwd(ACT_SIN_RELU, z, T(0), scale_below);   \
          }                                                              \
        }                                                                \
      }                                                                  \
    } else {                                                             \
      _Pragma("unroll") for (int fm = 0; fm < 2; ++fm) {                 \
        _Pragma("unroll") for (int fn = 0; fn < 2; ++fn) {               \
          _Pragma("unroll") for (int r = 0; r < 4; ++r) {                \
            const int m = (m0) + (wm) + fm * 16 + MAP::acc_row(lane, r); \
            const int i = (i0) + (wn) + fn * 16 + ((lane) & 15);         \
            if (m < (M) && i < (I)) {                                    \
              const long off =                                           \
                  (l) * (long)(M) * (I) + (long)m * (I) + i;             \
              T v = (acc)[fm][fn][r];                                    \
              if ((act_below) != ACT_NONE) {                             \
                EPI_BELOW_ACT_FACTOR(T, v, act_below, scale_below, Yb,   \
                                     Zb, off, Xb2, Wb, bb, l, M, m, i,   \
                                     Ib);                                \
              }                                                          \
              (dX)[off] = v;                                             \
            }                                                            \
          }                                                              \
        }                                                                \
      }                                                                  \
    }                                                                    \
  } while (0)

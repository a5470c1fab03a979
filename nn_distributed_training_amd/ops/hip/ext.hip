// Torch extension entry: dispatch + launch for the CDNA4 kernel library.
// Single translation unit (the kernel files are header-style templates).

#include <torch/extension.h>

#include "common.h"
#include "elementwise.hip"
#include "gemm.hip"
#include "gemm_mfma.hip"
#include "conv.hip"
#include "losses.hip"
#include "rollout.hip"
#include "advantage.hip"
#include "fused_mnist.hip"

#include <ATen/hip/HIPContext.h>

#include <map>

namespace {

inline hipStream_t cur_stream() {
  return at::hip::getCurrentHIPStream().stream();
}

inline int grid_1d(long total, int block = 256, int cap = 4096) {
  long g = (total + block - 1) / block;
  return (int)std::min<long>(g, cap);
}

#define CHECK_DEV(t) \
  TORCH_CHECK((t).is_cuda() && (t).is_contiguous(), #t " must be contiguous on GPU")

#define DISPATCH_FT(scalar_t_tensor, ...)                                  \
  AT_DISPATCH_FLOATING_TYPES(scalar_t_tensor.scalar_type(), "ndta_ops",    \
                             [&] { __VA_ARGS__ });

// data pointer of an optional tensor; nullptr when it is absent
template <typename T>
inline T* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}

// f(mode_c, pen_c): the optimizer mode (0 adam, 1 adamw, 2 sgd) and
// the consensus-penalty flag as compile-time constants for the
// fused_step*_k templates
template <typename F>
inline void dispatch_mode_pen(long mode, bool pen, F&& f) {
  auto with_pen = [&](auto mode_c) {
    pen ? f(mode_c, std::true_type{}) : f(mode_c, std::false_type{});
  };
  if (mode == 0) with_pen(std::integral_constant<int, 0>{});
  else if (mode == 1) with_pen(std::integral_constant<int, 1>{});
  else with_pen(std::integral_constant<int, 2>{});
}

// ---------------------------------------------------------------- ew --
void dinno_dual_threg(torch::Tensor local,
                      c10::optional<torch::Tensor> remote,
                      torch::Tensor offs, torch::Tensor idx,
                      torch::Tensor duals, torch::Tensor s_out,
                      double rho) {
  CHECK_DEV(local); CHECK_DEV(duals); CHECK_DEV(s_out);
  const long L = duals.size(0), n = duals.size(1);
  DISPATCH_FT(local, {
    hipLaunchKernelGGL(ew::dinno_dual_threg_k<scalar_t>,
        dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
        local.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(remote),
        offs.data_ptr<int>(), idx.data_ptr<int>(),
        duals.data_ptr<scalar_t>(), s_out.data_ptr<scalar_t>(),
        (scalar_t)rho, n, L);
  });
  HIP_CHECK_LAST();
}

void mix_rows(torch::Tensor local, c10::optional<torch::Tensor> remote,
              torch::Tensor offs, torch::Tensor idx, torch::Tensor w,
              torch::Tensor out) {
  CHECK_DEV(local); CHECK_DEV(out);
  TORCH_CHECK(local.data_ptr() != out.data_ptr(),
              "mix_rows: out must not alias the local table");
  const long L = out.size(0), n = out.size(1);
  DISPATCH_FT(local, {
    hipLaunchKernelGGL(ew::mix_rows_k<scalar_t>,
        dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
        local.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(remote),
        offs.data_ptr<int>(), idx.data_ptr<int>(),
        w.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(), n, L);
  });
  HIP_CHECK_LAST();
}

void dsgt_mix(torch::Tensor p_loc, torch::Tensor y_loc,
              c10::optional<torch::Tensor> remote, torch::Tensor offs,
              torch::Tensor idx, torch::Tensor w, torch::Tensor p_out,
              torch::Tensor y_mix, double alpha) {
  CHECK_DEV(p_loc); CHECK_DEV(y_loc); CHECK_DEV(p_out); CHECK_DEV(y_mix);
  TORCH_CHECK(p_loc.data_ptr() != p_out.data_ptr(),
              "dsgt_mix: p_out must not alias p_loc");
  const long L = p_out.size(0), n = p_out.size(1);
  DISPATCH_FT(p_loc, {
    hipLaunchKernelGGL(ew::dsgt_mix_k<scalar_t>,
        dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
        p_loc.data_ptr<scalar_t>(), y_loc.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(remote),
        offs.data_ptr<int>(), idx.data_ptr<int>(),
        w.data_ptr<scalar_t>(), p_out.data_ptr<scalar_t>(),
        y_mix.data_ptr<scalar_t>(), (scalar_t)alpha, n, L);
  });
  HIP_CHECK_LAST();
}

void gather_batch(torch::Tensor X_all, torch::Tensor idx,
                  torch::Tensor out, long idx_stride, long idx_off) {
  CHECK_DEV(X_all); CHECK_DEV(out);
  const long L = X_all.size(0), maxlen = X_all.size(1),
             Fdim = X_all.size(2);
  const long B = out.size(0) / L;
  const long total = out.numel();
  DISPATCH_FT(X_all, {
    hipLaunchKernelGGL(ew::gather_batch_k<scalar_t>,
        dim3(grid_1d(total)), dim3(ew::BLOCK), 0, cur_stream(),
        X_all.data_ptr<scalar_t>(), idx.data_ptr<long>(),
        out.data_ptr<scalar_t>(), maxlen, Fdim, B, idx_stride,
        idx_off, total);
  });
  HIP_CHECK_LAST();
}

void gather_targets(torch::Tensor Y_all, torch::Tensor idx,
                    torch::Tensor out, long idx_stride, long idx_off) {
  CHECK_DEV(Y_all); CHECK_DEV(out);
  const long L = Y_all.size(0), maxlen = Y_all.size(1);
  const long B = out.numel() / L;
  const long total = out.numel();
  // targets are long labels or floating densities
  auto launch = [&](auto elem) {
    using T = decltype(elem);
    hipLaunchKernelGGL(ew::gather_targets_k<T>,
        dim3(grid_1d(total)), dim3(ew::BLOCK), 0, cur_stream(),
        Y_all.data_ptr<T>(), idx.data_ptr<long>(), out.data_ptr<T>(),
        maxlen, B, idx_stride, idx_off, total);
  };
  if (Y_all.scalar_type() == torch::kLong) {
    launch(long{});
  } else {
    DISPATCH_FT(Y_all, { launch(scalar_t{}); });
  }
  HIP_CHECK_LAST();
}

void dsgt_y_update(torch::Tensor y_mix, torch::Tensor g_new,
                   torch::Tensor g_old, torch::Tensor y) {
  CHECK_DEV(y);
  const long total = y.numel();
  DISPATCH_FT(y, {
    hipLaunchKernelGGL(ew::dsgt_y_update_k<scalar_t>,
        dim3(grid_1d(total)), dim3(ew::BLOCK), 0, cur_stream(),
        y_mix.data_ptr<scalar_t>(), g_new.data_ptr<scalar_t>(),
        g_old.data_ptr<scalar_t>(), y.data_ptr<scalar_t>(), total);
  });
  HIP_CHECK_LAST();
}

void fused_step(torch::Tensor theta, torch::Tensor grad,
                c10::optional<torch::Tensor> dual,
                c10::optional<torch::Tensor> s,
                c10::optional<torch::Tensor> deg,
                c10::optional<torch::Tensor> m,
                c10::optional<torch::Tensor> v,
                double rho, double lr, double beta1, double beta2,
                double eps, double wd, long step_t, long mode,
                bool first_step, long nparts, bool zero_grad) {
  CHECK_DEV(theta); CHECK_DEV(grad);
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(grad.numel() == L * nparts * n, "grad/nparts mismatch");
  DISPATCH_FT(theta, {
    const scalar_t bc1 =
        (scalar_t)(1.0 - std::pow(beta1, (double)step_t));
    const scalar_t bc2 =
        (scalar_t)(1.0 - std::pow(beta2, (double)step_t));
    dispatch_mode_pen(mode, dual.has_value(), [&](auto mode_c,
                                                  auto pen_c) {
      hipLaunchKernelGGL(
          (ew::fused_step_k<scalar_t, decltype(mode_c)::value,
                            decltype(pen_c)::value>),
          dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
          theta.data_ptr<scalar_t>(), grad.data_ptr<scalar_t>(),
          opt_ptr<scalar_t>(dual), opt_ptr<scalar_t>(s),
          opt_ptr<int>(deg), opt_ptr<scalar_t>(m), opt_ptr<scalar_t>(v),
          (scalar_t)rho, (scalar_t)lr, (scalar_t)beta1,
          (scalar_t)beta2, (scalar_t)eps, (scalar_t)wd, bc1, bc2,
          first_step ? 1 : 0, (int)nparts, n, L, zero_grad ? 1 : 0);
    });
  });
  HIP_CHECK_LAST();
}

void dinno_dual_threg_sched(torch::Tensor local,
                            c10::optional<torch::Tensor> remote,
                            torch::Tensor offs, torch::Tensor idx,
                            torch::Tensor duals, torch::Tensor s_out,
                            torch::Tensor sched) {
  CHECK_DEV(local); CHECK_DEV(duals); CHECK_DEV(s_out);
  const long L = duals.size(0), n = duals.size(1);
  DISPATCH_FT(local, {
    hipLaunchKernelGGL(ew::dinno_dual_threg_sched_k<scalar_t>,
        dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
        local.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(remote),
        offs.data_ptr<int>(), idx.data_ptr<int>(),
        duals.data_ptr<scalar_t>(), s_out.data_ptr<scalar_t>(),
        sched.data_ptr<scalar_t>(), n, L);
  });
  HIP_CHECK_LAST();
}

void fused_step_sched(torch::Tensor theta, torch::Tensor grad,
                      c10::optional<torch::Tensor> dual,
                      c10::optional<torch::Tensor> s,
                      c10::optional<torch::Tensor> deg,
                      c10::optional<torch::Tensor> m,
                      c10::optional<torch::Tensor> v,
                      torch::Tensor sched, long pit,
                      double beta1, double beta2, double eps, double wd,
                      long mode, bool first_step, long nparts) {
  CHECK_DEV(theta); CHECK_DEV(grad);
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(grad.numel() == L * nparts * n, "grad/nparts mismatch");
  DISPATCH_FT(theta, {
    dispatch_mode_pen(mode, dual.has_value(), [&](auto mode_c,
                                                  auto pen_c) {
      hipLaunchKernelGGL(
          (ew::fused_step_sched_k<scalar_t, decltype(mode_c)::value,
                                  decltype(pen_c)::value>),
          dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
          theta.data_ptr<scalar_t>(), grad.data_ptr<scalar_t>(),
          opt_ptr<scalar_t>(dual), opt_ptr<scalar_t>(s),
          opt_ptr<int>(deg), opt_ptr<scalar_t>(m), opt_ptr<scalar_t>(v),
          sched.data_ptr<scalar_t>(), (int)pit,
          (scalar_t)beta1, (scalar_t)beta2, (scalar_t)eps,
          (scalar_t)wd, first_step ? 1 : 0, (int)nparts, n, L);
    });
  });
  HIP_CHECK_LAST();
}

void gather_batch_dev(torch::Tensor X_all, torch::Tensor idx,
                      torch::Tensor out, torch::Tensor offs_dev,
                      long pit, long idx_stride) {
  CHECK_DEV(X_all); CHECK_DEV(out);
  const long L = X_all.size(0), maxlen = X_all.size(1),
             Fdim = X_all.size(2);
  const long B = out.size(0) / L;
  const long total = out.numel();
  DISPATCH_FT(X_all, {
    hipLaunchKernelGGL(ew::gather_batch_dev_k<scalar_t>,
        dim3(grid_1d(total)), dim3(ew::BLOCK), 0, cur_stream(),
        X_all.data_ptr<scalar_t>(), idx.data_ptr<long>(),
        out.data_ptr<scalar_t>(), offs_dev.data_ptr<long>(), (int)pit,
        maxlen, Fdim, B, idx_stride, total);
  });
  HIP_CHECK_LAST();
}

void reduce_parts(torch::Tensor parts, torch::Tensor out,
                  long nparts) {
  CHECK_DEV(parts); CHECK_DEV(out);
  const long L = out.size(0), n = out.size(1);
  TORCH_CHECK(parts.numel() == L * nparts * n, "parts shape mismatch");
  DISPATCH_FT(out, {
    hipLaunchKernelGGL(ew::reduce_parts_k<scalar_t>,
        dim3(grid_1d(L * n)), dim3(ew::BLOCK), 0, cur_stream(),
        parts.data_ptr<scalar_t>(), out.data_ptr<scalar_t>(),
        (int)nparts, n, L);
  });
  HIP_CHECK_LAST();
}

void axpy(torch::Tensor x, torch::Tensor g, double alpha,
          bool zero_grad) {
  CHECK_DEV(x);
  DISPATCH_FT(x, {
    hipLaunchKernelGGL(ew::axpy_k<scalar_t>,
        dim3(grid_1d(x.numel())), dim3(ew::BLOCK), 0, cur_stream(),
        x.data_ptr<scalar_t>(), g.data_ptr<scalar_t>(),
        (scalar_t)alpha, x.numel(), zero_grad ? 1 : 0);
  });
  HIP_CHECK_LAST();
}

// -------------------------------------------------------------- gemm --
void linear_fwd(torch::Tensor X, torch::Tensor theta, torch::Tensor Y,
                c10::optional<torch::Tensor> Z, long w_off, long b_off,
                long M, long I, long O, long act, double scale) {
  CHECK_DEV(X); CHECK_DEV(theta); CHECK_DEV(Y);
  const long L = theta.size(0), n = theta.size(1);
  // MFMA pays only when M fills the 64-row tiles across the chip;
  // small-M layers (MNIST fc, per-node B=64) stay on the VALU kernels.
  // I must be even for the 16-byte staging loads (vec2 alignment).
  const bool use_mfma = (M >= 128 && O >= 16 && I >= 8 && I % 2 == 0);
  DISPATCH_FT(X, {
    auto zp = opt_ptr<scalar_t>(Z);
    if (use_mfma) {
      dim3 grid((O + 63) / 64, (M + 63) / 64, L);
      hipLaunchKernelGGL(gmfma::mfma_fwd_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          X.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y.data_ptr<scalar_t>(), zp, n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)act, (scalar_t)scale);
    } else if (I <= 4 && M >= 1024 && O >= 64 && O <= 1024 &&
               O % 64 == 0) {
      // register-resident encode kernel: one thread per output
      // column (blockDim == O), W row + bias in registers, scalar
      // X-row loads, compile-time-I guard-free dot
      const long blocks = std::min<long>(M, 8192);
      dim3 grid(blocks, 1, L);
      auto launch_enc = [&](auto ik_tag) {
        constexpr int IK = decltype(ik_tag)::value;
        hipLaunchKernelGGL((gemm::encode_fwd_k<scalar_t, IK>), grid,
            dim3((int)O), 0, cur_stream(), X.data_ptr<scalar_t>(),
            theta.data_ptr<scalar_t>(), Y.data_ptr<scalar_t>(), zp, n,
            w_off, b_off, (int)M, (int)O, (int)act, (scalar_t)scale);
      };
      if (I == 1) launch_enc(std::integral_constant<int, 1>{});
      else if (I == 2) launch_enc(std::integral_constant<int, 2>{});
      else if (I == 3) launch_enc(std::integral_constant<int, 3>{});
      else launch_enc(std::integral_constant<int, 4>{});
    } else if (I <= 4 && M >= 1024) {
      const long total = (long)M * O;
      const long blocks =
          std::min<long>((total + 255) / 256, 2048);
      const size_t shmem = (size_t)(O * I + O) * sizeof(scalar_t);
      hipLaunchKernelGGL((gemm::linear_fwd_smallk_k<scalar_t, 4>),
          dim3(blocks, 1, L), dim3(256), shmem, cur_stream(),
          X.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y.data_ptr<scalar_t>(), zp, n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)act, (scalar_t)scale);
    } else {
      dim3 grid((O + 15) / 16, (M + 15) / 16, L);
      hipLaunchKernelGGL(gemm::linear_fwd_k<scalar_t>,
          grid, dim3(16, 16), 0, cur_stream(),
          X.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y.data_ptr<scalar_t>(), zp, n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)act, (scalar_t)scale);
    }
  });
  HIP_CHECK_LAST();
}

void act_grad(torch::Tensor dY, torch::Tensor Y,
              c10::optional<torch::Tensor> Z, torch::Tensor dZ,
              long act, double scale) {
  CHECK_DEV(dY); CHECK_DEV(dZ);
  DISPATCH_FT(dY, {
    hipLaunchKernelGGL(gemm::act_grad_k<scalar_t>,
        dim3(grid_1d(dY.numel())), dim3(256), 0, cur_stream(),
        dY.data_ptr<scalar_t>(), Y.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(Z), dZ.data_ptr<scalar_t>(), dY.numel(),
        (int)act, (scalar_t)scale);
  });
  HIP_CHECK_LAST();
}

// dX = dZ @ W with the BELOW layer's activation backward fused when
// act_below != 0 (Yb = below activation output, Zb = its pre-activation
// where needed, i.e. sin_relu).
void linear_bwd_dx(torch::Tensor dZ, torch::Tensor theta,
                   torch::Tensor dX,
                   c10::optional<torch::Tensor> Yb,
                   c10::optional<torch::Tensor> Zb,
                   long act_below, double scale_below,
                   long w_off, long M, long I, long O,
                   c10::optional<torch::Tensor> Xb2,
                   long wb_off, long bb_off, long Ib) {
  CHECK_DEV(dZ); CHECK_DEV(dX);
  const long L = theta.size(0), n = theta.size(1);
  const bool use_mfma =
      (M >= 128 && I >= 16 && O >= 8 && I % 2 == 0 && O % 2 == 0);
  DISPATCH_FT(dZ, {
    auto ybp = opt_ptr<scalar_t>(Yb);
    auto zbp = opt_ptr<scalar_t>(Zb);
    auto xb2p = opt_ptr<scalar_t>(Xb2);
    TORCH_CHECK(act_below == 0 || ybp != nullptr,
                "act_below needs Yb");
    TORCH_CHECK(xb2p == nullptr || Ib <= 4,
                "z-recompute supports below-layer in_dim <= 4");
    static const bool dx_new = []() {
      const char* e = getenv("NDTA_DX_NEW");
      return !(e && e[0] == '0');
    }();
    if (use_mfma && dx_new) {
      dim3 grid((I + 63) / 64, (M + 63) / 64, L);
      hipLaunchKernelGGL(gmfma::mfma_dx_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          dX.data_ptr<scalar_t>(), ybp, zbp, (int)act_below,
          (scalar_t)scale_below, n, w_off, (int)M, (int)I, (int)O,
          xb2p, wb_off, bb_off, (int)Ib);
    } else if (use_mfma) {
      dim3 grid((I + 63) / 64, (M + 63) / 64, L);
      hipLaunchKernelGGL(gmfma::mfma_dx16_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          dX.data_ptr<scalar_t>(), ybp, zbp, (int)act_below,
          (scalar_t)scale_below, n, w_off, (int)M, (int)I, (int)O,
          xb2p, wb_off, bb_off, (int)Ib);
    } else {
      dim3 grid((I + 15) / 16, (M + 15) / 16, L);
      hipLaunchKernelGGL(gemm::linear_bwd_dx_k<scalar_t>,
          grid, dim3(16, 16), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          dX.data_ptr<scalar_t>(), ybp, zbp, (int)act_below,
          (scalar_t)scale_below, n, w_off, (int)M, (int)I, (int)O,
          xb2p, wb_off, bb_off, (int)Ib);
    }
  });
  HIP_CHECK_LAST();
}

// Which dW/db kernel a [M, I] x [M, O] layer shape gets. This is the
// only place the thresholds are written: linear_bwd_dw switches on it,
// dw_conv_bwd_idx merges launches where it is Small, and the stacked
// engine asks dw_accumulates() which layers need a zeroed grad slice.
enum class DwKernel { Direct, Mfma, SkinnyI, SkinnyO, SmallChunked, Small };

inline DwKernel dw_kernel_for(long M, long I, long O) {
  if (M >= 256 && O % 64 == 0 && I % 16 == 0 && I <= 448 && O <= 512) {
    return DwKernel::Direct;
  }
  if (M >= 256 && I >= 16 && O >= 16) return DwKernel::Mfma;
  if (M > 2048 && I <= 4 && O <= 256) return DwKernel::SkinnyI;
  if (M > 2048 && O <= 4 && I <= 256) return DwKernel::SkinnyO;
  if (M > 2048) return DwKernel::SmallChunked;
  return DwKernel::Small;
}

// true where linear_bwd_dw ADDS into gstack, so the layer's slice must
// be zero on entry; the Small 16x16-tile store-path kernel overwrites
bool dw_accumulates(long M, long I, long O) {
  return dw_kernel_for(M, I, O) != DwKernel::Small;
}

// dW/db. PRECONDITION where dw_accumulates(M, I, O): the layer's slice
// of gstack is zeroed (the stacked engine zeroes the whole grad stack
// at backward start).
void linear_bwd_dw(torch::Tensor dZ, torch::Tensor X,
                   torch::Tensor gstack, long w_off, long b_off,
                   long M, long I, long O) {
  CHECK_DEV(dZ); CHECK_DEV(X); CHECK_DEV(gstack);
  const long L = gstack.size(0), n = gstack.size(1);
  DISPATCH_FT(dZ, {
    switch (dw_kernel_for(M, I, O)) {
    case DwKernel::Direct: {
      // full-I tiles: dZ and X each fetched from HBM exactly once;
      // direct-global fragment reads (both operands m-row-major), no
      // LDS/barriers — see gemm_mfma.hip mfma_dw_direct_k rationale.
      // Partial tiles go to per-chunk SLABS + a reduce kernel (plain
      // stores; the nchunk-way atomic burst measured ~2.8x roofline);
      // NDTA_DW_ATOMIC=1 selects the atomic epilogue for A/B runs.
      static const bool force_atomic = []() {
        const char* e = getenv("NDTA_DW_ATOMIC");
        return e && e[0] == '1';
      }();
      const long otiles = O / 64;
      long nchunk = std::max<long>(1, 512 / std::max<long>(1, otiles * L));
      nchunk = std::min<long>(nchunk, (M + 63) / 64);
      dim3 grid(1, otiles, L * nchunk);
      torch::Tensor parts;
      scalar_t* pp = nullptr;
      if (!force_atomic) {
        parts = torch::empty({L * nchunk * O * I}, gstack.options());
        pp = parts.data_ptr<scalar_t>();
      }
      auto launch_direct = [&](auto nimax) {
        hipLaunchKernelGGL(
            (gmfma::mfma_dw_direct_k<scalar_t, decltype(nimax)::value>),
            grid, dim3(512), 0, cur_stream(),
            dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
            gstack.data_ptr<scalar_t>(), pp, n, w_off, b_off,
            (int)M, (int)I, (int)O, (int)nchunk);
      };
      // fi_per == 1: NIMAX=1 keeps the load loops guard-free
      if (I <= 64) launch_direct(std::integral_constant<int, 1>{});
      else if (I <= 256) launch_direct(std::integral_constant<int, 4>{});
      else launch_direct(std::integral_constant<int, 7>{});
      if (pp != nullptr) {
        const long tile = O * I;
        dim3 rgrid(grid_1d(tile), 1, L);
        hipLaunchKernelGGL(gmfma::dw_reduce_parts_k<scalar_t>,
            rgrid, dim3(256), 0, cur_stream(),
            pp, gstack.data_ptr<scalar_t>(), n, w_off, tile,
            (int)nchunk);
      }
      break;
    }
    case DwKernel::Mfma: {
      // fill the chip: tiles * L * nchunk ≈ 2048 blocks
      const long tiles = ((I + 63) / 64) * ((O + 63) / 64);
      long nchunk = std::max<long>(1, 2048 / std::max<long>(1, tiles * L));
      nchunk = std::min<long>(nchunk, (M + 63) / 64);
      dim3 grid((I + 63) / 64, (O + 63) / 64, L * nchunk);
      hipLaunchKernelGGL(gmfma::mfma_dw_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
          gstack.data_ptr<scalar_t>(), n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)nchunk);
      break;
    }
    case DwKernel::SkinnyI: {
      long nchunk = std::max<long>(1, 1024 / std::max<long>(1, L));
      nchunk = std::min<long>(nchunk, (M + 255) / 256);
      if (I == 2 && O == 256) {  // FourierNet encode shape: all
        // bounds compile-time, unconditional loads (trap 4c)
        hipLaunchKernelGGL((gemm::dw_skinny_i_exact_k<scalar_t, 2>),
            dim3(1, 1, L * nchunk), dim3(256), 0, cur_stream(),
            dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
            gstack.data_ptr<scalar_t>(), n, w_off, b_off,
            (int)M, (int)I, (int)O, (int)nchunk);
      } else {
        hipLaunchKernelGGL((gemm::dw_skinny_i_k<scalar_t, 4>),
            dim3(1, 1, L * nchunk), dim3(256), 0, cur_stream(),
            dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
            gstack.data_ptr<scalar_t>(), n, w_off, b_off,
            (int)M, (int)I, (int)O, (int)nchunk);
      }
      break;
    }
    case DwKernel::SkinnyO: {
      long nchunk = std::max<long>(1, 1024 / std::max<long>(1, L));
      nchunk = std::min<long>(nchunk, (M + 255) / 256);
      hipLaunchKernelGGL((gemm::dw_skinny_o_k<scalar_t, 4>),
          dim3(1, 1, L * nchunk), dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
          gstack.data_ptr<scalar_t>(), n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)nchunk);
      break;
    }
    case DwKernel::SmallChunked: {
      const long total = O * I + O;
      long nchunk = std::max<long>(
          1, 2048 / std::max<long>(1, ((total + 255) / 256) * L));
      nchunk = std::min<long>(nchunk, (M + 255) / 256);
      dim3 grid((total + 255) / 256, 1, L * nchunk);
      hipLaunchKernelGGL(gemm::dw_small_chunked_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
          gstack.data_ptr<scalar_t>(), n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)nchunk);
      break;
    }
    case DwKernel::Small: {
      dim3 grid((I + 15) / 16, (O + 15) / 16, L);
      hipLaunchKernelGGL(gemm::linear_bwd_dw_k<scalar_t>,
          grid, dim3(16, 16), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(),
          gstack.data_ptr<scalar_t>(), n, w_off, b_off,
          (int)M, (int)I, (int)O);
      break;
    }
    }
  });
  HIP_CHECK_LAST();
}

// -------------------------------------------------------------- conv --
// f(kmax_c): KMAX sizes the conv kernels' per-thread dW register
// block; the K<=5 variant saves 48 VGPRs over the generic K<=7 one
// (occupancy)
template <typename Fn>
inline void dispatch_kmax(long K, Fn&& f) {
  if (K <= 5) f(std::integral_constant<int, 5>{});
  else f(std::integral_constant<int, 7>{});
}

// conv backward splits each (node, filter)'s batch into this many
// chunks, one block each
inline int conv_bwd_nchunk(long B) { return (int)std::min<long>(B, 32); }

// The launchers take the image source as (src_idx, idx_stride, idx_off,
// maxlen): X is the resident dataset [L, maxlen, IMG*IMG] read through
// the sampler's index stream (no gather_batch launch, no xb buffer
// round-trip); nullptr, 0, 0, 0 means X is the batch itself.
void launch_conv_fwd(const torch::Tensor& X, const torch::Tensor& theta,
                     const torch::Tensor& Y, const torch::Tensor& idx,
                     long w_off, long b_off, long B, long F, long K,
                     long IMG,
                     const long* src_idx, long idx_stride, long idx_off,
                     long maxlen) {
  CHECK_DEV(X); CHECK_DEV(theta); CHECK_DEV(Y);
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(K <= 7, "conv_pool_fwd supports kernel size <= 7");
  DISPATCH_FT(X, {
    const size_t shmem =
        (IMG * IMG + F * K * K + F) * sizeof(scalar_t);
    dispatch_kmax(K, [&](auto kmax) {
      hipLaunchKernelGGL(
          (conv::conv_pool_fwd_k<scalar_t, decltype(kmax)::value>),
          dim3(L * B), dim3(256), shmem, cur_stream(),
          X.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y.data_ptr<scalar_t>(), idx.data_ptr<unsigned char>(),
          n, w_off, b_off, (int)B, (int)F, (int)K, (int)IMG,
          src_idx, idx_stride, idx_off, maxlen);
    });
  });
  HIP_CHECK_LAST();
}

void launch_conv_bwd(const torch::Tensor& dY, const torch::Tensor& idx,
                     const torch::Tensor& X, const torch::Tensor& gstack,
                     long w_off, long b_off, long B, long F, long K,
                     long IMG,
                     const long* src_idx, long idx_stride, long idx_off,
                     long maxlen) {
  CHECK_DEV(dY); CHECK_DEV(X); CHECK_DEV(gstack);
  const long L = gstack.size(0), n = gstack.size(1);
  TORCH_CHECK(K <= 7, "conv_pool_bwd supports kernel size <= 7");
  // batch-chunked (l, f, chunk) grid with block-tree reduction +
  // atomics; measured best of three structures on the MNIST bench
  // (LDS-staged image variant was 2x slower — profiles/README.md)
  const int nchunk = conv_bwd_nchunk(B);
  DISPATCH_FT(dY, {
    dispatch_kmax(K, [&](auto kmax) {
      hipLaunchKernelGGL(
          (conv::conv_pool_bwd_k<scalar_t, decltype(kmax)::value>),
          dim3(L * F * nchunk), dim3(256), 0, cur_stream(),
          dY.data_ptr<scalar_t>(), idx.data_ptr<unsigned char>(),
          X.data_ptr<scalar_t>(), gstack.data_ptr<scalar_t>(),
          n, w_off, b_off, (int)B, (int)F, (int)K, (int)IMG, nchunk,
          src_idx, idx_stride, idx_off, maxlen);
    });
  });
  HIP_CHECK_LAST();
}

void conv_pool_fwd(torch::Tensor X, torch::Tensor theta, torch::Tensor Y,
                   torch::Tensor idx, long w_off, long b_off, long B,
                   long F, long K, long IMG) {
  launch_conv_fwd(X, theta, Y, idx, w_off, b_off, B, F, K, IMG, nullptr,
                  0, 0, 0);
}

void conv_pool_bwd(torch::Tensor dY, torch::Tensor idx, torch::Tensor X,
                   torch::Tensor gstack, long w_off, long b_off, long B,
                   long F, long K, long IMG) {
  launch_conv_bwd(dY, idx, X, gstack, w_off, b_off, B, F, K, IMG,
                  nullptr, 0, 0, 0);
}

void conv_pool_fwd_idx(torch::Tensor X_all, torch::Tensor src_idx,
                       long idx_stride, long idx_off,
                       torch::Tensor theta, torch::Tensor Y,
                       torch::Tensor idx, long w_off, long b_off,
                       long B, long F, long K, long IMG) {
  launch_conv_fwd(X_all, theta, Y, idx, w_off, b_off, B, F, K, IMG,
                  src_idx.data_ptr<long>(), idx_stride, idx_off,
                  X_all.size(1));
}

void conv_pool_bwd_idx(torch::Tensor dY, torch::Tensor idx,
                       torch::Tensor X_all, torch::Tensor src_idx,
                       long idx_stride, long idx_off,
                       torch::Tensor gstack, long w_off, long b_off,
                       long B, long F, long K, long IMG) {
  launch_conv_bwd(dY, idx, X_all, gstack, w_off, b_off, B, F, K, IMG,
                  src_idx.data_ptr<long>(), idx_stride, idx_off,
                  X_all.size(1));
}

// ------------------------------------------------------------ losses --
void mnist_train_step(
    torch::Tensor X_all, torch::Tensor Y_all, torch::Tensor idx,
    c10::optional<torch::Tensor> offs_dev, torch::Tensor theta,
    torch::Tensor grad, c10::optional<torch::Tensor> loss,
    long pit, long idx_off, long idx_stride,
    long wc_off, long bc_off, long w1_off, long b1_off, long w2_off,
    long b2_off, long B, long F, long K, long IMG, long H, long C,
    long TI, double loss_scale) {
  CHECK_DEV(X_all); CHECK_DEV(theta); CHECK_DEV(grad);
  const long L = theta.size(0), n = theta.size(1);
  const long NT = (B + TI - 1) / TI;
  TORCH_CHECK(grad.numel() == L * NT * n,
              "grad must be the [L, NT, n] per-tile slab buffer");
  const long maxlen = Y_all.size(1);
  TORCH_CHECK(bc_off == wc_off + F * K * K,
              "conv weight/bias must be contiguous in the flat layout");
  TORCH_CHECK(K <= 7, "fused mnist step supports kernel size <= 7");
  TORCH_CHECK(TI >= 1 && TI <= 8,
              "fused mnist step register tiling assumes TI <= 8");
  TORCH_CHECK(H <= 64 * TI || TI * H <= 512,
              "fused mnist step per-thread output budget exceeded");
  const long P = (IMG - (K - 1)) / 2;
  const long PF = F * P * P;
  dim3 grid((B + TI - 1) / TI, 1, L);
  DISPATCH_FT(X_all, {
    const size_t shmem =
        (size_t)(TI * (IMG * IMG + PF + 2 * H + C) + F * K * K + F +
                 C * H + C + 16 * 65) *
            sizeof(scalar_t) +
        ((size_t)TI * PF + 15) / 16 * 16 + (size_t)TI * sizeof(long);
    hipLaunchKernelGGL(fmnist::mnist_train_step_k<scalar_t>,
        grid, dim3(256), shmem, cur_stream(),
        X_all.data_ptr<scalar_t>(), Y_all.data_ptr<long>(),
        idx.data_ptr<long>(),
        opt_ptr<long>(offs_dev),
        theta.data_ptr<scalar_t>(), grad.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(loss),
        (int)pit, idx_off, idx_stride, maxlen, n,
        wc_off, bc_off, w1_off, b1_off, w2_off, b2_off,
        (int)B, (int)F, (int)K, (int)IMG, (int)H, (int)C, (int)TI,
        (int)NT, (scalar_t)loss_scale);
  });
  HIP_CHECK_LAST();
}

void logsoftmax(torch::Tensor Z, torch::Tensor P, long C) {
  CHECK_DEV(Z); CHECK_DEV(P);
  const long M = Z.numel() / C;
  DISPATCH_FT(Z, {
    hipLaunchKernelGGL(losses::logsoftmax_k<scalar_t>,
        dim3(grid_1d(M)), dim3(256), 0, cur_stream(),
        Z.data_ptr<scalar_t>(), P.data_ptr<scalar_t>(), M, (int)C);
  });
  HIP_CHECK_LAST();
}

void nll_bwd(torch::Tensor logp, torch::Tensor y, torch::Tensor dZ,
             c10::optional<torch::Tensor> loss, long C, long B,
             double loss_scale) {
  CHECK_DEV(logp); CHECK_DEV(dZ);
  const long M = logp.numel() / C;
  DISPATCH_FT(logp, {
    hipLaunchKernelGGL(losses::nll_bwd_k<scalar_t>,
        dim3(grid_1d(M)), dim3(256), 0, cur_stream(),
        logp.data_ptr<scalar_t>(), y.data_ptr<long>(),
        dZ.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(loss),
        M, (int)C, (int)B, (scalar_t)loss_scale);
  });
  HIP_CHECK_LAST();
}

void nll_fused(torch::Tensor Z, torch::Tensor Y_all,
               torch::Tensor idx, torch::Tensor dZ,
               c10::optional<torch::Tensor> loss,
               c10::optional<torch::Tensor> offs_dev, long pit,
               long idx_stride, long idx_off, long C, long B,
               double loss_scale) {
  CHECK_DEV(Z); CHECK_DEV(dZ);
  const long maxlen = Y_all.size(1);
  const long M = Z.numel() / C;
  DISPATCH_FT(Z, {
    hipLaunchKernelGGL(losses::nll_fused_k<scalar_t>,
        dim3(grid_1d(M)), dim3(256), 0, cur_stream(),
        Z.data_ptr<scalar_t>(), Y_all.data_ptr<long>(),
        idx.data_ptr<long>(), dZ.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(loss),
        opt_ptr<long>(offs_dev),
        (int)pit, maxlen, idx_stride, idx_off, M, (int)C, (int)B,
        (scalar_t)loss_scale);
  });
  HIP_CHECK_LAST();
}

void bce_bwd(torch::Tensor p, torch::Tensor tgt, torch::Tensor dZ,
             c10::optional<torch::Tensor> loss, long B,
             double loss_scale) {
  CHECK_DEV(p); CHECK_DEV(dZ);
  DISPATCH_FT(p, {
    hipLaunchKernelGGL(losses::bce_bwd_k<scalar_t>,
        dim3(grid_1d(p.numel())), dim3(256), 0, cur_stream(),
        p.data_ptr<scalar_t>(), tgt.data_ptr<scalar_t>(),
        dZ.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(loss),
        p.numel(), (int)B, (scalar_t)loss_scale);
  });
  HIP_CHECK_LAST();
}

void regression_bwd(torch::Tensor yhat, torch::Tensor tgt,
                    torch::Tensor dY, c10::optional<torch::Tensor> loss,
                    long B, double loss_scale, long mode) {
  CHECK_DEV(yhat); CHECK_DEV(dY);
  DISPATCH_FT(yhat, {
    auto launch = [&](auto mode_c) {
      hipLaunchKernelGGL(
          (losses::regression_bwd_k<scalar_t, decltype(mode_c)::value>),
          dim3(grid_1d(yhat.numel())), dim3(256), 0, cur_stream(),
          yhat.data_ptr<scalar_t>(), tgt.data_ptr<scalar_t>(),
          dY.data_ptr<scalar_t>(), opt_ptr<scalar_t>(loss),
          yhat.numel(), (int)B, (scalar_t)loss_scale);
    };
    if (mode == 0) launch(std::integral_constant<int, 0>{});
    else launch(std::integral_constant<int, 1>{});
  });
  HIP_CHECK_LAST();
}

// PPO clipped surrogate + critic MSE backward (losses.hip
// ppo_loss_bwd_k): mean/acts [L*M, A], the rest [L*M]; loss [L, 2] is
// accumulated into when given (the caller zeroes it).
void ppo_loss_bwd(torch::Tensor mean, torch::Tensor acts,
                  torch::Tensor old_logp, torch::Tensor adv,
                  torch::Tensor v, torch::Tensor rtgs,
                  torch::Tensor dmean, torch::Tensor dv,
                  c10::optional<torch::Tensor> loss, long M, double cov,
                  double clip, double critic_coef, double loss_scale) {
  CHECK_DEV(mean); CHECK_DEV(acts); CHECK_DEV(old_logp); CHECK_DEV(adv);
  CHECK_DEV(v); CHECK_DEV(rtgs); CHECK_DEV(dmean); CHECK_DEV(dv);
  TORCH_CHECK(mean.dim() == 2, "mean must be [L*M, A]");
  const long rows = mean.size(0), A = mean.size(1);
  TORCH_CHECK(A >= 1 && A <= losses::PPO_MAX_A,
              "ppo_loss_bwd supports action dim <= ", losses::PPO_MAX_A);
  TORCH_CHECK(M > 0 && rows % M == 0, "rows must be L*M");
  TORCH_CHECK(cov > 0, "cov must be positive");
  TORCH_CHECK(acts.numel() == rows * A && dmean.numel() == rows * A,
              "acts/dmean must match mean");
  for (const torch::Tensor* t : {&old_logp, &adv, &v, &rtgs, &dv}) {
    TORCH_CHECK(t->numel() == rows, "per-sample vectors must be [L*M]");
  }
  for (const torch::Tensor* t :
       {&acts, &old_logp, &adv, &v, &rtgs, &dmean, &dv}) {
    TORCH_CHECK(t->scalar_type() == mean.scalar_type(),
                "ppo_loss_bwd tensors must share one dtype");
  }
  if (loss.has_value()) {
    CHECK_DEV(*loss);
    TORCH_CHECK(loss->numel() == 2 * (rows / M) &&
                    loss->scalar_type() == mean.scalar_type(),
                "loss must be [L, 2] of the same dtype");
  }
  if (rows == 0) return;
  const double logc =
      0.5 * (double)A * std::log(2.0 * 3.14159265358979323846 * cov);
  DISPATCH_FT(mean, {
    hipLaunchKernelGGL(losses::ppo_loss_bwd_k<scalar_t>,
        dim3(grid_1d(rows)), dim3(256), 0, cur_stream(),
        mean.data_ptr<scalar_t>(), acts.data_ptr<scalar_t>(),
        old_logp.data_ptr<scalar_t>(), adv.data_ptr<scalar_t>(),
        v.data_ptr<scalar_t>(), rtgs.data_ptr<scalar_t>(),
        dmean.data_ptr<scalar_t>(), dv.data_ptr<scalar_t>(),
        opt_ptr<scalar_t>(loss), rows, (int)A, (int)M,
        (scalar_t)(1.0 / cov), (scalar_t)logc, (scalar_t)(1.0 - clip),
        (scalar_t)(1.0 + clip), (scalar_t)critic_coef,
        (scalar_t)loss_scale);
  });
  HIP_CHECK_LAST();
}

// One batch of SimpleTagEnv episodes on the device (rollout.hip
// ppo_rollout_k), one block per episode; the layer lists are the
// actor's shifted_plan (act: 0 none, 1 relu) and envp the env's
// constants in EnvParams order. Weights go to LDS where all N actors
// fit beside the reward row, else they are read in place;
// NDTA_ROLLOUT_WLDS=0/1 forces one or the other for A/B runs (1 only
// where they fit). The optional last_obs [N*E, obs_dim] receives the
// observation after every episode's last step (row l*E + e).
void ppo_rollout(torch::Tensor theta, std::vector<long> in_dims,
                 std::vector<long> out_dims, std::vector<long> w_offs,
                 std::vector<long> b_offs, std::vector<long> act_ids,
                 torch::Tensor resets, torch::Tensor obst,
                 torch::Tensor eps, torch::Tensor obs,
                 torch::Tensor acts, torch::Tensor logp,
                 torch::Tensor rews, torch::Tensor rtgs,
                 torch::Tensor ep_rew, long M, long ep_len, double cov,
                 double gamma, std::vector<double> envp,
                 c10::optional<torch::Tensor> last_obs) {
  CHECK_DEV(theta); CHECK_DEV(resets); CHECK_DEV(obst); CHECK_DEV(eps);
  CHECK_DEV(obs); CHECK_DEV(acts); CHECK_DEV(logp); CHECK_DEV(rews);
  CHECK_DEV(rtgs); CHECK_DEV(ep_rew);
  TORCH_CHECK(theta.dim() == 2, "theta must be the [N, n] stack");
  const long N = theta.size(0), n = theta.size(1);
  const long A = rollout::ACT_DIM;
  const long nl = (long)in_dims.size();
  TORCH_CHECK(N >= 1 && N <= rollout::MAX_N,
              "ppo_rollout supports at most ", rollout::MAX_N, " nodes");
  TORCH_CHECK(nl >= 1 && nl <= rollout::MAX_LAYERS,
              "ppo_rollout supports at most ", rollout::MAX_LAYERS,
              " layers");
  TORCH_CHECK((long)out_dims.size() == nl && (long)w_offs.size() == nl &&
                  (long)b_offs.size() == nl && (long)act_ids.size() == nl,
              "layer lists differ in length");
  TORCH_CHECK(envp.size() == 11, "envp must hold EnvParams' 11 values");
  TORCH_CHECK(M >= 1 && ep_len >= 1 && ep_len <= 4096 &&
                  N * M < (1L << 27),
              "ppo_rollout: bad M / ep_len");
  TORCH_CHECK(cov > 0, "cov must be positive");
  const long obs_dim = 2 * N + 6;
  const long E = (M + ep_len - 1) / ep_len;
  rollout::Plan plan;
  plan.nl = (int)nl;
  long span = 0, W = obs_dim;
  for (long i = 0; i < nl; ++i) {
    const long I = in_dims[i], O = out_dims[i];
    TORCH_CHECK(I >= 1 && I <= rollout::MAX_W && O >= 1 &&
                    O <= rollout::MAX_W,
                "ppo_rollout supports layer widths <= ", rollout::MAX_W);
    TORCH_CHECK(I == (i == 0 ? obs_dim : out_dims[i - 1]),
                "layer ", i, " does not take the layer below's output");
    TORCH_CHECK(act_ids[i] == ACT_NONE || act_ids[i] == ACT_RELU,
                "ppo_rollout supports relu/none activations");
    TORCH_CHECK(w_offs[i] >= 0 && b_offs[i] >= 0 &&
                    w_offs[i] + I * O <= n && b_offs[i] + O <= n,
                "layer ", i, " lies outside the parameter row");
    plan.in_dim[i] = (int)I; plan.out_dim[i] = (int)O;
    plan.w_off[i] = (int)w_offs[i]; plan.b_off[i] = (int)b_offs[i];
    plan.relu[i] = act_ids[i] == ACT_RELU ? 1 : 0;
    span = std::max(span, std::max(w_offs[i] + I * O, b_offs[i] + O));
    W = std::max(W, O);
  }
  TORCH_CHECK(out_dims[nl - 1] == A, "the actor's head must be ", A,
              " wide");
  TORCH_CHECK(n < (1L << 31), "parameter row too long");
  TORCH_CHECK(resets.scalar_type() == torch::kDouble &&
                  resets.numel() == E * (N + 1) * 2,
              "resets must be [E, N+1, 2] double");
  const long n_obst = obst.numel() / 2;
  TORCH_CHECK(obst.scalar_type() == torch::kDouble &&
                  obst.numel() == 2 * n_obst &&
                  n_obst <= rollout::MAX_OBST,
              "obst must be [<= ", rollout::MAX_OBST, ", 2] double");
  TORCH_CHECK(eps.numel() == E * ep_len * N * A,
              "eps must be [E, ep_len, N, A]");
  TORCH_CHECK(obs.numel() == N * M * obs_dim && acts.numel() == N * M * A &&
                  logp.numel() == N * M && rtgs.numel() == N * M,
              "obs/acts/logp/rtgs must be [N*M, .]");
  TORCH_CHECK(rews.scalar_type() == torch::kDouble && rews.numel() == M &&
                  ep_rew.scalar_type() == torch::kDouble &&
                  ep_rew.numel() == E,
              "rews [M] and ep_rew [E] must be double");
  for (const torch::Tensor* t : {&eps, &obs, &acts, &logp, &rtgs}) {
    TORCH_CHECK(t->scalar_type() == theta.scalar_type(),
                "ppo_rollout tensors must share theta's dtype");
  }
  if (last_obs.has_value()) {
    CHECK_DEV(*last_obs);
    TORCH_CHECK(last_obs->numel() == N * E * obs_dim &&
                    last_obs->scalar_type() == theta.scalar_type(),
                "ppo_rollout: last_obs must be [N*E, obs_dim] of theta's "
                "dtype");
  }
  rollout::EnvParams env{envp[0], envp[1], envp[2], envp[3], envp[4],
                         envp[5], envp[6], envp[7], envp[8], envp[9],
                         envp[10]};
  // a thread per (node, unit) and per observation element, plus the
  // reward thread at the block's end
  const long threads =
      (std::max(N * W, N * obs_dim + 1) + 63) / 64 * 64;
  TORCH_CHECK(threads <= 1024, "ppo_rollout block too large");
  static const int force_wlds = []() {
    const char* e = getenv("NDTA_ROLLOUT_WLDS");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
  }();
  const double logc =
      0.5 * (double)A * std::log(2.0 * 3.14159265358979323846 * cov);
  DISPATCH_FT(theta, {
    const size_t rew_bytes = (size_t)ep_len * sizeof(double);
    const size_t w_bytes = (size_t)(N * span) * sizeof(scalar_t);
    // static LDS of the kernel: the two activation buffers + env state
    const size_t fixed =
        2 * rollout::MAX_N * rollout::MAX_W * sizeof(scalar_t) + 1024;
    const bool fits = fixed + rew_bytes + w_bytes <= 156 * 1024;
    const bool wlds = fits && force_wlds != 0;
    auto launch = [&](auto wlds_c) {
      hipLaunchKernelGGL(
          (rollout::ppo_rollout_k<scalar_t, decltype(wlds_c)::value>),
          dim3(E), dim3(threads),
          rew_bytes + (decltype(wlds_c)::value ? w_bytes : 0),
          cur_stream(), theta.data_ptr<scalar_t>(), n, plan, (int)span,
          (int)W, resets.data_ptr<double>(), obst.data_ptr<double>(),
          eps.data_ptr<scalar_t>(), obs.data_ptr<scalar_t>(),
          acts.data_ptr<scalar_t>(), logp.data_ptr<scalar_t>(),
          rews.data_ptr<double>(), rtgs.data_ptr<scalar_t>(),
          ep_rew.data_ptr<double>(), (int)N, (int)n_obst, (int)M,
          (int)ep_len, (scalar_t)std::sqrt(cov), (scalar_t)logc, gamma,
          env, opt_ptr<scalar_t>(last_obs));
    };
    if (wlds) launch(std::true_type{});
    else launch(std::false_type{});
  });
  HIP_CHECK_LAST();
}

// GAE(lambda) advantages of all nodes in one launch (advantage.hip
// ppo_gae_k, one block per node): v [L*M] of T, rews double, [M] with
// rew_stride 0 (the device rollout's shared reward row) or [L*M] with
// rew_stride M; adv and the optional ret (the lambda-returns) [L*M] of
// T. Uniform episodes of ep_len steps, the last one cut at M; the
// optional v_last [L*E] of T (E = ceil(M / ep_len), row l*E + e)
// bootstraps every episode's end with gamma * v_last, and without it the
// ends are terminal. The unnormalised advantages wait in LDS for the node's mean and std; above
// LDS_MAX_M steps they wait in global memory instead: in adv itself
// where T is double, else in a double row allocated here.
void ppo_gae(torch::Tensor v, torch::Tensor rews, long rew_stride,
             torch::Tensor adv, c10::optional<torch::Tensor> ret, long M,
             long ep_len, double gamma, double lam,
             c10::optional<torch::Tensor> v_last) {
  CHECK_DEV(v); CHECK_DEV(rews); CHECK_DEV(adv);
  TORCH_CHECK(M >= 2, "ppo_gae: M must be at least 2 (unbiased std)");
  TORCH_CHECK(M < (1L << 31) - advantage::BLOCK, "ppo_gae: M too large");
  TORCH_CHECK(ep_len >= 1 && ep_len <= 4096,
              "ppo_gae: ep_len must be in 1..4096");
  TORCH_CHECK(gamma >= 0.0 && gamma <= 1.0 && lam >= 0.0 && lam <= 1.0,
              "ppo_gae: gamma and lam must be in [0, 1]");
  TORCH_CHECK(v.numel() >= M && v.numel() % M == 0,
              "ppo_gae: v must be [L*M]");
  const long L = v.numel() / M;
  TORCH_CHECK(L < (1L << 31), "ppo_gae: too many nodes for one grid");
  TORCH_CHECK(v.scalar_type() == torch::kFloat ||
                  v.scalar_type() == torch::kDouble,
              "ppo_gae: v must be float or double");
  TORCH_CHECK(rews.scalar_type() == torch::kDouble,
              "ppo_gae: rews must be double");
  TORCH_CHECK((rew_stride == 0 && rews.numel() == M) ||
                  (rew_stride == M && rews.numel() == L * M),
              "ppo_gae: rews must be [M] with stride 0 or [L*M] with "
              "stride M");
  TORCH_CHECK(adv.numel() == L * M &&
                  adv.scalar_type() == v.scalar_type() &&
                  adv.data_ptr() != v.data_ptr(),
              "ppo_gae: adv must be [L*M] of v's dtype, not v itself");
  if (ret.has_value()) {
    CHECK_DEV(*ret);
    TORCH_CHECK(ret->numel() == L * M &&
                    ret->scalar_type() == v.scalar_type() &&
                    ret->data_ptr() != v.data_ptr() &&
                    ret->data_ptr() != adv.data_ptr(),
                "ppo_gae: ret must be [L*M] of v's dtype, apart from v "
                "and adv");
  }
  if (v_last.has_value()) {
    CHECK_DEV(*v_last);
    const long E = (M + ep_len - 1) / ep_len;
    TORCH_CHECK(v_last->numel() == L * E &&
                    v_last->scalar_type() == v.scalar_type(),
                "ppo_gae: v_last must be [L*E] of v's dtype");
  }
  const bool lds = M <= advantage::LDS_MAX_M;
  torch::Tensor work;
  if (!lds) {
    work = v.scalar_type() == torch::kDouble
               ? adv
               : torch::empty({L * M}, v.options().dtype(torch::kDouble));
  }
  DISPATCH_FT(v, {
    hipLaunchKernelGGL(advantage::ppo_gae_k<scalar_t>, dim3(L),
        dim3(advantage::BLOCK), lds ? (size_t)M * sizeof(double) : 0,
        cur_stream(), v.data_ptr<scalar_t>(), rews.data_ptr<double>(),
        rew_stride, adv.data_ptr<scalar_t>(), opt_ptr<scalar_t>(ret),
        lds ? nullptr : work.data_ptr<double>(), (int)M, (int)ep_len,
        gamma, gamma * lam, opt_ptr<scalar_t>(v_last));
  });
  HIP_CHECK_LAST();
}

// fc1 dW/db + gather-sourced conv dW/db in ONE launch (fused_mnist.hip
// dw_conv_bwd_k) where the dW shape takes the small store-path kernel;
// any other shape keeps the two launches. Same preconditions as
// linear_bwd_dw + conv_pool_bwd_idx: the conv slice of gstack is zero.
void dw_conv_bwd_idx(torch::Tensor dZ, torch::Tensor X,
                     torch::Tensor dY, torch::Tensor pidx,
                     torch::Tensor X_all, torch::Tensor src_idx,
                     long idx_stride, long idx_off,
                     torch::Tensor gstack, long w_off, long b_off,
                     long M, long I, long O, long cw_off, long cb_off,
                     long F, long K, long IMG) {
  if (dw_kernel_for(M, I, O) != DwKernel::Small) {
    linear_bwd_dw(dZ, X, gstack, w_off, b_off, M, I, O);
    conv_pool_bwd_idx(dY, pidx, X_all, src_idx, idx_stride, idx_off,
                      gstack, cw_off, cb_off, M, F, K, IMG);
    return;
  }
  CHECK_DEV(dZ); CHECK_DEV(X); CHECK_DEV(dY); CHECK_DEV(X_all);
  CHECK_DEV(gstack);
  const long L = gstack.size(0), n = gstack.size(1);
  const long maxlen = X_all.size(1);
  TORCH_CHECK(K <= 7, "conv_pool_bwd supports kernel size <= 7");
  const int nchunk = conv_bwd_nchunk(M);
  const long gx = (I + 15) / 16, gy = (O + 15) / 16;
  const long n_dw = gx * gy * L;
  const long n_cv = L * F * nchunk;
  DISPATCH_FT(dZ, {
    dispatch_kmax(K, [&](auto kmax) {
      hipLaunchKernelGGL(
          (fmnist::dw_conv_bwd_k<scalar_t, decltype(kmax)::value>),
          dim3(n_dw + n_cv), dim3(256), 0, cur_stream(),
          dZ.data_ptr<scalar_t>(), X.data_ptr<scalar_t>(), w_off, b_off,
          (int)M, (int)I, (int)O, (int)gx, (int)gy, (int)n_dw,
          dY.data_ptr<scalar_t>(), pidx.data_ptr<unsigned char>(),
          X_all.data_ptr<scalar_t>(), cw_off, cb_off, (int)F, (int)K,
          (int)IMG, nchunk, src_idx.data_ptr<long>(), idx_stride,
          idx_off, maxlen, gstack.data_ptr<scalar_t>(), n);
    });
  });
  HIP_CHECK_LAST();
}

// fc_fwd_split_k's workspace: per device the partial-z1 slabs
// [tiles, S, 16, 64] and one int32 ticket per row tile. Owned here so
// the Python-visible calls need no extra argument and no per-call
// memset: the tickets are zero when allocated and every launch's
// reducer blocks leave them zero again. Grown on demand, never freed
// (torch tensors must not be destroyed after the runtime at exit).
struct FcSplitWs {
  torch::Tensor slabs, tickets;
  // one int32 ticket per node for the backward launch that carries the
  // primal step (dw_dx0_conv_bwd_k with STEP on), kept zero the same way
  torch::Tensor step_tickets;
};

FcSplitWs& fc_ws_of(const torch::Tensor& like) {
  static auto* ws = new std::map<int, FcSplitWs>();
  return (*ws)[like.get_device()];
}

FcSplitWs& fc_split_ws(const torch::Tensor& like, long slab_elems,
                       long tiles) {
  FcSplitWs& w = fc_ws_of(like);
  const long need = slab_elems * (long)like.element_size();
  if (!w.slabs.defined() || w.slabs.numel() < need) {
    w.slabs = torch::empty(
        {need}, like.options().dtype(torch::kUInt8));
  }
  if (!w.tickets.defined() || w.tickets.numel() < tiles) {
    w.tickets = torch::zeros(
        {tiles}, like.options().dtype(torch::kInt32));
  }
  return w;
}

// K slices per row tile of fc_fwd_split_k. 4 puts 128 blocks of 27
// MFMA k-steps on the chip at the MNIST shape (profiles/README.md has
// the sweep); NDTA_FC_SPLIT_S overrides it for such sweeps. Wide
// layers get more slices so that a slice's operand image fits LDS.
inline long fc_split_slices(long I, long elem_size) {
  static const long s_env = []() {
    const char* e = getenv("NDTA_FC_SPLIT_S");
    const long v = e ? atol(e) : 0;
    return v >= 1 && v <= 64 ? v : 4;
  }();
  const long lds_cap = 160 * 1024;
  const long ksteps = (I + 3) / 4;
  long S = s_env;
  while (fmnist::fc_split_lds_elems(4 * (int)((ksteps + S - 1) / S)) *
             elem_size > lds_cap) {
    ++S;
  }
  return S;
}

// Which kernels the fc block runs on. This is the only place the
// threshold is written. Split: fc_fwd_split_k + fc_dx0_k, while the
// split forward's grid (row tiles x slices, one block per CU: its
// operand image is ~100 KB of LDS) fits the chip in one wave of blocks.
// Past that the blocks queue behind each other and the one-launch
// fc_block_k, which already has a block for every other CU there, is
// faster: at 32 nodes x 64 rows (128 tiles, 512 split blocks) the
// split measured 4.9k rounds/s against 5.7k (profiles/README.md).
// NDTA_FC_SPLIT=0/1 forces one or the other for A/B runs.
enum class FcKernel { Split, OneLaunch };

inline FcKernel fc_kernel_for(long tiles, long S) {
  static const int force = []() {
    const char* e = getenv("NDTA_FC_SPLIT");
    return e ? (e[0] == '0' ? 0 : 1) : -1;
  }();
  if (force >= 0) return force ? FcKernel::Split : FcKernel::OneLaunch;
  return tiles * S <= 256 ? FcKernel::Split : FcKernel::OneLaunch;
}

// the fc block without fc1 dW/db (those are the caller's). Split: the
// split-K fc1 forward whose last-arriving slice block runs the fc2
// forward, the loss and the fc2 backward, then dX0 as a grid of its
// own (left out with want_dx0 = false, for a caller whose backward
// computes dX0 itself). OneLaunch: fc_block_k, which always writes dx0.
void fc_block_launch(torch::Tensor x0, torch::Tensor theta,
                     torch::Tensor Y_all, torch::Tensor idx,
                     long idx_stride, long idx_off, torch::Tensor grad,
                     torch::Tensor dx0, torch::Tensor dz1g,
                     c10::optional<torch::Tensor> loss, long w1_off,
                     long b1_off, long w2_off, long b2_off, long M,
                     long I, long H, long C, double loss_scale,
                     bool mask_dx0, bool want_dx0 = true) {
  CHECK_DEV(x0); CHECK_DEV(theta); CHECK_DEV(grad); CHECK_DEV(dx0);
  CHECK_DEV(dz1g);
  const long L = theta.size(0), n = theta.size(1);
  const long maxlen = Y_all.size(1);
  TORCH_CHECK(H >= 1 && H <= 64 && C >= 1 && C <= 16 && I >= 1 &&
              M >= 1, "fc_block: 1 <= H <= 64, 1 <= C <= 16");
  const long mtiles = (M + fmnist::FC_RT - 1) / fmnist::FC_RT;
  const long tiles = mtiles * L;
  const long S = fc_split_slices(I, x0.element_size());
  const long KS = 4 * (((I + 3) / 4 + S - 1) / S);
  const long KSP = fmnist::fc_split_ksp((int)KS);
  if (fc_kernel_for(tiles, S) == FcKernel::OneLaunch) {
    DISPATCH_FT(x0, {
      hipLaunchKernelGGL(fmnist::fc_block_k<scalar_t>,
          dim3(mtiles, 1, L), dim3(512), 0, cur_stream(),
          x0.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y_all.data_ptr<long>(), idx.data_ptr<long>(), idx_stride,
          idx_off, maxlen, grad.data_ptr<scalar_t>(),
          dx0.data_ptr<scalar_t>(), dz1g.data_ptr<scalar_t>(),
          opt_ptr<scalar_t>(loss),
          n, w1_off, b1_off, w2_off, b2_off, (int)M, (int)I, (int)H,
          (int)C, (scalar_t)loss_scale, mask_dx0 ? 1 : 0);
    });
    HIP_CHECK_LAST();
    return;
  }
  FcSplitWs& ws = fc_split_ws(x0, tiles * S * fmnist::FC_RT * 64, tiles);
  DISPATCH_FT(x0, {
    const size_t shmem =
        fmnist::fc_split_lds_elems((int)KS) * sizeof(scalar_t);
    hipLaunchKernelGGL(fmnist::fc_fwd_split_k<scalar_t>,
        dim3(tiles * S), dim3(256), shmem, cur_stream(),
        x0.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
        Y_all.data_ptr<long>(), idx.data_ptr<long>(), idx_stride,
        idx_off, maxlen, grad.data_ptr<scalar_t>(),
        dz1g.data_ptr<scalar_t>(), opt_ptr<scalar_t>(loss),
        reinterpret_cast<scalar_t*>(ws.slabs.data_ptr()),
        ws.tickets.data_ptr<int>(),
        n, w1_off, b1_off, w2_off, b2_off, (int)M, (int)I, (int)H,
        (int)C, (scalar_t)loss_scale, (int)mtiles, (int)S, (int)KS,
        (int)KSP);
    if (want_dx0) {
      hipLaunchKernelGGL(fmnist::fc_dx0_k<scalar_t>,
          dim3((I + 15) / 16, (M + 63) / 64, L), dim3(256), 0,
          cur_stream(),
          x0.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          dz1g.data_ptr<scalar_t>(), dx0.data_ptr<scalar_t>(),
          n, w1_off, (int)M, (int)I, (int)H, mask_dx0 ? 1 : 0);
    }
  });
  HIP_CHECK_LAST();
}

// the fc block: fc1+fc2 fwd, NLL, full fc backward (see fused_mnist.hip
// fc_fwd_split_k, fc_dx0_k). Caller pre-zeroes the grad stack.
void fc_block(torch::Tensor x0, torch::Tensor theta,
              torch::Tensor Y_all, torch::Tensor idx, long idx_stride,
              long idx_off, torch::Tensor grad, torch::Tensor dx0,
              torch::Tensor dz1g,
              c10::optional<torch::Tensor> loss, long w1_off,
              long b1_off, long w2_off, long b2_off, long M, long I,
              long H, long C, double loss_scale, bool mask_dx0) {
  fc_block_launch(x0, theta, Y_all, idx, idx_stride, idx_off, grad,
                  dx0, dz1g, loss, w1_off, b1_off, w2_off, b2_off, M, I,
                  H, C, loss_scale, mask_dx0);
  // fc1 dW/db from the exported dz1 (store-path kernel: overwrite,
  // no atomics)
  linear_bwd_dw(dz1g, x0, grad, w1_off, b1_off, M, I, H);
}

// Whether the backward of the conv -> fc1 model computes dX0 inside the
// merged launch (fused_mnist.hip dw_dx0_conv_bwd_k) instead of reading
// it from memory. This is the only place the condition is written: the
// fc block is on its split path (the one-launch fc_block_k writes dX0
// anyway), fc1's dW takes the Small kernel (the one the merged launches
// carry), a 16-column strip of I lies inside one filter, and K is one
// of the exact tap-loop sizes. NDTA_BWD_DX0=0 keeps the two launches
// (fc_dx0_k, dw_conv_bwd_k) for A/B runs.
inline bool bwd_dx0_fused(long L, long M, long I, long H, long F, long K,
                          long IMG, long elem_size) {
  static const bool off = []() {
    const char* e = getenv("NDTA_BWD_DX0");
    return e && e[0] == '0';
  }();
  if (off) return false;
  const long P = (IMG - (K - 1)) / 2;
  if (L < 1 || M < 1 || P < 1 || I != F * P * P) return false;
  const long tiles = (M + fmnist::FC_RT - 1) / fmnist::FC_RT * L;
  return fc_kernel_for(tiles, fc_split_slices(I, elem_size)) ==
             FcKernel::Split &&
         dw_kernel_for(M, I, H) == DwKernel::Small &&
         (P * P) % 16 == 0 && (K == 5 || K == 7) && H >= 1 && H <= 64;
}

bool bwd_dx0_fused_for(long L, long M, long I, long H, long F, long K,
                       long IMG, long elem_size) {
  return bwd_dx0_fused(L, M, I, H, F, K, IMG, elem_size);
}

// A DiNNO primal step's arguments, as fused_step_dual and fused_step
// take them; `dual`: the step carries the round's dual ascent.
struct StepArgs {
  c10::optional<torch::Tensor> remote;
  torch::Tensor offs, idx, deg, duals, s;
  c10::optional<torch::Tensor> m, v;
  double rho, lr, beta1, beta2, eps, wd;
  long step_t, mode;
  bool first_step, dual;
};

// today's step launch on theta, from a gradient in `grad`
void step_unfused(const StepArgs& st, torch::Tensor theta,
                  torch::Tensor grad);

// Whether the backward launch of the conv -> fc1 model also takes the
// DiNNO primal step that follows it (fused_mnist.hip dw_dx0_conv_bwd_k
// with STEP on), from theta_in into a second buffer theta_out. This is
// the only place the condition is written: the launch is the one
// bwd_dx0_fused chooses, the gradient is a plain [L, n] stack (nparts 1)
// and there are at most STEP_DUAL_LMAX local nodes, as for
// step_dual_fused. NDTA_BWD_STEP=0 keeps the step a launch of its own
// for A/B runs.
inline bool bwd_step_fused(long L, long M, long I, long H, long F, long K,
                           long IMG, long elem_size, long nparts) {
  static const bool off = []() {
    const char* e = getenv("NDTA_BWD_STEP");
    return e && e[0] == '0';
  }();
  return !off && nparts == 1 && L <= ew::STEP_DUAL_LMAX &&
         bwd_dx0_fused(L, M, I, H, F, K, IMG, elem_size);
}

bool bwd_step_fused_for(long L, long M, long I, long H, long F, long K,
                        long IMG, long elem_size, long nparts) {
  return bwd_step_fused(L, M, I, H, F, K, IMG, elem_size, nparts);
}

// the step's tensors against theta_in [L, n]; the kernel indexes all of
// them with theta's (l, e)
void check_bwd_step(const StepArgs& st, const torch::Tensor& theta_in,
                    const torch::Tensor& theta_out, long w2_off,
                    long b2_off, long H, long C) {
  const long L = theta_in.size(0), n = theta_in.size(1);
  const auto dt = theta_in.scalar_type();
  CHECK_DEV(theta_out);
  TORCH_CHECK(theta_out.scalar_type() == dt &&
                  theta_out.numel() == L * n &&
                  theta_out.data_ptr() != theta_in.data_ptr(),
              "bwd step: theta_out must be a second [L, n] buffer");
  for (const auto* t : {&st.duals, &st.s}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == dt && t->numel() == L * n,
                "bwd step: duals and s must be [L, n] of theta's dtype");
  }
  for (const auto* t : {&st.offs, &st.idx, &st.deg}) {
    TORCH_CHECK(t->is_cuda() && t->is_contiguous() &&
                    t->scalar_type() == torch::kInt,
                "bwd step: int32 offs, idx and deg expected");
  }
  TORCH_CHECK(st.offs.numel() == L + 1 && st.deg.numel() == L,
              "bwd step: offs [L+1] and deg [L] expected");
  for (const auto* t : {&st.remote, &st.m, &st.v}) {
    TORCH_CHECK(!t->has_value() ||
                    ((*t)->is_cuda() && (*t)->is_contiguous() &&
                     (*t)->scalar_type() == dt),
                "bwd step: remote, m and v must be contiguous on GPU, of "
                "theta's dtype");
  }
  TORCH_CHECK(!st.remote.has_value() || st.remote->numel() % n == 0,
              "bwd step: remote [R-L, n]");
  TORCH_CHECK(st.mode == 2 ||
                  (st.m.has_value() && st.v.has_value() &&
                   st.m->numel() == L * n && st.v->numel() == L * n),
              "bwd step: Adam modes need m and v [L, n]");
  TORCH_CHECK(C >= 1 && w2_off >= 0 && w2_off + C * H <= n &&
                  b2_off >= 0 && b2_off + C <= n,
              "bwd step: fc2 slices must lie inside [0, n)");
}

// fc1 dW/db + dX0 + gather-sourced conv dW/db in ONE launch. Caller has
// checked bwd_dx0_fused. With `step` (caller has checked bwd_step_fused)
// the launch also takes that primal step from theta into *theta_out;
// fc2's grad slices, which it then consumes, are [C, H] at w2_off and
// [C] at b2_off.
void launch_dw_dx0_conv_bwd(
    const torch::Tensor& dz1, const torch::Tensor& x0,
    const torch::Tensor& theta, const torch::Tensor& pidx,
    const torch::Tensor& X_all, const torch::Tensor& src_idx,
    long idx_stride, long idx_off, const torch::Tensor& gstack,
    long w1_off, long b1_off, long M, long I, long H, long cw_off,
    long cb_off, long F, long K, long IMG,
    const StepArgs* step = nullptr,
    const torch::Tensor* theta_out = nullptr, long w2_off = 0,
    long b2_off = 0, long C = 0) {
  CHECK_DEV(dz1); CHECK_DEV(x0); CHECK_DEV(theta); CHECK_DEV(pidx);
  CHECK_DEV(X_all); CHECK_DEV(src_idx); CHECK_DEV(gstack);
  const long L = gstack.size(0), n = gstack.size(1);
  const long maxlen = X_all.size(1);
  TORCH_CHECK(theta.size(0) == L && theta.size(1) == n,
              "theta and gstack must both be [L, n]");
  TORCH_CHECK(dz1.numel() >= L * M * H && x0.numel() >= L * M * I &&
                  pidx.numel() >= L * M * I,
              "dz1 [L*M, H], x0 and pidx [L*M, I] expected");
  TORCH_CHECK(w1_off >= 0 && w1_off + H * I <= n && b1_off >= 0 &&
                  b1_off + H <= n && cw_off >= 0 &&
                  cw_off + F * K * K <= n && cb_off >= 0 &&
                  cb_off + F <= n, "layer slices must lie inside [0, n)");
  TORCH_CHECK(X_all.numel() >= L * maxlen * IMG * IMG &&
                  idx_off >= 0 && idx_off + M <= idx_stride &&
                  src_idx.numel() >= L * idx_stride,
              "X_all [L, maxlen, IMG*IMG], src_idx [L, idx_stride]");
  const long gx = (I + 15) / 16, gy = (H + 15) / 16;
  const long n_dw = gx * gy * L;
  const long cv_gx = I / 16, cv_gy = (M + 63) / 64;
  const long n_cv = cv_gx * cv_gy * L;
  int* tickets = nullptr;
  if (step != nullptr) {
    TORCH_CHECK(theta_out != nullptr, "bwd step: theta_out missing");
    check_bwd_step(*step, theta, *theta_out, w2_off, b2_off, H, C);
    FcSplitWs& ws = fc_ws_of(theta);
    if (!ws.step_tickets.defined() || ws.step_tickets.numel() < L) {
      ws.step_tickets = torch::zeros(
          {std::max<long>(L, ew::STEP_DUAL_LMAX)},
          theta.options().dtype(torch::kInt32));
    }
    tickets = ws.step_tickets.data_ptr<int>();
  }
  DISPATCH_FT(dz1, {
    fmnist::bwd_step_t<scalar_t> sp{};
    if (step != nullptr) {
      const StepArgs& st = *step;
      sp.a = {theta.data_ptr<scalar_t>(),
              theta_out->data_ptr<scalar_t>(),
              opt_ptr<scalar_t>(st.remote), st.offs.data_ptr<int>(),
              st.idx.data_ptr<int>(), st.deg.data_ptr<int>(),
              st.duals.data_ptr<scalar_t>(), st.s.data_ptr<scalar_t>(),
              opt_ptr<scalar_t>(st.m), opt_ptr<scalar_t>(st.v),
              (scalar_t)st.rho, (scalar_t)st.lr, (scalar_t)st.beta1,
              (scalar_t)st.beta2, (scalar_t)st.eps, (scalar_t)st.wd,
              (scalar_t)(1.0 - std::pow(st.beta1, (double)st.step_t)),
              (scalar_t)(1.0 - std::pow(st.beta2, (double)st.step_t)),
              n, (int)L};
      sp.mode = (int)st.mode;
      sp.load_mv = (st.mode != 2 && !st.first_step) ? 1 : 0;
      sp.w2_off = w2_off;
      sp.b2_off = b2_off;
      sp.C = (int)C;
      sp.F = (int)F;
      sp.tickets = tickets;
    }
    const auto go = [&](auto step_c) {
      dispatch_kmax(K, [&](auto kmax) {
        hipLaunchKernelGGL(
            (fmnist::dw_dx0_conv_bwd_k<scalar_t, decltype(kmax)::value,
                                       decltype(step_c)::value>),
            dim3(n_dw + n_cv), dim3(256), 0, cur_stream(),
            dz1.data_ptr<scalar_t>(), x0.data_ptr<scalar_t>(), w1_off,
            b1_off, (int)M, (int)I, (int)H, (int)gx, (int)gy,
            theta.data_ptr<scalar_t>(), pidx.data_ptr<unsigned char>(),
            X_all.data_ptr<scalar_t>(), cw_off, cb_off, (int)IMG,
            (int)cv_gx, (int)cv_gy, (int)n_cv, src_idx.data_ptr<long>(),
            idx_stride, idx_off, maxlen, gstack.data_ptr<scalar_t>(), n,
            sp);
      });
    };
    if (step == nullptr) {
      go(std::integral_constant<int, fmnist::STEP_NONE>{});
    } else if (step->dual) {
      go(std::integral_constant<int, fmnist::STEP_DUAL>{});
    } else {
      go(std::integral_constant<int, fmnist::STEP_PLAIN>{});
    }
  });
  HIP_CHECK_LAST();
}

// The whole backward below the fc block from dz1: fc1 dW/db and conv
// dW/db, with dX0 = (dz1 @ W1) * relu'(x0) in between. One launch where
// bwd_dx0_fused says so; elsewhere fc_dx0_k into a scratch dX0, then
// dw_conv_bwd_idx. The conv slice of gstack is zero on entry.
void dw_dx0_conv_bwd_idx(torch::Tensor dz1, torch::Tensor x0,
                         torch::Tensor theta, torch::Tensor pidx,
                         torch::Tensor X_all, torch::Tensor src_idx,
                         long idx_stride, long idx_off,
                         torch::Tensor gstack, long w1_off, long b1_off,
                         long M, long I, long H, long cw_off,
                         long cb_off, long F, long K, long IMG) {
  const long L = gstack.size(0), n = gstack.size(1);
  if (bwd_dx0_fused(L, M, I, H, F, K, IMG, x0.element_size())) {
    launch_dw_dx0_conv_bwd(dz1, x0, theta, pidx, X_all, src_idx,
                           idx_stride, idx_off, gstack, w1_off, b1_off,
                           M, I, H, cw_off, cb_off, F, K, IMG);
    return;
  }
  CHECK_DEV(dz1); CHECK_DEV(x0); CHECK_DEV(theta);
  TORCH_CHECK(H >= 1 && H <= 64 && M >= 1 && I >= 1,
              "dw_dx0_conv_bwd_idx: 1 <= H <= 64");
  TORCH_CHECK(theta.size(0) == L && theta.size(1) == n &&
                  dz1.numel() >= L * M * H && x0.numel() >= L * M * I,
              "theta [L, n], dz1 [L*M, H], x0 [L*M, I] expected");
  torch::Tensor dx0 = torch::empty_like(x0);
  DISPATCH_FT(x0, {
    hipLaunchKernelGGL(fmnist::fc_dx0_k<scalar_t>,
        dim3((I + 15) / 16, (M + 63) / 64, L), dim3(256), 0,
        cur_stream(),
        x0.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
        dz1.data_ptr<scalar_t>(), dx0.data_ptr<scalar_t>(),
        n, w1_off, (int)M, (int)I, (int)H, 1);
  });
  HIP_CHECK_LAST();
  dw_conv_bwd_idx(dz1, x0, dx0, pidx, X_all, src_idx, idx_stride,
                  idx_off, gstack, w1_off, b1_off, M, I, H, cw_off,
                  cb_off, F, K, IMG);
}

// One native call per forward+backward of the conv -> fc1 -> fc2 -> NLL
// model on the index-sourced path: conv forward, the fc block (split-K
// forward + tail), then the merged fc1-dW + dX0 + conv-backward launch:
// three launches on the current stream, and dx0 is not touched. Where
// bwd_dx0_fused says no, the fc block writes dx0 (fc_dx0_k or
// fc_block_k) and dw_conv_bwd_idx reads it, as before. At ~10 us of
// host time per pybind call, separate calls no longer hid under the
// iteration's GPU time. Caller pre-zeroes the
// grad stack (and the loss slot).
void mnist_fwd_bwd(torch::Tensor X_all, torch::Tensor src_idx,
                   long idx_stride, long idx_off, torch::Tensor theta,
                   torch::Tensor Y_all, torch::Tensor x0,
                   torch::Tensor pidx, torch::Tensor grad,
                   torch::Tensor dx0, torch::Tensor dz1g,
                   c10::optional<torch::Tensor> loss, long cw_off,
                   long cb_off, long F, long K, long IMG, long w1_off,
                   long b1_off, long w2_off, long b2_off, long M, long I,
                   long H, long C, double loss_scale) {
  conv_pool_fwd_idx(X_all, src_idx, idx_stride, idx_off, theta, x0,
                    pidx, cw_off, cb_off, M, F, K, IMG);
  const bool fused = bwd_dx0_fused(theta.size(0), M, I, H, F, K, IMG,
                                   x0.element_size());
  fc_block_launch(x0, theta, Y_all, src_idx, idx_stride, idx_off, grad,
                  dx0, dz1g, loss, w1_off, b1_off, w2_off, b2_off, M, I,
                  H, C, loss_scale, true, !fused);
  if (fused) {
    launch_dw_dx0_conv_bwd(dz1g, x0, theta, pidx, X_all, src_idx,
                           idx_stride, idx_off, grad, w1_off, b1_off, M,
                           I, H, cw_off, cb_off, F, K, IMG);
  } else {
    dw_conv_bwd_idx(dz1g, x0, dx0, pidx, X_all, src_idx, idx_stride,
                    idx_off, grad, w1_off, b1_off, M, I, H, cw_off,
                    cb_off, F, K, IMG);
  }
}

// Whether the first primal step of a DiNNO round carries the round's
// dual ascent (elementwise.hip fused_step_dual_k) instead of following a
// dinno_dual_threg launch. This is the only place the condition is
// written: a plain [L, n] gradient (nparts 1; the megakernel's per-tile
// slabs keep the two launches) and at most STEP_DUAL_LMAX local nodes,
// which one block's threads cover. NDTA_STEP_DUAL=0 keeps the two
// launches for A/B runs.
inline bool step_dual_fused(long L, long nparts) {
  static const bool off = []() {
    const char* e = getenv("NDTA_STEP_DUAL");
    return e && e[0] == '0';
  }();
  return !off && nparts == 1 && L >= 1 && L <= ew::STEP_DUAL_LMAX;
}

bool step_dual_fused_for(long L, long nparts) {
  return step_dual_fused(L, nparts);
}

// columns per block of fused_step_dual_k (the block is columns x L
// threads): 64, so the MNIST model's n = 28,440 at L = 8 is 445 blocks of
// 512 threads, fused_step_k's thread count; 32 and 128 measured the same
// within the run-to-run spread (profiles/README.md).
constexpr int STEP_DUAL_COLS = 64;
static_assert(STEP_DUAL_COLS * ew::STEP_DUAL_LMAX <= ew::STEP_DUAL_THREADS,
              "a block of columns x L threads must fit");

// Dual ascent + first primal step of a DiNNO round: the results of
// dinno_dual_threg followed by fused_step (with penalty), bit for bit.
// One launch where step_dual_fused says so, else those two.
void fused_step_dual(torch::Tensor theta, torch::Tensor grad,
                     c10::optional<torch::Tensor> remote,
                     torch::Tensor offs, torch::Tensor idx,
                     torch::Tensor deg, torch::Tensor duals,
                     torch::Tensor s_out,
                     c10::optional<torch::Tensor> m,
                     c10::optional<torch::Tensor> v,
                     double rho, double lr, double beta1, double beta2,
                     double eps, double wd, long step_t, long mode,
                     bool first_step, long nparts, bool zero_grad) {
  CHECK_DEV(theta); CHECK_DEV(grad); CHECK_DEV(duals); CHECK_DEV(s_out);
  const long L = theta.size(0), n = theta.size(1);
  if (!step_dual_fused(L, nparts)) {
    dinno_dual_threg(theta, remote, offs, idx, duals, s_out, rho);
    fused_step(theta, grad, duals, s_out, deg, m, v, rho, lr, beta1,
               beta2, eps, wd, step_t, mode, first_step, nparts,
               zero_grad);
    return;
  }
  TORCH_CHECK(grad.numel() == L * n && duals.numel() == L * n &&
                  s_out.numel() == L * n,
              "fused_step_dual: grad, duals and s must be [L, n]");
  CHECK_DEV(offs); CHECK_DEV(idx); CHECK_DEV(deg);
  TORCH_CHECK(offs.scalar_type() == torch::kInt &&
                  idx.scalar_type() == torch::kInt &&
                  deg.scalar_type() == torch::kInt &&
                  offs.numel() == L + 1 && deg.numel() == L,
              "fused_step_dual: int32 offs [L+1], idx and deg [L] expected");
  for (const auto* t : {&remote, &m, &v}) {
    TORCH_CHECK(!t->has_value() ||
                    ((*t)->is_cuda() && (*t)->is_contiguous() &&
                     (*t)->scalar_type() == theta.scalar_type()),
                "fused_step_dual: remote, m and v must be contiguous on "
                "GPU, of theta's dtype");
  }
  TORCH_CHECK(grad.scalar_type() == theta.scalar_type() &&
                  duals.scalar_type() == theta.scalar_type() &&
                  s_out.scalar_type() == theta.scalar_type() &&
                  (!remote.has_value() || remote->numel() % n == 0),
              "fused_step_dual: grad, duals, s of theta's dtype; remote "
              "[R-L, n]");
  TORCH_CHECK(mode == 2 || (m.has_value() && v.has_value() &&
                            m->numel() == L * n && v->numel() == L * n),
              "fused_step_dual: Adam modes need m and v [L, n]");
  const int cols = STEP_DUAL_COLS;
  DISPATCH_FT(theta, {
    const scalar_t bc1 =
        (scalar_t)(1.0 - std::pow(beta1, (double)step_t));
    const scalar_t bc2 =
        (scalar_t)(1.0 - std::pow(beta2, (double)step_t));
    dispatch_mode_pen(mode, first_step, [&](auto mode_c, auto first_c) {
      hipLaunchKernelGGL(
          (ew::fused_step_dual_k<scalar_t, decltype(mode_c)::value,
                                 decltype(first_c)::value>),
          dim3(grid_1d(n, cols)), dim3(cols, L), 0, cur_stream(),
          theta.data_ptr<scalar_t>(), grad.data_ptr<scalar_t>(),
          opt_ptr<scalar_t>(remote), offs.data_ptr<int>(),
          idx.data_ptr<int>(), deg.data_ptr<int>(),
          duals.data_ptr<scalar_t>(), s_out.data_ptr<scalar_t>(),
          opt_ptr<scalar_t>(m), opt_ptr<scalar_t>(v),
          (scalar_t)rho, (scalar_t)lr, (scalar_t)beta1,
          (scalar_t)beta2, (scalar_t)eps, (scalar_t)wd, bc1, bc2,
          n, (int)L, zero_grad ? 1 : 0);
    });
  });
  HIP_CHECK_LAST();
}

void step_unfused(const StepArgs& st, torch::Tensor theta,
                  torch::Tensor grad) {
  if (st.dual) {
    fused_step_dual(theta, grad, st.remote, st.offs, st.idx, st.deg,
                    st.duals, st.s, st.m, st.v, st.rho, st.lr, st.beta1,
                    st.beta2, st.eps, st.wd, st.step_t, st.mode,
                    st.first_step, 1, true);
  } else {
    fused_step(theta, grad, st.duals, st.s, st.deg, st.m, st.v, st.rho,
               st.lr, st.beta1, st.beta2, st.eps, st.wd, st.step_t,
               st.mode, st.first_step, 1, true);
  }
}

// dw_dx0_conv_bwd_idx followed by the DiNNO primal step on its gradient
// (fused_step_dual where `dual`, else fused_step with the penalty; the
// grad stack is cleared as it is consumed). Where bwd_step_fused says so
// this is ONE launch that reads theta_in and writes the stepped theta to
// theta_out, and the call returns true; the fc1 slice of gstack is then
// never written. Elsewhere the two launches run as before, theta_in is
// stepped in place, theta_out is not touched and the call returns false.
// The conv and fc2 slices of gstack hold this iteration's sums on entry
// (fc2's complete, conv's zero).
bool dw_dx0_conv_bwd_step_idx(
    torch::Tensor dz1, torch::Tensor x0, torch::Tensor theta_in,
    torch::Tensor theta_out, torch::Tensor pidx, torch::Tensor X_all,
    torch::Tensor src_idx, long idx_stride, long idx_off,
    torch::Tensor gstack, long w1_off, long b1_off, long M, long I,
    long H, long cw_off, long cb_off, long F, long K, long IMG,
    long w2_off, long b2_off, long C,
    c10::optional<torch::Tensor> remote, torch::Tensor offs,
    torch::Tensor idx, torch::Tensor deg, torch::Tensor duals,
    torch::Tensor s, c10::optional<torch::Tensor> m,
    c10::optional<torch::Tensor> v, double rho, double lr, double beta1,
    double beta2, double eps, double wd, long step_t, long mode,
    bool first_step, bool dual) {
  const StepArgs st{remote, offs, idx, deg, duals, s, m, v, rho, lr,
                    beta1, beta2, eps, wd, step_t, mode, first_step, dual};
  if (bwd_step_fused(theta_in.size(0), M, I, H, F, K, IMG,
                     x0.element_size(), 1)) {
    launch_dw_dx0_conv_bwd(dz1, x0, theta_in, pidx, X_all, src_idx,
                           idx_stride, idx_off, gstack, w1_off, b1_off,
                           M, I, H, cw_off, cb_off, F, K, IMG, &st,
                           &theta_out, w2_off, b2_off, C);
    return true;
  }
  dw_dx0_conv_bwd_idx(dz1, x0, theta_in, pidx, X_all, src_idx, idx_stride,
                      idx_off, gstack, w1_off, b1_off, M, I, H, cw_off,
                      cb_off, F, K, IMG);
  step_unfused(st, theta_in, gstack);
  return false;
}

// mnist_fwd_bwd on theta_in followed by the DiNNO primal step, as one
// native call: three launches where bwd_step_fused says so (the backward
// launch carries the step and writes theta_out; returns true), else
// mnist_fwd_bwd's launches and the step launch on theta_in (theta_out is
// not touched; returns false). Either way the grad stack is all zeros
// afterwards if it was on entry. No loss output: the caller of a round
// that tracks the training loss keeps the separate calls.
bool mnist_fwd_bwd_step(
    torch::Tensor X_all, torch::Tensor src_idx, long idx_stride,
    long idx_off, torch::Tensor theta_in, torch::Tensor theta_out,
    torch::Tensor Y_all, torch::Tensor x0, torch::Tensor pidx,
    torch::Tensor grad, torch::Tensor dx0, torch::Tensor dz1g,
    c10::optional<torch::Tensor> loss, long cw_off, long cb_off, long F,
    long K, long IMG, long w1_off, long b1_off, long w2_off, long b2_off,
    long M, long I, long H, long C, double loss_scale,
    c10::optional<torch::Tensor> remote, torch::Tensor offs,
    torch::Tensor idx, torch::Tensor deg, torch::Tensor duals,
    torch::Tensor s, c10::optional<torch::Tensor> m,
    c10::optional<torch::Tensor> v, double rho, double lr, double beta1,
    double beta2, double eps, double wd, long step_t, long mode,
    bool first_step, bool dual) {
  const StepArgs st{remote, offs, idx, deg, duals, s, m, v, rho, lr,
                    beta1, beta2, eps, wd, step_t, mode, first_step, dual};
  if (!bwd_step_fused(theta_in.size(0), M, I, H, F, K, IMG,
                      x0.element_size(), 1)) {
    mnist_fwd_bwd(X_all, src_idx, idx_stride, idx_off, theta_in, Y_all,
                  x0, pidx, grad, dx0, dz1g, loss, cw_off, cb_off, F, K,
                  IMG, w1_off, b1_off, w2_off, b2_off, M, I, H, C,
                  loss_scale);
    step_unfused(st, theta_in, grad);
    return false;
  }
  conv_pool_fwd_idx(X_all, src_idx, idx_stride, idx_off, theta_in, x0,
                    pidx, cw_off, cb_off, M, F, K, IMG);
  fc_block_launch(x0, theta_in, Y_all, src_idx, idx_stride, idx_off, grad,
                  dx0, dz1g, loss, w1_off, b1_off, w2_off, b2_off, M, I,
                  H, C, loss_scale, true, false);
  launch_dw_dx0_conv_bwd(dz1g, x0, theta_in, pidx, X_all, src_idx,
                         idx_stride, idx_off, grad, w1_off, b1_off, M, I,
                         H, cw_off, cb_off, F, K, IMG, &st, &theta_out,
                         w2_off, b2_off, C);
  return true;
}

#ifdef NDTA_FC_PHASE_CLOCK
// diagnostic build only: [blocks, 8] wall_clock64 stamps of the last
// fc_block launch (see fused_mnist.hip FC_STAMP)
torch::Tensor fc_phase_clock() {
  auto t = torch::zeros({fmnist::FC_CLK_BLOCKS, 8}, torch::kLong);
  const hipError_t err = hipMemcpyFromSymbol(
      t.data_ptr(), HIP_SYMBOL(fmnist::fc_phase_stamps),
      sizeof(unsigned long long) * fmnist::FC_CLK_BLOCKS * 8);
  TORCH_CHECK(err == hipSuccess, "fc_phase_clock: ",
              hipGetErrorString(err));
  return t;
}
#endif

// consensus-error metric: normalized pairwise distances + distance to
// the normalized mean (reference dist_mnist_problem.py:152-175) on the
// all-gathered [N, n] stack — returns (D [N,N], Dm [N,1])
std::vector<torch::Tensor> consensus_cdist(torch::Tensor stack) {
  CHECK_DEV(stack);
  const long N = stack.size(0), n = stack.size(1);
  auto opts = stack.options();
  auto norms = torch::empty({N}, opts);
  auto D = torch::empty({N, N}, opts);
  auto mean = torch::empty({n}, opts);
  auto Dm = torch::empty({N, 1}, opts);
  DISPATCH_FT(stack, {
    hipLaunchKernelGGL(ew::row_norms_k<scalar_t>,
        dim3(N), dim3(ew::BLOCK), 0, cur_stream(),
        stack.data_ptr<scalar_t>(), norms.data_ptr<scalar_t>(), n);
    hipLaunchKernelGGL(ew::pairwise_normed_dist_k<scalar_t>,
        dim3(N * N), dim3(ew::BLOCK), 0, cur_stream(),
        stack.data_ptr<scalar_t>(), norms.data_ptr<scalar_t>(),
        D.data_ptr<scalar_t>(), N, n);
    hipLaunchKernelGGL(ew::normed_mean_k<scalar_t>,
        dim3(grid_1d(n)), dim3(ew::BLOCK), 0, cur_stream(),
        stack.data_ptr<scalar_t>(), norms.data_ptr<scalar_t>(),
        mean.data_ptr<scalar_t>(), N, n);
    hipLaunchKernelGGL(ew::dist_to_mean_k<scalar_t>,
        dim3(N), dim3(ew::BLOCK), 0, cur_stream(),
        stack.data_ptr<scalar_t>(), norms.data_ptr<scalar_t>(),
        mean.data_ptr<scalar_t>(), Dm.data_ptr<scalar_t>(), n);
  });
  HIP_CHECK_LAST();
  return {D, Dm};
}

// ----------------------------------------------------------- chains --
// One pybind call per forward / backward pass instead of one per
// layer-op: host profiling (BENCH r2b timing_breakdown) measured
// ~10 us of python+pybind overhead PER ext call, making the host the
// bottleneck of the MNIST round (~23 calls x 10 us vs ~115 us of GPU
// work). These chains launch exactly the kernels the python loops in
// ops/stacked.py forward()/backward() launched, in the same order.
//
// spec: CPU int64 [nl, 7] rows = (kind, w_off, b_off, in_dim,
//       out_dim, act, ksize); kind 0 = linear, 1 = conv_pool;
//       act = ACT_* id (5 = logsoftmax -> linear 'none' + row kernel).
//       Written by StackedEngine._chain_meta() in ops/stacked.py.
// scales: CPU float64 [nl] activation scales.
enum SpecCol {
  SP_KIND, SP_W_OFF, SP_B_OFF, SP_IN_DIM, SP_OUT_DIM, SP_ACT, SP_KSIZE,
  SP_NCOLS
};

void fwd_chain(torch::Tensor spec, torch::Tensor scales,
               c10::optional<torch::Tensor> X_all,
               c10::optional<torch::Tensor> idx, long idx_stride,
               long idx_off,
               torch::Tensor xb, torch::Tensor theta,
               std::vector<torch::Tensor> acts,
               std::vector<c10::optional<torch::Tensor>> zs,
               std::vector<c10::optional<torch::Tensor>> idxs,
               c10::optional<torch::Tensor> logp, long M,
               bool train_skip_logp) {
  TORCH_CHECK(spec.device().is_cpu() && scales.device().is_cpu() &&
                  spec.size(1) == SP_NCOLS,
              "spec [nl, 7] / scales must be CPU tensors");
  const auto sp = spec.accessor<long, 2>();
  const auto sc = scales.accessor<double, 1>();
  const long nl = spec.size(0);
  if (X_all.has_value()) {
    gather_batch(*X_all, *idx, xb, idx_stride, idx_off);
  }
  torch::Tensor cur = xb;
  for (long li = 0; li < nl; ++li) {
    const long kind = sp[li][SP_KIND], w_off = sp[li][SP_W_OFF],
               b_off = sp[li][SP_B_OFF], in_dim = sp[li][SP_IN_DIM],
               out_dim = sp[li][SP_OUT_DIM], act = sp[li][SP_ACT],
               ksize = sp[li][SP_KSIZE];
    torch::Tensor out = acts[li];
    if (kind == 1) {
      conv_pool_fwd(cur, theta, out, *idxs[li], w_off, b_off, M,
                    out_dim, ksize, in_dim);
      cur = out;
    } else if (act == ACT_LOGSOFTMAX) {
      linear_fwd(cur, theta, out, c10::nullopt, w_off, b_off, M,
                 in_dim, out_dim, ACT_NONE, 1.0);
      if (!train_skip_logp) {
        logsoftmax(out, *logp, out_dim);
        cur = *logp;
      } else {
        cur = out;
      }
    } else {
      linear_fwd(cur, theta, out, zs[li], w_off, b_off, M, in_dim,
                 out_dim, act, sc[li]);
      cur = out;
    }
  }
}

// Backward chain: loss head + layer loop, mirroring
// ops/stacked.py StackedEngine.backward.
// loss_kind: 0 = fused NLL (classification), 1 = BCE+sigmoid,
//            2 = MSE, 3 = L1.
void bwd_chain(torch::Tensor spec, torch::Tensor scales,
               torch::Tensor xb, torch::Tensor theta,
               torch::Tensor grad,
               std::vector<torch::Tensor> acts,
               std::vector<c10::optional<torch::Tensor>> zs,
               std::vector<torch::Tensor> dzs,
               std::vector<c10::optional<torch::Tensor>> idxs,
               long loss_kind,
               c10::optional<torch::Tensor> Y_all,
               c10::optional<torch::Tensor> idx,
               c10::optional<torch::Tensor> graph_offs, long pit,
               long idx_stride, long idx_off,
               c10::optional<torch::Tensor> yb,
               c10::optional<torch::Tensor> loss, double loss_scale,
               long M, long zero_mode) {
  TORCH_CHECK(spec.device().is_cpu() && scales.device().is_cpu() &&
                  spec.size(1) == SP_NCOLS,
              "spec [nl, 7] / scales must be CPU tensors");
  const auto sp = spec.accessor<long, 2>();
  const auto sc = scales.accessor<double, 1>();
  const long nl = spec.size(0);
  if (zero_mode == 1) {
    grad.zero_();
  } else if (zero_mode == 2) {
    // conv slices only (kind == 1 rows)
    for (long li = 0; li < nl; ++li) {
      if (sp[li][SP_KIND] == 1) {
        const long F = sp[li][SP_OUT_DIM], K = sp[li][SP_KSIZE];
        const long w_off = sp[li][SP_W_OFF];
        grad.index({torch::indexing::Slice(),
                    torch::indexing::Slice(w_off, w_off + F * K * K + F)})
            .zero_();
      }
    }
  }
  if (loss.has_value()) loss->zero_();

  const long last = nl - 1;
  torch::Tensor dz = dzs[last];
  if (loss_kind == 0) {
    nll_fused(acts[last], *Y_all, *idx, dz, loss, graph_offs, pit,
              idx_stride, idx_off, sp[last][SP_OUT_DIM], M, loss_scale);
  } else if (loss_kind == 1) {
    bce_bwd(acts[last], *yb, dz, loss, M, loss_scale);
  } else {
    auto dy = torch::empty_like(dz);
    regression_bwd(acts[last], *yb, dy, loss, M, loss_scale,
                   loss_kind == 2 ? 0 : 1);
    act_grad(dy, acts[last], c10::nullopt, dz, sp[last][SP_ACT],
             sc[last]);
  }

  for (long li = last; li >= 0; --li) {
    const long kind = sp[li][SP_KIND], w_off = sp[li][SP_W_OFF],
               b_off = sp[li][SP_B_OFF], in_dim = sp[li][SP_IN_DIM],
               out_dim = sp[li][SP_OUT_DIM];
    torch::Tensor below = li > 0 ? acts[li - 1] : xb;
    dz = dzs[li];
    if (kind == 1) {
      conv_pool_bwd(dz, *idxs[li], below, grad, w_off, b_off, M,
                    out_dim, sp[li][SP_KSIZE], in_dim);
      continue;  // conv is the first layer: no dX
    }
    linear_bwd_dw(dz, below, grad, w_off, b_off, M, in_dim, out_dim);
    if (li > 0) {
      const long act_b_raw = sp[li - 1][SP_ACT];
      const long act_b =
          (act_b_raw == ACT_NONE || act_b_raw == ACT_LOGSOFTMAX)
              ? 0 : act_b_raw;
      c10::optional<torch::Tensor> xb2;
      long wb_off = 0, bb_off = 0, ib = 0;
      if (act_b == ACT_SIN_RELU && !zs[li - 1].has_value()) {
        xb2 = li - 1 > 0 ? acts[li - 2] : xb;
        wb_off = sp[li - 1][SP_W_OFF];
        bb_off = sp[li - 1][SP_B_OFF];
        ib = sp[li - 1][SP_IN_DIM];
      }
      linear_bwd_dx(
          dz, theta, dzs[li - 1],
          act_b ? c10::optional<torch::Tensor>(acts[li - 1])
                : c10::nullopt,
          zs[li - 1], act_b, sc[li - 1], w_off, M, in_dim, out_dim,
          xb2, wb_off, bb_off, ib);
    }
  }
}

// keyed bijection of [0, n) written into `out` (int64, contiguous):
// the online-density sampler's shuffle (ops/stacked.py
// _OnlineWindowSampler) — one launch instead of a device randperm's
// rocprim sort chain
void feistel_perm(torch::Tensor out, long n, long lb, long key) {
  CHECK_DEV(out);
  TORCH_CHECK(out.scalar_type() == torch::kLong,
              "feistel_perm: out must be int64");
  TORCH_CHECK(out.numel() >= n, "feistel_perm: out too small");
  int bits = 1;
  while ((1L << bits) < n) ++bits;
  const int hb = std::max(1, (bits + 1) / 2);
  hipLaunchKernelGGL(ew::feistel_perm_k,
      dim3(grid_1d(n)), dim3(ew::BLOCK), 0, cur_stream(),
      out.data_ptr<long>(), n, lb, (unsigned long long)key, hb);
  HIP_CHECK_LAST();
}

}  // namespace

PYBIND11_MODULE(TORCH_EXTENSION_NAME, mod) {
  mod.def("dinno_dual_threg", &dinno_dual_threg);
  mod.def("mix_rows", &mix_rows);
  mod.def("dsgt_mix", &dsgt_mix);
  mod.def("dsgt_y_update", &dsgt_y_update);
  mod.def("fused_step", &fused_step);
  mod.def("axpy", &axpy);
  mod.def("reduce_parts", &reduce_parts);
  mod.def("gather_batch", &gather_batch);
  mod.def("gather_batch_dev", &gather_batch_dev);
  mod.def("dinno_dual_threg_sched", &dinno_dual_threg_sched);
  mod.def("fused_step_sched", &fused_step_sched);
  mod.def("gather_targets", &gather_targets);
  mod.def("linear_fwd", &linear_fwd);
  mod.def("act_grad", &act_grad);
  mod.def("linear_bwd_dx", &linear_bwd_dx);
  mod.def("linear_bwd_dw", &linear_bwd_dw);
  mod.def("dw_accumulates", &dw_accumulates);
  mod.def("conv_pool_fwd", &conv_pool_fwd);
  mod.def("conv_pool_bwd", &conv_pool_bwd);
  mod.def("conv_pool_fwd_idx", &conv_pool_fwd_idx);
  mod.def("conv_pool_bwd_idx", &conv_pool_bwd_idx);
  mod.def("logsoftmax", &logsoftmax);
  mod.def("nll_bwd", &nll_bwd);
  mod.def("nll_fused", &nll_fused);
  mod.def("mnist_train_step", &mnist_train_step);
  mod.def("bce_bwd", &bce_bwd);
  mod.def("regression_bwd", &regression_bwd);
  mod.def("ppo_loss_bwd", &ppo_loss_bwd);
  // the trailing optional outputs/inputs default to None, so the
  // positional calls from before they existed keep working
  namespace py = pybind11;
  mod.def("ppo_rollout", &ppo_rollout, py::arg("theta"),
          py::arg("in_dims"), py::arg("out_dims"), py::arg("w_offs"),
          py::arg("b_offs"), py::arg("act_ids"), py::arg("resets"),
          py::arg("obst"), py::arg("eps"), py::arg("obs"),
          py::arg("acts"), py::arg("logp"), py::arg("rews"),
          py::arg("rtgs"), py::arg("ep_rew"), py::arg("M"),
          py::arg("ep_len"), py::arg("cov"), py::arg("gamma"),
          py::arg("envp"), py::arg("last_obs") = py::none());
  mod.def("ppo_gae", &ppo_gae, py::arg("v"), py::arg("rews"),
          py::arg("rew_stride"), py::arg("adv"), py::arg("ret"),
          py::arg("M"), py::arg("ep_len"), py::arg("gamma"),
          py::arg("lam"), py::arg("v_last") = py::none());
  mod.def("feistel_perm", &feistel_perm);
  mod.def("consensus_cdist", &consensus_cdist);
  mod.def("fc_block", &fc_block);
  mod.def("dw_conv_bwd_idx", &dw_conv_bwd_idx);
  mod.def("mnist_fwd_bwd", &mnist_fwd_bwd);
  mod.def("dw_dx0_conv_bwd_idx", &dw_dx0_conv_bwd_idx);
  mod.def("bwd_dx0_fused_for", &bwd_dx0_fused_for);
  mod.def("step_dual_fused_for", &step_dual_fused_for);
  mod.def("fused_step_dual", &fused_step_dual);
  mod.def("bwd_step_fused_for", &bwd_step_fused_for);
  mod.def("dw_dx0_conv_bwd_step_idx", &dw_dx0_conv_bwd_step_idx);
  mod.def("mnist_fwd_bwd_step", &mnist_fwd_bwd_step);
#ifdef NDTA_FC_PHASE_CLOCK
  mod.def("fc_phase_clock", &fc_phase_clock);
#endif
  mod.def("fwd_chain", &fwd_chain);
  mod.def("bwd_chain", &bwd_chain);
}

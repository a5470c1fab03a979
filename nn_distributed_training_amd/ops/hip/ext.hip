// Torch extension entry: dispatch + launch for the CDNA4 kernel library.
// Single translation unit (the kernel files are header-style templates).

#include <torch/extension.h>

#include "common.h"
#include "elementwise.hip"
#include "gemm.hip"
#include "gemm_mfma.hip"
#include "gemm_bf16.hip"
#include "gemm_bf16_act.hip"
#include "mlp_fused.hip"
#include "conv.hip"
#include "losses.hip"
#include "rollout.hip"
#include "advantage.hip"
#include "fused_mnist.hip"
#include "ppo_fused.hip"
#include "mlp_grad_fused.hip"
#include "eval.hip"
#include "mlp_eval.hip"

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
// gemm_prec of the linear ops: 0 = native (the tensor's own dtype on
// the f32/f64 MFMA), 1 = bf16 operands with fp32 accumulation on the
// bf16 MFMA (gemm_bf16.hip). This is the only place the bf16 choice is
// written: it holds for fp32 tensors where the layer shape meets the
// op's MFMA threshold (mfma_shape: use_mfma in linear_fwd /
// linear_bwd_dx, Direct or Mfma from dw_kernel_for in linear_bwd_dw);
// every other shape takes the kernel it takes natively.
inline bool use_bf16_gemm(long gemm_prec, const torch::Tensor& t,
                          bool mfma_shape) {
  TORCH_CHECK(gemm_prec == 0 || gemm_prec == 1,
              "gemm_prec must be 0 (native) or 1 (bf16)");
  TORCH_CHECK(gemm_prec == 0 || t.scalar_type() == torch::kFloat,
              "gemm_prec = 1 (bf16 operands) needs fp32 tensors");
  return gemm_prec == 1 && mfma_shape;
}

// MFMA pays only when M fills the 64-row tiles across the chip;
// small-M layers (MNIST fc, per-node B=64) stay on the VALU kernels.
// I must be even for the 16-byte staging loads (vec2 alignment).
inline bool fwd_mfma_shape(long M, long I, long O) {
  return M >= 128 && O >= 16 && I >= 8 && I % 2 == 0;
}

// the register-resident encode kernel's shapes (encode_fwd_k)
inline bool fwd_encode_shape(long M, long I, long O) {
  return !fwd_mfma_shape(M, I, O) && I <= 4 && M >= 1024 && O >= 64 &&
         O <= 1024 && O % 64 == 0;
}

inline bool dx_mfma_shape(long M, long I, long O) {
  return M >= 128 && I >= 16 && O >= 8 && I % 2 == 0 && O % 2 == 0;
}

inline bool is_bf16(const torch::Tensor& t) {
  return t.scalar_type() == torch::kBFloat16;
}

// A bf16 X or Y: the activation-storage kernels of gemm_bf16_act.hip.
// The storage type comes from the tensors; a shape, activation or Z
// stash those kernels do not take is an error, never another path.
void linear_fwd_act_bf16(const torch::Tensor& X, const torch::Tensor& theta,
                         torch::Tensor& Y,
                         const c10::optional<torch::Tensor>& Z, long w_off,
                         long b_off, long M, long I, long O, long act,
                         double scale, long gemm_prec) {
  const bool xb = is_bf16(X), yb = is_bf16(Y);
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(gemm_prec == 1 && theta.scalar_type() == torch::kFloat,
              "bf16 activation storage needs gemm_prec = 1 and an fp32 "
              "parameter stack");
  TORCH_CHECK((xb || X.scalar_type() == torch::kFloat) &&
                  (yb || Y.scalar_type() == torch::kFloat),
              "bf16 activation storage: X and Y must be bf16 or fp32");
  TORCH_CHECK(!Z.has_value(),
              "bf16 activation storage: a layer with a Z stash keeps "
              "fp32 storage");
  TORCH_CHECK(X.is_contiguous() && Y.is_contiguous() &&
                  X.numel() == L * M * I && Y.numel() == L * M * O,
              "bf16 activation storage: X [L*M, I], Y [L*M, O] contiguous");
  float* th = theta.data_ptr<float>();
  if (!xb && fwd_encode_shape(M, I, O)) {
    const long blocks = std::min<long>(M, 8192);
    dim3 grid(blocks, 1, L);
    auto launch_enc = [&](auto ik_tag) {
      constexpr int IK = decltype(ik_tag)::value;
      hipLaunchKernelGGL((gbf16a::encode_bf16_k<IK>), grid, dim3((int)O),
          0, cur_stream(), X.data_ptr<float>(), th,
          reinterpret_cast<__bf16*>(Y.data_ptr()), n, w_off, b_off,
          (int)M, (int)O, (int)act, (float)scale);
    };
    if (I == 1) launch_enc(std::integral_constant<int, 1>{});
    else if (I == 2) launch_enc(std::integral_constant<int, 2>{});
    else if (I == 3) launch_enc(std::integral_constant<int, 3>{});
    else launch_enc(std::integral_constant<int, 4>{});
    HIP_CHECK_LAST();
    return;
  }
  TORCH_CHECK(fwd_mfma_shape(M, I, O),
              "bf16 activation storage: forward needs an MFMA shape "
              "(M >= 128, O >= 16, I >= 8, I even) or the encode shape, "
              "got M=", M, " I=", I, " O=", O);
  TORCH_CHECK(!xb || I % 8 == 0,
              "bf16 activation storage: a bf16 X needs I % 8 == 0");
  TORCH_CHECK(!yb || O % 8 == 0,
              "bf16 activation storage: a bf16 Y needs O % 8 == 0");
  dim3 grid((O + 63) / 64, (M + 63) / 64, L);
  auto launch = [&](auto xb_tag, auto yb_tag) {
    hipLaunchKernelGGL(
        (gbf16a::act_fwd_k<decltype(xb_tag)::value,
                           decltype(yb_tag)::value>),
        grid, dim3(256), 0, cur_stream(), X.data_ptr(), th, Y.data_ptr(),
        n, w_off, b_off, (int)M, (int)I, (int)O, (int)act, (float)scale);
  };
  if (xb && yb) launch(std::true_type{}, std::true_type{});
  else if (xb) launch(std::true_type{}, std::false_type{});
  else launch(std::false_type{}, std::true_type{});
  HIP_CHECK_LAST();
}

void linear_fwd(torch::Tensor X, torch::Tensor theta, torch::Tensor Y,
                c10::optional<torch::Tensor> Z, long w_off, long b_off,
                long M, long I, long O, long act, double scale,
                long gemm_prec = 0) {
  CHECK_DEV(X); CHECK_DEV(theta); CHECK_DEV(Y);
  if (is_bf16(X) || is_bf16(Y)) {
    linear_fwd_act_bf16(X, theta, Y, Z, w_off, b_off, M, I, O, act, scale,
                        gemm_prec);
    return;
  }
  const long L = theta.size(0), n = theta.size(1);
  const bool use_mfma = fwd_mfma_shape(M, I, O);
  if (use_bf16_gemm(gemm_prec, theta, use_mfma)) {
    dim3 grid((O + 63) / 64, (M + 63) / 64, L);
    hipLaunchKernelGGL(gbf16::bf16_fwd_k, grid, dim3(256), 0,
        cur_stream(), X.data_ptr<float>(), theta.data_ptr<float>(),
        Y.data_ptr<float>(), opt_ptr<float>(Z), n, w_off, b_off,
        (int)M, (int)I, (int)O, (int)act, (float)scale);
    HIP_CHECK_LAST();
    return;
  }
  DISPATCH_FT(X, {
    auto zp = opt_ptr<scalar_t>(Z);
    if (use_mfma) {
      dim3 grid((O + 63) / 64, (M + 63) / 64, L);
      hipLaunchKernelGGL(gmfma::mfma_fwd_k<scalar_t>,
          grid, dim3(256), 0, cur_stream(),
          X.data_ptr<scalar_t>(), theta.data_ptr<scalar_t>(),
          Y.data_ptr<scalar_t>(), zp, n, w_off, b_off,
          (int)M, (int)I, (int)O, (int)act, (scalar_t)scale);
    } else if (fwd_encode_shape(M, I, O)) {
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
                   long wb_off, long bb_off, long Ib,
                   long gemm_prec = 0) {
  CHECK_DEV(dZ); CHECK_DEV(dX);
  const long L = theta.size(0), n = theta.size(1);
  const bool use_mfma = dx_mfma_shape(M, I, O);
  TORCH_CHECK(act_below == 0 || Yb.has_value(), "act_below needs Yb");
  TORCH_CHECK(!Xb2.has_value() || Ib <= 4,
              "z-recompute supports below-layer in_dim <= 4");
  if (Yb.has_value() && is_bf16(*Yb)) {
    // bf16 activation storage (gemm_bf16_act.hip): the mask comes from
    // the bf16 bits; what act_dx_k does not take is an error
    CHECK_DEV(*Yb);
    TORCH_CHECK(gemm_prec == 1 && theta.scalar_type() == torch::kFloat &&
                    dZ.scalar_type() == torch::kFloat &&
                    dX.scalar_type() == torch::kFloat,
                "bf16 activation storage needs gemm_prec = 1 and fp32 "
                "theta, dZ and dX");
    TORCH_CHECK(use_mfma && I % 8 == 0,
                "bf16 activation storage: dX needs an MFMA shape "
                "(M >= 128, I >= 16, O >= 8, both even) and I % 8 == 0, "
                "got M=", M, " I=", I, " O=", O);
    TORCH_CHECK(act_below == ACT_NONE || act_below == ACT_RELU ||
                    (act_below == ACT_SIN_RELU && Xb2.has_value() &&
                     !Zb.has_value()),
                "bf16 activation storage: the layer below must be relu, "
                "none, or sin_relu with z recomputed (in_dim <= 4); "
                "sigmoid / tanh read y and keep fp32 storage");
    TORCH_CHECK(!Xb2.has_value() || Xb2->scalar_type() == torch::kFloat,
                "bf16 activation storage: Xb2 must be fp32");
    TORCH_CHECK(Yb->is_contiguous() && Yb->numel() == L * M * I &&
                    dZ.is_contiguous() && dX.is_contiguous() &&
                    dZ.numel() == L * M * O && dX.numel() == L * M * I,
                "bf16 activation storage: dZ [L*M, O], dX and Yb "
                "[L*M, I] contiguous");
    dim3 grid((I + 63) / 64, (M + 63) / 64, L);
    hipLaunchKernelGGL(gbf16a::act_dx_k, grid, dim3(256), 0, cur_stream(),
        dZ.data_ptr<float>(), theta.data_ptr<float>(),
        dX.data_ptr<float>(),
        reinterpret_cast<const __bf16*>(Yb->data_ptr()), (int)act_below,
        (float)scale_below, n, w_off, (int)M, (int)I, (int)O,
        opt_ptr<float>(Xb2), wb_off, bb_off, (int)Ib);
    HIP_CHECK_LAST();
    return;
  }
  if (use_bf16_gemm(gemm_prec, theta, use_mfma)) {
    dim3 grid((I + 63) / 64, (M + 63) / 64, L);
    hipLaunchKernelGGL(gbf16::bf16_dx_k, grid, dim3(256), 0,
        cur_stream(), dZ.data_ptr<float>(), theta.data_ptr<float>(),
        dX.data_ptr<float>(), opt_ptr<float>(Yb), opt_ptr<float>(Zb),
        (int)act_below, (float)scale_below, n, w_off, (int)M, (int)I,
        (int)O, opt_ptr<float>(Xb2), wb_off, bb_off, (int)Ib);
    HIP_CHECK_LAST();
    return;
  }
  DISPATCH_FT(dZ, {
    auto ybp = opt_ptr<scalar_t>(Yb);
    auto zbp = opt_ptr<scalar_t>(Zb);
    auto xb2p = opt_ptr<scalar_t>(Xb2);
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
inline bool dw_mfma_shape(long M, long I, long O) {
  const DwKernel k = dw_kernel_for(M, I, O);
  return k == DwKernel::Direct || k == DwKernel::Mfma;
}

bool dw_accumulates(long M, long I, long O, long gemm_prec = 0) {
  // bf16_dw_k writes slabs that dw_reduce_parts_k folds with plain
  // stores, db included: that path overwrites
  if (gemm_prec == 1 && dw_mfma_shape(M, I, O)) return false;
  return dw_kernel_for(M, I, O) != DwKernel::Small;
}

// dW/db. PRECONDITION where dw_accumulates(M, I, O, gemm_prec): the
// layer's slice of gstack is zeroed (the stacked engine zeroes the
// whole grad stack at backward start).
void linear_bwd_dw(torch::Tensor dZ, torch::Tensor X,
                   torch::Tensor gstack, long w_off, long b_off,
                   long M, long I, long O, long gemm_prec = 0) {
  CHECK_DEV(dZ); CHECK_DEV(X); CHECK_DEV(gstack);
  const long L = gstack.size(0), n = gstack.size(1);
  const bool xbf = is_bf16(X);
  if (xbf) {
    // bf16 activation storage (gemm_bf16_act.hip act_dw_k)
    TORCH_CHECK(gemm_prec == 1 && gstack.scalar_type() == torch::kFloat &&
                    dZ.scalar_type() == torch::kFloat,
                "bf16 activation storage needs gemm_prec = 1 and fp32 "
                "dZ and grad");
    TORCH_CHECK(dw_mfma_shape(M, I, O) && I % 8 == 0,
                "bf16 activation storage: dW needs an MFMA shape "
                "(M >= 256, I >= 16, O >= 16) and I % 8 == 0, got M=", M,
                " I=", I, " O=", O);
    TORCH_CHECK(X.is_contiguous() && X.numel() == L * M * I &&
                    dZ.is_contiguous() && dZ.numel() == L * M * O,
                "bf16 activation storage: dZ [L*M, O], X [L*M, I] "
                "contiguous");
  }
  if (use_bf16_gemm(gemm_prec, gstack, dw_mfma_shape(M, I, O))) {
    // M chunks of whole 64-row stages, about 1024 blocks in all; the
    // last chunk alone is ragged and none is empty, so every slab
    // element is written
    const long tiles = ((I + 63) / 64) * ((O + 63) / 64);
    long nchunk = std::max<long>(1, 1024 / std::max<long>(1, tiles * L));
    nchunk = std::min<long>(nchunk, (M + 63) / 64);
    const long mc = ((M + nchunk - 1) / nchunk + 63) / 64 * 64;
    nchunk = (M + mc - 1) / mc;
    torch::Tensor parts =
        torch::empty({L * nchunk * (O * I + O)}, gstack.options());
    // bias right behind the weights (every ModelSpec layer): chunk
    // slabs are [dW | db] and one reduce launch folds both; any other
    // layout keeps two slab arrays and two launches
    const bool joint = b_off == w_off + O * I;
    float* pp = parts.data_ptr<float>();
    float* dbp = joint ? pp + O * I : pp + L * nchunk * O * I;
    const long pstride = joint ? O * I + O : O * I;
    const long dbstride = joint ? O * I + O : O;
    dim3 grid((I + 63) / 64, (O + 63) / 64, L * nchunk);
    if (xbf) {
      hipLaunchKernelGGL(gbf16a::act_dw_k, grid, dim3(256), 0,
          cur_stream(), dZ.data_ptr<float>(),
          reinterpret_cast<const __bf16*>(X.data_ptr()), pp, dbp, pstride,
          dbstride, (int)M, (int)I, (int)O, (int)mc, (int)nchunk);
    } else {
      hipLaunchKernelGGL(gbf16::bf16_dw_k, grid, dim3(256), 0,
          cur_stream(), dZ.data_ptr<float>(), X.data_ptr<float>(), pp,
          dbp, pstride, dbstride, (int)M, (int)I, (int)O, (int)mc,
          (int)nchunk);
    }
    hipLaunchKernelGGL(gmfma::dw_reduce_parts_k<float>,
        dim3(grid_1d(pstride), 1, L), dim3(256), 0, cur_stream(),
        pp, gstack.data_ptr<float>(), n, w_off, pstride, (int)nchunk);
    if (!joint) {
      hipLaunchKernelGGL(gmfma::dw_reduce_parts_k<float>,
          dim3(grid_1d(O), 1, L), dim3(256), 0, cur_stream(),
          dbp, gstack.data_ptr<float>(), n, b_off, O, (int)nchunk);
    }
    HIP_CHECK_LAST();
    return;
  }
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

// ---- every node's PPO gradient row in one launch (ppo_fused.hip) ------
// ppo_grads_plan is the one place that decides whether a pair of nets
// is fusable and lays out the block's LDS; ppo_grads_fusable and
// ppo_grads_limit (the violated limit in words, "" where there is none)
// answer from it and ppo_grads_fused launches from it. The layer lists
// are those of ppo_rollout: the actor's shifted_plan, then the critic's.
struct PpoPlan {
  std::string why;  // empty: fusable
  ppof::Prog prog = {};
  long lds = 0;     // dynamic LDS bytes
};

PpoPlan ppo_grads_plan(
    const std::vector<long>& a_in, const std::vector<long>& a_out,
    const std::vector<long>& a_w, const std::vector<long>& a_b,
    const std::vector<long>& a_act, const std::vector<long>& c_in,
    const std::vector<long>& c_out, const std::vector<long>& c_w,
    const std::vector<long>& c_b, const std::vector<long>& c_act, long N,
    long n, long M, at::ScalarType dtype) {
  PpoPlan pl;
  auto no = [&](std::string why) -> PpoPlan& {
    pl.why = std::move(why);
    return pl;
  };
  if (dtype != torch::kFloat && dtype != torch::kDouble) {
    return no("dtype must be float32 or float64");
  }
  const long esz = dtype == torch::kDouble ? 8 : 4;
  const long TM = dtype == torch::kDouble
      ? ppof::tile_rows<double>::value : ppof::tile_rows<float>::value;
  if (N < 1 || N > 65535 || M < 1 || N * M >= (1L << 27)) {
    return no("needs 1 <= N <= 65535 nodes and N*M < 2^27 rows");
  }
  if (n < 1 || n >= (1L << 31)) return no("parameter row too long");
  const std::vector<long>* ls[2][5] = {
      {&a_in, &a_out, &a_w, &a_b, &a_act},
      {&c_in, &c_out, &c_w, &c_b, &c_act}};
  auto p16 = [](long v) { return (v + 15) / 16 * 16; };
  ppof::Prog& pg = pl.prog;
  pg.dz[0] = 0;
  pg.dz[1] = (int)(TM * ppof::LDZ);
  long lds_el = 0, slab = 0;
  for (int k = 0; k < 2; ++k) {
    const char* who = k == 0 ? "actor" : "critic";
    const auto& in = *ls[k][0];
    const auto& out = *ls[k][1];
    const auto& wo = *ls[k][2];
    const auto& bo = *ls[k][3];
    const auto& act = *ls[k][4];
    const long nl = (long)in.size();
    if (nl < 1 || nl > ppof::MAXL) {
      return no(std::string(who) + " must have 1 to " +
                std::to_string(ppof::MAXL) + " linear layers");
    }
    if ((long)out.size() != nl || (long)wo.size() != nl ||
        (long)bo.size() != nl || (long)act.size() != nl) {
      return no("layer lists differ in length");
    }
    ppof::Net& nt = pg.net[k];
    nt.nl = (int)nl;
    long cur = 2 * TM * ppof::LDZ, lo = n, hi = 0, sum = 0;
    for (long i = 0; i < nl; ++i) {
      const long I = in[i], O = out[i];
      if (I < 1 || O < 1 || I > ppof::MAX_W || O > ppof::MAX_W) {
        return no(std::string(who) + " layer widths must be 1 to " +
                  std::to_string(ppof::MAX_W));
      }
      if (I != (i == 0 ? (*ls[0][0])[0] : out[i - 1])) {
        return no(std::string(who) + " layer " + std::to_string(i) +
                  " does not take the layer below's output");
      }
      if (act[i] != (i == nl - 1 ? ACT_NONE : ACT_RELU)) {
        return no("hidden activations must be relu and the output "
                  "layer linear");
      }
      if (wo[i] < 0 || bo[i] < 0 || wo[i] + I * O > n || bo[i] + O > n) {
        return no(std::string(who) + " layer " + std::to_string(i) +
                  " lies outside the parameter row");
      }
      nt.in_dim[i] = (int)I; nt.out_dim[i] = (int)O;
      nt.w_off[i] = (int)wo[i]; nt.b_off[i] = (int)bo[i];
      lo = std::min({lo, wo[i], bo[i]});
      hi = std::max({hi, wo[i] + I * O, bo[i] + O});
      sum += I * O + O;
      // the layer's input image, weight image and bias
      nt.aimg[i] = (int)cur; cur += TM * (p16(I) + 2);
      nt.wimg[i] = (int)cur; cur += p16(O) * (p16(I) + 2);
      nt.bimg[i] = (int)cur; cur += p16(O);
    }
    // the reducer overwrites [base, base + span) from slabs in which
    // every word is some layer's: no gaps
    if (hi - lo != sum) {
      return no(std::string(who) +
                " layers must tile one contiguous slice of the row");
    }
    nt.base = (int)lo;
    nt.span = (int)sum;
    slab = std::max(slab, sum + 1);
    lds_el = std::max(lds_el, cur);
  }
  if (a_out.back() > losses::PPO_MAX_A) {
    return no("action dim must be <= " +
              std::to_string(losses::PPO_MAX_A));
  }
  if (c_out.back() != 1) return no("the critic's head must be 1 wide");
  pg.slab = (int)slab;
  pl.lds = lds_el * esz;
  if (pl.lds + ppof::STATIC_LDS > ppof::LDS_BUDGET) {
    return no("the nets' LDS images need " + std::to_string(pl.lds) +
              " bytes, over the " +
              std::to_string(ppof::LDS_BUDGET - ppof::STATIC_LDS) +
              " of one block");
  }
  return pl;
}

bool ppo_grads_fusable(
    std::vector<long> a_in, std::vector<long> a_out,
    std::vector<long> a_w, std::vector<long> a_b,
    std::vector<long> a_act, std::vector<long> c_in,
    std::vector<long> c_out, std::vector<long> c_w,
    std::vector<long> c_b, std::vector<long> c_act, long N, long n,
    long M, at::ScalarType dtype) {
  return ppo_grads_plan(a_in, a_out, a_w, a_b, a_act, c_in, c_out, c_w,
                        c_b, c_act, N, n, M, dtype).why.empty();
}

std::string ppo_grads_limit(
    std::vector<long> a_in, std::vector<long> a_out,
    std::vector<long> a_w, std::vector<long> a_b,
    std::vector<long> a_act, std::vector<long> c_in,
    std::vector<long> c_out, std::vector<long> c_w,
    std::vector<long> c_b, std::vector<long> c_act, long N, long n,
    long M, at::ScalarType dtype) {
  return ppo_grads_plan(a_in, a_out, a_w, a_b, a_act, c_in, c_out, c_w,
                        c_b, c_act, N, n, M, dtype).why;
}

// ppo_grad_fused_k's workspace per device: the dW/db/loss slabs
// [N, 2, tiles, slab] and one int32 ticket per (node, net). As with
// FcSplitWs: no per-call memset (the tickets are zero when allocated and
// every launch's reducers leave them zero), grown on demand, never freed.
struct PpoFusedWs {
  torch::Tensor slabs, tickets;
};

PpoFusedWs& ppo_fused_ws(const torch::Tensor& like, long slab_elems,
                         long ntickets) {
  static auto* ws = new std::map<int, PpoFusedWs>();
  PpoFusedWs& w = (*ws)[like.get_device()];
  const long need = slab_elems * (long)like.element_size();
  if (!w.slabs.defined() || w.slabs.numel() < need) {
    w.slabs = torch::empty({need}, like.options().dtype(torch::kUInt8));
  }
  if (!w.tickets.defined() || w.tickets.numel() < ntickets) {
    w.tickets =
        torch::zeros({ntickets}, like.options().dtype(torch::kInt32));
  }
  return w;
}

// grad [N, n] and loss [N, 2] (actor term, critic term; unscaled means)
// are overwritten, both nets' slices of every row; neither needs to be
// zero on entry. obs/acts [N*M, .], the rest [N*M], all of theta's
// dtype.
void ppo_grads_fused(
    torch::Tensor theta, torch::Tensor obs, torch::Tensor acts,
    torch::Tensor old_logp, torch::Tensor adv, torch::Tensor vtarg,
    torch::Tensor grad, torch::Tensor loss, std::vector<long> a_in,
    std::vector<long> a_out, std::vector<long> a_w,
    std::vector<long> a_b, std::vector<long> a_act,
    std::vector<long> c_in, std::vector<long> c_out,
    std::vector<long> c_w, std::vector<long> c_b,
    std::vector<long> c_act, long M, double cov, double clip,
    double critic_coef, double loss_scale) {
  CHECK_DEV(theta); CHECK_DEV(obs); CHECK_DEV(acts); CHECK_DEV(old_logp);
  CHECK_DEV(adv); CHECK_DEV(vtarg); CHECK_DEV(grad); CHECK_DEV(loss);
  TORCH_CHECK(theta.dim() == 2, "theta must be the [N, n] stack");
  const long N = theta.size(0), n = theta.size(1);
  PpoPlan pl = ppo_grads_plan(a_in, a_out, a_w, a_b, a_act, c_in, c_out,
                              c_w, c_b, c_act, N, n, M,
                              theta.scalar_type());
  TORCH_CHECK(pl.why.empty(), "ppo_grads_fused: ", pl.why,
              " (ppo_grads_fusable decides)");
  TORCH_CHECK(cov > 0, "cov must be positive");
  const long A = a_out.back(), obs_dim = a_in[0], rows = N * M;
  TORCH_CHECK(grad.dim() == 2 && grad.size(0) == N && grad.size(1) == n,
              "grad must be [N, n] like theta");
  TORCH_CHECK(loss.numel() == 2 * N, "loss must be [N, 2]");
  TORCH_CHECK(obs.numel() == rows * obs_dim && acts.numel() == rows * A,
              "obs / acts must be [N*M, obs_dim] / [N*M, A]");
  for (const torch::Tensor* t : {&old_logp, &adv, &vtarg}) {
    TORCH_CHECK(t->numel() == rows, "per-sample vectors must be [N*M]");
  }
  for (const torch::Tensor* t :
       {&obs, &acts, &old_logp, &adv, &vtarg, &grad, &loss}) {
    TORCH_CHECK(t->scalar_type() == theta.scalar_type(),
                "ppo_grads_fused tensors must share theta's dtype");
  }
  const double logc =
      0.5 * (double)A * std::log(2.0 * 3.14159265358979323846 * cov);
  DISPATCH_FT(theta, {
    constexpr int TM = ppof::tile_rows<scalar_t>::value;
    const long tiles = (M + TM - 1) / TM;
    PpoFusedWs& ws =
        ppo_fused_ws(theta, N * 2 * tiles * (long)pl.prog.slab, N * 2);
    const void* fn = reinterpret_cast<const void*>(
        ppof::ppo_grad_fused_k<scalar_t, TM>);
    static bool lds_raised = false;  // once per dtype: > 64 KB of LDS
    if (!lds_raised) {
      TORCH_CHECK(hipFuncSetAttribute(
                      fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                      ppof::LDS_BUDGET - ppof::STATIC_LDS) == hipSuccess,
                  "ppo_grads_fused: cannot raise the dynamic LDS limit");
      lds_raised = true;
    }
    hipLaunchKernelGGL((ppof::ppo_grad_fused_k<scalar_t, TM>),
        dim3(tiles, 2, N), dim3(256), (size_t)pl.lds, cur_stream(),
        theta.data_ptr<scalar_t>(), obs.data_ptr<scalar_t>(),
        acts.data_ptr<scalar_t>(), old_logp.data_ptr<scalar_t>(),
        adv.data_ptr<scalar_t>(), vtarg.data_ptr<scalar_t>(),
        grad.data_ptr<scalar_t>(), loss.data_ptr<scalar_t>(),
        reinterpret_cast<scalar_t*>(ws.slabs.data_ptr()),
        ws.tickets.data_ptr<int>(), pl.prog, n, (int)M, (int)A,
        (scalar_t)(1.0 / cov), (scalar_t)logc, (scalar_t)(1.0 - clip),
        (scalar_t)(1.0 + clip), (scalar_t)critic_coef,
        (scalar_t)loss_scale);
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

// ---- whole-MLP forward in one launch (mlp_fused.hip) ------------------
// mlp_plan is the one place that decides whether a chain is fusable
// and lays out the block's LDS; mlp_fwd_fusable answers from it and
// mlp_fwd_fused launches from it. A chain that is not fusable is no
// error: fwd_chain then runs its layered loop.
struct MlpPlan {
  bool ok = false;
  mlpf::Prog prog = {};
  long lds = 0;
};

inline bool mlp_act_ok(long act, bool lift) {
  return act == ACT_NONE || act == ACT_RELU || act == ACT_SIGMOID ||
         act == ACT_TANH || (lift && act == ACT_SIN_RELU);
}

MlpPlan mlp_plan(const torch::Tensor& spec, long M, long gemm_prec,
                 at::ScalarType dtype) {
  TORCH_CHECK(spec.device().is_cpu() && spec.dim() == 2 &&
                  spec.size(1) == SP_NCOLS &&
                  spec.scalar_type() == torch::kLong,
              "spec must be a CPU int64 [nl, 7] tensor");
  MlpPlan pl;
  const auto sp = spec.accessor<long, 2>();
  const long nl = spec.size(0);
  if (gemm_prec != 1 || dtype != torch::kFloat || M < 128 ||
      M > (1L << 30) || nl < 2 || nl > mlpf::MAXL) {
    return pl;
  }
  const bool has_tail =
      nl >= 3 && sp[nl - 1][SP_OUT_DIM] <= mlpf::TAIL_OUT;
  auto r32 = [](long v) { return (v + 31) / 32 * 32; };
  long img = 0, par = 0;  // bytes of weight images, floats of fp32 params
  for (long li = 0; li < nl; ++li) {
    const long in = sp[li][SP_IN_DIM], out = sp[li][SP_OUT_DIM],
               act = sp[li][SP_ACT];
    if (sp[li][SP_KIND] != 0 || in < 1 || out < 1) return pl;
    if (li > 0 && in != sp[li - 1][SP_OUT_DIM]) return pl;
    if (!mlp_act_ok(act, li == 0)) return pl;  // no Z stash, no logsoftmax
    mlpf::Layer& y = pl.prog.ly[li];
    y.w_off = sp[li][SP_W_OFF];
    y.b_off = sp[li][SP_B_OFF];
    y.in = (int)in;
    y.out = (int)out;
    y.act = (int)act;
    y.scale = 1.f;
    y.img = 0;
    y.par = (int)par;
    y.vec = 0;
    if (li == 0) {
      if (in > mlpf::LIFT_IN || out > mlpf::LIFT_OUT) return pl;
      par += r32(out) * 5;
    } else if (has_tail && li == nl - 1) {
      par += mlpf::TAIL_OUT * 64 + mlpf::TAIL_OUT;  // in <= 64: chain
    } else {
      if (in > mlpf::TRUNK_IN || out > mlpf::TRUNK_OUT) return pl;
      y.img = (int)img;
      img += mlpf::TRUNK_OUT * (r32(in) + 8) * 2;
      par += mlpf::TRUNK_OUT;
    }
  }
  mlpf::Prog& pg = pl.prog;
  pg.nl = (int)nl;
  pg.has_tail = has_tail ? 1 : 0;
  pg.off_wide = (int)img;
  pg.off_narrow = pg.off_wide + mlpf::TM * mlpf::LDW * 2;
  pg.off_tail = pg.off_narrow + mlpf::TM * mlpf::LDN * 2;
  pg.off_par = pg.off_tail + (has_tail ? mlpf::TM * mlpf::LDT * 4 : 0);
  pl.lds = pg.off_par + par * 4;
  pl.ok = pl.lds <= mlpf::LDS_BUDGET;
  return pl;
}

bool mlp_fwd_fusable(torch::Tensor spec, long M, long gemm_prec,
                     at::ScalarType dtype) {
  return mlp_plan(spec, M, gemm_prec, dtype).ok;
}

// acts: one entry per layer, [L*M, out] fp32. All present = the
// training forward (every layer stashed for bwd_chain); only the last
// present = inference. max_blocks > 0 caps the persistent grid.
void mlp_fwd_fused(torch::Tensor spec, torch::Tensor scales,
                   torch::Tensor xb, torch::Tensor theta,
                   std::vector<c10::optional<torch::Tensor>> acts, long M,
                   long max_blocks = 0) {
  CHECK_DEV(xb); CHECK_DEV(theta);
  TORCH_CHECK(theta.dim() == 2 && theta.is_contiguous() &&
                  xb.is_contiguous(),
              "mlp_fwd_fused: theta [L, n] and xb must be contiguous");
  MlpPlan pl = mlp_plan(spec, M, 1, theta.scalar_type());
  TORCH_CHECK(pl.ok && xb.scalar_type() == torch::kFloat,
              "mlp_fwd_fused: this chain is not fusable "
              "(mlp_fwd_fusable decides)");
  mlpf::Prog& pg = pl.prog;
  const long nl = pg.nl, L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(scales.device().is_cpu() && scales.numel() == nl &&
                  scales.scalar_type() == torch::kDouble &&
                  (long)acts.size() == nl,
              "mlp_fwd_fused: scales / acts need one entry per layer");
  TORCH_CHECK(max_blocks >= 0 && L >= 1 &&
                  xb.numel() == L * M * pg.ly[0].in,
              "mlp_fwd_fused: xb must be [L*M, in_dim]");
  TORCH_CHECK(acts[nl - 1].has_value(),
              "mlp_fwd_fused: the last acts entry is the output");
  long present = 0;
  for (long li = 0; li < nl; ++li) present += acts[li].has_value();
  TORCH_CHECK(present == nl || present == 1,
              "mlp_fwd_fused: give every layer's buffer or the last only");
  const auto sc = scales.accessor<double, 1>();
  for (long li = 0; li < nl; ++li) {
    mlpf::Layer& y = pg.ly[li];
    y.scale = (float)sc[li];
    TORCH_CHECK(y.w_off >= 0 && y.b_off >= 0 &&
                    y.w_off + (long)y.in * y.out <= n &&
                    y.b_off + y.out <= n,
                "mlp_fwd_fused: layer ", li, " lies outside the stack");
    pg.stash[li] = nullptr;
    if (!acts[li].has_value()) continue;
    const torch::Tensor& a = *acts[li];
    CHECK_DEV(a);
    TORCH_CHECK(a.scalar_type() == torch::kFloat && a.is_contiguous() &&
                    a.numel() == L * M * y.out,
                "mlp_fwd_fused: acts[", li, "] must be fp32 [L*M, out]");
    pg.stash[li] = a.data_ptr<float>();
    y.vec = (y.out % 4 == 0 &&
             reinterpret_cast<uintptr_t>(pg.stash[li]) % 16 == 0) ? 1 : 0;
  }
  const long total = L * ((M + mlpf::TM - 1) / mlpf::TM);
  const long cap = max_blocks > 0
      ? max_blocks
      : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const dim3 grid((unsigned)std::min(total, cap));
  auto launch = [&](auto stash_tag) {
    constexpr bool STASH = decltype(stash_tag)::value;
    static bool lds_raised = false;  // once per variant: > 64 KB of LDS
    if (!lds_raised) {
      TORCH_CHECK(hipFuncSetAttribute(
                      reinterpret_cast<const void*>(
                          mlpf::mlp_fwd_fused_k<STASH>),
                      hipFuncAttributeMaxDynamicSharedMemorySize,
                      (int)mlpf::LDS_BUDGET) == hipSuccess,
                  "mlp_fwd_fused: cannot raise the dynamic LDS limit");
      lds_raised = true;
    }
    hipLaunchKernelGGL(mlpf::mlp_fwd_fused_k<STASH>, grid, dim3(256),
        (size_t)pl.lds, cur_stream(), xb.data_ptr<float>(),
        theta.data_ptr<float>(), pg, n, (int)M, (int)L);
  };
  if (present == nl) launch(std::true_type{});
  else launch(std::false_type{});
  HIP_CHECK_LAST();
}

// ---- MNIST validation in one launch (eval.hip) ------------------------
// evalk_plan is the one place that decides whether mnist_eval_k takes a
// shape and lays out the block's LDS: x0 [R][XS], the two W1 stage
// buffers (which the image groups and the tail alias), the conv weights
// and bias. R = 32 where that fits the CU's 160 KB, else 16, else the
// shape is not fusable. mnist_eval_fusable answers from it and
// mnist_eval launches from it.
struct EvalPlan {
  std::string why;  // empty: fusable
  evalk::Plan prog = {};
  long lds = 0;
};

EvalPlan evalk_plan(long F, long K, long H, long C, long IMG, long V,
                    long Bv, at::ScalarType dtype) {
  EvalPlan pl;
  if (dtype != torch::kFloat && dtype != torch::kDouble) {
    pl.why = "dtype must be float32 or float64";
  } else if (IMG != evalk::IMG) {
    pl.why = "images must be 28x28";
  } else if (K < 1 || K > 7) {
    pl.why = "conv kernel size must be in [1, 7]";
  } else if (F < 1 || F > 4096) {
    pl.why = "conv filters must be in [1, 4096]";
  } else if (H < 1 || H > 64 || C < 1 || C > 16) {
    pl.why = "needs 1 <= H <= 64 and 1 <= C <= 16";
  } else if (V < 1 || V > (1L << 30) || Bv < 1 || Bv > (1L << 30)) {
    pl.why = "needs 1 <= V, Bv <= 2^30";
  }
  if (!pl.why.empty()) return pl;
  evalk::Plan& pg = pl.prog;
  const long P = (IMG - (K - 1)) / 2;
  pg.F = (int)F; pg.K = (int)K; pg.P = (int)P; pg.I = (int)(F * P * P);
  pg.H = (int)H; pg.C = (int)C;
  pg.XS = evalk::x0_stride(pg.I);
  const long esz = dtype == torch::kDouble ? 8 : 4;
  const long wgt = (F * K * K + F + 1) / 2 * 2;
  for (int R : {32, 16}) {
    pg.R = R;
    pg.off_stage = R * pg.XS;
    pg.off_wgt = pg.off_stage + evalk::STAGE;
    pl.lds = (pg.off_wgt + wgt) * esz;
    if (pl.lds <= 160 * 1024) return pl;
  }
  pl.why = "a 16-row x0 tile does not fit the 160 KB of LDS";
  return pl;
}

bool mnist_eval_fusable(long F, long K, long H, long C, long IMG, long V,
                        long Bv, at::ScalarType dtype) {
  return evalk_plan(F, K, H, C, IMG, V, Bv, dtype).why.empty();
}

// X_val [V, IMG*IMG] and y_val [V] (int64) are shared by all L nodes of
// theta [L, n]; correct [L, V] (bool or uint8) and loss_sum [L] are
// overwritten. loss_sum[l] is the sum over chunks of Bv rows of the
// chunk-mean NLL, whatever the kernel's own tiling.
void mnist_eval(torch::Tensor X_val, torch::Tensor y_val,
                torch::Tensor theta, torch::Tensor correct,
                torch::Tensor loss_sum, long cw_off, long cb_off,
                long w1_off, long b1_off, long w2_off, long b2_off, long F,
                long K, long H, long C, long IMG, long V, long Bv) {
  CHECK_DEV(X_val); CHECK_DEV(y_val); CHECK_DEV(theta); CHECK_DEV(correct);
  CHECK_DEV(loss_sum);
  EvalPlan pl = evalk_plan(F, K, H, C, IMG, V, Bv, theta.scalar_type());
  TORCH_CHECK(pl.why.empty(), "mnist_eval: ", pl.why,
              " (mnist_eval_fusable decides)");
  evalk::Plan& pg = pl.prog;
  TORCH_CHECK(theta.dim() == 2, "mnist_eval: theta must be [L, n]");
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(L >= 1 && L <= 65535, "mnist_eval: 1 <= L <= 65535");
  TORCH_CHECK(X_val.scalar_type() == theta.scalar_type() &&
                  loss_sum.scalar_type() == theta.scalar_type() &&
                  X_val.numel() == V * IMG * IMG && loss_sum.numel() == L,
              "mnist_eval: X_val must be [V, IMG*IMG] and loss_sum [L], "
              "both of theta's dtype");
  TORCH_CHECK(y_val.scalar_type() == torch::kLong && y_val.numel() == V,
              "mnist_eval: y_val must be int64 [V]");
  TORCH_CHECK(correct.element_size() == 1 && correct.numel() == L * V,
              "mnist_eval: correct must be bool or uint8 [L, V]");
  const long I = pg.I;
  auto inside = [&](long off, long len) {
    return off >= 0 && off + len <= n;
  };
  TORCH_CHECK(inside(cw_off, F * K * K) && inside(cb_off, F) &&
                  inside(w1_off, H * I) && inside(b1_off, H) &&
                  inside(w2_off, C * H) && inside(b2_off, C),
              "mnist_eval: a layer lies outside the stack");
  pg.cw_off = cw_off; pg.cb_off = cb_off; pg.w1_off = w1_off;
  pg.b1_off = b1_off; pg.w2_off = w2_off; pg.b2_off = b2_off;
  const long tiles = (V + pg.R - 1) / pg.R;
  // part [L, tiles] in the slab bytes, one ticket per node: the fc
  // block's workspace, whose launches leave their tickets zero as well
  FcSplitWs& ws = fc_split_ws(theta, L * tiles, L);
  DISPATCH_FT(theta, {
    dispatch_kmax(K, [&](auto kmax) {
      auto kern = evalk::mnist_eval_k<scalar_t, decltype(kmax)::value>;
      static bool lds_raised = false;  // once per variant: > 64 KB of LDS
      if (!lds_raised) {
        TORCH_CHECK(hipFuncSetAttribute(
                        reinterpret_cast<const void*>(kern),
                        hipFuncAttributeMaxDynamicSharedMemorySize,
                        160 * 1024) == hipSuccess,
                    "mnist_eval: cannot raise the dynamic LDS limit");
        lds_raised = true;
      }
      hipLaunchKernelGGL(kern, dim3(tiles, L), dim3(256), (size_t)pl.lds,
          cur_stream(), X_val.data_ptr<scalar_t>(),
          y_val.data_ptr<long>(), theta.data_ptr<scalar_t>(),
          static_cast<unsigned char*>(correct.data_ptr()),
          loss_sum.data_ptr<scalar_t>(),
          reinterpret_cast<scalar_t*>(ws.slabs.data_ptr()),
          ws.tickets.data_ptr<int>(), pg, n, (int)V, (int)Bv);
    });
  });
  HIP_CHECK_LAST();
}

// ---- density-MLP validation in one launch (mlp_eval.hip) --------------
// mlp_eval_plan is the one place that decides whether mlp_eval_k takes a
// chain and lays out the block's LDS: the wide image [R][ldw], the two
// narrow images [R][66], the two W stages, the inputs and the row
// losses. R is 64 (float) / 32 (double); at the widest chain the layout
// is 118,528 B / 135,936 B, so every chain inside the limits fits the
// CU's 160 KB. loss_kind 0 is predict mode, 1 BCE, 2 MSE, 3 L1.
// mlp_eval_fusable answers from it and mlp_eval launches from it.
struct MlpEvalPlan {
  std::string why;  // empty: fusable
  mlpe::Plan prog = {};
  long lds = 0;
};

MlpEvalPlan mlp_eval_plan(const torch::Tensor& spec, long V, long Bv,
                          long loss_kind, at::ScalarType dtype) {
  TORCH_CHECK(spec.device().is_cpu() && spec.dim() == 2 &&
                  spec.size(1) == SP_NCOLS &&
                  spec.scalar_type() == torch::kLong,
              "spec must be a CPU int64 [nl, 7] tensor");
  MlpEvalPlan pl;
  const auto sp = spec.accessor<long, 2>();
  const long nl = spec.size(0);
  if (dtype != torch::kFloat && dtype != torch::kDouble) {
    pl.why = "dtype must be float32 or float64";
  } else if (nl < 2 || nl > mlpe::MAXL) {
    pl.why = "needs 2..8 linear layers";
  } else if (V < 1 || V > (1L << 30) || Bv < 1 || Bv > (1L << 30)) {
    pl.why = "needs 1 <= V, Bv <= 2^30";
  } else if (loss_kind < 0 || loss_kind > 3) {
    pl.why = "loss_kind must be 0 (predict), 1 (BCE), 2 (MSE) or 3 (L1)";
  } else if (loss_kind != 0 && sp[nl - 1][SP_OUT_DIM] != 1) {
    pl.why = "a loss needs a head of width 1";
  }
  mlpe::Plan& pg = pl.prog;
  for (long li = 0; li < nl && pl.why.empty(); ++li) {
    const long in = sp[li][SP_IN_DIM], out = sp[li][SP_OUT_DIM],
               act = sp[li][SP_ACT];
    const bool lift = li == 0, tail = li == nl - 1;
    if (sp[li][SP_KIND] != 0 || in < 1 || out < 1 ||
        (li > 0 && in != sp[li - 1][SP_OUT_DIM])) {
      pl.why = "needs linear layers, each fed by the one below";
    } else if (lift && (in > mlpe::LIFT_IN ||
                        out > (nl == 2 ? mlpe::NARROW : mlpe::WIDE))) {
      pl.why = "first layer needs in <= 4 and out <= 256 (64 before the "
               "last)";
    } else if (!lift && !tail && out > mlpe::NARROW) {
      pl.why = "a hidden layer above the first needs out <= 64";
    } else if (tail && out > mlpe::TAIL_OUT) {
      pl.why = "last layer needs out <= 4";
    } else if (tail ? !(act == ACT_NONE || act == ACT_SIGMOID ||
                        act == ACT_TANH)
                    : !mlp_act_ok(act, lift)) {
      pl.why = "an activation the kernel does not have";
    }
    pg.ly[li] = {sp[li][SP_W_OFF], sp[li][SP_B_OFF], (int)in, (int)out,
                 (int)act};
  }
  if (!pl.why.empty()) return pl;
  const long R = dtype == torch::kDouble ? 16 * mlpe::frags<double>()
                                         : 16 * mlpe::frags<float>();
  const int out0 = pg.ly[0].out;
  pg.nl = (int)nl;
  pg.loss_kind = (int)loss_kind;
  pg.ldw = mlpe::wide_stride(out0);
  pg.cp = 4;
  while (pg.cp < out0) pg.cp *= 2;
  pg.off_nar = (int)(R * pg.ldw);
  pg.off_stage = pg.off_nar + (int)(2 * R * mlpe::NLD);
  pg.off_x = pg.off_stage + mlpe::STAGE;
  pg.off_rl = pg.off_x + (int)(R * mlpe::LIFT_IN);
  pl.lds = (pg.off_rl + R) * (dtype == torch::kDouble ? 8 : 4);
  return pl;
}

bool mlp_eval_fusable(torch::Tensor spec, long V, long Bv, long loss_kind,
                      at::ScalarType dtype) {
  return mlp_eval_plan(spec, V, Bv, loss_kind, dtype).why.empty();
}

// X_val [V, in] is shared by all L nodes of theta [L, n]. Loss mode
// (loss_kind 1..3): y_val [V] and loss_sum [L]; loss_sum[l] is
// overwritten with the sum over chunks of Bv rows of the chunk-mean
// loss, whatever the kernel's own tiling. Predict mode (loss_kind 0):
// yhat [L, V, out] is overwritten.
void mlp_eval(torch::Tensor spec, torch::Tensor scales, torch::Tensor X_val,
              c10::optional<torch::Tensor> y_val, torch::Tensor theta,
              c10::optional<torch::Tensor> loss_sum,
              c10::optional<torch::Tensor> yhat, long V, long Bv,
              long loss_kind) {
  CHECK_DEV(X_val); CHECK_DEV(theta);
  MlpEvalPlan pl =
      mlp_eval_plan(spec, V, Bv, loss_kind, theta.scalar_type());
  TORCH_CHECK(pl.why.empty(), "mlp_eval: ", pl.why,
              " (mlp_eval_fusable decides)");
  mlpe::Plan& pg = pl.prog;
  TORCH_CHECK(theta.dim() == 2, "mlp_eval: theta must be [L, n]");
  const long L = theta.size(0), n = theta.size(1);
  TORCH_CHECK(L >= 1 && L <= 65535, "mlp_eval: 1 <= L <= 65535");
  TORCH_CHECK(scales.device().is_cpu() && scales.numel() == pg.nl &&
                  scales.scalar_type() == torch::kDouble,
              "mlp_eval: scales needs one float64 entry per layer");
  pg.scale = scales.accessor<double, 1>()[0];
  const auto dt = theta.scalar_type();
  TORCH_CHECK(X_val.scalar_type() == dt &&
                  X_val.numel() == V * pg.ly[0].in,
              "mlp_eval: X_val must be [V, in] of theta's dtype");
  for (int li = 0; li < pg.nl; ++li) {
    const mlpe::Layer& y = pg.ly[li];
    TORCH_CHECK(y.w_off >= 0 && y.b_off >= 0 &&
                    y.w_off + (long)y.in * y.out <= n &&
                    y.b_off + y.out <= n,
                "mlp_eval: layer ", li, " lies outside the stack");
  }
  const bool predict = loss_kind == 0;
  const long out = pg.ly[pg.nl - 1].out;
  auto given = [&](const c10::optional<torch::Tensor>& t, long numel) {
    return t.has_value() && t->is_cuda() && t->is_contiguous() &&
           t->scalar_type() == dt && t->numel() == numel;
  };
  if (predict) {
    TORCH_CHECK(!y_val.has_value() && !loss_sum.has_value() &&
                    given(yhat, L * V * out),
                "mlp_eval: predict mode takes yhat [L, V, out] of theta's "
                "dtype and neither y_val nor loss_sum");
  } else {
    TORCH_CHECK(given(y_val, V) && given(loss_sum, L) && !yhat.has_value(),
                "mlp_eval: loss mode takes y_val [V] and loss_sum [L] of "
                "theta's dtype and no yhat");
  }
  const long R = dt == torch::kDouble ? 16 * mlpe::frags<double>()
                                      : 16 * mlpe::frags<float>();
  const long tiles = (V + R - 1) / R;
  // part [L, tiles] in the slab bytes, one ticket per node: the fc
  // block's workspace, as mnist_eval
  FcSplitWs& ws = fc_split_ws(theta, L * tiles, L);
  DISPATCH_FT(theta, {
    auto kern = mlpe::mlp_eval_k<scalar_t>;
    static bool lds_raised = false;  // once per variant: > 64 KB of LDS
    if (!lds_raised) {
      TORCH_CHECK(hipFuncSetAttribute(
                      reinterpret_cast<const void*>(kern),
                      hipFuncAttributeMaxDynamicSharedMemorySize,
                      160 * 1024) == hipSuccess,
                  "mlp_eval: cannot raise the dynamic LDS limit");
      lds_raised = true;
    }
    hipLaunchKernelGGL(kern, dim3(tiles, L), dim3(256), (size_t)pl.lds,
        cur_stream(), X_val.data_ptr<scalar_t>(),
        predict ? nullptr : y_val->data_ptr<scalar_t>(),
        theta.data_ptr<scalar_t>(),
        predict ? nullptr : loss_sum->data_ptr<scalar_t>(),
        predict ? yhat->data_ptr<scalar_t>() : nullptr,
        reinterpret_cast<scalar_t*>(ws.slabs.data_ptr()),
        ws.tickets.data_ptr<int>(), pg, n, (int)V, (int)Bv);
  });
  HIP_CHECK_LAST();
}

// ---- whole gradient row in one launch (mlp_grad_fused.hip) ------------
// mlp_grad_plan is the one place that decides whether mlp_grad_fused_k
// takes a chain and lays out its LDS: what mlp_plan accepts, narrowed to
// lift + trunk(s) + tail with the activations the backward phases know,
// a regression loss_kind, and weight / bias slices that tile [0, end)
// (n >= 0: end == n), so that writing them is writing the row.
struct MlpGradPlan {
  bool ok = false;
  mlpg::Prog prog = {};
  long lds = 0;
};

MlpGradPlan mlp_grad_plan(const torch::Tensor& spec, long M,
                          long gemm_prec, at::ScalarType dtype,
                          long loss_kind, long n = -1) {
  MlpGradPlan gp;
  const MlpPlan fp = mlp_plan(spec, M, gemm_prec, dtype);
  if (!fp.ok || !fp.prog.has_tail || loss_kind < 1 || loss_kind > 3) {
    return gp;
  }
  mlpg::Prog& pg = gp.prog;
  pg.f = fp.prog;
  const int nl = pg.f.nl, nt = nl - 2;
  std::vector<std::pair<long, long>> slices;
  for (int li = 0; li < nl; ++li) {
    const mlpf::Layer& y = pg.f.ly[li];
    const int a = y.act;
    const bool act_ok =
        li == 0 ? (a == ACT_SIN_RELU || a == ACT_RELU || a == ACT_NONE)
        : li <= nt ? (a == ACT_RELU || a == ACT_NONE)
                   : (a == ACT_NONE || a == ACT_SIGMOID || a == ACT_TANH);
    if (!act_ok) return gp;
    slices.push_back({y.w_off, (long)y.in * y.out});
    slices.push_back({y.b_off, (long)y.out});
    pg.vec[li] = (y.w_off % 4 == 0 && y.in % 4 == 0) ? 1 : 0;
  }
  if (loss_kind == 1 && pg.f.ly[nl - 1].act != ACT_SIGMOID) return gp;
  std::sort(slices.begin(), slices.end());
  long end = 0;
  for (const auto& s : slices) {
    if (s.first != end) return gp;
    end += s.second;
  }
  if ((n >= 0 && end != n) || end >= (1L << 30)) return gp;
  pg.nt = nt;
  pg.loss_kind = (int)loss_kind;
  pg.slab = (int)((end + 1 + 3) / 4 * 4);
  // the weight images and the wide image stay where mlp_plan put them
  const long par_bytes = fp.lds - pg.f.off_par;
  pg.off_act = pg.f.off_wide + mlpf::TM * mlpf::LDW * 2;
  pg.off_dz = pg.off_act + (nt - 1) * mlpg::IMG_N;
  pg.f.off_narrow = pg.off_act;
  pg.f.off_tail = pg.off_dz + 2 * mlpg::IMG_N;
  pg.off_x = pg.f.off_tail + mlpf::TM * mlpf::LDT * 4;
  pg.off_hz = pg.off_x + mlpf::TM * 4 * 4;
  pg.off_red = pg.off_hz + mlpf::TM * 4 * 4;
  pg.f.off_par = pg.off_red + mlpg::RED_FLOATS * 4;
  gp.lds = pg.f.off_par + par_bytes;
  gp.ok = gp.lds <= mlpf::LDS_BUDGET;
  return gp;
}

bool mlp_grads_fusable(torch::Tensor spec, long M, long gemm_prec,
                       at::ScalarType dtype, long loss_kind) {
  return mlp_grad_plan(spec, M, gemm_prec, dtype, loss_kind).ok;
}

// mlp_grad_fused_k's workspace per device: the gradient slabs [L, J,
// slab] and one int32 ticket per node. As with PpoFusedWs: no per-call
// memset (the tickets are zero when allocated and every launch's
// reducers leave them zero), grown on demand, never freed.
PpoFusedWs& mlp_grad_ws(const torch::Tensor& like, long slab_elems,
                        long ntickets) {
  static auto* ws = new std::map<int, PpoFusedWs>();
  PpoFusedWs& w = (*ws)[like.get_device()];
  if (!w.slabs.defined() || w.slabs.numel() < slab_elems) {
    w.slabs = torch::empty({slab_elems}, like.options());
  }
  if (!w.tickets.defined() || w.tickets.numel() < ntickets) {
    w.tickets =
        torch::zeros({ntickets}, like.options().dtype(torch::kInt32));
  }
  return w;
}

// grad [L, n] and the optional loss [L] (unscaled per-node means) are
// overwritten; neither needs to be zero on entry. xb [L*M, in], yb
// [L*M, out] of the tail. max_blocks > 0 caps the persistent grid.
void mlp_grads_fused(torch::Tensor spec, torch::Tensor scales,
                     torch::Tensor xb, torch::Tensor yb,
                     torch::Tensor theta, torch::Tensor grad,
                     c10::optional<torch::Tensor> loss, long loss_kind,
                     double loss_scale, long M, long max_blocks = 0) {
  CHECK_DEV(xb); CHECK_DEV(yb); CHECK_DEV(theta); CHECK_DEV(grad);
  TORCH_CHECK(theta.dim() == 2 && theta.is_contiguous() &&
                  xb.is_contiguous() && yb.is_contiguous() &&
                  grad.is_contiguous(),
              "mlp_grads_fused: theta [L, n], grad, xb and yb must be "
              "contiguous");
  const long L = theta.size(0), n = theta.size(1);
  MlpGradPlan gp = mlp_grad_plan(spec, M, 1, theta.scalar_type(),
                                 loss_kind, n);
  TORCH_CHECK(gp.ok && xb.scalar_type() == torch::kFloat &&
                  yb.scalar_type() == torch::kFloat &&
                  grad.scalar_type() == torch::kFloat,
              "mlp_grads_fused: this chain, loss or stack is not fusable "
              "(mlp_grads_fusable decides; the layers' slices must tile "
              "the whole row)");
  mlpg::Prog& pg = gp.prog;
  const long nl = pg.f.nl;
  TORCH_CHECK(scales.device().is_cpu() && scales.numel() == nl &&
                  scales.scalar_type() == torch::kDouble,
              "mlp_grads_fused: scales needs one entry per layer");
  TORCH_CHECK(max_blocks >= 0 && L >= 1 &&
                  xb.numel() == L * M * pg.f.ly[0].in &&
                  yb.numel() == L * M * pg.f.ly[nl - 1].out,
              "mlp_grads_fused: xb / yb must be [L*M, in] / [L*M, out]");
  TORCH_CHECK(grad.dim() == 2 && grad.size(0) == L && grad.size(1) == n,
              "mlp_grads_fused: grad must be [L, n] like theta");
  float* loss_p = nullptr;
  if (loss.has_value()) {
    CHECK_DEV(*loss);
    TORCH_CHECK(loss->scalar_type() == torch::kFloat &&
                    loss->is_contiguous() && loss->numel() == L,
                "mlp_grads_fused: loss must be fp32 [L]");
    loss_p = loss->data_ptr<float>();
  }
  const auto sc = scales.accessor<double, 1>();
  for (long li = 0; li < nl; ++li) {
    pg.f.ly[li].scale = (float)sc[li];
    pg.f.stash[li] = nullptr;
  }
  pg.w = (float)loss_scale / (float)M;
  const long tpn = (M + mlpf::TM - 1) / mlpf::TM, total = L * tpn;
  const long cap = max_blocks > 0
      ? max_blocks
      : at::cuda::getCurrentDeviceProperties()->multiProcessorCount;
  const long G = std::min(total, cap);
  // the kernel's owner(): block b holds tiles [total*b/G, total*(b+1)/G)
  auto owner = [&](long t) {
    long b = t * G / total;
    while (total * (b + 1) / G <= t) ++b;
    while (total * b / G > t) --b;
    return b;
  };
  long J = 1;
  for (long l = 0; l < L; ++l) {
    J = std::max(J, owner((l + 1) * tpn - 1) - owner(l * tpn) + 1);
  }
  pg.J = (int)J;
  PpoFusedWs& ws = mlp_grad_ws(theta, L * J * (long)pg.slab, L);
  static bool lds_raised = false;  // > 64 KB of LDS
  if (!lds_raised) {
    TORCH_CHECK(hipFuncSetAttribute(
                    reinterpret_cast<const void*>(mlpg::mlp_grad_fused_k),
                    hipFuncAttributeMaxDynamicSharedMemorySize,
                    (int)mlpf::LDS_BUDGET) == hipSuccess,
                "mlp_grads_fused: cannot raise the dynamic LDS limit");
    lds_raised = true;
  }
  hipLaunchKernelGGL(mlpg::mlp_grad_fused_k, dim3((unsigned)G), dim3(256),
      (size_t)gp.lds, cur_stream(), xb.data_ptr<float>(),
      yb.data_ptr<float>(), theta.data_ptr<float>(),
      grad.data_ptr<float>(), loss_p, ws.slabs.data_ptr<float>(),
      ws.tickets.data_ptr<int>(), pg, n, (int)M, (int)L);
  HIP_CHECK_LAST();
}

// Whether the engine stores layer li's activation as bf16 (the kernels
// of gemm_bf16_act.hip): only where the producer is one of those
// kernels and EVERY consumer already rounds the buffer to bf16, so the
// stored bits are the operands the fp32 buffer would have given. The
// engine asks here (ops/stacked.py _alloc_bufs) instead of re-deriving.
bool act_storage_bf16(torch::Tensor spec, long li, long M, long gemm_prec,
                      at::ScalarType dtype) {
  TORCH_CHECK(spec.device().is_cpu() && spec.dim() == 2 &&
                  spec.size(1) == SP_NCOLS,
              "spec must be a CPU [nl, 7] tensor");
  const auto sp = spec.accessor<long, 2>();
  const long nl = spec.size(0);
  if (gemm_prec != 1 || dtype != torch::kFloat) return false;
  if (li < 0 || li >= nl - 1) return false;  // the last layer stays fp32
  if (sp[li][SP_KIND] != 0 || sp[li + 1][SP_KIND] != 0) return false;
  const long in = sp[li][SP_IN_DIM], out = sp[li][SP_OUT_DIM],
             act = sp[li][SP_ACT], out2 = sp[li + 1][SP_OUT_DIM];
  // relu / none need no z; sin_relu only where the engine keeps no Z
  // stash for it (z recomputed from an in_dim <= 4 input)
  if (!(act == ACT_RELU || act == ACT_NONE ||
        (act == ACT_SIN_RELU && in <= 4))) {
    return false;
  }
  if (out % 8 != 0) return false;
  // producer: act_fwd_k (a bf16 input has in % 8 == 0 by this same
  // rule one layer down) or encode_bf16_k
  if (!fwd_mfma_shape(M, in, out) && !fwd_encode_shape(M, in, out)) {
    return false;
  }
  // consumers: the next layer's forward, dW and dX on the bf16 MFMA
  return fwd_mfma_shape(M, out, out2) && dx_mfma_shape(M, out, out2) &&
         dw_mfma_shape(M, out, out2);
}

// fuse (trailing, default 0): 1 = run a chain that mlp_fwd_fusable
// accepts as the optional gather plus ONE mlp_fwd_fused launch; any
// other chain, and fuse = 0, run the layered loop below unchanged. An
// acts entry may be None only for a layer the fused launch does not
// stash.
void fwd_chain(torch::Tensor spec, torch::Tensor scales,
               c10::optional<torch::Tensor> X_all,
               c10::optional<torch::Tensor> idx, long idx_stride,
               long idx_off,
               torch::Tensor xb, torch::Tensor theta,
               std::vector<c10::optional<torch::Tensor>> acts,
               std::vector<c10::optional<torch::Tensor>> zs,
               std::vector<c10::optional<torch::Tensor>> idxs,
               c10::optional<torch::Tensor> logp, long M,
               bool train_skip_logp, long gemm_prec = 0, long fuse = 0) {
  TORCH_CHECK(spec.device().is_cpu() && scales.device().is_cpu() &&
                  spec.size(1) == SP_NCOLS,
              "spec [nl, 7] / scales must be CPU tensors");
  TORCH_CHECK(fuse == 0 || fuse == 1, "fuse must be 0 or 1");
  const auto sp = spec.accessor<long, 2>();
  const auto sc = scales.accessor<double, 1>();
  const long nl = spec.size(0);
  if (X_all.has_value()) {
    gather_batch(*X_all, *idx, xb, idx_stride, idx_off);
  }
  if (fuse == 1 &&
      mlp_fwd_fusable(spec, M, gemm_prec, theta.scalar_type())) {
    mlp_fwd_fused(spec, scales, xb, theta, acts, M);
    return;
  }
  torch::Tensor cur = xb;
  for (long li = 0; li < nl; ++li) {
    const long kind = sp[li][SP_KIND], w_off = sp[li][SP_W_OFF],
               b_off = sp[li][SP_B_OFF], in_dim = sp[li][SP_IN_DIM],
               out_dim = sp[li][SP_OUT_DIM], act = sp[li][SP_ACT],
               ksize = sp[li][SP_KSIZE];
    TORCH_CHECK(acts[li].has_value(),
                "fwd_chain: the layered path needs every acts buffer");
    torch::Tensor out = *acts[li];
    if (kind == 1) {
      conv_pool_fwd(cur, theta, out, *idxs[li], w_off, b_off, M,
                    out_dim, ksize, in_dim);
      cur = out;
    } else if (act == ACT_LOGSOFTMAX) {
      linear_fwd(cur, theta, out, c10::nullopt, w_off, b_off, M,
                 in_dim, out_dim, ACT_NONE, 1.0, gemm_prec);
      if (!train_skip_logp) {
        logsoftmax(out, *logp, out_dim);
        cur = *logp;
      } else {
        cur = out;
      }
    } else {
      linear_fwd(cur, theta, out, zs[li], w_off, b_off, M, in_dim,
                 out_dim, act, sc[li], gemm_prec);
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
               long M, long zero_mode, long gemm_prec = 0) {
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
    linear_bwd_dw(dz, below, grad, w_off, b_off, M, in_dim, out_dim,
                  gemm_prec);
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
          xb2, wb_off, bb_off, ib, gemm_prec);
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
  namespace py = pybind11;
  // gemm_prec trails with a default (0 = native, 1 = bf16 operands),
  // so the positional calls from before it existed keep working
  mod.def("linear_fwd", &linear_fwd, py::arg("X"), py::arg("theta"),
          py::arg("Y"), py::arg("Z"), py::arg("w_off"), py::arg("b_off"),
          py::arg("M"), py::arg("I"), py::arg("O"), py::arg("act"),
          py::arg("scale"), py::arg("gemm_prec") = 0);
  mod.def("act_grad", &act_grad);
  mod.def("linear_bwd_dx", &linear_bwd_dx, py::arg("dZ"),
          py::arg("theta"), py::arg("dX"), py::arg("Yb"), py::arg("Zb"),
          py::arg("act_below"), py::arg("scale_below"), py::arg("w_off"),
          py::arg("M"), py::arg("I"), py::arg("O"), py::arg("Xb2"),
          py::arg("wb_off"), py::arg("bb_off"), py::arg("Ib"),
          py::arg("gemm_prec") = 0);
  mod.def("linear_bwd_dw", &linear_bwd_dw, py::arg("dZ"), py::arg("X"),
          py::arg("gstack"), py::arg("w_off"), py::arg("b_off"),
          py::arg("M"), py::arg("I"), py::arg("O"),
          py::arg("gemm_prec") = 0);
  mod.def("dw_accumulates", &dw_accumulates, py::arg("M"), py::arg("I"),
          py::arg("O"), py::arg("gemm_prec") = 0);
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
  mod.def("ppo_rollout", &ppo_rollout, py::arg("theta"),
          py::arg("in_dims"), py::arg("out_dims"), py::arg("w_offs"),
          py::arg("b_offs"), py::arg("act_ids"), py::arg("resets"),
          py::arg("obst"), py::arg("eps"), py::arg("obs"),
          py::arg("acts"), py::arg("logp"), py::arg("rews"),
          py::arg("rtgs"), py::arg("ep_rew"), py::arg("M"),
          py::arg("ep_len"), py::arg("cov"), py::arg("gamma"),
          py::arg("envp"), py::arg("last_obs") = py::none());
  mod.def("ppo_grads_fusable", &ppo_grads_fusable);
  mod.def("ppo_grads_limit", &ppo_grads_limit);
  mod.def("ppo_grads_fused", &ppo_grads_fused);
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
  mod.def("fwd_chain", &fwd_chain, py::arg("spec"), py::arg("scales"),
          py::arg("X_all"), py::arg("idx"), py::arg("idx_stride"),
          py::arg("idx_off"), py::arg("xb"), py::arg("theta"),
          py::arg("acts"), py::arg("zs"), py::arg("idxs"),
          py::arg("logp"), py::arg("M"), py::arg("train_skip_logp"),
          py::arg("gemm_prec") = 0, py::arg("fuse") = 0);
  mod.def("mlp_fwd_fusable", &mlp_fwd_fusable, py::arg("spec"),
          py::arg("M"), py::arg("gemm_prec"), py::arg("dtype"));
  mod.def("mlp_fwd_fused", &mlp_fwd_fused, py::arg("spec"),
          py::arg("scales"), py::arg("xb"), py::arg("theta"),
          py::arg("acts"), py::arg("M"), py::arg("max_blocks") = 0);
  mod.def("mlp_grads_fusable", &mlp_grads_fusable, py::arg("spec"),
          py::arg("M"), py::arg("gemm_prec"), py::arg("dtype"),
          py::arg("loss_kind"));
  mod.def("mlp_grads_fused", &mlp_grads_fused, py::arg("spec"),
          py::arg("scales"), py::arg("xb"), py::arg("yb"),
          py::arg("theta"), py::arg("grad"), py::arg("loss"),
          py::arg("loss_kind"), py::arg("loss_scale"), py::arg("M"),
          py::arg("max_blocks") = 0);
  mod.def("mnist_eval_fusable", &mnist_eval_fusable, py::arg("F"),
          py::arg("K"), py::arg("H"), py::arg("C"), py::arg("IMG"),
          py::arg("V"), py::arg("Bv"), py::arg("dtype"));
  mod.def("mnist_eval", &mnist_eval, py::arg("X_val"), py::arg("y_val"),
          py::arg("theta"), py::arg("correct"), py::arg("loss_sum"),
          py::arg("cw_off"), py::arg("cb_off"), py::arg("w1_off"),
          py::arg("b1_off"), py::arg("w2_off"), py::arg("b2_off"),
          py::arg("F"), py::arg("K"), py::arg("H"), py::arg("C"),
          py::arg("IMG"), py::arg("V"), py::arg("Bv"));
  mod.def("mlp_eval_fusable", &mlp_eval_fusable, py::arg("spec"),
          py::arg("V"), py::arg("Bv"), py::arg("loss_kind"),
          py::arg("dtype"));
  mod.def("mlp_eval", &mlp_eval, py::arg("spec"), py::arg("scales"),
          py::arg("X_val"), py::arg("y_val"), py::arg("theta"),
          py::arg("loss_sum"), py::arg("yhat"), py::arg("V"),
          py::arg("Bv"), py::arg("loss_kind"));
  mod.def("act_storage_bf16", &act_storage_bf16, py::arg("spec"),
          py::arg("li"), py::arg("M"), py::arg("gemm_prec"),
          py::arg("dtype"));
  mod.def("bwd_chain", &bwd_chain, py::arg("spec"), py::arg("scales"),
          py::arg("xb"), py::arg("theta"), py::arg("grad"),
          py::arg("acts"), py::arg("zs"), py::arg("dzs"),
          py::arg("idxs"), py::arg("loss_kind"), py::arg("Y_all"),
          py::arg("idx"), py::arg("graph_offs"), py::arg("pit"),
          py::arg("idx_stride"), py::arg("idx_off"), py::arg("yb"),
          py::arg("loss"), py::arg("loss_scale"), py::arg("M"),
          py::arg("zero_mode"), py::arg("gemm_prec") = 0);
}

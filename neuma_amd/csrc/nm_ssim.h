// The 11-tap Gaussian window and the LDS tile shape shared by the two SSIM kernels: the loss of loss_utils.py
// (nm_regist.hip: zero padding, fixed C1 / C2, value + adjoint) and the torchmetrics metric (nm_metrics.hip: valid windows only,
// C1 / C2 from the data range, fp64 moments).  Only the window and the tiling are common; the kernels stay separate.
#pragma once
#include <math.h>

constexpr int kTW = 64, kTH = 16, kR = 5, kWin = 2 * kR + 1;   // output tile 16 x 64 per workgroup, 5-pixel halo
constexpr int kLW = kTW + 2 * kR, kLH = kTH + 2 * kR;           // 74 x 26 loaded

struct Window {
  float w[kWin];
};

struct Window64 {
  double w[kWin];
};

static inline Window ssim_window() {
  // loss_utils.py:26-29: exp(-(x - 5)^2 / (2 sigma^2)) / sum, sigma = 1.5 (the reference builds it in fp32 from python floats)
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    g[k] = (double)(float)exp(-(double)((k - kR) * (k - kR)) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  Window W;
  for (int k = 0; k < kWin; ++k) W.w[k] = (float)(g[k] / sum);
  return W;
}

static inline Window64 ssim_window64() {
  // torchmetrics' _gaussian (kernel 11, sigma 1.5) in fp64: taps that sum to 1 within fp64 rounding.  The fp32 taps sum to
  // 1 + 3e-8, which a flat window turns into a variance of -3e-8 against C2 = 9e-4: 1e-4 of SSIM per flat pixel.
  double g[kWin], sum = 0.0;
  for (int k = 0; k < kWin; ++k) {
    g[k] = exp(-(double)((k - kR) * (k - kR)) / (2.0 * 1.5 * 1.5));
    sum += g[k];
  }
  Window64 W;
  for (int k = 0; k < kWin; ++k) W.w[k] = g[k] / sum;
  return W;
}

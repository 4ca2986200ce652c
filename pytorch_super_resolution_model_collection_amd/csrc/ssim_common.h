// What the device SSIM (ssim.hip: k_ssim_partial / k_ssim_final) and its host twin (srk_ssim_host) share: the 11-tap
// window, the three evaluation domains and the formula.  DESIGN.md 18 has the definition and the arithmetic.
#ifndef SRK_SSIM_COMMON_H_
#define SRK_SSIM_COMMON_H_
#include "color_common.h"

namespace srk {

constexpr int kSsimTaps = 11, kSsimHalo = kSsimTaps - 1;

// g[i] = exp(-(i - 5)^2 / (2 * 1.5^2)) / sum, to 17 significant digits (the doubles nearest to what numpy's exp gives,
// so the 11 values sum to 1 within one rounding; exp() is not a constant expression, hence literals).
struct SsimWindow {
  double g[kSsimTaps];
};
constexpr SsimWindow make_ssim_window() {
  return {{0.0010283800844791101, 0.007598758135239185, 0.036000772128430829, 0.10936068950970002, 0.21300553771125369,
           0.26601172486179436, 0.21300553771125369, 0.10936068950970002, 0.036000772128430829, 0.007598758135239185,
           0.0010283800844791101}};
}
static constexpr SsimWindow kSsimWinHost = make_ssim_window();
__constant__ const SsimWindow kSsimWinDev = make_ssim_window();

// The value of a pixel as it enters the moments.  'float': clamp(pred, 0, 1) against gt as it is, what k_psnr_partial
// compares.  'u8' / 'y8': the BYTE (0 .. 255, exact in fp32) of quant_u8, for 'y8' on three channels Pillow's luma of the
// three bytes; the moments are then taken with dynamic range L = 255, which is the same number as dividing by 255 first
// and never rounds i / 255.
__host__ __device__ __forceinline__ float ssim_pred_float(float v) { return fminf(fmaxf(v, 0.f), 1.f); }
__host__ __device__ __forceinline__ float ssim_luma(const int16_t* fwd, float r, float g, float b) {
  return (float)((fwd[quant_u8(r)] + fwd[256 + quant_u8(g)] + fwd[512 + quant_u8(b)]) >> 6);
}
__host__ __device__ __forceinline__ double ssim_range(int domain) { return domain == SRK_SSIM_FLOAT ? 1.0 : 255.0; }

// E[ab] - E[a] E[b]: the ONE expression that var_x, var_y and cov come from, so that identical planes give exactly the
// same numerator and denominator (one fused multiply-add, the same rounding on the host and on the device).
__host__ __device__ __forceinline__ double ssim_central(double eab, double ea, double eb) { return fma(-ea, eb, eab); }

// Wang et al. (2004), eq. 13, from the five windowed moments; range = L, C1 = (0.01 L)^2, C2 = (0.03 L)^2.
__host__ __device__ __forceinline__ double ssim_from_moments(double mx, double my, double exx, double eyy, double exy,
                                                             double range) {
#pragma clang fp contract(off)
  const double c1 = (0.01 * range) * (0.01 * range), c2 = (0.03 * range) * (0.03 * range);
  const double vx = ssim_central(exx, mx, mx), vy = ssim_central(eyy, my, my), cov = ssim_central(exy, mx, my);
  const double mxy = mx * my, mxx = mx * mx, myy = my * my;
  return ((2.0 * mxy + c1) * (2.0 * cov + c2)) / ((mxx + myy + c1) * (vx + vy + c2));
}

// The training loss 1 - mean(SSIM) (ssim_loss.hip; L = 1, pred unclamped): the map value S of one position
// -- the very expression of ssim_from_moments, so the loss of planes in [0, 1] is 1 - srk_ssim -- and what that
// position hands back to the pixels of its window through the adjoint G^T of the window:
//   d(sum S)/dx = G^T pm + 2 x * G^T pxx + y * G^T pxy,   pm = dS/dmx, pxx = dS/dexx, pxy = dS/dexy (include/srk.h).
// On flat planes the three terms are ~1/C2 = 1e3 times their sum, hence double to the end.
__host__ __device__ __forceinline__ double ssim_loss_terms(double mx, double my, double exx, double eyy, double exy,
                                                           double& pm, double& pxx, double& pxy) {
#pragma clang fp contract(off)
  const double c1 = 0.01 * 0.01, c2 = 0.03 * 0.03;
  const double vx = ssim_central(exx, mx, mx), vy = ssim_central(eyy, my, my), cov = ssim_central(exy, mx, my);
  const double mxy = mx * my, mxx = mx * mx, myy = my * my;
  const double a1 = 2.0 * mxy + c1, a2 = 2.0 * cov + c2, b1 = mxx + myy + c1, b2 = vx + vy + c2;
  const double s = (a1 * a2) / (b1 * b2);
  const double ib1 = 1.0 / b1, ib2 = 1.0 / b2;   // (three divisions a position instead of six: they are half its cost)
  pm = 2.0 * my * (a2 - a1) * ib1 * ib2 - 2.0 * mx * s * ib1 + 2.0 * mx * s * ib2;
  pxx = -s * ib2;
  pxy = 2.0 * a1 * ib1 * ib2;
  return s;
}

__host__ __device__ __forceinline__ double psnr_from_mse(double mse) {
  return mse == 0.0 ? 100.0 : 10.0 * log10(1.0 / mse);
}

}  // namespace srk
#endif  // SRK_SSIM_COMMON_H_

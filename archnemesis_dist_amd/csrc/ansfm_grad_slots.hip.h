// ansfm_grad_slots.hip.h -- the device functions the gradient kernels of ansfm_rt_kernels.hip.h, ansfm_transit_kernels.hip.h,
// ansfm_occultation_kernels.hip.h and ansfm_limb_kernels.hip.h share: how the g-contracted derivative of a layer's total
// opacity with respect to one parameter of dSPECOUT is put together (ForwardModel_0.py:3868-3872, :3989), and the Planck
// function with its temperature derivative (:6274-6281).  No kernel here.
#pragma once
#include <hip/hip_runtime.h>

namespace ansfm {

// sum_g w_g dTAUTOT[g][kpar][lay] before any x SCALE, for weights w_g the caller chose:
//   ys = sum_g w_g dk[slot][g] of the slot slot_of_param[kpar] points to (unused when slot < 0), Xs = sum_g w_g.
// A gas slot carries d tau / d amount per m^-2 (x 1e-4 to the reference's cm^-2, :3870); slot NP1 - 1 is the temperature
// (:3872).  dcont [n][NPAR][L][Wpad] (dTAUCON) and dcont_gas [L][Wpad] (one array for every gas parameter) may be nullptr.
__device__ __forceinline__ double dtau_param_gsum(int slot, double ys, double Xs, int NP1, const double *dcont, const double *dcont_gas,
                                                  size_t m, int NPAR, int NVMR, int kpar, int L, int lay, int Wpad, int nu)
{
    double v = 0.0;
    if (slot >= 0) v = ys * ((slot == NP1 - 1) ? 1.0 : 1.0e-4);      // :3870 / :3872
    if (dcont) v += dcont[((m * NPAR + kpar) * L + lay) * Wpad + nu] * Xs;
    if (dcont_gas && kpar < NVMR) v += dcont_gas[(size_t)lay * Wpad + nu] * Xs;
    return v;
}

// B and dB/dT of the Planck function at y (wavenumber, or wavelength when ispace != 0) and temperature T
// (ForwardModel_0.py:6274-6281), for k_thermal_rtg, the gradient seam and k_limb_planck
__device__ __forceinline__ void planckg_dev(int ispace, double y, double T, double &bb, double &dBdT)
{
    const double c1 = 1.1911e-12, c2 = 1.439;
    double a, ap;
    if (ispace == 0) { a = c1 * (y * y * y); ap = c1 * c2 * (y * y * y * y) / (T * T); }
    else { a = c1 * (y * y * y * y * y) / 1.0e4; ap = c1 * c2 * (y * y * y * y * y * y) / 1.0e4 / (T * T); }
    const double e = exp(c2 * y / T);
    const double b = e - 1.0;
    bb = a / b;
    dBdT = e * ap / (b * b);
}

}  // namespace ansfm

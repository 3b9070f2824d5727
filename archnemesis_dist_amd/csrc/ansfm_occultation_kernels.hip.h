// ansfm_occultation_kernels.hip.h -- solar occultation with analytic gradients on gfx950 (fp64): the tangent paths mixed to the
// measurement's geometries on the device, before anything of the size of dSPECOUT (NWAVE, NPAR, LIMAX, NPATH) is stored (unit:
// ansfm_occultation.hip).
//
// nemesisSOfmg (ForwardModel_0.py:983-1249) takes the transmission of the limb paths that bracket every tangent height of the
// measurement, maps dSPECOUT to the state vector path by path and only then interpolates to the tangent heights (:1208-1232).
// Every step after the transmission is linear, so the interpolation -- a sparse mixing matrix C (Q, P) from paths to outputs --
// is applied first.  With the path matrix Sm[l][p] = sum of SCALE over the entries of path p in layer l (both legs):
//     e[w,g,p]      = exp(-sum_l Sm[l][p] (TAUGAS[w,g,l] + cont[w,l]))         T[w,p]   = sum_g dg e[w,g,p]
//     MOD[w,q]      = xfac[w] sum_p C[q,p] T[w,p]
//     B[w,g,l,q]    = sum_p C[q,p] Sm[l][p] e[w,g,p]
//     dMOD[w,k,l,q] = -xfac[w] sum_g dg B[w,g,l,q] dTAUTOT[w,g,k,l]            (NaN -> 0 on this element, nan_to_num :4507)
// dMOD has the layout of the reference's dSPECOUT with LIMAX -> L and NPATH -> Q: 8 W NPAR L Q bytes, in HBM as a whole
// (slabbing the spectral axis to bound it is not done here).  k_occ_paths forms e, k_occ_grad the rest.  Sums run in a fixed
// order and nothing is accumulated atomically: equal inputs, equal bits.
//
// The path pass, the contraction and the block-row-0 sums are ansfm_pathmix_kernels.hip.h's, with the LDS budget of k_occ_grad;
// this header binds them to the occultation's columns.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_pathmix_kernels.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

struct OccParams {
    const double *tau;       // [L][G][Wpad]
    const double *cont;      // [L][Wpad] or nullptr
    const double *delg;      // [G]
    const double *xfac;      // [W] or nullptr (1)
    const int32_t *col_ptr;  // [P + 1] entries of path p in Sm: col_ptr[p] .. col_ptr[p + 1]
    const int32_t *col_lay;  // [nnz] their layers
    const double *col_val;   // [nnz] Sm[l][p]
    const int32_t *mix_ptr;  // [Q + 1] entries of geometry q in C
    const int32_t *mix_path; // [mix nnz] their paths
    const double *mix_val;   // [mix nnz] C[q][p]
    const int32_t *lq_ptr;   // [L Q + 1] entries of (layer l, geometry q) in C o Sm, at l Q + q
    const int32_t *lq_path;  // [lq nnz] their paths
    const double *lq_val;    // [lq nnz] C[q][p] Sm[l][p]
    double *tpart;           // [P][G][Wpad] e = exp(-tau_path) of every g-ordinate
    double *mod;             // [W][Q]
    double *trans;           // [W][P]
    double *dmod;            // [W][NPAR][L][Q]
    const double *dk;        // [L][NP1][G][Wpad]
    const double *dcont;     // [NPAR][L][Wpad] or nullptr
    const double *dcont_gas; // [L][Wpad] or nullptr (as RtGParams)
    int W, Wpad, G, L, P, Q;
    int NPAR, NVMR, NP1;
    int SC;                  // slots of dk a chunk stages
    unsigned gas_mask;
    signed char slot_of_param[kMaxPar];
};

// One wave per (wavenumber tile of 64, g): path_pass.  grid (Wpad / 64, G), block 64, LDS L x 512 B.
__global__ __launch_bounds__(kWave) void k_occ_paths(OccParams q)
{
    extern __shared__ double tile[];
    path_pass(q, tile);
}

// mix_contract with the columns dg B[g] = dg sum_i C[q][p_i] Sm[l][p_i] e[g][p_i] formed from tpart inside the loop (2 G loads of e
// per bracketing pair, from L2: e is P G Wpad doubles) and the value finished as -xfac v; block row 0 also writes T[w][p] and
// MOD[w][q].  grid (Wpad / 64, L), block 256, LDS (SC + kMixWaves) x G x 512 B.
__global__ __launch_bounds__(kMixWaves * kWave) void k_occ_grad(OccParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1);
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const size_t GWp = (size_t)q.G * q.Wpad;
    const double xf = mix_factor(q.xfac, nu, q.W);
    const int32_t *ptr = q.lq_ptr + (size_t)blockIdx.y * q.Q;
    mix_contract(
        q, lds, [&](int, int iq) { return ptr[iq] != ptr[iq + 1]; },
        [&](int iq, double *wg, double &Xs) {
            const int i0 = ptr[iq], i1 = ptr[iq + 1];
            for (int g = 0; g < q.G; ++g) {
                double b = 0.0;
                for (int i = i0; i < i1; ++i) b += q.lq_val[i] * q.tpart[(size_t)q.lq_path[i] * GWp + (size_t)g * q.Wpad + nu];
                b *= q.delg[g];
                wg[g * kWave + lane] = b;
                Xs += b;
            }
        },
        [&](double v, int, int) { return -xf * v; });
    if (blockIdx.y == 0) mix_path_sums(q, q.tpart, xf, q.trans);
}

}  // namespace ansfm

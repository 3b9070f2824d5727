// ansfm_transit_kernels.hip.h -- primary-transit depth with analytic gradients on gfx950 (fp64), collapsed before anything of
// the size of dSPECOUT (NWAVE, NPAR, LIMAX, NPATH) is stored (unit: ansfm_transit.hip).
//
// nemesisPTfm (ForwardModel_0.py:1838-1995) takes the transmission of one limb path per layer and integrates the absorbing
// annuli over tangent height by the trapezoid of :1949-1954:  AREA[w] = sum_p c_p (1 - T[w,p]).  With the path matrix
// Sm[l][p] = sum of SCALE over the entries of path p in layer l (both legs of the limb path):
//     tau_path[w,g,p] = sum_l Sm[l][p] (TAUGAS[w,g,l] + cont[w,l])       T[w,p] = sum_g dg exp(-tau_path)
//     A[w,g,l]        = sum_p c_p exp(-tau_path[w,g,p]) Sm[l][p]         dAREA[w,k,l] = sum_g dg A[w,g,l] dTAUTOT[w,g,k,l]
// (d(1 - T) = +exp dtau: the signs are folded in).  k_transit_sens forms A, k_transit_grad contracts it with the opacity
// derivatives of the gradient merge.  Sums run in a fixed order and nothing is accumulated atomically: equal inputs, equal bits.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_pathmix_kernels.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

// One wave per (wavenumber tile of 64, g).  The LDS tile [max(L, P)][64] holds the total opacity of every layer while the paths
// are summed (path_pass), then c_p exp(-tau_path) of every path while the layers are: a gather through Sm compressed by layer,
// whose indices and values are uniform over the wave as in the path pass.  A lane touches its own column of the tile and its own
// elements of tpart only, so no barrier is needed.  grid (Wpad / 64, G), block 64, LDS max(L, P) x 512 B.
__global__ __launch_bounds__(kWave) void k_transit_sens(TransitParams q)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x, g = blockIdx.y, G = q.G;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;      // < Wpad: every array read or written here is padded to it
    const size_t GWp = (size_t)G * q.Wpad, at = (size_t)g * q.Wpad + nu;
    path_pass(q, tile);
    for (int p = 0; p < q.P; ++p) tile[p * kWave + lane] = q.weight[p] * q.tpart[(size_t)p * GWp + at];
    for (int l = 0; l < q.L; ++l) {
        const int i1 = q.row_ptr[l + 1];
        double a = 0.0;
#pragma unroll 4
        for (int i = q.row_ptr[l]; i < i1; ++i) a += q.row_val[i] * tile[q.row_path[i] * kWave + lane];
        q.sens[(size_t)l * GWp + at] = a;
    }
}

// One wave per (wavenumber tile, row y): layer y's dAREA[w][k][y] for every parameter k, straight into the reference's layout
// [W][NPAR][L][1]; path y's T[w][y]; row 0 also AREA[w].  The opacity derivatives dk [L][NP1][G][Wpad] are read once, in whole
// 512-byte rows.  LDS [G + NP1][64]: dg A of every g-ordinate, then the contraction of every slot, a lane's own column again.
// NaN -> 0 (nan_to_num, :4507) on the collapsed element.  grid (Wpad / 64, max(L, P)), block 64.
__global__ __launch_bounds__(kWave) void k_transit_grad(TransitParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x, y = blockIdx.y, G = q.G, NP1 = q.NP1;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const size_t GWp = (size_t)G * q.Wpad;
    const bool live = nu < (size_t)q.W;
    if (y < q.L) {
        double *wg = lds, *ysl = lds + G * kWave;
        double Xs = 0.0;
        for (int g = 0; g < G; ++g) {
            const double w = q.delg[g] * q.sens[(size_t)y * GWp + (size_t)g * q.Wpad + nu];
            wg[g * kWave + lane] = w;
            Xs += w;
        }
        const double *dkl = q.dk + (size_t)y * NP1 * GWp + nu;
        for (int s = 0; s < NP1; ++s) {
            if (!((q.gas_mask >> (s == NP1 - 1 ? 31 : s)) & 1u)) continue;     // slot_of_param points away from it
            double ys = 0.0;
            for (int g = 0; g < G; ++g) ys += wg[g * kWave + lane] * dkl[((size_t)s * G + g) * q.Wpad];
            ysl[s * kWave + lane] = ys;
        }
        for (int kpar = 0; kpar < q.NPAR; ++kpar) {
            const int slot = q.slot_of_param[kpar];
            double v = dtau_param_gsum(slot, slot >= 0 ? ysl[slot * kWave + lane] : 0.0, Xs, NP1, q.dcont, q.dcont_gas, (size_t)0,
                                       q.NPAR, q.NVMR, kpar, q.L, y, q.Wpad, (int)nu);
            if (v != v) v = 0.0;
            if (live) q.darea[(nu * q.NPAR + kpar) * q.L + y] = v;
        }
    }
    if (y < q.P) {
        double T = 0.0;
        for (int g = 0; g < G; ++g) T += q.delg[g] * q.tpart[(size_t)y * GWp + (size_t)g * q.Wpad + nu];
        if (live) q.trans[nu * q.P + y] = T;
    }
    if (y == 0) {
        double area = 0.0;
        for (int p = 0; p < q.P; ++p) {
            double T = 0.0;
            for (int g = 0; g < G; ++g) T += q.delg[g] * q.tpart[(size_t)p * GWp + (size_t)g * q.Wpad + nu];
            area += q.weight[p] * (1.0 - T);
        }
        if (live) q.area[nu] = area;
    }
}

}  // namespace ansfm

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
// LDS budget of k_occ_grad (design statements, not measurements).  A block of 4 waves serves one (64-wavenumber tile, layer).
// Its LDS holds a chunk of SC slots of the layer's slab of dk, SC x G x 512 B, read from HBM once per block and shared by every
// geometry, and one column set dg B [G][64] per wave, 4 x G x 512 B.  The block is held to 80 KiB, half of the 160 KiB of a CU,
// so that two blocks (8 waves, 2 per SIMD) are resident and one block's staging of a chunk overlaps the other's contraction.
// At G = 20, S = 8: the waves' columns take 40 KiB, which leaves 40 KiB = 4 slots; the 9 slots go in 3 even chunks of 3
// (30 KiB + 40 KiB = 70 KiB a block, 2 blocks per CU).  Holding the whole slab (90 KiB + 40 KiB) would leave one block, 1 wave
// per SIMD, with nothing to hide the staging behind; a smaller budget (3 blocks at 53 KiB) would leave 1 slot a chunk and 9
// barrier pairs.  The price of a chunk is that a wave forms dg B of a geometry again (2 G loads of e per bracketing pair, from
// L2: e is P G Wpad doubles).  Where G is so large that 80 KiB hold no slot beside the columns, the block takes up to 160 KiB.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_merge_common.hip.h"
#include "ansfm_grad_slots.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

constexpr int kOccWaves = 4;                       // waves of a k_occ_grad block
constexpr size_t kOccLdsTwoBlocks = 80 * 1024;     // LDS of a block when two are to share a CU
constexpr size_t kOccLdsOneBlock = 160 * 1024;

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

// One wave per (wavenumber tile of 64, g): the first half of k_transit_sens.  The LDS tile [L][64] holds the total opacity of
// every layer while the paths are summed through Sm compressed by path; indices and values are uniform over the wave.  A lane
// touches its own column of the tile and its own elements of tpart only, so no barrier is needed.
// grid (Wpad / 64, G), block 64, LDS L x 512 B.
__global__ __launch_bounds__(kWave) void k_occ_paths(OccParams q)
{
    extern __shared__ double tile[];
    const int lane = threadIdx.x, g = blockIdx.y;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;      // < Wpad: every array read or written here is padded to it
    const size_t GWp = (size_t)q.G * q.Wpad, at = (size_t)g * q.Wpad + nu;
    for (int l = 0; l < q.L; ++l)
        tile[l * kWave + lane] = q.tau[(size_t)l * GWp + at] + (q.cont ? q.cont[(size_t)l * q.Wpad + nu] : 0.0);
    for (int p = 0; p < q.P; ++p) {
        const int i1 = q.col_ptr[p + 1];
        double t = 0.0;
#pragma unroll 4
        for (int i = q.col_ptr[p]; i < i1; ++i) t += q.col_val[i] * tile[q.col_lay[i] * kWave + lane];
        q.tpart[(size_t)p * GWp + at] = exp(-t);
    }
}

// One block of kOccWaves waves per (wavenumber tile, layer l); lanes run over wavenumbers.  The slots of the layer's slab of dk
// are staged in LDS in chunks of q.SC (slots the gas selection leaves out are neither staged nor read).  The geometries that
// have an entry in layer l are dealt to the waves in turn; for each of its geometries a wave forms dg B[g] in its own LDS
// columns, with their sum over g for the continuum terms, contracts every parameter whose slot lies in the chunk against the
// staged slab, goes through dtau_param_gsum as k_transit_grad does, and writes dMOD[w][k][l][q].  Parameters without a slot are
// written with the first chunk.  A geometry without an entry in the layer gets zeros without a read of tpart.  Block row 0 also
// writes T[w][p] and MOD[w][q].  grid (Wpad / 64, L), block 256, LDS (SC + kOccWaves) x G x 512 B.
__global__ __launch_bounds__(kOccWaves * kWave) void k_occ_grad(OccParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), l = blockIdx.y;
    const int G = q.G, NP1 = q.NP1, Q = q.Q;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const size_t GWp = (size_t)G * q.Wpad;
    const bool live = nu < (size_t)q.W;
    const double mxf = live ? (q.xfac ? -q.xfac[nu] : -1.0) : 0.0;
    double *slab = lds, *wg = lds + (size_t)q.SC * G * kWave + (size_t)wave * G * kWave;
    const double *dkl = q.dk + (size_t)l * NP1 * GWp + (size_t)blockIdx.x * kWave;
    const int32_t *ptr = q.lq_ptr + (size_t)l * Q;

    for (int c0 = 0; c0 < NP1; c0 += q.SC) {
        const int cn = min(q.SC, NP1 - c0);
        if (c0) __syncthreads();                                   // every wave is done with the chunk before
        for (int row = wave; row < cn * G; row += kOccWaves) {      // row = (slot - c0) G + g: 512 B of dk each
            const int s = c0 + row / G;
            if ((q.gas_mask >> (s == NP1 - 1 ? 31 : s)) & 1u)
                slab[row * kWave + lane] = dkl[((size_t)c0 * G + row) * q.Wpad + lane];
        }
        __syncthreads();
        int n = 0;
        for (int iq = 0; iq < Q; ++iq) {
            const int i0 = ptr[iq], i1 = ptr[iq + 1];
            if (i0 == i1) {                                        // no path of this geometry crosses the layer
                if (c0 == 0 && iq % kOccWaves == wave && live)
                    for (int kpar = 0; kpar < q.NPAR; ++kpar) q.dmod[((nu * q.NPAR + kpar) * q.L + l) * Q + iq] = 0.0;
                continue;
            }
            if (n++ % kOccWaves != wave) continue;
            double Xs = 0.0;
            for (int g = 0; g < G; ++g) {
                double b = 0.0;
                for (int i = i0; i < i1; ++i) b += q.lq_val[i] * q.tpart[(size_t)q.lq_path[i] * GWp + (size_t)g * q.Wpad + nu];
                b *= q.delg[g];
                wg[g * kWave + lane] = b;
                Xs += b;
            }
            for (int kpar = 0; kpar < q.NPAR; ++kpar) {
                const int slot = q.slot_of_param[kpar];
                if (slot < 0 ? c0 != 0 : (slot < c0 || slot >= c0 + cn)) continue;
                double ys = 0.0;
                if (slot >= 0) {
                    const double *sl = slab + (size_t)(slot - c0) * G * kWave + lane;
                    for (int g = 0; g < G; ++g) ys += wg[g * kWave + lane] * sl[g * kWave];
                }
                double v = mxf * dtau_param_gsum(slot, ys, Xs, NP1, q.dcont, q.dcont_gas, (size_t)0, q.NPAR, q.NVMR, kpar, q.L, l,
                                                 q.Wpad, (int)nu);
                if (v != v) v = 0.0;
                if (live) q.dmod[((nu * q.NPAR + kpar) * q.L + l) * Q + iq] = v;
            }
        }
    }
    if (l == 0) {
        for (int p = wave; p < q.P; p += kOccWaves) {
            double T = 0.0;
            for (int g = 0; g < G; ++g) T += q.delg[g] * q.tpart[(size_t)p * GWp + (size_t)g * q.Wpad + nu];
            if (live) q.trans[nu * q.P + p] = T;
        }
        for (int iq = wave; iq < Q; iq += kOccWaves) {
            double m = 0.0;
            for (int i = q.mix_ptr[iq]; i < q.mix_ptr[iq + 1]; ++i) {
                double T = 0.0;
                for (int g = 0; g < G; ++g) T += q.delg[g] * q.tpart[(size_t)q.mix_path[i] * GWp + (size_t)g * q.Wpad + nu];
                m += q.mix_val[i] * T;
            }
            if (live) q.mod[nu * Q + iq] = -mxf * m;
        }
    }
}

}  // namespace ansfm

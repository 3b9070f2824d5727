// ansfm_limb_kernels.hip.h -- limb thermal emission with analytic gradients on gfx950 (fp64): the tangent paths mixed to the
// measurement's geometries on the device, before anything of the size of dSPECOUT (NWAVE, NPAR, LIMAX, NPATH) is stored (unit:
// ansfm_limb.hip).
//
// nemesisLfmg (ForwardModel_0.py:1372-1521) takes the thermal emission of the limb paths that bracket every tangent height of
// the measurement, maps dSPECOUT to the state vector path by path and only then interpolates to the tangent heights
// (:1475-1496).  Every step after the radiative transfer is linear, so the interpolation -- a sparse mixing matrix C (Q, P) from
// paths to geometries -- is applied first.  Path p has the entries j < NLAYIN[p] with layer l_j, SCALE s_j, EMTEMP th_j
// (:6444-6476, as k_thermal_rtg):
//     tau_j[w,g]    = s_j (TAUGAS[w,g,l_j] + cont[w,l_j])          T_-1 = 1,  T_j = T_{j-1} exp(-tau_j)
//     spec[w,g,p]   = sum_j (T_{j-1} - T_j) B(th_j)
//     A_j[w,g,p]    = T_j B(th_j) - sum_{m>j} (T_{m-1} - T_m) B(th_m)                         (d spec / d tau_j)
//     E[w,g,l,q]    = sum_p C[q,p] sum_{j: l_j = l} s_j A_j[w,g,p]
//     Z[w,l,q]      = sum_g dg sum_p C[q,p] sum_{j: l_j = l} (T_{j-1} - T_j) dB/dT(th_j)
//     SPEC[w,p]     = sum_g dg spec[w,g,p]                          MOD[w,q] = xfac[w] sum_p C[q,p] SPEC[w,p]
//     dMOD[w,k,l,q] = xfac[w] (sum_g dg E[w,g,l,q] dTAUTOT[w,g,k,l] + [k == NVMR] Z[w,l,q])    (NaN -> 0 on this element)
// Limb paths only: the lower boundary contributes nothing (:6479-6483); the entry refuses a path that reaches the ground.  dMOD
// has the layout of the reference's dSPECOUT with LIMAX -> L and NPATH -> Q: 8 W NPAR L Q bytes, in HBM as a whole.  Sums run in a
// fixed order and nothing is accumulated atomically: equal inputs, equal bits.
//
// k_limb_planck fills B and dB/dT for every bit-distinct EMTEMP value (they do not depend on g), k_limb_sens forms spec, dg E
// and the partial sums of Z, k_limb_grad the rest.
//
// k_limb_sens.  One wave serves one (64-wavenumber tile, geometry, group of g-ordinates): the geometry and the g-groups are on
// the grid, not looped over inside a block of waves that covers all g, because a spectral window of 1024 wavenumbers has 16
// tiles only; with Q = 10 and 4 g-groups that is 640 waves.  The price: a path that two adjacent geometries share is walked once
// for each, and Z comes out as GS partial sums [GS][Q][L][Wpad] that k_limb_grad adds in order.  LDS: the rows E [L][64] of the
// current g and Z [L][64] of the group, 2 L x 512 B = L KiB, which caps L at 160 (the 160 KiB of a CU); a lane touches its own
// column only, so there is no barrier.  At L = 100 one block (one wave) is resident per CU, with nothing to hide its dependent
// loads and exp chain behind.  Measured once at W = 1024, G = 20, L = 100, Q = 10, P = 20: 2.74 ms with k_limb_planck, as long
// as the gradient merge, and 0.42 ms for k_limb_grad; the route as a whole 7.6 ms against 25.2 ms un-collapsed (DESIGN.md
// 4.2l).  A_j needs T_{j-1} on the way back; instead of parking T in HBM the forward pass runs twice and the tail sum is formed
// as spec - prefix_j.  That costs a second exp per entry and an absolute error of a few 2^-53 spec on A_j (the tail sum itself
// would carry that relative to the tail), far inside 1e-10 of the slab's largest element; it saves a workspace of LIMAX x 512 B
// a wave and its write and read.  The second pass repeats the first's operations in order, so its T_j are the first's bit for
// bit.
//
// The contraction of k_limb_grad and its block-row-0 sums are ansfm_pathmix_kernels.hip.h's, with their LDS budget; this header
// binds them to the limb's columns and its Z term.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_pathmix_kernels.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

constexpr int kLimbGroups = 4;                      // g-groups of k_limb_sens at most
constexpr int kLimbMaxLayers = 160;                 // 2 L x 512 B of LDS in k_limb_sens

struct LimbParams {
    const double *tau;        // [L][G][Wpad]
    const double *cont;       // [L][Wpad] or nullptr
    const double *delg;       // [G]
    const double *xfac;       // [W] or nullptr (1)
    const double *wave;       // [W]
    const int32_t *nlayin;    // [P]
    const int32_t *layinc;    // [LIMAX][P], read for j < nlayin[p] only
    const int32_t *tidx;      // [LIMAX][P] index of EMTEMP[j][p] among the distinct values
    const double *scale;      // [LIMAX][P]
    const double *tvals;      // [NT] the distinct EMTEMP values
    const int32_t *mix_ptr;   // [Q + 1] entries of geometry q in C
    const int32_t *mix_path;  // [mix nnz] their paths
    const int32_t *mix_first; // [mix nnz] 1: the first entry that names this path (it writes spec)
    const double *mix_val;    // [mix nnz] C[q][p]
    const int32_t *orphan;    // [n_orphan] paths no geometry names: spec only
    const int32_t *hit;       // [L][Q] 1: a path of geometry q has an entry in layer l
    double *btab, *dbtab;     // [NT][Wpad] B and dB/dT
    double *spec;             // [P][G][Wpad]
    double *E;                // [Q][L][G][Wpad] dg E, rows with hit only
    double *Zp;               // [GS][Q][L][Wpad] partial sums of Z over the g of a group, rows with hit only
    double *mod;              // [W][Q]
    double *specout;          // [W][P]
    double *dmod;             // [W][NPAR][L][Q]
    const double *dk;         // [L][NP1][G][Wpad]
    const double *dcont;      // [NPAR][L][Wpad] or nullptr
    const double *dcont_gas;  // [L][Wpad] or nullptr (as RtGParams)
    int W, Wpad, G, L, P, Q;
    int GS, NT, n_orphan, ispace;
    int NPAR, NVMR, NP1;
    int SC;                   // slots of dk a chunk stages
    unsigned gas_mask;
    signed char slot_of_param[kMaxPar];
};

// grid (Wpad / 64, NT), block 64: B and dB/dT of distinct temperature t at every wavenumber (padding lanes: the last one's)
__global__ __launch_bounds__(kWave) void k_limb_planck(LimbParams q)
{
    const size_t nu = (size_t)blockIdx.x * kWave + threadIdx.x;
    const double wv = q.wave[nu < (size_t)q.W ? nu : (size_t)q.W - 1];
    double bb, dB;
    planckg_dev(q.ispace, q.ispace == 0 ? wv : 1.0e4 / wv, q.tvals[blockIdx.y], bb, dB);
    q.btab[(size_t)blockIdx.y * q.Wpad + nu] = bb;
    q.dbtab[(size_t)blockIdx.y * q.Wpad + nu] = dB;
}

// The emission of path p at g-ordinate g: the forward pass of :6446-6452 (product form of the transmission, as k_thermal_rtg)
__device__ __forceinline__ double limb_forward(const LimbParams &q, int p, size_t at, size_t GWp, size_t nu)
{
    const int nl = q.nlayin[p];
    double T = 1.0, sp = 0.0;
    for (int j = 0; j < nl; ++j) {
        const size_t e = (size_t)j * q.P + p;
        const int l = q.layinc[e];
        const double t = (q.tau[(size_t)l * GWp + at] + (q.cont ? q.cont[(size_t)l * q.Wpad + nu] : 0.0)) * q.scale[e];
        const double Tn = T * exp(-t);
        sp += (T - Tn) * q.btab[(size_t)q.tidx[e] * q.Wpad + nu];
        T = Tn;
    }
    return sp;
}

// One wave per (wavenumber tile, geometry iq, g-group gs); lanes run over wavenumbers; indices and weights are uniform over the
// wave.  For every g of the group (g = gs, gs + GS, ...) and every path of the geometry's mix row: the forward pass (spec, stored
// by the first mix entry that names the path), then the same pass again with A_j = T_j B_j - (spec - prefix_j), accumulating
// C s_j A_j into the LDS row of layer l_j and C dg (T_{j-1} - T_j) dB/dT into the group's Z row.  Rows of layers with an entry
// (hit) are written out, dg E after every g and Z after the last.  Block row Q walks the paths no geometry names, for SPEC.
// grid (Wpad / 64, Q + 1 if there are such paths, GS), block 64, LDS 2 L x 512 B.
__global__ __launch_bounds__(kWave) void k_limb_sens(LimbParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x, iq = blockIdx.y, gs = blockIdx.z;
    const int G = q.G, L = q.L, Q = q.Q;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;      // < Wpad: every array read or written here is padded to it
    const size_t GWp = (size_t)G * q.Wpad;
    if (iq == Q) {
        for (int g = gs; g < G; g += q.GS)
            for (int o = 0; o < q.n_orphan; ++o) {
                const int p = q.orphan[o];
                const size_t at = (size_t)g * q.Wpad + nu;
                q.spec[(size_t)p * GWp + at] = limb_forward(q, p, at, GWp, nu);
            }
        return;
    }
    double *Et = lds + lane, *Zt = lds + (size_t)L * kWave + lane;
    const int i0 = q.mix_ptr[iq], i1 = q.mix_ptr[iq + 1];
    for (int l = 0; l < L; ++l) Zt[l * kWave] = 0.0;
    for (int g = gs; g < G; g += q.GS) {
        const double dg = q.delg[g];
        const size_t at = (size_t)g * q.Wpad + nu;
        for (int l = 0; l < L; ++l) Et[l * kWave] = 0.0;
        for (int i = i0; i < i1; ++i) {
            const int p = q.mix_path[i], nl = q.nlayin[p];
            const double c = q.mix_val[i], cdg = c * dg;
            const double sp = limb_forward(q, p, at, GWp, nu);
            if (q.mix_first[i]) q.spec[(size_t)p * GWp + at] = sp;
            double T = 1.0, pre = 0.0;
            for (int j = 0; j < nl; ++j) {
                const size_t e = (size_t)j * q.P + p;
                const int l = q.layinc[e];
                const double s = q.scale[e];
                const size_t tb = (size_t)q.tidx[e] * q.Wpad + nu;
                const double bb = q.btab[tb], dB = q.dbtab[tb];
                const double t = (q.tau[(size_t)l * GWp + at] + (q.cont ? q.cont[(size_t)l * q.Wpad + nu] : 0.0)) * s;
                const double Tn = T * exp(-t), d = T - Tn;
                pre += d * bb;
                Et[l * kWave] += (c * s) * (Tn * bb - (sp - pre));
                Zt[l * kWave] += cdg * (d * dB);
                T = Tn;
            }
        }
        for (int l = 0; l < L; ++l)
            if (q.hit[(size_t)l * Q + iq]) q.E[(((size_t)iq * L + l) * G + g) * q.Wpad + nu] = dg * Et[l * kWave];
    }
    for (int l = 0; l < L; ++l)
        if (q.hit[(size_t)l * Q + iq]) q.Zp[(((size_t)gs * Q + iq) * L + l) * q.Wpad + nu] = Zt[l * kWave];
}

// mix_contract with the columns dg E[g] copied from k_limb_sens's rows and the value finished as (v + Z at k == NVMR, the GS
// partial sums in order) xfac; block row 0 also writes SPEC[w][p] and MOD[w][q].
// grid (Wpad / 64, L), block 256, LDS (SC + kMixWaves) x G x 512 B.
__global__ __launch_bounds__(kMixWaves * kWave) void k_limb_grad(LimbParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x & (kWave - 1), l = blockIdx.y;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;
    const double xf = mix_factor(q.xfac, nu, q.W);
    const int32_t *hit = q.hit + (size_t)l * q.Q;
    mix_contract(
        q, lds, [&](int, int iq) { return hit[iq] != 0; },
        [&](int iq, double *wg, double &Xs) {
            const double *El = q.E + (((size_t)iq * q.L + l) * q.G) * q.Wpad + nu;
            for (int g = 0; g < q.G; ++g) {
                const double b = El[(size_t)g * q.Wpad];
                wg[g * kWave + lane] = b;
                Xs += b;
            }
        },
        [&](double v, int kpar, int iq) {
            if (kpar == q.NVMR) {                                  // :6467-6468
                double Z = 0.0;
                for (int gs = 0; gs < q.GS; ++gs) Z += q.Zp[(((size_t)gs * q.Q + iq) * q.L + l) * q.Wpad + nu];
                v += Z;
            }
            return v * xf;                                         // :4247
        });
    if (l == 0) mix_path_sums(q, q.spec, xf, q.specout);
}

}  // namespace ansfm

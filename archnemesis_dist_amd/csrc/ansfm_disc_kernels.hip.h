// ansfm_disc_kernels.hip.h -- disc-averaged thermal emission with analytic gradients on gfx950 (fp64): the averaging points of
// an unresolved planet mixed to the measurement's geometries on the device, before anything of the size of dSPECOUT
// (NWAVE, NPAR, NLAYIN, 1) per point is stored (unit: ansfm_disc.hip).
//
// nemesisdiscfmg (ForwardModel_0.py:1719-1834) runs process_IAV (:1998-2078) once per averaging point -- paths, CIRSrad with
// gradients, map2pro, map2xvec -- and only then forms the weighted sum with WGEOM (:1789-1794).  Every step after the radiative
// transfer is linear, so the sum -- a mixing matrix C (Q, P) from points to geometries -- is applied first.  The points of a
// geometry are paths through ONE layer sequence (calc_pathg sets LAYANG = 0 for every emission angle >= 0, :3118) that differ in
// SCALE only: N entries j with layer l_j and temperature th_j, SCALE s_jp for path p.  Unlike the limb case the sequence may end
// at the lower boundary (:6479-6498), which then emits R and contributes dTSURF:
//     tau_jp[w,g]   = s_jp (TAUGAS[w,g,l_j] + cont[w,l_j])          T_-1,p = 1,  T_jp = T_{j-1,p} exp(-tau_jp)
//     ground        = lay_press[l_{N-1}] > lay_press[l_{int(N/2)-1}]                           (host; index -1 wraps, as in Python)
//     R, dR         = TSURF <= 0 ? B, dB/dT at th_{N-1} : EMISSIVITY[w] x (B, dB/dT at TSURF)                    (:6485-6491)
//     spec[w,g,p]   = sum_j (T_{j-1,p} - T_jp) B(th_j) + [ground] T_{N-1,p} R
//     A_jp          = T_jp B(th_j) - sum_{m>j} (T_{m-1,p} - T_mp) B(th_m) - [ground] T_{N-1,p} R          (d spec_p / d tau_jp)
//     E[w,g,l,q]    = sum_p C[q,p] sum_{j: l_j = l} s_jp A_jp
//     Z[w,l,q]      = sum_g dg sum_p C[q,p] sum_{j: l_j = l} (T_{j-1,p} - T_jp) dB/dT(th_j)
//     SPEC[w,p]     = sum_g dg spec[w,g,p]                           MOD[w,q] = xfac[w] sum_p C[q,p] SPEC[w,p]
//     dTSMOD[w,q]   = xfac[w] sum_g dg sum_p C[q,p] [ground] T_{N-1,p} dR                                        (:6494, :4246)
//     dMOD[w,k,l,q] = xfac[w] (sum_g dg E[w,g,l,q] dTAUTOT[w,g,k,l] + [k == NVMR] Z[w,l,q])    (NaN -> 0 on this element)
// The reference's quirks stay: with TSURF <= 0, dTSMOD is still T_end dB/dT(th_{N-1}), and the bottom layer's temperature column
// gets no dR term.  dMOD has the layout of the reference's dSPECOUT with NLAYIN -> L and NPATH -> Q.  Sums run in a fixed order
// and nothing is accumulated atomically: equal inputs, equal bits.
//
// k_disc_planck fills B and dB/dT for every bit-distinct th_j and, in one more row, R and dR of the ground (k_limb_planck's
// scheme); k_disc_sens forms spec, dg E, the partial sums of Z and the ground's sum_p C T_end dR; k_disc_grad the rest.
//
// k_disc_sens.  One wave serves one (64-wavenumber tile, geometry, group of g-ordinates), lanes over wavenumbers, as
// k_limb_sens.  What differs: the paths of the geometry's mix row walk the sequence in lock-step, kDiscChunk = 8 at a time.  Per
// entry the wave reads tau[l_j], cont[l_j], B and dB/dT ONCE for the chunk (k_limb_sens reads them once per path and pass); the
// per-path T_p, prefix, spec_p and ground term live in registers (arrays of kDiscChunk with compile-time indices after full
// unrolling; a short chunk skips its absent paths by a wave-uniform test), and the chunk makes ONE accumulation per entry into
// the LDS rows E[l][64] and Z[l][64] instead of one per path.  The two forward passes of k_limb_sens stay (the tail sum is
// spec_atm - prefix_j, the ground term T_end R subtracted explicitly; the second pass repeats the first's operations in order,
// so its T_jp are the first's bit for bit).  LDS: 2 L x 512 B = L KiB, which caps L at 160; a lane touches its own column only,
// so there is no barrier.  Budget: at kDiscChunk = 8 the per-path state is 4 doubles x 8 = 64 VGPRs beside the entry's operands
// and the unrolled exp chains; the compiler reports 166 VGPRs (3 waves a SIMD), ScratchSize 0 and no VGPR spill.  LDS, not
// registers, limits occupancy (L = 100: 100 KiB, one block a CU).  The issue behind this kernel asked that nothing spill; that
// is not met for the scalar file: the compiler reports 40 SGPR spills, to VGPR lanes (v_writelane / v_readlane, no memory), all
// of them outside the per-path exp steps (k_limb_sens: 23).  Tried and not kept, none of them brought the count down: a chunk of
// 4 (33), the chunk's weights in LDS instead of scalar registers (45), the workspace and index pointers derived in the kernel
// from two bases instead of passed (58).  Measured at W = 1024, G = 20, L = 100 with k_disc_planck: 0.35 ms for 3 paths, 0.59 ms
// for 8.
//
// The grid.  The override sends Q = 1; with the limb kernel's 4 g-groups a window of 1024 wavenumbers would be 16 x 1 x 4 = 64
// waves on 256 CUs.  So the number of g-groups grows until the grid has 256 blocks or every g has its own:
//     GS = min(G, max(4, ceil(256 / ((Wpad / 64) x rows)))),   rows = Q + (1 if some path is named by no geometry)
// (disc_groups below; include/ansfm.h states it with the scratch).  Z comes out as GS partial sums [GS][Q][L][Wpad] that
// k_disc_grad adds in order.
//
// The contraction of k_disc_grad and its block-row-0 sums are ansfm_pathmix_kernels.hip.h's, with their LDS budget; this header
// binds them to the disc's columns, its Z term and dTSMOD.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_pathmix_kernels.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

constexpr int kDiscChunk = 8;                       // paths that walk the sequence in lock-step
constexpr int kDiscMinGroups = 4;                   // g-groups of k_disc_sens at least (where G allows)
constexpr int kDiscFillBlocks = 256;                // blocks of k_disc_sens the g-groups are to reach
constexpr int kDiscMaxLayers = 160;                 // 2 L x 512 B of LDS in k_disc_sens

// g-groups of k_disc_sens for `tiles` wavenumber tiles and `rows` block rows (the formula above)
inline int disc_groups(int G, int tiles, int rows)
{
    const int per = tiles * rows;
    return std::min(G, std::max(kDiscMinGroups, (kDiscFillBlocks + per - 1) / per));
}

struct DiscParams {
    const double *tau;        // [L][G][Wpad]
    const double *cont;       // [L][Wpad] or nullptr
    const double *delg;       // [G]
    const double *xfac;       // [W] or nullptr (1)
    const double *wave;       // [W]
    const double *emis;       // [W] or nullptr (TSURF <= 0)
    const int32_t *layinc;    // [N]
    const int32_t *tidx;      // [N] index of EMTEMP[j] among the distinct values
    const double *scale;      // [N][P]
    const double *smix;       // [N][mix nnz] SCALE[j][mix_path[i]]: a chunk's scales lie side by side
    const double *tvals;      // [NT] the distinct EMTEMP values
    const int32_t *mix_ptr;   // [Q + 1] entries of geometry q in C
    const int32_t *mix_path;  // [mix nnz] their paths
    const int32_t *mix_first; // [mix nnz] 1: the first entry that names this path (it writes spec)
    const double *mix_val;    // [mix nnz] C[q][p]
    const int32_t *orphan;    // [n_orphan] paths no geometry names: spec only
    const int32_t *hit;       // [L][Q] 1: geometry q has a path and the sequence an entry in layer l
    double *btab, *dbtab;     // [NT + 1][Wpad] B and dB/dT; row NT: R and dR of the ground
    double *spec;             // [P][G][Wpad]
    double *E;                // [Q][L][G][Wpad] dg E, rows with hit only
    double *Zp;               // [GS][Q][L][Wpad] partial sums of Z over the g of a group, rows with hit only
    double *tsg;              // [Q][G][Wpad] sum_p C [ground] T_end dR
    double *mod;              // [W][Q]
    double *dtsmod;           // [W][Q]
    double *specout;          // [W][P]
    double *dmod;             // [W][NPAR][L][Q]
    const double *dk;         // [L][NP1][G][Wpad]
    const double *dcont;      // [NPAR][L][Wpad] or nullptr
    const double *dcont_gas;  // [L][Wpad] or nullptr (as RtGParams)
    double tsurf;
    int W, Wpad, G, L, P, Q, N, mnz;
    int GS, NT, n_orphan, ispace, ground;
    int NPAR, NVMR, NP1;
    int SC;                   // slots of dk a chunk stages
    unsigned gas_mask;
    signed char slot_of_param[kMaxPar];
};

// grid (Wpad / 64, NT + 1), block 64: B and dB/dT of distinct temperature t at every wavenumber (padding lanes: the last
// one's); row NT: the ground's R and dR of :6485-6491
__global__ __launch_bounds__(kWave) void k_disc_planck(DiscParams q)
{
    const size_t nu = (size_t)blockIdx.x * kWave + threadIdx.x;
    const size_t wi = nu < (size_t)q.W ? nu : (size_t)q.W - 1;
    const double wv = q.wave[wi];
    const int t = blockIdx.y;
    const bool surface = t == q.NT && q.tsurf > 0.0;
    const double temp = t < q.NT ? q.tvals[t] : (surface ? q.tsurf : q.tvals[q.tidx[q.N - 1]]);
    double bb, dB;
    planckg_dev(q.ispace, q.ispace == 0 ? wv : 1.0e4 / wv, temp, bb, dB);
    if (surface) { bb *= q.emis[wi]; dB *= q.emis[wi]; }
    q.btab[(size_t)t * q.Wpad + nu] = bb;
    q.dbtab[(size_t)t * q.Wpad + nu] = dB;
}

// The emission of one path at g-ordinate g with the ground's term: for the paths no geometry names
__device__ __forceinline__ double disc_forward_one(const DiscParams &q, int p, size_t at, size_t GWp, size_t nu)
{
    double T = 1.0, sp = 0.0;
    for (int j = 0; j < q.N; ++j) {
        const int l = q.layinc[j];
        const double t = (q.tau[(size_t)l * GWp + at] + (q.cont ? q.cont[(size_t)l * q.Wpad + nu] : 0.0)) * q.scale[(size_t)j * q.P + p];
        const double Tn = T * exp(-t);
        sp += (T - Tn) * q.btab[(size_t)q.tidx[j] * q.Wpad + nu];
        T = Tn;
    }
    return q.ground ? sp + T * q.btab[(size_t)q.NT * q.Wpad + nu] : sp;
}

// One wave per (wavenumber tile, geometry iq, g-group gs); lanes run over wavenumbers; indices, weights and SCALE are uniform
// over the wave (SCALE is staged a second time by mix entry, smix, so that a chunk reads its scales of an entry side by side).
// For every g of the group (g = gs, gs + GS, ...) and every chunk of kDiscChunk paths of the geometry's mix row: the forward
// pass of all the chunk's paths in lock-step (spec, stored by the first mix entry that names a path), then the same pass again
// with A_jp = T_jp B_j - (spec_atm,p - prefix_jp) - [ground] T_end,p R, adding sum_p C s_jp A_jp to the LDS row of layer l_j and
// dg sum_p C (T_{j-1,p} - T_jp) dB/dT to the group's Z row, each once per entry.  Rows of layers with an entry (hit) are written
// out, dg E after every g and Z after the last; sum_p C [ground] T_end,p dR goes to tsg per g.  Block row Q walks the paths no
// geometry names, for SPEC.  grid (Wpad / 64, Q + 1 if there are such paths, GS), block 64, LDS 2 L x 512 B.
__global__ __launch_bounds__(kWave) void k_disc_sens(DiscParams q)
{
    extern __shared__ double lds[];
    const int lane = threadIdx.x, iq = blockIdx.y, gs = blockIdx.z;
    const int G = q.G, L = q.L, Q = q.Q, N = q.N;
    const size_t nu = (size_t)blockIdx.x * kWave + lane;      // < Wpad: every array read or written here is padded to it
    const size_t GWp = (size_t)G * q.Wpad;
    if (iq == Q) {
        for (int g = gs; g < G; g += q.GS)
            for (int o = 0; o < q.n_orphan; ++o) {
                const int p = q.orphan[o];
                const size_t at = (size_t)g * q.Wpad + nu;
                q.spec[(size_t)p * GWp + at] = disc_forward_one(q, p, at, GWp, nu);
            }
        return;
    }
    // what the entry loops read lies behind per-lane pointers: the scalar registers are left to the chunk's weights and scales
    double *Et = lds + lane, *Zt = lds + (size_t)L * kWave + lane;
    const int i0 = q.mix_ptr[iq], i1 = q.mix_ptr[iq + 1], Wpad = q.Wpad, ground = q.ground;
    const double *bt = q.btab + nu, *dbt = q.dbtab + nu, *contl = q.cont ? q.cont + nu : nullptr;
    const int32_t *layinc = q.layinc, *tidx = q.tidx;
    const double R = ground ? bt[(size_t)q.NT * Wpad] : 0.0, dR = ground ? dbt[(size_t)q.NT * Wpad] : 0.0;
    for (int l = 0; l < L; ++l) Zt[l * kWave] = 0.0;
    for (int g = gs; g < G; g += q.GS) {
        const double dg = q.delg[g];
        const size_t at = (size_t)g * Wpad + nu;
        const double *taul = q.tau + at;
        double ts = 0.0;
        for (int l = 0; l < L; ++l) Et[l * kWave] = 0.0;
        for (int c0 = i0; c0 < i1; c0 += kDiscChunk) {
            const int np = min(kDiscChunk, i1 - c0);
            const double *smix = q.smix + c0;
            const size_t mnz = (size_t)q.mnz;
            double ck[kDiscChunk], T[kDiscChunk], sp[kDiscChunk], gt[kDiscChunk];
#pragma unroll
            for (int k = 0; k < kDiscChunk; ++k) {
                ck[k] = k < np ? q.mix_val[c0 + k] : 0.0;
                T[k] = 1.0; sp[k] = 0.0;
            }
            for (int j = 0; j < N; ++j) {
                const int l = layinc[j];
                const double base = taul[(size_t)l * GWp] + (contl ? contl[(size_t)l * Wpad] : 0.0);
                const double bb = bt[(size_t)tidx[j] * Wpad];
                const double *sj = smix + (size_t)j * mnz;
#pragma unroll
                for (int k = 0; k < kDiscChunk; ++k)
                    if (k < np) {
                        const double Tn = T[k] * exp(-(base * sj[k]));
                        sp[k] += (T[k] - Tn) * bb;
                        T[k] = Tn;
                    }
            }
#pragma unroll
            for (int k = 0; k < kDiscChunk; ++k)
                if (k < np) {
                    gt[k] = ground ? T[k] * R : 0.0;                   // :6493
                    ts += ck[k] * T[k];                                // :6494, times dR below
                    if (q.mix_first[c0 + k]) q.spec[(size_t)q.mix_path[c0 + k] * GWp + at] = ground ? sp[k] + gt[k] : sp[k];
                    T[k] = 1.0;
                }
            double pre[kDiscChunk];
#pragma unroll
            for (int k = 0; k < kDiscChunk; ++k) pre[k] = 0.0;
            for (int j = 0; j < N; ++j) {
                const int l = layinc[j];
                const double base = taul[(size_t)l * GWp] + (contl ? contl[(size_t)l * Wpad] : 0.0);
                const size_t tb = (size_t)tidx[j] * Wpad;
                const double bb = bt[tb], dB = dbt[tb];
                const double *sj = smix + (size_t)j * mnz;
                double ea = 0.0, za = 0.0;
#pragma unroll
                for (int k = 0; k < kDiscChunk; ++k)
                    if (k < np) {
                        const double s = sj[k];
                        const double Tn = T[k] * exp(-(base * s)), d = T[k] - Tn;
                        pre[k] += d * bb;
                        ea += (ck[k] * s) * (Tn * bb - (sp[k] - pre[k]) - gt[k]);      // :6498 with dtolddq = -dtau T_end
                        za += ck[k] * (d * dB);
                        T[k] = Tn;
                    }
                Et[l * kWave] += ea;
                Zt[l * kWave] += dg * za;
            }
        }
        for (int l = 0; l < L; ++l)
            if (q.hit[(size_t)l * Q + iq]) q.E[(((size_t)iq * L + l) * G + g) * Wpad + nu] = dg * Et[l * kWave];
        q.tsg[((size_t)iq * G + g) * Wpad + nu] = ground ? ts * dR : 0.0;
    }
    for (int l = 0; l < L; ++l)
        if (q.hit[(size_t)l * Q + iq]) q.Zp[(((size_t)gs * Q + iq) * L + l) * Wpad + nu] = Zt[l * kWave];
}

// mix_contract with the columns dg E[g] copied from k_disc_sens's rows and the value finished as (v + Z at k == NVMR, the GS
// partial sums in order) xfac; block row 0 also writes SPEC[w][p], MOD[w][q] and dTSMOD[w][q] = xfac sum_g dg tsg[q][g].
// grid (Wpad / 64, L), block 256, LDS (SC + kMixWaves) x G x 512 B.
__global__ __launch_bounds__(kMixWaves * kWave) void k_disc_grad(DiscParams q)
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
    if (l == 0) {
        mix_path_sums(q, q.spec, xf, q.specout);
        const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x / kWave);
        for (int iq = wave; iq < q.Q; iq += kMixWaves) {
            double s = 0.0;
            for (int g = 0; g < q.G; ++g) s += q.delg[g] * q.tsg[((size_t)iq * q.G + g) * q.Wpad + nu];
            if (nu < (size_t)q.W) q.dtsmod[nu * q.Q + iq] = xf * s;        // :4246
        }
    }
}

}  // namespace ansfm

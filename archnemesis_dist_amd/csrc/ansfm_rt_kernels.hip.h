// ansfm_rt_kernels.hip.h -- RT kernels of the correlated-k path: thermal emission, transmission and single scattering, the
// prefix sharing of a batch, the analytic gradients and the array-level gradient seam (unit: ansfm_rt.hip).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_merge_common.hip.h"
#include "ansfm_grad_slots.hip.h"
#include "ansfm_rt_params.h"

namespace ansfm {

// ------------------------------------------------------------------------------------------------
// K3+K4+K5+K6 fused: total opacity, LAYINC gather * SCALE, layer loop with Planck emission,
// ground / solar terms, unit factor and g-quadrature.   "thermal_rt"
// Block = 64 wavenumbers x GY g-groups; thread (lane, gy) integrates g = gy, gy+GY, ...
// ------------------------------------------------------------------------------------------------
constexpr int kGY = 8;       // g-groups per block of the forward RT kernel (157 wavenumber tiles at C2: more waves per tile)
constexpr int kGPer = kMaxG / kGY;  // 4

// same[m][lay] = the opacity row of (m, lay) is state 0's row and (cont != nullptr) so is its continuum, bit for bit.
// grid (L, n - 1), block 256
__global__ void k_rt_same(int L, int Wpad, const int32_t *__restrict__ slot, const double *__restrict__ cont, unsigned char *same)
{
    const int lay = blockIdx.x, m = blockIdx.y + 1;
    int differs = slot[(size_t)m * L + lay] != slot[lay];
    if (!differs && cont) {
        const long long *a = reinterpret_cast<const long long *>(cont + ((size_t)m * L + lay) * Wpad);
        const long long *b = reinterpret_cast<const long long *>(cont + (size_t)lay * Wpad);
        for (int i = threadIdx.x; i < Wpad; i += blockDim.x) differs |= (a[i] != b[i]);
    }
    differs = __syncthreads_or(differs);
    if (threadIdx.x == 0) same[(size_t)m * L + lay] = differs ? 0 : 1;
}

// Single scattering (mode 2 on sca / phase): same[m][ip][lay] = as k_rt_same, and the scattering opacity of (m, lay) and the
// phase function of path ip there are state 0's as well, bit for bit.  cont / sca [n][L][Wpad], phase [n][P][L][Wpad].
// grid (L, n - 1), block 256
__global__ void k_rt_same_ss(int L, int Wpad, int P, const int32_t *__restrict__ slot, const double *__restrict__ cont,
                             const double *__restrict__ sca, const double *__restrict__ phase, unsigned char *same)
{
    const int lay = blockIdx.x, m = blockIdx.y + 1;
    int differs = slot[(size_t)m * L + lay] != slot[lay];
    for (int c = 0; c < 2 && !differs; ++c) {
        const double *arr = c ? sca : cont;
        if (!arr) continue;
        const long long *a = reinterpret_cast<const long long *>(arr + ((size_t)m * L + lay) * Wpad);
        const long long *b = reinterpret_cast<const long long *>(arr + (size_t)lay * Wpad);
        for (int i = threadIdx.x; i < Wpad; i += blockDim.x) differs |= (a[i] != b[i]);
    }
    differs = __syncthreads_or(differs);               // block-uniform from here on
    for (int ip = 0; ip < P; ++ip) {
        int d = differs;
        if (!d) {
            const long long *a = reinterpret_cast<const long long *>(phase + (((size_t)m * P + ip) * L + lay) * Wpad);
            const long long *b = reinterpret_cast<const long long *>(phase + ((size_t)ip * L + lay) * Wpad);
            for (int i = threadIdx.x; i < Wpad; i += blockDim.x) d |= (a[i] != b[i]);
            d = __syncthreads_or(d);
        }
        if (threadIdx.x == 0) same[((size_t)m * P + ip) * L + lay] = d ? 0 : 1;
    }
}

// jstart[m][ip] = number of leading layers of path ip that state m shares with state 0 (one wave per (m, ip); m = 0: 0)
// per_path: same is k_rt_same_ss's [n][P][L], not k_rt_same's [n][L]
__global__ __launch_bounds__(64) void k_rt_jstart(int n, int L, int P, int LIMAX, const int32_t *__restrict__ nlayin,
                                                  const int32_t *__restrict__ layinc, const double *__restrict__ scale,
                                                  const double *__restrict__ emtemp, const unsigned char *__restrict__ same,
                                                  int32_t *jstart, int per_path)
{
    const int idx = blockIdx.x, lane = threadIdx.x;
    const int m = idx / P, ip = idx % P;
    int first = 0;
    if (m > 0) {
        const int nl = nlayin[ip];
        const size_t pm = (size_t)m * LIMAX * P + ip, p0 = ip;
        const unsigned char *same_m = same + (per_path ? ((size_t)m * P + ip) * L : (size_t)m * L);
        first = nl;
        for (int j0 = 0; j0 < nl; j0 += 64) {
            const int j = j0 + lane;
            bool bad = false;
            if (j < nl) {
                const int lay = layinc[(size_t)j * P + ip];
                bad = !same_m[lay] ||
                      __double_as_longlong(scale[pm + (size_t)j * P]) != __double_as_longlong(scale[p0 + (size_t)j * P]) ||
                      __double_as_longlong(emtemp[pm + (size_t)j * P]) != __double_as_longlong(emtemp[p0 + (size_t)j * P]);
            }
            const unsigned long long hit = __builtin_amdgcn_ballot_w64(bad);
            if (hit != 0) { first = j0 + __builtin_ctzll(hit); break; }
        }
    }
    if (lane == 0) jstart[idx] = first;
}

__device__ __forceinline__ double planck_bb(double a, double c2y, double T)
{
    return a / (exp(c2y / T) - 1.0);  // ForwardModel_0.py:6223-6225
}

// BATCH: the build for many models per launch (a Jacobian's states).  One block is eight waves, two per SIMD; at the
// kernel's natural 142 registers a second block does not fit on the CU, and a batch has the blocks to fill it: capped at 128
// (14 spilled) the 201 states of a C3 Jacobian take 9.2 instead of 11.4 ms.  A single model has 157 blocks for 256 CUs and
// only pays for the spills (0.093 -> 0.107 ms): it keeps the uncapped build.
// SS: the build for mode 2 on the vertical opacities (p.sca, p.phase with a model axis; CIRSrad's single-scattering branch):
// the scattering opacity and the phase function of layer j + 1 are fetched with its opacities, ahead of layer j's arithmetic.
// The other builds keep the run-time p.mode (the array-level seam's p.omega among them) and are not touched by it.
// SS == 2: the same on rows (p.ss_by_row: sca [rows][Wpad], phase [P][rows][Wpad], read through the opacity row of the layer like
// a continuum by row) -- builds of their own, so that the dense SS builds keep their code.
template <bool BATCH, int PREFIX = 0, int SS = 0>
__global__ __launch_bounds__(kWave *kGY) __attribute__((amdgpu_waves_per_eu(BATCH ? 4 : 1, BATCH ? 4 : 8))) void k_thermal_rt(RtParams p)
{
    __shared__ double red[kGY][kWave];
    const int lane = threadIdx.x, gy = threadIdx.y;
    // grid = (models, paths, wavenumber tiles): the models of a batch that share opacity rows (de-duplicated Jacobian
    // states) run next to each other on a wavenumber tile, so the rows are re-read out of L2 instead of HBM
    const int nu = blockIdx.z * kWave + lane;
    const int nuc = nu < p.W ? nu : p.W - 1;
    const int ip = blockIdx.y, m = blockIdx.x + (PREFIX != 0 ? p.m0 : 0);
    const int nl = p.nlayin[ip];
    const int G = p.G;
    const double c1 = 1.1911e-12, c2 = 1.439;  // ForwardModel_0.py:6214-6215
    const double wv = p.wave[nuc];
    double y, a;
    if (p.ispace == 0) { y = wv; a = c1 * (y * y * y); }
    else { y = 1.0e4 / wv; a = c1 * (y * y * y * y * y) / 1.0e4; }
    const double c2y = c2 * y;

    double taud[kGPer], trold[kGPer], spec[kGPer];
#pragma unroll
    for (int k = 0; k < kGPer; ++k) { taud[k] = 0.0; trold[k] = 1.0; spec[k] = 0.0; }

    const size_t pathbase = (size_t)m * p.LIMAX * p.P + ip;
    // Per-layer metadata of the path (opacity row, SCALE, Planck function at EMTEMP) once into LDS: the layer loop then
    // has no dependent index -> row -> data chain, and the opacity loads of layer j+1 are issued before layer j is
    // integrated (the loop is a serial recurrence in the optical depth; without this it runs at memory latency).
    extern __shared__ double rt_meta[];                 // [3][LIMAX]: row index (as double), scale, B(nu-independent part: T)
    double *m_row = rt_meta, *m_sc = rt_meta + p.LIMAX, *m_T = rt_meta + 2 * p.LIMAX;
    for (int j = lane + gy * kWave; j < nl; j += kWave * kGY) {
        const int lay = p.layinc[(size_t)j * p.P + ip];
        const size_t ri = p.tau_slot ? (size_t)p.tau_slot[(size_t)m * p.L + lay] : (size_t)m * p.L + lay;
        m_row[j] = (double)ri;                          // < 2^53, exact
        m_sc[j] = p.scale[pathbase + (size_t)j * p.P];
        m_T[j] = p.emtemp[pathbase + (size_t)j * p.P];
        rt_meta[3 * p.LIMAX + j] = (double)lay;
    }
    __syncthreads();
    const double *m_lay = rt_meta + 3 * p.LIMAX;
    auto fetch = [&](int j, double tv[kGPer], double &tc, double &em) {
        const size_t ri = (size_t)m_row[j];
        const int lay = (int)m_lay[j];
        const double *trow = p.tau + (ri * G) * p.Wpad + nu;
        tc = p.cont ? p.cont[(p.cont_by_row ? ri : (size_t)m * p.L + lay) * p.Wpad + nu] : 0.0;
        em = p.emi ? p.emi[(size_t)j * p.Wpad + nu] : 0.0;
#pragma unroll
        for (int k = 0; k < kGPer; ++k) {
            const int g = gy + k * kGY;
            tv[k] = (g < G) ? trow[(size_t)g * p.Wpad] : 0.0;
        }
    };
    // mode 2 (single scattering): ssfac = mu0 / (mu0 + mu) and the solar flux over 4 pi, wave-uniform per path (:6557-6559)
    const double PI_ = 3.141592653589793;
    double ssfac = 0.0, mu0s = 0.0, sflux = 0.0;
    if (SS != 0 || p.mode == 2) {
        const double mu = cos(p.emiss_ang[ip] / 180. * PI_);
        mu0s = cos(p.sol_ang[ip] / 180. * PI_);
        ssfac = mu0s / (mu0s + mu);
        sflux = p.solflux ? p.solflux[nuc] : 0.0;
    }
    // SS: the scattering opacity and the phase function of layer j, fetched with its opacities
    auto fetch_ss = [&](int j, double sp[2]) {
        if constexpr (SS == 2) {
            const size_t ri = (size_t)m_row[j];
            sp[0] = p.sca[ri * p.Wpad + nu];
            sp[1] = p.phase[((size_t)ip * p.rows + ri) * p.Wpad + nu];
        } else {
            const int lay = (int)m_lay[j];
            sp[0] = p.sca[((size_t)m * p.L + lay) * p.Wpad + nu];
            sp[1] = p.phase[(((size_t)m * p.P + ip) * p.L + lay) * p.Wpad + nu];
        }
    };
    auto scatter_term = [&](int j, int k, double tvk, double tc, double dtr) -> double {
        // (trold - tr) * ssfac * omega * phase * SOLFLUX / (4 pi), in the reference's order of operations (:6577)
        const int lay = (int)m_lay[j];
        const int g = gy + k * kGY;
        double om;
        if (p.omega) om = p.omega[((size_t)j * G + g) * p.Wpad + nu];
        else {              // one model; launch_rt sends p.sca to the SS builds.  Kept: without it the mode-0 builds compile differently
            const double tt = tvk + tc;                                   // vertical TAUTOT of the layer (:3989)
            om = (tt > 0.0) ? p.sca[(size_t)lay * p.Wpad + nu] / tt : 0.0;
        }
        const double ph = p.phase[((size_t)ip * p.L + lay) * p.Wpad + nu];
        return dtr * ssfac * om * ph * sflux / (4. * PI_);
    };
    double tvA[kGPer], tvB[kGPer], tcA = 0.0, tcB = 0.0, emA = 0.0, emB = 0.0;
    double ssA[2], ssB[2];                               // SS: fetch_ss's values beside tvA / tvB
    const double *ss = ssA;                              // ... of the layer being integrated
    auto integrate = [&](int j, const double tv[kGPer], double tc, double em) {
        const double sc = m_sc[j];
        const double bb = planck_bb(a, c2y, m_T[j]);
#pragma unroll
        for (int k = 0; k < kGPer; ++k) {
            const int g = gy + k * kGY;
            if (g < G) {
                const double t = (tv[k] + tc) * sc;  // :3989, :4006
                taud[k] += t;
                const double tr = exp(-taud[k]);
                if constexpr (SS != 0) {                  // scatter_term on the fetched values, the same order of operations
                    const double tt = tv[k] + tc;
                    const double om = (tt > 0.0) ? ss[0] / tt : 0.0;
                    spec[k] += (trold[k] - tr) * ssfac * om * ss[1] * sflux / (4. * PI_);
                } else if (p.mode == 2) spec[k] += scatter_term(j, k, tv[k], tc, trold[k] - tr);   // before the thermal term (:6577-6581)
                spec[k] += (trold[k] - tr) * bb;  // :6345-6348
                if (p.emi) spec[k] += em * tr;
                trold[k] = tr;
            }
        }
    };
    // the record after layer jd of the path: [ip][jd][3][G][Wpad]
    auto record = [&](int jd) -> double * { return p.prefix + (((size_t)ip * p.LIMAX + jd) * 3) * (size_t)G * p.Wpad + nu; };
    auto leave = [&](int jd) {
        if constexpr (PREFIX == 1) {
            double *r = record(jd);
#pragma unroll
            for (int k = 0; k < kGPer; ++k) {
                const int g = gy + k * kGY;
                if (g < G) {
                    r[(size_t)g * p.Wpad] = taud[k]; r[((size_t)G + g) * p.Wpad] = trold[k]; r[((size_t)2 * G + g) * p.Wpad] = spec[k];
                }
            }
        }
    };
    int j = 0;
    if constexpr (PREFIX == 2) {
        j = p.jstart[(size_t)m * p.P + ip];              // block-uniform
        if (j > 0) {
            const double *r = record(j - 1);
#pragma unroll
            for (int k = 0; k < kGPer; ++k) {
                const int g = gy + k * kGY;
                if (g < G) {
                    taud[k] = r[(size_t)g * p.Wpad]; trold[k] = r[((size_t)G + g) * p.Wpad]; spec[k] = r[((size_t)2 * G + g) * p.Wpad];
                }
            }
        }
    }
    if (j < nl) fetch(j, tvA, tcA, emA);
    if constexpr (SS != 0) { if (j < nl) fetch_ss(j, ssA); }
    for (; j + 1 < nl; j += 2) {                         // ping-pong buffers: no register rotation
        fetch(j + 1, tvB, tcB, emB);
        if constexpr (SS != 0) { fetch_ss(j + 1, ssB); ss = ssA; }
        integrate(j, tvA, tcA, emA);
        leave(j);
        if (j + 2 < nl) fetch(j + 2, tvA, tcA, emA);
        if constexpr (SS != 0) { if (j + 2 < nl) fetch_ss(j + 2, ssA); ss = ssB; }
        integrate(j + 1, tvB, tcB, emB);
        leave(j + 1);
    }
    if constexpr (SS != 0) ss = ssA;
    if (j < nl) { integrate(j, tvA, tcA, emA); leave(j); }
    // surface / bottom-of-atmosphere term  (:6354-6365)
    int i1 = (int)(nl / 2.0) - 1;
    if (i1 < 0) i1 += nl;
    const double *lp = p.lay_press + (size_t)m * p.L;
    const double p1 = lp[p.layinc[(size_t)i1 * p.P + ip]];
    const double p2 = lp[p.layinc[(size_t)(nl - 1) * p.P + ip]];
    double radground = 0.0;
    const bool ground = p2 > p1;
    if (ground) {
        const double ts = p.tsurf[m];
        if (ts <= 0.0) radground = planck_bb(a, c2y, p.emtemp[pathbase + (size_t)(nl - 1) * p.P]);
        else radground = planck_bb(a, c2y, ts) * (p.emissivity ? p.emissivity[nuc] : 0.0);
    }
    const double sola = p.sol_ang ? p.sol_ang[ip] : 180.0;
    const double emia = p.emiss_ang ? p.emiss_ang[ip] : 180.0;
    const bool solar_on = (emia < 90.) && (sola < 90.);
    double solterm = 0.0, muratio = 0.0;
    if (solar_on) {
        const double PI = 3.141592653589793;
        const double mu = cos(emia / 180. * PI), mu0 = cos(sola / 180. * PI);
        muratio = mu / mu0;
        solterm = (p.solflux ? p.solflux[nuc] : 0.0) * (p.reflectance ? p.reflectance[nuc] : 0.0);
    }
    const double xf = p.xfac ? p.xfac[nuc] : 1.0;
    double acc = 0.0;
#pragma unroll
    for (int k = 0; k < kGPer; ++k) {
        const int g = gy + k * kGY;
        if (g < G) {
            double s = spec[k];
            if (p.mode == 1) s = exp(-taud[k]);                               // :4116, xfac = solar flux when IFORM = 4 (:4119-4127)
            else if (SS != 0 || p.mode == 2) {                                     // :6585-6596: lower boundary whatever the geometry
                const double ts = p.tsurf[m];
                double rg;
                if (ts <= 0.0) rg = planck_bb(a, c2y, p.emtemp[pathbase + (size_t)(nl - 1) * p.P]);
                else rg = planck_bb(a, c2y, ts) * (p.emissivity ? p.emissivity[nuc] : 0.0);
                s += trold[k] * rg;
                s += trold[k] * sflux * mu0s * (p.brdf ? p.brdf[(size_t)nuc * p.P + ip] : 0.0);
            } else {
                if (ground) s += trold[k] * radground;
                if (solar_on) s += trold[k] * exp(-taud[k] * muratio) * solterm;  // :6368-6373
            }
            s = s * xf;                                                       // :4244
            if (p.per_g) {
                if (nu < p.W) p.out[((size_t)m * p.W + nu) * G + g] = s;
            } else {
                acc += s * p.delg[g];                                         // :4504
            }
        }
    }
    if (!p.per_g) {
        red[gy][lane] = acc;
        __syncthreads();
        if (gy == 0 && nu < p.W) {
            double t = red[0][lane];
#pragma unroll
            for (int k = 1; k < kGY; ++k) t += red[k][lane];
            p.out[((size_t)m * p.W + nu) * p.P + ip] = t;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// K3g+K4g+K6: thermal emission with analytic gradients.   "thermal_rtg"
// calc_thermal_emission_spectrumg (ForwardModel_0.py:6380-6504) carries dtr/dq for every
// (parameter, layer) through the layer loop: O(NPAR*Li^2) per (nu,g).  The recursion is linear in
// dTAU, so   dspec/dq[k,m] = c_m * dTAU[k,m]  (+ (trold_m - tr_m) dB/dT_m for k == NVMR)   with
//     c_m = tr_m B_m - R_m ,   R_m = sum_{j>m} (trold_j - tr_j) B_j + trold_N * radground ,
// one backward sweep (O(Li)); the g-quadrature (:4507) is folded in:
//     out[k,m] = xfac * ( SCALE_m * ( fac_k * sum_g dg c_g dk[slot_k][g] + dcont_k * sum_g dg c_g )
//                         + [k==NVMR] dBdT_m * sum_g dg (trold_m - tr_m)_g )
// so neither dTAUTOT_LAYINC (W,G,NPAR,Li,P) nor dSPECOUT (W,G,NPAR,Li) is materialised.
// Block = 64 wavenumbers x 4 g-groups; pass 1 stores trold_j per (g) to a workspace.  B and dB/dT: planckg_dev of
// ansfm_grad_slots.hip.h.
// ------------------------------------------------------------------------------------------------

// GY = g-groups (waves) per wavenumber tile: the kernel streams (S+1) gradient rows per layer and C2 has only 157 tiles,
// so the launch picks the largest GY whose reduction buffer fits in LDS (16 up to S = 12).
template <int GY>
__global__ __launch_bounds__(kWave *GY) void k_thermal_rtg(RtGParams q)
{
    constexpr int kGPerG = kMaxG / GY;
    const RtParams &p = q.r;
    extern __shared__ double red[];  // [NP1+2][GY][kWave]
    const int lane = threadIdx.x, gy = threadIdx.y;
    // grid = (models, paths, wavenumber tiles): the models of a batch that share opacity rows (de-duplicated Jacobian
    // states) run next to each other on a wavenumber tile, so the rows are re-read out of L2 instead of HBM
    const int nu = blockIdx.z * kWave + lane;
    const int nuc = nu < p.W ? nu : p.W - 1;
    const int ip = blockIdx.y, m = blockIdx.x;
    const int nl = p.nlayin[ip];
    const bool transmission = p.mode == 1;   // calculate_transmission_spectrum with return_grad (:4110-4131)
    const int G = p.G, NP1 = q.NP1, NR = NP1 + 2;
    const double wv = p.wave[nuc];
    const double y = (p.ispace == 0) ? wv : 1.0e4 / wv;
    const size_t pathbase = (size_t)m * p.LIMAX * p.P + ip;
    const size_t GWp = (size_t)G * p.Wpad;
    double *tws = q.trold_ws + (((size_t)m * p.P + ip) * (p.LIMAX + 1)) * GWp + nu;

    double trold[kGPerG], spec[kGPerG];
#pragma unroll
    for (int k = 0; k < kGPerG; ++k) { trold[k] = 1.0; spec[k] = 0.0; }
    // ---- pass 1: forward, product form tr = trold*exp(-tau_j) (:6446-6452) -----------------------------
    for (int j = 0; j < nl; ++j) {
        const int lay = p.layinc[(size_t)j * p.P + ip];
        const double sc = p.scale[pathbase + (size_t)j * p.P];
        const double T = p.emtemp[pathbase + (size_t)j * p.P];
        const double tc = p.cont ? p.cont[((size_t)m * p.L + lay) * p.Wpad + nu] : 0.0;
        double bb = 0.0, dB = 0.0;
        if (!transmission) planckg_dev(p.ispace, y, T, bb, dB);
        const double *trow = p.tau + (((size_t)m * p.L + lay) * G) * p.Wpad + nu;
#pragma unroll
        for (int k = 0; k < kGPerG; ++k) {
            const int g = gy + k * GY;
            if (g < G) {
                tws[(size_t)j * GWp + (size_t)g * p.Wpad] = trold[k];
                const double t = (trow[(size_t)g * p.Wpad] + tc) * sc;
                const double tr = trold[k] * exp(-t);
                spec[k] += (trold[k] - tr) * bb;
                trold[k] = tr;
            }
        }
    }
    int i1 = (int)(nl / 2.0) - 1;
    if (i1 < 0) i1 += nl;
    const double *lp = p.lay_press + (size_t)m * p.L;
    const bool ground = !transmission && lp[p.layinc[(size_t)(nl - 1) * p.P + ip]] > lp[p.layinc[(size_t)i1 * p.P + ip]];
    double radground = 0.0, dradgrounddT = 0.0;
    if (ground) {
        const double ts = p.tsurf[m];
        if (ts <= 0.0) planckg_dev(p.ispace, y, p.emtemp[pathbase + (size_t)(nl - 1) * p.P], radground, dradgrounddT);
        else {
            planckg_dev(p.ispace, y, ts, radground, dradgrounddT);
            const double em = p.emissivity ? p.emissivity[nuc] : 0.0;
            radground *= em;
            dradgrounddT *= em;
        }
    }
    const double xf = p.xfac ? p.xfac[nuc] : 1.0;
    double R[kGPerG];
    {
        double accs = 0.0, acct = 0.0;
#pragma unroll
        for (int k = 0; k < kGPerG; ++k) {
            const int g = gy + k * GY;
            R[k] = 0.0;
            if (g < G) {
                double sgl = transmission ? trold[k] : spec[k];     // mode 1: exp(-tau of the path) (:4110)
                if (ground) sgl += trold[k] * radground;
                accs += (sgl * xf) * p.delg[g];
                acct += ((ground ? trold[k] * dradgrounddT : 0.0) * xf) * p.delg[g];
                R[k] = ground ? trold[k] * radground : 0.0;
            }
        }
        red[(0 * GY + gy) * kWave + lane] = accs;
        red[(1 * GY + gy) * kWave + lane] = acct;
        __syncthreads();
        if (gy == 0 && nu < p.W) {
            double a = 0.0, b = 0.0;
#pragma unroll
            for (int k = 0; k < GY; ++k) { a += red[(0 * GY + k) * kWave + lane]; b += red[(1 * GY + k) * kWave + lane]; }
            p.out[((size_t)m * p.W + nu) * p.P + ip] = a;
            q.dtsurf[((size_t)m * p.W + nu) * p.P + ip] = b;
        }
        __syncthreads();
    }
    // ---- pass 2: backward sweep ------------------------------------------------------------------------
    double trnext[kGPerG];  // tr_m = trold_{m+1}
    double trfin[kGPerG];   // transmission of the whole path
#pragma unroll
    for (int k = 0; k < kGPerG; ++k) trnext[k] = trfin[k] = trold[k];
    double *dsp = q.dspec + (((size_t)m * p.P + ip) * q.NPAR) * (size_t)p.LIMAX * p.Wpad + nu;
    for (int mm = nl - 1; mm >= 0; --mm) {
        const int lay = p.layinc[(size_t)mm * p.P + ip];
        const double sc = p.scale[pathbase + (size_t)mm * p.P];
        const double T = p.emtemp[pathbase + (size_t)mm * p.P];
        double bb = 0.0, dB = 0.0;
        if (!transmission) planckg_dev(p.ispace, y, T, bb, dB);
        const double *dkl = q.dk + (((size_t)m * p.L + lay) * NP1) * GWp + nu;
        double X = 0.0, Z = 0.0;
        double *rb = red;
        (void)NR;
        double cg[kGPerG];
#pragma unroll
        for (int k = 0; k < kGPerG; ++k) {
            const int g = gy + k * GY;
            cg[k] = 0.0;
            if (g < G) {
                const double to = tws[(size_t)mm * GWp + (size_t)g * p.Wpad];
                const double tr = trnext[k];
                const double c = transmission ? -trfin[k] : tr * bb - R[k];   // mode 1: d exp(-tau) / d tau_m (:4129)
                const double dgk = p.delg[g];
                cg[k] = c * dgk;
                X += cg[k];
                Z += (to - tr) * dgk;
                R[k] += (to - tr) * bb;
                trnext[k] = to;
            }
        }
        __syncthreads();   // the previous layer's partial sums have been consumed by every thread
        for (int sidx = 0; sidx < NP1; ++sidx) {
            if (!((q.gas_mask >> (sidx == NP1 - 1 ? 31 : sidx)) & 1u)) continue;     // slot_of_param points away from it
            double ysum = 0.0;
#pragma unroll
            for (int k = 0; k < kGPerG; ++k) {
                const int g = gy + k * GY;
                if (g < G) ysum += cg[k] * dkl[((size_t)sidx * G + g) * p.Wpad];
            }
            rb[((2 + sidx) * GY + gy) * kWave + lane] = ysum;
        }
        rb[(0 * GY + gy) * kWave + lane] = X;
        rb[(1 * GY + gy) * kWave + lane] = Z;
        __syncthreads();
        double Xs = 0.0, Zs = 0.0;
#pragma unroll
        for (int k = 0; k < GY; ++k) { Xs += rb[(0 * GY + k) * kWave + lane]; Zs += rb[(1 * GY + k) * kWave + lane]; }
        for (int kpar = gy; kpar < q.NPAR; kpar += GY) {
            const int slot = q.slot_of_param[kpar];
            double ys = 0.0;
            if (slot >= 0) {
#pragma unroll
                for (int k = 0; k < GY; ++k) ys += rb[((2 + slot) * GY + k) * kWave + lane];
            }
            double v = dtau_param_gsum(slot, ys, Xs, NP1, q.dcont, q.dcont_gas, (size_t)m, q.NPAR, q.NVMR, kpar, p.L, lay, p.Wpad, nu);
            v *= sc;                                               // :4012
            if (kpar == q.NVMR && !transmission) v += Zs * dB;     // :6467-6468
            v *= xf;                                               // :4247
            if (v != v) v = 0.0;                                   // nan_to_num :4507
            dsp[((size_t)kpar * p.LIMAX + mm) * p.Wpad] = v;
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Array-level seam of calc_thermal_emission_spectrumg (ForwardModel_0.py:6380-6504) on the reference's layouts: one
// thread per (wavenumber, g).  The reference carries d tr / dq for every (parameter, layer) pair through the layer loop,
// O(NPAR Li^2); the recursion is linear in dTAU, so (as in k_thermal_rtg)
//     dspec[k][m] = dTAU[k][m] * (tr_m B_m - R_m) + [k == NVMR] (trold_m - tr_m) dB/dT_m ,
//     R_m = sum_{j > m} (trold_j - tr_j) B_j + tr_N * radground
// -- a forward pass that parks trold_j in the output's parameter-0 row and one backward sweep.
// ------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(128) void k_thermal_emission_g_seam(int ispace, int W, int G, int NPAR, int Li, int NVMR,
                                                                  const double *__restrict__ wave,
                                                                  const double *__restrict__ tau,      // [W][G][Li]
                                                                  const double *__restrict__ dtau,     // [W][G][NPAR][Li]
                                                                  const double *__restrict__ temp,     // [Li]
                                                                  const double *__restrict__ press,    // [Li]
                                                                  double tsurf, const double *__restrict__ emissivity,
                                                                  double *__restrict__ spec,           // [W][G]
                                                                  double *__restrict__ dspec,          // [W][G][NPAR][Li]
                                                                  double *__restrict__ dtsurf)         // [W][G]
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)W * G) return;
    const int w = (int)(idx / G);
    const double wv = wave[w];
    const double y = (ispace == 0) ? wv : 1.0e4 / wv;
    const double *t = tau + idx * Li;
    const double *dt = dtau + idx * (size_t)NPAR * Li;
    double *ds = dspec + idx * (size_t)NPAR * Li;
    double trold = 1.0, sp = 0.0;
    for (int j = 0; j < Li; ++j) {                       // :6446-6452, product form of the transmission
        double bb, dB;
        planckg_dev(ispace, y, temp[j], bb, dB);
        const double tr = trold * exp(-t[j]);
        sp += (trold - tr) * bb;
        ds[j] = trold;                                   // parked: read back (then overwritten) by the sweep
        trold = tr;
    }
    int i1 = (int)(Li / 2.0) - 1;                        // python index int(NLAYIN/2)-1, -1 wraps to the last layer
    if (i1 < 0) i1 += Li;
    double radground = 0.0, dradground = 0.0, R = 0.0;
    if (press[Li - 1] > press[i1]) {                     // not a limb path: the lower boundary contributes (:6479-6496)
        if (tsurf <= 0.0) planckg_dev(ispace, y, temp[Li - 1], radground, dradground);
        else {
            planckg_dev(ispace, y, tsurf, radground, dradground);
            radground *= emissivity[w];
            dradground *= emissivity[w];
        }
        sp += trold * radground;
        R = trold * radground;
    }
    spec[idx] = sp;
    dtsurf[idx] = (press[Li - 1] > press[i1]) ? trold * dradground : 0.0;
    double trn = trold;                                  // tr_m = trold_{m+1}
    for (int m = Li - 1; m >= 0; --m) {
        double bb, dB;
        planckg_dev(ispace, y, temp[m], bb, dB);
        const double to = ds[m];
        const double c = trn * bb - R;
        for (int k = 0; k < NPAR; ++k) {
            double v = dt[(size_t)k * Li + m] * c;
            if (k == NVMR) v += (to - trn) * dB;         // :6467-6468
            ds[(size_t)k * Li + m] = v;
        }
        R += (to - trn) * bb;
        trn = to;
    }
}

// internal dspec[P][NPAR][LIMAX][Wpad] -> reference dSPECOUT[W][NPAR][LIMAX][P]
__global__ void k_dspec_to_ref(const double *__restrict__ src, double *__restrict__ dst, int W, int Wpad,
                               int NPAR, int LIMAX, int P, const int32_t *__restrict__ nlayin)
{
    size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    size_t total = (size_t)W * NPAR * LIMAX * P;
    if (idx >= total) return;
    int ip = (int)(idx % P);
    size_t r = idx / P;
    int j = (int)(r % LIMAX); r /= LIMAX;
    int k = (int)(r % NPAR);
    int w = (int)(r / NPAR);
    dst[idx] = (j < nlayin[ip]) ? src[(((size_t)ip * NPAR + k) * LIMAX + j) * Wpad + w] : 0.0;
}

}  // namespace ansfm

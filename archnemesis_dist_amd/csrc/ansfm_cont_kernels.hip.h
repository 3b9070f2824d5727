// ansfm_cont_kernels.hip.h -- continuum opacities of the layers.
//
// ForwardModel_0.calc_tau_cia (:4516-4760): collision-induced absorption.  Per layer the CIA table K_CIA[pair][para]
// [T][wavenumber] is interpolated bilinearly in (temperature, para-H2 fraction) and linearly in wavenumber
// (scipy interp1d), multiplied by the two partners' mixing ratios and by TOTAM^2/DELH; the gradients with respect to
// the mixing ratios and temperature go with it.  The host resolves what does not depend on wavenumber (brackets and
// weights per layer, which atmospheric gases a pair refers to, the ortho/para selection) -- see ansfm_calc_tau_cia;
// the (wavenumber x layer) work is here, one thread per (wavenumber, layer).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ansfm {

struct CiaLayer {       // what calc_tau_cia derives per layer before touching the spectral axis (:4588-4666)
    int itl, ithi, ipl, iphi;
    double fhl_t, fhh_t, dfhldT, fhl_f, fhh_f, xfac;
};

struct CiaParams {
    const double *waven;        // [W] ascending
    const double *cia_waven;    // [NWC]
    const double *K;            // [NPAIR][NPE][NT][NWC]
    const CiaLayer *lay;        // [L]
    const int32_t *g1, *g2;     // [NPAIR] atmospheric gas of each partner, -1: pair not used
    const double *q;            // [L][NVMR]
    const double *k_co2, *k_n2n2, *k_n2h2;   // [W] or nullptr
    double *tau;                // [W][L]
    double *dtau;               // [W][L][NVMR+2] (zeroed) or nullptr
    int W, NWC, NPAIR, NPE, NT, L, NVMR, covers, ico2, in2, ih2;
};

// The record of one layer (:4588-4666), including the reference's overwrite of temp1 in the upper para-fraction clamp
// (:4623); comparisons of fabs() values, differences and quotients only, so the host (ansfm_calc_tau_cia) and the device
// (k_cia_rows_prep) give the same bits.  The caller has made sure that the brackets stay inside K_CIA, or tests them.
__host__ __device__ inline CiaLayer cia_layer(double temp1, double frac1, double xfac, int NT, const double *cia_temp, int nfrac,
                                              const double *cia_frac, int NPARA)
{
    int it = 0;
    for (int k = 1; k < NT; ++k) if (fabs(cia_temp[k] - temp1) < fabs(cia_temp[it] - temp1)) it = k;
    int itl, ithi;
    if (cia_temp[it] >= temp1) {
        ithi = it;
        if (it == 0) { temp1 = cia_temp[0]; itl = 0; ithi = 1; } else itl = it - 1;
    } else {
        itl = it;
        if (it == NT - 1) { temp1 = cia_temp[it]; ithi = NT - 1; itl = NT - 2; } else ithi = it + 1;
    }
    int ip = 0;
    for (int k = 1; k < nfrac; ++k) if (fabs(cia_frac[k] - frac1) < fabs(cia_frac[ip] - frac1)) ip = k;
    int ipl, iphi;
    if (cia_frac[ip] >= frac1) {
        iphi = ip;
        if (ip == 0) { frac1 = cia_frac[0]; ipl = 0; iphi = 1; } else ipl = ip - 1;
    } else {
        ipl = ip;
        if (ip == NPARA - 1) { temp1 = cia_frac[ip]; iphi = NPARA - 1; ipl = NPARA - 2; } else iphi = ip + 1;
    }
    if (NPARA == 0) { ipl = 0; iphi = 0; }
    CiaLayer c;
    c.itl = itl; c.ithi = ithi; c.ipl = ipl; c.iphi = iphi;
    c.fhl_t = (temp1 - cia_temp[itl]) / (cia_temp[ithi] - cia_temp[itl]);
    c.fhh_t = (cia_temp[ithi] - temp1) / (cia_temp[ithi] - cia_temp[itl]);
    c.dfhldT = 1.0 / (cia_temp[ithi] - cia_temp[itl]);
    c.fhl_f = 0.5; c.fhh_f = 0.5;
    if (nfrac > 1 && ipl >= 0 && iphi >= 0 && ipl < nfrac && iphi < nfrac) {
        c.fhl_f = (frac1 - cia_frac[ipl]) / (cia_frac[iphi] - cia_frac[ipl]);
        c.fhh_f = (cia_frac[iphi] - frac1) / (cia_frac[iphi] - cia_frac[ipl]);
    }
    c.xfac = xfac;
    return c;
}

// sum over the pairs of k_cia q1 q2 at wavenumber x (index w of the k_co2 / k_n2n2 / k_n2h2 vectors) for a layer of record c
// and mixing ratios q[NVMR]; TAUCIA = the sum * c.xfac.  d: the layer's NVMR + 2 gradient slots (zeroed), ds doubles apart, or
// nullptr.  One body for k_tau_cia, k_tau_cont_rows and k_dtau_cont_rows: they give the same bits.
__device__ __forceinline__ double cia_sum(const CiaParams &p, const CiaLayer &c, double x, int w, const double *q, double *d,
                                          int ds = 1)
{
    double sum1 = 0.0;
    if (p.covers) {
        int lo = 0, hi = p.NWC;          // scipy interp1d: idx = clip(searchsorted(x, xn, 'left'), 1, n-1)
        while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.cia_waven[mid] < x) lo = mid + 1; else hi = mid; }
        const int iw = lo < 1 ? 1 : (lo > p.NWC - 1 ? p.NWC - 1 : lo);
        const double xlo = p.cia_waven[iw - 1], dx = p.cia_waven[iw] - xlo;
        const size_t sT = (size_t)p.NWC, sP = (size_t)p.NT * p.NWC, sPair = (size_t)p.NPE * p.NT * p.NWC;
        for (int ip = 0; ip < p.NPAIR; ++ip) {
            const int g1 = p.g1[ip], g2 = p.g2[ip];
            if (g1 < 0 || g2 < 0) continue;
            const double *Kp = p.K + ip * sPair;
            double kt[2], dk[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                const int i = iw - 1 + e;
                const double a = Kp[c.ipl * sP + c.itl * sT + i], b = Kp[c.ipl * sP + c.ithi * sT + i];
                const double cc = Kp[c.iphi * sP + c.itl * sT + i], dd = Kp[c.iphi * sP + c.ithi * sT + i];
                const double ktlo = a * c.fhh_t + b * c.fhl_t, kthi = cc * c.fhh_t + dd * c.fhl_t;
                kt[e] = ktlo * c.fhh_f + kthi * c.fhl_f;
                dk[e] = (kthi - ktlo) * c.dfhldT;
            }
            const double k_cia = ((kt[1] - kt[0]) / dx) * (x - xlo) + kt[0];
            const double dkdT = ((dk[1] - dk[0]) / dx) * (x - xlo) + dk[0];
            sum1 = sum1 + k_cia * q[g1] * q[g2];
            if (d) {
                d[g1 * ds] = d[g1 * ds] + q[g2] * k_cia;
                d[g2 * ds] = d[g2 * ds] + q[g1] * k_cia;
                d[(p.NVMR - 2) * ds] = d[(p.NVMR - 2) * ds] + dkdT * q[g1] * q[g2];      // slot NVMR-2, as the reference (:4695)
            }
        }
    }
    if (p.ico2 >= 0) {
        const double k = p.k_co2[w];
        sum1 = sum1 + k * q[p.ico2] * q[p.ico2];
        if (d) d[p.ico2 * ds] = d[p.ico2 * ds] + 2. * q[p.ico2] * k;
    }
    if (p.in2 >= 0) {
        const double k = p.k_n2n2[w];
        sum1 = sum1 + k * q[p.in2] * q[p.in2];
        if (d) d[p.in2 * ds] = d[p.in2 * ds] + 2. * q[p.in2] * k;
    }
    if (p.in2 >= 0 && p.ih2 >= 0) {
        const double k = p.k_n2h2[w];
        sum1 = sum1 + k * q[p.in2] * q[p.ih2];
        if (d) {
            d[p.ih2 * ds] = d[p.ih2 * ds] + q[p.in2] * k;
            d[p.in2 * ds] = d[p.in2 * ds] + q[p.ih2] * k;
        }
    }
    return sum1;
}

__global__ __launch_bounds__(128) void k_tau_cia(CiaParams p)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y;
    if (w >= p.W) return;
    const CiaLayer c = p.lay[l];
    double *d = p.dtau ? p.dtau + ((size_t)w * p.L + l) * (p.NVMR + 2) : nullptr;
    const double sum1 = cia_sum(p, c, p.waven[w], w, p.q + (size_t)l * p.NVMR, d);
    p.tau[(size_t)w * p.L + l] = sum1 * c.xfac;
    if (d)
        for (int s = 0; s < p.NVMR + 2; ++s) d[s] = d[s] * c.xfac;
}

// ------------------------------------------------------------------------------------------------------------------
// Rayleigh scattering opacity of the layers: ForwardModel_0.calc_tau_rayleighj (:5525, IRAY 1, gas giants, Allen 1976),
// calc_tau_rayleighv2 (:5647, IRAY 2, CO2, Ityaksov et al. 2008), calc_tau_rayleighls (:5712, IRAY 4, Jovian air after
// Sromovsky: H2 / He / CH4 / NH3 weighted by the layer's composition) and the older calc_tau_rayleighv (:5598, not
// selected by any IRAY).  tau[w][l] = k(w[, l]) * TOTAM[l], dtau[w][l] = k.  One thread per (wavenumber, layer); the
// operation order of the reference's expressions is kept.
// ------------------------------------------------------------------------------------------------------------------
struct RayParams {
    const double *wavec;        // [W] wavenumber (ISPACE 0) or wavelength in micron (ISPACE 1)
    const double *totam;        // [L]
    const double *f4;           // mode 4: [L][4] mixing ratios of H2, He, CH4, NH3 (0 where the gas is absent)
    double *tau, *dtau;         // [W][L]  (batch: [n][W][Lm], the L = n * Lm layers of n states; dtau may be null)
    int W, L, mode, ispace;     // mode = IRAY (1, 2, 4); 12 = calc_tau_rayleighv
    int Lm;                     // layers per state of a batch, 0 = one state
};

// k(wavenumber[, composition of the layer]) of the four parametrisations: TAURAY = k * TOTAM
__device__ __forceinline__ double rayleigh_k(int mode, int ispace, double v, const double *f4row)
{
#pragma clang fp contract(off)      // n*n - 1 with n = 1 + 4e-4 cancels: a fused multiply-add would differ from NumPy by 1e-13
    const double PI = 3.141592653589793;
    double k = 0.0;
    if (mode == 1) {                                           // :5543-5577
        const double AH2 = 13.58E-5, BH2 = 7.52E-3, AHe = 3.48E-5, BHe = 2.30E-3, fH2 = 0.864;
        const double kb = 1.37971e-23, P0 = 1.01325e5, T0 = 273.15;
        const double LAMBDA = (ispace == 0) ? 1. / v * 1.0e-2 : v * 1.0e-6;
        double x = 1.0 / (LAMBDA * 1.0e6);
        const double nH2 = AH2 * (1.0 + BH2 * x * x);
        const double nHe = AHe * (1.0 + BHe * x * x);
        const double nAir = fH2 * nH2 + (1 - fH2) * nHe;
        const double temp = 32 * (PI * PI * PI) * (nAir * nAir);
        const double N0 = P0 / (kb * T0);
        x = N0 * LAMBDA * LAMBDA;
        const double faniso = (6.0 + 3.0 * 0.0) / (6.0 - 7.0 * 0.0);
        k = temp * faniso / (3. * (x * x));
    } else if (mode == 12) {                                   // :5620-5632
        const double LAMBDA = (ispace == 0) ? 1. / v * 1.0e4 : v;
        const double l2 = LAMBDA * LAMBDA;
        k = 8.8e-28 / (l2 * l2) * 1.0e-4;
    } else if (mode == 2) {                                    // :5670-5695
        const double LAMBDA = (ispace == 0) ? 1. / v * 1.0e4 : v;
        const double dens = 2.5475605e+19;
        const double lam = LAMBDA * 1.0e-4;
        const double f_king = 1.14 + (25.3e-12) / (lam * lam);
        const double nu2 = 1. / lam / lam;
        const double term1 = 5799.3 / (16.618e9 - nu2) + 120.05 / (7.9609e9 - nu2) + 5.3334 / (5.6306e9 - nu2) +
                             4.3244 / (4.6020e9 - nu2) + 1.218e-5 / (5.84745e6 - nu2);
        const double n = 1.0 + 1.1427e3 * term1;
        const double r = (n * n - 1) / (n * n + 2.0);
        const double factor1 = r * r;
        const double l2 = lam * lam;
        k = (24. * (PI * PI * PI) / (l2 * l2) / (dens * dens)) * factor1 * f_king;
        k = k * 1.0e-4;
    } else {                                                     // mode 4, :5745-5824
        const double *f = f4row;
        const double fh2 = f[0], fhe = f[1], fch4 = f[2], fnh3 = f[3];
        double fheh2 = 0.0, fch4h2 = 0.0;
        if (fh2 > 0.0) { fheh2 = fhe / fh2; fch4h2 = fch4 / fh2; }
        double comp[4];
        comp[0] = (1.0 - fnh3) / (1.0 + fheh2 + fch4h2);
        comp[1] = fheh2 * comp[0];
        comp[2] = fch4h2 * comp[0];
        comp[3] = fnh3;
        const double losch = 2.687e19 * 1.0E+12;                 // loschpm3 as the reference forms it (:5786)
        const double wl = (ispace == 0) ? 1. / v * 1.0e4 : v;
        const double A[4] = {13.58e-5, 3.48e-5, 37.0e-5, 37.0e-5};
        const double B[4] = {7.52e-3, 2.3e-3, 12.0e-3, 12.0e-3};
        const double D[4] = {0.0221, 0.025, .0922, .0922};
        double xc1 = 0.0, sumwt = 0.0;
        const double wl2 = wl * wl;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const double nr = 1.0 + A[j] * (1.0 + B[j] / wl2);
            const double t = nr * nr - 1.0;
            xc1 = xc1 + (t * t) * comp[j] * (6.0 + 3.0 * D[j]) / (6.0 - 7.0 * D[j]);
            sumwt = sumwt + comp[j];
        }
        const double fact = 8.0 * (PI * PI * PI) / (3.0 * (wl2 * wl2) * (losch * losch));
        k = fact * xc1 * 1.0E-8 / sumwt * 1.0e-4;
    }
    return k;
}

__global__ __launch_bounds__(128) void k_tau_rayleigh(RayParams p)
{
#pragma clang fp contract(off)
    // one thread per output element in storage order (layer fastest): the [W][L] / [n][W][Lm] arrays are written in whole
    // cache lines (a thread per wavenumber and a block row per layer wrote 8 bytes every L * 8: 3.1 ms for the 201 states
    // of a C3 Jacobian)
    const size_t flat = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int Lm = p.Lm ? p.Lm : p.L;
    if (flat >= (size_t)p.W * p.L) return;
    const int lm = (int)(flat % Lm), w = (int)((flat / Lm) % p.W), l = (int)(flat / ((size_t)Lm * p.W)) * Lm + lm;
    const double k = rayleigh_k(p.mode, p.ispace, p.wavec[w], p.mode == 4 ? p.f4 + (size_t)l * 4 : nullptr);
    p.tau[flat] = k * p.totam[l];
    if (p.dtau) p.dtau[flat] = k;
}

// The same for the distinct layers of a batch, in the layout the thermal RT reads ([row][Wpad], zero beyond W): row r is
// layer work[r] (flattened (state, layer); nullptr: r itself) of totam [n * L] / f4 [n * L][4].  One thread per (row, wavenumber).
__global__ __launch_bounds__(256) void k_tau_rayleigh_rows(int rows, int W, int Wpad, int mode, int ispace, const double *__restrict__ wavec,
                                                           const int32_t *__restrict__ work, const double *__restrict__ totam,
                                                           const double *__restrict__ f4, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const size_t flat = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (flat >= (size_t)rows * Wpad) return;
    const int w = (int)(flat % Wpad), r = (int)(flat / Wpad);
    if (w >= W) { out[flat] = 0.0; return; }
    const int l = work ? work[r] : r;
    const double k = rayleigh_k(mode, ispace, wavec[w], mode == 4 ? f4 + (size_t)l * 4 : nullptr);
    out[flat] = k * totam[l];
}

// ------------------------------------------------------------------------------------------------------------------
// Aerosol opacity of the layers: ForwardModel_0.calc_tau_dust (:4790-4867).  Per aerosol population the extinction and
// scattering cross sections tabulated on Scatter.WAVE are interpolated to the calculation grid with scipy's
// interp1d(kind='cubic') = the not-a-knot cubic spline (piecewise coefficients from the host, ansfm_calc_tau_dust), or
// linearly when only two points are tabulated; where the spline leaves the physical range (ksca < 0 < kext, kext < 0 <
// ksca, kext < ksca -- all three tested on the spline values, :4849-4851) the linear interpolant replaces it
// (:4853-4859).  tau = k * 1e-4 * CONT[layer][population], dtau/dq = k * 1e-4.  One thread per (wavenumber, population).
// ------------------------------------------------------------------------------------------------------------------
struct DustParams {
    const double *wavec;        // [W]
    const double *swave;        // [NWS] ascending
    const double *kext, *ksca;  // [NWS][NDUST] tabulated values
    const double *cext, *csca;  // [NDUST][NWS-1][3] spline coefficients b, c, d per interval (cubic only)
    const double *cont;         // [L][NDUST]
    double *taudust, *tauclscat, *dtaudust, *dtauclscat;   // [W][L][NDUST]
    int W, NWS, NDUST, L, cubic;
};

// extinction and scattering cross section of population i at x: the spline or its linear replacement (:4849-4859).  One body
// for k_tau_dust and k_dust_kext_grid (ansfm_upload_dust).
__device__ __forceinline__ void dust_k(const DustParams &p, double x, int i, double &kext, double &ksca)
{
    const int n = p.NWS;
    // spline interval: x in [x_a, x_a+1] (the last one closed); interp1d's: searchsorted(left) clipped to [1, n-1], minus 1
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (p.swave[mid] < x) lo = mid + 1; else hi = mid; }
    int idx = lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo);
    const int a = idx - 1;
    const double xa = p.swave[a], xb = p.swave[a + 1];
    const double ea = p.kext[(size_t)a * p.NDUST + i], eb = p.kext[(size_t)(a + 1) * p.NDUST + i];
    const double sa = p.ksca[(size_t)a * p.NDUST + i], sb = p.ksca[(size_t)(a + 1) * p.NDUST + i];
    const double lin_e = ((eb - ea) / (xb - xa)) * (x - xa) + ea;
    const double lin_s = ((sb - sa) / (xb - xa)) * (x - xa) + sa;
    kext = lin_e; ksca = lin_s;
    if (p.cubic) {
        const double t = x - xa;
        const double *ce = p.cext + ((size_t)i * (n - 1) + a) * 3;
        const double *cs = p.csca + ((size_t)i * (n - 1) + a) * 3;
        const double se = ea + t * (ce[0] + t * (ce[1] + t * ce[2]));
        const double ss = sa + t * (cs[0] + t * (cs[1] + t * cs[2]));
        const bool inv_s = (ss < 0) && (se > 0), inv_e = (se < 0) && (ss > 0), inv_b = (se < ss);
        kext = (inv_e || inv_b) ? lin_e : se;
        ksca = (inv_s || inv_b) ? lin_s : ss;
    }
}

__global__ __launch_bounds__(128) void k_tau_dust(DustParams p)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (w >= p.W) return;
    double kext, ksca;
    dust_k(p, p.wavec[w], i, kext, ksca);
    const double de = kext * 1.0e-4, ds = ksca * 1.0e-4;
    for (int j = 0; j < p.L; ++j) {
        const double c = p.cont[(size_t)j * p.NDUST + i];
        const size_t o = ((size_t)w * p.L + j) * p.NDUST + i;
        p.taudust[o] = de * c;
        p.tauclscat[o] = ds * c;
        p.dtaudust[o] = de;
        p.dtauclscat[o] = ds;
    }
}

// ansfm_upload_dust: the extinction and scattering cross sections on the table's grid, kext_w / ksca_w [NDUST][Wpad] (zero
// beyond W), as k_tau_dust evaluates them.  One thread per (wavenumber, population).
__global__ __launch_bounds__(128) void k_dust_kext_grid(DustParams p, int Wpad, double *__restrict__ kext_w, double *__restrict__ ksca_w)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, i = blockIdx.y;
    if (w >= Wpad) return;
    double kext = 0.0, ksca = 0.0;
    if (w < p.W) dust_k(p, p.wavec[w], i, kext, ksca);
    kext_w[(size_t)i * Wpad + w] = kext;
    ksca_w[(size_t)i * Wpad + w] = ksca;
}

// ------------------------------------------------------------------------------------------------------------------
// The continuum of the distinct layers of a batch from the context's resident sources (ansfm_upload_cia, ansfm_upload_dust)
// and the Rayleigh parametrisations, in the layout the thermal RT reads ([row][Wpad], zero beyond W):
//     cont[row][w] = (TAUCIA + TAUDUST) + TAURAY          (calculate_layer_opacity :3989; an absent term is left out)
// Row r is layer work[r] (flattened (state, layer); nullptr: r itself) of the per-layer arrays.  Every term is rounded as the
// array-level kernels round it to memory before the sums -- no product is fused into a sum here.
// ------------------------------------------------------------------------------------------------------------------
struct ContRowsParams {
    CiaParams cia;              // the resident table (waven, tau, dtau, W, L unused); lay [rows] by k_cia_rows_prep; q [n L][NVMR]
    const double *cia_temp, *cia_frac;   // [NT], [nfrac]
    const double *wave;         // [W] the table's grid
    const int32_t *work;        // [rows] or nullptr
    const double *temp, *frac, *totam, *delh;   // [n L]
    const double *kext_w;       // [NDUST][Wpad]
    const double *cont;         // [n L][NDUST]
    const double *f4;           // [n L][4], ray_mode 4
    double *out;                // [rows][Wpad]
    CiaLayer *lay;              // [rows]
    int rows, W, Wpad, ispace, use_cia, nfrac, NPARA, NDUST, ray_mode;
};

// One thread per row: the CIA record of the row's layer (the host loop of ansfm_calc_tau_cia; xfac as calc_tau_cia forms it,
// (TOTAM 1e-4)^2 / (DELH 1e2))
__global__ __launch_bounds__(64) void k_cia_rows_prep(ContRowsParams p)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x * blockDim.x + threadIdx.x;
    if (r >= p.rows) return;
    const int l = p.work ? p.work[r] : r;
    const double t = p.totam[l] * 1.0e-4;
    const double xfac = (t * t) / (p.delh[l] * 1.0e2);
    p.lay[r] = cia_layer(p.temp[l], p.frac[l], xfac, p.cia.NT, p.cia_temp, p.nfrac, p.cia_frac, p.NPARA);
}

// One thread per (row, wavenumber), a block within one row (blockIdx.x), coalesced along the wavenumbers
__global__ __launch_bounds__(256) void k_tau_cont_rows(ContRowsParams p)
{
#pragma clang fp contract(off)
    const int r = blockIdx.x, w = blockIdx.y * blockDim.x + threadIdx.x;
    if (w >= p.Wpad) return;
    double *out = p.out + (size_t)r * p.Wpad + w;
    if (w >= p.W) { *out = 0.0; return; }
    const int l = p.work ? p.work[r] : r;
    const double v = p.wave[w];
    double tau = 0.0;
    bool any = false;
    if (p.use_cia) {
        const CiaLayer c = p.lay[r];
        const double x = p.ispace == 0 ? v : 1.e4 / v;             // :4565
        const double sum1 = cia_sum(p.cia, c, x, w, p.cia.q + (size_t)l * p.cia.NVMR, nullptr);
        tau = sum1 * c.xfac;
        any = true;
    }
    if (p.NDUST > 0) {
        double dust = 0.0;
        for (int d = 0; d < p.NDUST; ++d) {
            const double de = p.kext_w[(size_t)d * p.Wpad + w] * 1.0e-4;
            double t = de * p.cont[(size_t)l * p.NDUST + d];
            t = (t != t) ? 0.0 : t;                                  // np.nan_to_num; +-inf end at the bounds of the clip
            t = t > 0.0 ? t : 0.0;                                   // np.clip(., 0, 1e20)  (:3966)
            t = t < 1.0e20 ? t : 1.0e20;
            dust = d == 0 ? t : dust + t;                            // np.sum over fewer than 8 populations: in order
        }
        tau = any ? tau + dust : dust;
        any = true;
    }
    if (p.ray_mode) {
        const double ray = rayleigh_k(p.ray_mode, p.ispace, v, p.ray_mode == 4 ? p.f4 + (size_t)l * 4 : nullptr) * p.totam[l];
        tau = any ? tau + ray : ray;
    }
    *out = tau;
}

// ------------------------------------------------------------------------------------------------------------------
// The same rows for the multiple-scattering batch (ansfm_cirsrad_ck_scatter_batch_cont), which needs the terms apart and the
// scattering side of the aerosols: the five arrays of calculate_layer_opacity (:3963-3972) and scloud11wave (:5107-5113) in
// the layout ansfm_cirsrad_ck_scatter_batch_rows takes, taucia / taudust / tauray / tauscat [rows][W] and lfrac
// [rows][NDUST][W], wavenumber fastest.  Per population d, rounded as k_tau_dust rounds them to memory,
//     e_d = (kext_w[d][w] 1e-4) CONT[l][d],   s_d = (ksca_w[d][w] 1e-4) CONT[l][d]
//     TAUDUST = sum_d clip(nan_to_num(e_d), 0, 1e20)      TAUSCAT = sum_d s_d  (raw: neither clip nor nan_to_num, :3972)
//     lfrac[d] = s_d / TAUSCAT where TAUSCAT > 0, else 0  (a true division)
// both sums in the order of d (NumPy adds fewer than 8 terms in order).  TAUCIA and TAURAY as k_tau_cont_rows forms them.  An
// array whose term is not used is null and not written.
// ------------------------------------------------------------------------------------------------------------------
struct MsContRowsParams {
    ContRowsParams c;           // as k_tau_cont_rows takes it (out unused); c.lay filled by k_cia_rows_prep for these rows
    const double *ksca_w;       // [NDUST][Wpad]
    double *taucia, *taudust, *tauray, *tauscat;   // [rows][W]
    double *lfrac;              // [rows][NDUST][W]
};

// One thread per (row, wavenumber), a block within one row (blockIdx.x), coalesced along the wavenumbers.  s_d is formed
// twice, for the sum and for the fractions: no per-thread array, no scratch memory.
__global__ __launch_bounds__(256) void k_ms_cont_rows(MsContRowsParams p)
{
#pragma clang fp contract(off)
    const ContRowsParams &c = p.c;
    const int r = blockIdx.x, w = blockIdx.y * blockDim.x + threadIdx.x;
    if (w >= c.W) return;
    const int l = c.work ? c.work[r] : r;
    const size_t o = (size_t)r * c.W + w;
    const double v = c.wave[w];
    if (c.use_cia) {
        const CiaLayer cl = c.lay[r];
        const double x = c.ispace == 0 ? v : 1.e4 / v;             // :4565
        const double sum1 = cia_sum(c.cia, cl, x, w, c.cia.q + (size_t)l * c.cia.NVMR, nullptr);
        p.taucia[o] = sum1 * cl.xfac;
    }
    if (c.NDUST > 0) {
        const double *cont = c.cont + (size_t)l * c.NDUST;
        double dust = 0.0, sca = 0.0;
        for (int d = 0; d < c.NDUST; ++d) {
            const double de = c.kext_w[(size_t)d * c.Wpad + w] * 1.0e-4, ds = p.ksca_w[(size_t)d * c.Wpad + w] * 1.0e-4;
            double t = de * cont[d];
            const double s = ds * cont[d];
            t = (t != t) ? 0.0 : t;                                  // np.nan_to_num; +-inf end at the bounds of the clip
            t = t > 0.0 ? t : 0.0;                                   // np.clip(., 0, 1e20)  (:3966)
            t = t < 1.0e20 ? t : 1.0e20;
            dust = d == 0 ? t : dust + t;
            sca = d == 0 ? s : sca + s;
        }
        p.taudust[o] = dust;
        p.tauscat[o] = sca;
        for (int d = 0; d < c.NDUST; ++d) {
            const double s = (p.ksca_w[(size_t)d * c.Wpad + w] * 1.0e-4) * cont[d];
            p.lfrac[((size_t)r * c.NDUST + d) * c.W + w] = sca > 0.0 ? s / sca : 0.0;       // :5108-5113
        }
    }
    if (c.ray_mode)
        p.tauray[o] = rayleigh_k(c.ray_mode, c.ispace, v, c.ray_mode == 4 ? c.f4 + (size_t)l * 4 : nullptr) * c.totam[l];
}

// ------------------------------------------------------------------------------------------------------------------
// The same rows for the single-scattering batch (ansfm_cirsrad_ck_singlescatt_batch_cont), in the layouts its RT kernel reads by
// row, zero beyond W: the continuum of k_tau_cont_rows, the scattering opacity and the layer-mean phase function of every path
// (calculate_single_scattering_plane_parallel_spectrum, :4316-4321):
//     cont[row][w]  = (TAUCIA + TAUDUST) + TAURAY                                      (an absent term is left out)
//     sca[row][w]   = TAURAY + TAUSCAT,  TAUSCAT = sum_d s_d (raw, in the order of d),  s_d = (ksca_w[d][w] 1e-4) CONT[l][d]
//     phase[ip][row][w] = num > 0 ? num / (TAURAY + TAUSCAT) : num,
//                   num = pf[w][ip][0] s_0 + ... + pf[w][ip][ND-1] s_{ND-1} + pf[w][ip][ND] TAURAY
// with pf = phase_fn [W][P][NDUST + 1] (calc_phase / calc_phase_ray at each path's scattering angle).  Every product is rounded,
// then added in that order, the first term starting the sum (np.sum over a middle axis adds in order).  A term that is not used
// is the reference's array of zeros: TAURAY = 0 still adds pf 0 to num (its sign can matter to a zero sum) and 0 to the divisor.
// ------------------------------------------------------------------------------------------------------------------
struct SsContRowsParams {
    ContRowsParams c;           // as k_tau_cont_rows takes it: c.out = cont [rows][Wpad]; c.lay filled by k_cia_rows_prep
    const double *ksca_w;       // [NDUST][Wpad]
    const double *phase_fn;     // [W][P][NDUST + 1]
    double *sca;                // [rows][Wpad]
    double *phase;              // [P][rows][Wpad]
    int P;
};

// One thread per (row, wavenumber), a block within one row (blockIdx.x), coalesced along the wavenumbers.  s_d is formed again
// for every path: no per-thread array, no scratch memory.
__global__ __launch_bounds__(256) void k_ss_cont_rows(SsContRowsParams p)
{
#pragma clang fp contract(off)
    const ContRowsParams &c = p.c;
    const int r = blockIdx.x, w = blockIdx.y * blockDim.x + threadIdx.x;
    if (w >= c.Wpad) return;
    const size_t o = (size_t)r * c.Wpad + w, RW = (size_t)c.rows * c.Wpad;
    if (w >= c.W) {
        c.out[o] = 0.0; p.sca[o] = 0.0;
        for (int ip = 0; ip < p.P; ++ip) p.phase[(size_t)ip * RW + o] = 0.0;
        return;
    }
    const int l = c.work ? c.work[r] : r;
    const double v = c.wave[w];
    double tau = 0.0, tauscat = 0.0, ray = 0.0;
    bool any = false;
    if (c.use_cia) {
        const CiaLayer cl = c.lay[r];
        const double x = c.ispace == 0 ? v : 1.e4 / v;             // :4565
        const double sum1 = cia_sum(c.cia, cl, x, w, c.cia.q + (size_t)l * c.cia.NVMR, nullptr);
        tau = sum1 * cl.xfac;
        any = true;
    }
    const double *cont = c.NDUST > 0 ? c.cont + (size_t)l * c.NDUST : nullptr;
    if (c.NDUST > 0) {
        double dust = 0.0;
        for (int d = 0; d < c.NDUST; ++d) {
            const double de = c.kext_w[(size_t)d * c.Wpad + w] * 1.0e-4, ds = p.ksca_w[(size_t)d * c.Wpad + w] * 1.0e-4;
            double t = de * cont[d];
            const double s = ds * cont[d];
            t = (t != t) ? 0.0 : t;                                  // np.nan_to_num; +-inf end at the bounds of the clip
            t = t > 0.0 ? t : 0.0;                                   // np.clip(., 0, 1e20)  (:3966)
            t = t < 1.0e20 ? t : 1.0e20;
            dust = d == 0 ? t : dust + t;
            tauscat = d == 0 ? s : tauscat + s;
        }
        tau = any ? tau + dust : dust;
        any = true;
    }
    if (c.ray_mode) {
        ray = rayleigh_k(c.ray_mode, c.ispace, v, c.ray_mode == 4 ? c.f4 + (size_t)l * 4 : nullptr) * c.totam[l];
        tau = any ? tau + ray : ray;
    }
    c.out[o] = tau;
    const double tsca = ray + tauscat;                               // an unused term: the reference's zeros
    p.sca[o] = tsca;
    const double *pf = p.phase_fn + (size_t)w * p.P * (c.NDUST + 1);
    for (int ip = 0; ip < p.P; ++ip, pf += c.NDUST + 1) {
        double num = 0.0;
        for (int d = 0; d < c.NDUST; ++d) {
            const double s = (p.ksca_w[(size_t)d * c.Wpad + w] * 1.0e-4) * cont[d];
            const double t = pf[d] * s;
            num = d == 0 ? t : num + t;
        }
        const double t = pf[c.NDUST] * ray;
        num = c.NDUST == 0 ? t : num + t;
        p.phase[(size_t)ip * RW + o] = num > 0.0 ? num / tsca : num;
    }
}

// ------------------------------------------------------------------------------------------------------------------
// The gradients of k_tau_cont_rows' continuum, dTAUCON of calculate_layer_opacity (:3940-3981), from the same resident sources and
// straight in the layout the gradient RT reads: dcont[m][kpar][l][w] ([n][NPAR][L][Wpad], zero beyond W), NPAR = NVMR + 2 +
// NDUST.  Row r = m * L + l is layer r of the per-layer arrays (no work list: a gradient call is one state, or a few).
//     kpar < NVMR            (d[kpar] * xfac) / TOTAM[l]  (+ the Rayleigh k, dTAURAY, of every gas: :3955-3957)
//     kpar == NVMR           d[NVMR] * xfac: calc_tau_cia never fills the temperature slot, its dkdT term lands in NVMR - 2 (:4741)
//     kpar == NVMR + 1 + i   kext_w[i][w] * 1e-4: the raw dTAUDUST1, neither nan_to_num nor clip (:3966 acts on the opacity only)
//     kpar == NPAR - 1       0 (para-H2, flagh2p = False)
// d is what cia_sum accumulates for k_tau_cia; every term is rounded as the array-level kernels and NumPy's assembly round it:
// d * xfac to memory, a true division by TOTAM, then the sum with the Rayleigh term (the first add, to zero, is exact).  An
// absent term is left out.  cia_sum indexes d by the gas: the thread's NVMR + 2 slots are a column of LDS, blockDim.x doubles
// apart (a private array would go to scratch memory), so a wave's ds_read_b64 of one slot covers consecutive banks.
// ------------------------------------------------------------------------------------------------------------------
constexpr int kDContBlock = 128;    // threads: (NVMR + 2) * 128 * 8 bytes of dynamic LDS, 48 KiB at ANSFM_MAX_CONT_GRAD_SLOTS

struct DContRowsParams {
    ContRowsParams c;           // as k_tau_cont_rows takes it (work, out unused); c.lay filled by k_cia_rows_prep for these rows
    double *dout;               // [n][NPAR][L][Wpad]
    int L, NVMR, NPAR;
};

// One thread per (row, wavenumber), a block within one row (blockIdx.x): every parameter's store is coalesced along the wavenumbers
__global__ __launch_bounds__(kDContBlock) void k_dtau_cont_rows(DContRowsParams p)
{
#pragma clang fp contract(off)
    extern __shared__ double dcont_slots[];                          // [NVMR + 2][blockDim.x]
    const ContRowsParams &c = p.c;
    const int r = blockIdx.x, w = blockIdx.y * blockDim.x + threadIdx.x;
    if (w >= c.Wpad) return;
    const int m = r / p.L, l = r - m * p.L;
    const size_t sk = (size_t)p.L * c.Wpad;                          // from one parameter to the next
    double *out = p.dout + ((size_t)m * p.NPAR * p.L + l) * c.Wpad + w;
    if (w >= c.W) {
        for (int k = 0; k < p.NPAR; ++k) out[k * sk] = 0.0;
        return;
    }
    const int ds = blockDim.x;
    double *d = dcont_slots + threadIdx.x;
    const double v = c.wave[w];
    double xfac = 0.0, totam = 1.0;
    if (c.use_cia) {
        for (int s = 0; s < p.NVMR + 2; ++s) d[s * ds] = 0.0;
        const CiaLayer cl = c.lay[r];
        const double x = c.ispace == 0 ? v : 1.e4 / v;               // :4565
        cia_sum(c.cia, cl, x, w, c.cia.q + (size_t)r * p.NVMR, d, ds);
        xfac = cl.xfac;
        totam = c.totam[r];
    }
    const double ray = c.ray_mode ? rayleigh_k(c.ray_mode, c.ispace, v, c.ray_mode == 4 ? c.f4 + (size_t)r * 4 : nullptr) : 0.0;
    for (int k = 0; k < p.NVMR; ++k) {
        double g = 0.0;
        if (c.use_cia) {
            const double dx = d[k * ds] * xfac;                      // dTAUCIA as k_tau_cia stores it
            g = dx / totam;
        }
        if (c.ray_mode) g = c.use_cia ? g + ray : ray;
        out[k * sk] = g;
    }
    out[p.NVMR * sk] = c.use_cia ? d[p.NVMR * ds] * xfac : 0.0;
    for (int k = p.NVMR + 1; k < p.NPAR; ++k) {
        const int i = k - (p.NVMR + 1);
        out[k * sk] = i < c.NDUST ? c.kext_w[(size_t)i * c.Wpad + w] * 1.0e-4 : 0.0;
    }
}

}  // namespace ansfm

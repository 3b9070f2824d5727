// ansfm_ms_chain_steps.h -- the steps of scloud11wave_core (Multiple_Scattering_Core.py:651-960) that depend on scalars and
// pointers only, not on where a chain kernel keeps its matrices: k_ms_chain (LDS), k_ms_chain16 (matrix cores) and
// k_ms_chain_lane (registers) call them, each with its own libm (a functor: k_ms_chain16's calls are out of line).  Every
// expression keeps the operands and the order the reference has.  No HIP header: a plain C++17 compiler builds it
// (tests/host/ms_steps_main.cpp).  DESIGN.md 4.4, "Shared steps".
#pragma once
#include <math.h>

#include "ansfm_ms_params.h"

#if defined(__HIPCC__)
#define ANSFM_HD __host__ __device__
#else
#define ANSFM_HD
#endif
#define ANSFM_STEP ANSFM_HD inline __attribute__((always_inline))

namespace ansfm {

constexpr double kMsPi = 3.141592653589793;

// ---- a block's inputs -------------------------------------------------------------------------------------------------
// taus / omegas / bnu: [model of the launch][wavenumber of the slab]; tauray / lfrac: by model over the whole axis, or
// (cont_local) by launch position; the phase matrices and the Hansen factors in their window (ppl *= fc, :232).
struct MsChainInputs {
    const double *taus_w, *omegas_w, *bnu_w, *tauray_w, *lfrac_m, *PPL, *PMI, *FC;
    int wcn;                 // the wavenumber index lfrac_m is read at
};
// ml: position of the model in the launch, mg: the model, wl: wavenumber within the slab, widx = w0 + wl, nn = nmu * nmu
ANSFM_STEP MsChainInputs ms_chain_inputs(const MsParams &p, int ml, int mg, int wl, int widx, int ig, int ic, int nn)
{
    MsChainInputs in;
    const size_t wrow = (size_t)ml * p.wcount + wl;
    in.taus_w = p.taus + (wrow * p.ng + ig) * p.nlay;
    in.omegas_w = p.omegas + (wrow * p.ng + ig) * p.nlay;
    const int mc = p.cont_local ? ml : mg;
    in.wcn = p.cont_local ? wl : widx;
    in.bnu_w = p.bnu + wrow * p.nlay;
    in.tauray_w = p.tauray + (size_t)mc * p.st_wl + (size_t)in.wcn * p.nlay;
    in.lfrac_m = p.lfrac + (size_t)mc * p.st_wcl;
    const size_t wpw = (size_t)(widx - p.pw0);
    in.PPL = p.ppl + ((wpw * (p.nf + 1) + ic) * p.ncomp) * nn;
    in.PMI = p.pmi + ((wpw * (p.nf + 1) + ic) * p.ncomp) * nn;
    in.FC = p.fc + (((size_t)ig * p.nwin + wpw) * p.ncomp) * nn;
    return in;
}

// ---- a layer's scalars (:846-860 and the head of calc_rtj_matrix :566-600) -----------------------------------------------
enum MsLayerKind { kMsLayerEmpty = 0, kMsLayerAbsorbing = 1, kMsLayerScattering = 2 };
struct MsLayerScalars {
    double tauscat, omega;   // the aerosols' scattering opacity; (tauscat + taur) / taut (NaN in an empty layer: not read)
    MsLayerKind kind;
};
ANSFM_STEP MsLayerScalars ms_layer_scalars(double taut, double omega_in, double taur)
{
    MsLayerScalars s;
    double omega = omega_in;
    if (omega < 0) omega = 0.0;
    if (omega > 1) omega = 1.0;
    double tauscat = taut * omega;
    tauscat = tauscat - taur;
    if (tauscat < 0) tauscat = 0.0;
    omega = (tauscat + taur) / taut;
    s.tauscat = tauscat;
    s.omega = omega;
    s.kind = (taut == 0) ? kMsLayerEmpty : (omega == 0) ? kMsLayerAbsorbing : kMsLayerScattering;
    return s;
}

// ---- start of the doubling (double1 :321-340) ----------------------------------------------------------------------------
struct MsDoublingStart {
    double con, tau0, fr, fs;   // omega pi (twice that at order 0); opacity of the 2^-nd sub-layer; Rayleigh / aerosol shares
    int nd;                     // doublings
};
template <class Log2, class Exp2>
ANSFM_STEP MsDoublingStart ms_doubling_start(double taut, double omega, double tauscat, double taur, int ic, Log2 log2f, Exp2 exp2f)
{
    MsDoublingStart d;
    d.fr = taur / (tauscat + taur);
    d.fs = tauscat / (tauscat + taur);
    double con = omega * kMsPi;
    con *= (ic == 0) ? 2.0 : 1.0;
    d.con = con;
    d.nd = (int)(log2f(taut) + 12);   // python int(): truncation toward zero
    d.tau0 = taut * ((d.nd >= 1) ? 1.0 / exp2f((double)d.nd) : 1.0);
    return d;
}

// ---- phase matrices of a layer: the mix of the components' (:601-615) -------------------------------------------------------
// An accessor gives element e of component c: pf(c) = P++ times the Hansen factor, pm(c) = P+-.
struct MsPhaseGlobal {       // global memory, 64-bit element index
    const double *PPL, *PMI, *FC;
    int nn, e;
    ANSFM_STEP double pf(int c) const { return PPL[(size_t)c * nn + e] * FC[(size_t)c * nn + e]; }
    ANSFM_STEP double pm(int c) const { return PMI[(size_t)c * nn + e]; }
};
struct MsPhaseGlobal32 {     // one uniform base per array and component, 32-bit byte offsets: no 64-bit address pair per element
    const double *PPL, *PMI, *FC;
    int nn;
    unsigned eo;             // 8 e
    ANSFM_STEP double at(const double *base, int c) const
    {
        return *reinterpret_cast<const double *>(reinterpret_cast<const char *>(base + (size_t)c * nn) + eo);
    }
    ANSFM_STEP double pf(int c) const { return at(PPL, c) * at(FC, c); }
    ANSFM_STEP double pm(int c) const { return at(PMI, c); }
};
struct MsPhaseLds {          // k_ms_chain16<PHASE_LDS>: lane-private [comp][2][4][64], the product with the factor already taken
    const double *phl;
    int r, lane;
    ANSFM_STEP double pf(int c) const { return phl[((c * 2 + 0) * 4 + r) * 64 + lane]; }
    ANSFM_STEP double pm(int c) const { return phl[((c * 2 + 1) * 4 + r) * 64 + lane]; }
};
// lfrac_m [wavenumber][ncont][nlay]: the aerosols' fractions, read at (wcn, c, k); Rayleigh is component ncont
template <class At>
ANSFM_STEP void ms_phase_mix(const At &at, double fr, double fs, int iray, int ncont, const double *lfrac_m, int wcn, int nlay, int k,
                             double &a, double &b)
{
    a = (iray > 0) ? fr * at.pf(ncont) : 0.0;
    b = (iray > 0) ? fr * at.pm(ncont) : 0.0;
    for (int c = 0; c < ncont; ++c) {
        const double f = lfrac_m[((size_t)wcn * ncont + c) * nlay + k];
        a += fs * at.pf(c) * f;
        b += fs * at.pm(c) * f;
    }
}

// ---- surface operator (:824-836): element (i, j) of 2 (brdf pi) mu_j w_j xfac ----------------------------------------------
ANSFM_STEP double ms_surface_element(const double *brdf, int widx, int n, int i, int j, int nf, int ic, double mu_j, double wt_j, double xfac)
{
    return (2. * (brdf[(((size_t)widx * n + i) * n + j) * (nf + 1) + ic] * kMsPi) * mu_j * wt_j) * xfac;
}

// ---- per path (:886-945) ---------------------------------------------------------------------------------------------------
struct MsPathAngles { double zmu0, zmu, solar1; };
template <class Cos>
ANSFM_STEP MsPathAngles ms_path_angles(const MsParams &p, Cos cosf, bool lookup, int widx, int ipath)
{
    MsPathAngles a;
    const double sol_ang = p.sol_ang[ipath];
    const double emiss_ang = lookup ? 180. - p.emiss_ang[ipath] : p.emiss_ang[ipath];   // new_emi :900-903
    if (sol_ang > 90.0) { a.zmu0 = cosf((180 - sol_ang) * kMsPi / 180.0); a.solar1 = p.solar[widx] * 0.0; }
    else { a.zmu0 = cosf(sol_ang * kMsPi / 180.0); a.solar1 = p.solar[widx]; }
    a.zmu = cosf(emiss_ang * kMsPi / 180.0);
    return a;
}
// j with mu[j] >= z > mu[j + 1] in the descending quadrature mu[0 .. nq) (nq: the quadrature's own points where it is padded to
// more slots); nq - 2 at or below the last point, 0 above the first
ANSFM_STEP int ms_bracket(const double *mu, int nq, double z)
{
    int b = 0;
    for (int j = 0; j < nq - 1; ++j) if (z <= mu[j] && z > mu[j + 1]) b = j;
    if (z <= mu[nq - 1]) b = nq - 2;
    return b;
}
// yx[2 a + b]: the sample at (mu0 bracket + a, mu bracket + b); t along mu, u along mu0
ANSFM_STEP double ms_bilinear(const double yx[4], double t, double u)
{
    return (1 - t) * (1 - u) * yx[0] + t * (1 - u) * yx[1] + t * u * yx[3] + (1 - t) * u * yx[2];
}
// the order's term of the azimuth series: cos(ic phi), twice that for ic > 0
template <class Cos>
ANSFM_STEP double ms_azimuth_term(double v, int ic, double aphi, Cos cosf)
{
    double drad = v * cosf(ic * aphi * kMsPi / 180.0);
    if (ic > 0) drad *= 2;
    return drad;
}
// The four samples from matrices with a leading dimension (LDS): look-down R u0+ + T u- + J; look-up at the bottom of the
// atmosphere T u0+ + R u- + J (:929-933) or, above a surface, idown's upl with minv = (E - rc rs)^-1, v0 = rc radg + jc
ANSFM_STEP void ms_path_samples_ld(double yx[4], bool lookup, int lowbc, int ic, int n, int ld, const double *rc, const double *tc,
                                   const double *jc, const double *radg, const double *minv, const double *v0, const double *wt,
                                   int isol, int iemm, double solar1)
{
    int ico = 0;
    for (int imu0 = isol; imu0 < isol + 2; ++imu0) {
        const double s0 = solar1 / (2.0 * kMsPi * wt[imu0]);
        for (int imu = iemm; imu < iemm + 2; ++imu) {
            if (!lookup) {
                double bcom = 0.0;   // (T utmi)[imu], utmi = radg for ic == 0 else 0
                if (ic == 0) for (int kk = 0; kk < n; ++kk) bcom += tc[imu * ld + kk] * radg[kk];
                yx[ico++] = (rc[imu * ld + imu0] * s0 + bcom) + jc[imu];
            } else if (lowbc == 0) {
                double bcom = 0.0;
                if (ic == 0) for (int kk = 0; kk < n; ++kk) bcom += rc[imu * ld + kk] * radg[kk];
                yx[ico++] = (tc[imu * ld + imu0] * s0 + bcom) + jc[imu];
            } else {
                double upl = 0.0;
                for (int kk = 0; kk < n; ++kk) upl += minv[imu * ld + kk] * (tc[kk * ld + imu0] * s0 + v0[kk]);
                yx[ico++] = upl;
            }
        }
    }
}

// One path's term of Fourier order ic from such matrices: the angles, their brackets in the quadrature mu[0 .. nq) with the
// weights wt, the four samples, the interpolation and the azimuth factor
template <class Cos>
ANSFM_STEP double ms_path_drad_ld(const MsParams &p, Cos cosf, bool lookup, int widx, int ic, int ipath, int n, int nq, int ld,
                                  const double *mu, const double *wt, const double *rc, const double *tc, const double *jc,
                                  const double *radg, const double *minv, const double *v0)
{
    const MsPathAngles a = ms_path_angles(p, cosf, lookup, widx, ipath);
    const int isol = ms_bracket(mu, nq, a.zmu0);
    const int iemm = ms_bracket(mu, nq, a.zmu);
    const double u = (mu[isol] - a.zmu0) / (mu[isol] - mu[isol + 1]);
    const double t = (mu[iemm] - a.zmu) / (mu[iemm] - mu[iemm + 1]);
    double yx[4];
    ms_path_samples_ld(yx, lookup, p.lowbc, ic, n, ld, rc, tc, jc, radg, minv, v0, wt, isol, iemm, a.solar1);
    return ms_azimuth_term(ms_bilinear(yx, t, u), ic, p.aphi[ipath], cosf);
}

// ---- one term of the Fourier sum with the reference's break (:945-958): true = two consecutive small terms, stop -----------
ANSFM_STEP bool ms_fourier_step(double drad, double &rad, bool &conv1)
{
    rad += drad;
    const double conv = fabs(drad / rad);
    if (conv < 1e-5 && conv1) return true;
    conv1 = (conv < 1e-5);
    return false;
}

}  // namespace ansfm

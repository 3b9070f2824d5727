// ansfm_surface_kernels.hip.h -- surface reflection on gfx950 (fp64): the Hapke and Oren-Nayar BRDF and the BRDF matrix of the
// doubling method.
//
// Restates Surface_0.calc_Hapke_BRDFx (Surface_0.py:1334-1439, with calc_Hapke_E1 / E2 / nu / eff_angles / H / hgphase),
// calc_OrenNayar_BRDFx (:1777-1824) and the azimuth integration of ForwardModel_0.calc_brdf_matrix (ForwardModel_0.py:5168-5249);
// the arithmetic is written down in tests/brdf_cases.py (hapke_np, oren_nayar_np, brdf_matrix_np), operation by operation
// in the reference's order.
//   k_brdf_points   one thread per (wavenumber, angle triple) -> BRDF[W][NTHETA]  (Surface_0.calc_BRDF)
//   k_brdf_azimuth  one thread per azimuth node k: what depends on k alone (cos phix, sin^2(phix / 2), f(phi), phix / 180)
//   k_brdf_matrix   one thread per (wavenumber, j, i): the nodes k = 0 .. NPHI in order, NF + 1 accumulators
//                   += (wphi[k] BRDF) cos(ic k dphi), written to BRDF_mat[w][i][j][0 .. NF]; the (W, NTHETA) array of the
//                   reference never exists.  What does not depend on k -- gamma, r0, theta_bar, chi, tan(theta_bar), and
//                   E1 / E2 / nu, cos, sin of both angles -- is formed once per thread in front of the loop.
// The point function is one: hapke_wave (per wavenumber), hapke_angle (per angle), hapke_azimuth (per azimuth) and hapke_eval
// (what is left) are the pieces brdf_point puts together for one point and k_brdf_matrix takes apart over its loop, so both
// kernels give the same bits for the same point.
//
// Rules that are part of the results: phi = 180 - phi_nemesis folded into [0, 180]; e >= 90 or i >= 90 gives 0; cg is clamped
// to [0, 1]; f(phi) = 0 iff |phix| == 180; E1 = E2 = 0 iff theta_bar == 0 or the angle is exactly 0; of (i, e) the smaller
// angle -- i when they are equal -- takes the reference's `i <= e` roles (its two branches are one formula with the roles
// exchanged, so no lane diverges).  At opposition arccos turns one ulp of cg into 1.5e-8 rad of phase angle: cg is formed
// with the reference's operations in its order, nothing in this header is contracted into fma, and sqrt is IEEE's.  What is
// left to differ from NumPy are cos, sin, tan, exp, log, acos and pow.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ansfm {

constexpr int kBrdfBlock = 256;       // threads per workgroup of both kernels; (w, j, i) is flat, so a block spans wavenumbers
constexpr int kBrdfMaxNF = 32;        // Fourier orders of k_brdf_matrix: the accumulators live in registers
constexpr double kBrdfPi = 3.141592653589793;

struct HapkeWave {                    // per wavenumber
    double w, K, BS0, rhs, BC0, rhc, G1, G2, F;   // rhs = 1 / hs, rhc = 1 / hc
    double r0, tb, ttb, chi;          // theta_bar (degrees), tan(theta_bar), chi
};

struct HapkeAngle {                   // per incidence or emission angle
    double x, c, s, E1, E2, nu;       // degrees, cos, sin
};

struct HapkeAzimuth {                 // per azimuth
    double cphi, sphi2, fphi, phipi;  // cos(phix), sin^2(phix / 2), f(phi), phirad / pi
};

__device__ __forceinline__ double brdf_rad(double deg)
{
#pragma clang fp contract(off)
    return deg / 180. * kBrdfPi;
}

__device__ __forceinline__ HapkeWave hapke_wave(const double *__restrict__ params, size_t nwave, size_t w)
{
#pragma clang fp contract(off)
    HapkeWave h;
    h.w = params[w]; h.K = params[nwave + w]; h.BS0 = params[2 * nwave + w]; h.rhs = 1. / params[3 * nwave + w];
    h.BC0 = params[4 * nwave + w]; h.rhc = 1. / params[5 * nwave + w];
    const double rough = params[6 * nwave + w];
    h.G1 = params[7 * nwave + w]; h.G2 = params[8 * nwave + w]; h.F = params[9 * nwave + w];
    const double gamma = __dsqrt_rn(1. - h.w);
    h.r0 = (1. - gamma) / (1. + gamma);
    h.tb = rough * (1. - h.r0);
    h.ttb = tan(brdf_rad(h.tb));
    h.chi = 1. / __dsqrt_rn(1. + kBrdfPi * (h.ttb * h.ttb));
    return h;
}

__device__ __forceinline__ HapkeAngle hapke_angle(const HapkeWave &h, double x)
{
#pragma clang fp contract(off)
    HapkeAngle a;
    const double xr = brdf_rad(x);
    a.x = x; a.c = cos(xr); a.s = sin(xr);
    if (h.tb == 0.0 || x == 0.0) {
        a.E1 = 0.0; a.E2 = 0.0;
    } else {
        const double t = tan(xr);
        a.E1 = exp(-2.0 / kBrdfPi / h.ttb / t);
        a.E2 = exp(-1.0 / kBrdfPi / (h.ttb * h.ttb) / (t * t));
    }
    a.nu = h.chi * (a.c + a.s * h.ttb * a.E2 / (2.0 - a.E1));
    return a;
}

// phix: the azimuth already folded into [0, 180]
__device__ __forceinline__ HapkeAzimuth hapke_azimuth(double phix)
{
#pragma clang fp contract(off)
    HapkeAzimuth z;
    const double phirad = brdf_rad(phix);
    z.cphi = cos(phirad);
    const double sh = sin(phirad / 2.);
    z.sphi2 = sh * sh;
    z.fphi = fabs(phix) == 180. ? 0.0 : exp(-2. * fabs(tan(brdf_rad(phix / 2.))));
    z.phipi = phirad / kBrdfPi;
    return z;
}

__device__ __forceinline__ double hapke_H(double w, double x, double r0)
{
#pragma clang fp contract(off)
    return 1.0 / (1.0 - w * x * (r0 + (1.0 - 2.0 * r0 * x) / 2.0 * log((1.0 + x) / x)));
}

// i, e: incidence and emission, both below 90 degrees
__device__ __forceinline__ double hapke_eval(const HapkeWave &h, const HapkeAngle &i, const HapkeAngle &e, const HapkeAzimuth &z)
{
#pragma clang fp contract(off)
    const double mu = e.c, mu0 = i.c;
    double cg = mu * mu0 + __dsqrt_rn(1. - mu * mu) * __dsqrt_rn(1. - mu0 * mu0) * z.cphi;
    if (cg > 1.0) cg = 1.0;
    if (cg < 0.0) cg = 0.0;
    const double g = acos(cg) / kBrdfPi * 180.;
    const bool ile = i.x <= e.x;
    const HapkeAngle &s = ile ? i : e, &l = ile ? e : i;
    const double den = 2.0 - l.E1 - z.phipi * s.E1;
    const double eff_s = h.chi * (s.c + s.s * h.ttb * (z.cphi * l.E2 + z.sphi2 * s.E2) / den);
    const double eff_l = h.chi * (l.c + l.s * h.ttb * (l.E2 - z.sphi2 * s.E2) / den);
    const double mu0eff = ile ? eff_s : eff_l, mueff = ile ? eff_l : eff_s;
    const double S = mueff / e.nu * mu0 / i.nu * h.chi / (1.0 - z.fphi + z.fphi * h.chi * s.c / s.nu);
    const double tg = tan(brdf_rad(g / 2.));
    const double Bs = h.BS0 / (1. + h.rhs * tg);
    const double q = h.rhc * tg;
    const double Bc = h.BC0 / (1. + (1.3 + h.K) * (q + q * q));
    const double H0e = hapke_H(h.w, mu0eff / h.K, h.r0), He = hapke_H(h.w, mueff / h.K, h.r0);
    const double cth = cos(brdf_rad(g));
    const double t1 = (1. - h.G1 * h.G1) / pow(1. - 2. * h.G1 * cth + h.G1 * h.G1, 1.5);
    const double t2 = (1. - h.G2 * h.G2) / pow(1. - 2. * h.G2 * cth + h.G2 * h.G2, 1.5);
    const double phase = h.F * t1 + (1.0 - h.F) * t2;
    const double r = h.K * h.w / (4. * kBrdfPi) * mu0eff / (mu0eff + mueff) * (phase * (1. + Bs) + (H0e * He - 1.)) * (1. + Bc) * S;
    return r / mu0;
}

// the fold of :1363-1381
__device__ __forceinline__ double brdf_fold(double phi_nemesis)
{
#pragma clang fp contract(off)
    const double phi = 180. - phi_nemesis;
    return phi > 180. ? 180. - (phi - 180.) : (phi < 0. ? -phi : phi);
}

__device__ __forceinline__ double oren_nayar_point(double A, double rough, double i, double e, double phi)
{
#pragma clang fp contract(off)
    const double irad = brdf_rad(i), erad = brdf_rad(e), sigma = brdf_rad(rough);
    const double alpha = fmax(irad, erad), beta = fmin(irad, erad);
    const double s2 = sigma * sigma, cphi = cos(brdf_rad(phi)), sa = sin(alpha), b2 = 2. * beta / kBrdfPi;
    const double C1 = 1.0 - 0.5 * s2 / (s2 + 0.33);
    const double C2 = 0.45 * s2 / (s2 + 0.09) * (cphi >= 0 ? sa : sa - pow(b2, 3.));
    const double a4 = 4. * alpha * beta / (kBrdfPi * kBrdfPi);
    const double C3 = 0.125 * s2 / (s2 + 0.09) * (a4 * a4);
    const double B1 = A / kBrdfPi * (C1 + cphi * C2 * tan(beta) + (1. - fabs(cphi)) * C3 * tan((alpha + beta) / 2.));
    const double B2 = 0.17 * (A * A) / kBrdfPi * s2 / (s2 + 0.13) * (1.0 - cphi * (b2 * b2));
    return B1 + B2;
}

// The BRDF at one point: lowbc 1 LAMBERTIAN, 2 HAPKE, 3 OREN_NAYAR (the host admits no other); params[npar][nwave]
__device__ __forceinline__ double brdf_point(int lowbc, const double *__restrict__ params, size_t nwave, size_t w, double sol, double emi,
                                             double azi)
{
#pragma clang fp contract(off)
    if (lowbc == 1) return params[w] / kBrdfPi;
    if (lowbc == 3) return oren_nayar_point(params[w], params[nwave + w], sol, emi, azi);
    if (emi >= 90. || sol >= 90.) return 0.0;
    const HapkeWave h = hapke_wave(params, nwave, w);
    return hapke_eval(h, hapke_angle(h, sol), hapke_angle(h, emi), hapke_azimuth(brdf_fold(azi)));
}

__global__ void __launch_bounds__(kBrdfBlock)
k_brdf_points(int lowbc, size_t nwave, size_t ntheta, const double *__restrict__ params, const double *__restrict__ sol,
              const double *__restrict__ emi, const double *__restrict__ azi, double *__restrict__ brdf)
{
    const size_t t = (size_t)blockIdx.x * kBrdfBlock + threadIdx.x;
    if (t >= nwave * ntheta) return;
    const size_t w = t / ntheta, a = t - w * ntheta;
    brdf[t] = brdf_point(lowbc, params, nwave, w, sol[a], emi[a], azi[a]);
}

// azi[4][nphi + 1]: cos(phix), sin^2(phix / 2), f(phi), phirad / pi
__global__ void __launch_bounds__(kBrdfBlock)
k_brdf_azimuth(int nk, const double *__restrict__ phix, double *__restrict__ azi)
{
    const int k = blockIdx.x * kBrdfBlock + threadIdx.x;
    if (k >= nk) return;
    const HapkeAzimuth z = hapke_azimuth(phix[k]);
    azi[k] = z.cphi; azi[nk + k] = z.sphi2; azi[2 * nk + k] = z.fphi; azi[3 * nk + k] = z.phipi;
}

// NACC >= nf + 1 accumulators in registers (the loop over them is unrolled; those beyond nf are never touched).
// lowbc 2: the integration; lowbc 1: plane 0 = albedo / pi, set (:5205-5209); the host zeroes the matrix for the rest.
template <int NACC>
__global__ void __launch_bounds__(kBrdfBlock)
k_brdf_matrix(int lowbc, size_t nwave, int nmu, int nphi, int nf, const double *__restrict__ params, const double *__restrict__ ang,
              const double *__restrict__ azi, const double *__restrict__ wphi, const double *__restrict__ cosk,
              double *__restrict__ brdf_mat)
{
#pragma clang fp contract(off)
    const size_t t = (size_t)blockIdx.x * kBrdfBlock + threadIdx.x, per = (size_t)nmu * nmu;
    if (t >= nwave * per) return;
    const size_t w = t / per;
    const int r = (int)(t - w * per), i = r / nmu, j = r - i * nmu;          // j, the solar angle, runs fastest: so does the output
    double *out = brdf_mat + t * (size_t)(nf + 1);                           // [w][i][j][ic]
    double acc[NACC];
#pragma unroll
    for (int ic = 0; ic < NACC; ++ic) acc[ic] = 0.0;
    if (lowbc == 1) {
        acc[0] = params[w] / kBrdfPi;
    } else if (ang[i] < 90. && ang[j] < 90.) {
        const int nk = nphi + 1;
        const HapkeWave h = hapke_wave(params, nwave, w);
        const HapkeAngle sol = hapke_angle(h, ang[j]), emi = hapke_angle(h, ang[i]);
        for (int k = 0; k < nk; ++k) {
            const HapkeAzimuth z = {azi[k], azi[nk + k], azi[2 * nk + k], azi[3 * nk + k]};
            const double wb = wphi[k] * hapke_eval(h, sol, emi, z);
#pragma unroll
            for (int ic = 0; ic < NACC; ++ic)
                if (ic <= nf) acc[ic] += wb * cosk[(size_t)ic * nk + k];
        }
    }
#pragma unroll
    for (int ic = 0; ic < NACC; ++ic)
        if (ic <= nf) out[ic] = acc[ic];
}

}  // namespace ansfm

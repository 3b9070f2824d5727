// ansfm_hgfit_kernels.hip.h -- double Henyey-Greenstein fit of a phase function on gfx950 (fp64).
//
// Restates Scatter_0.subfithgm (Scatter_0.py:1948) = mrqminl (:2017) over mrqcofl (:2096), subhgphas (:2122) and henyey
// (:2159): a Levenberg-Marquardt chain on (f, g1, g2) against the log of the phase function, once per wavelength.  The
// arithmetic is written down in tests/hgfit_cases.py (subfithgm_np, order="kernel"), operation by operation.
//   k_hg_fit   one wavefront per fit, lane i holds the angles i, i + 64, ...: per call of mrqminl the double-HG function at the
//              trial point and at its three perturbed points, kk / cphase, log, dy, and the ten sums (six of alpha, three of
//              beta, chisq) reduced together
// The sums have one order: each lane adds its own angles in ascending order, then the halving tree lane i += lane i + s
// (s = 32 .. 1) across the wavefront, and lane 0's value is broadcast -- every lane then holds the same bits, so the 3 x 3
// normal equations (Gaussian elimination with partial pivoting, every lane redundantly), the clip of the trial point and the
// accept / reject branch are wave-uniform.  h(g1) and h(g2) of the unperturbed point are computed once per angle and used in
// all four functions (the reference computes them again, to the same bits).  The first angle of a lane stays in registers;
// the angles of the later passes come from memory, where the lane wrote log(phase) itself.  No LDS, no atomics.
// Nothing is contracted into fma: what is left to differ from NumPy are pow and log (cos is the host's).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ansfm {

constexpr int kHgLanes = 64;           // angles per pass = lanes of a wavefront
constexpr int kHgWaves = 4;            // wavefronts (fits) per workgroup
constexpr int kHgNphaseCap = 8192;     // angles of a phase function
constexpr int kHgCalls = 1000;         // calls of mrqminl a fit may take (nover, :1983)

struct HgFitParams {
    int nfit, nphase;
    const double *calpha;              // [nphase] cos(theta)
    double *lphase;                    // [nfit][nphase] the phase functions; from angle 64 on the kernel leaves their logarithms here
    double *out;                       // [4][nfit] f, g1, g2, rms
    int32_t *counts;                   // [nfit][2] calls of mrqminl, accepted ones
    int32_t *fail;                     // [nfit] 1: an exact zero pivot ended the fit
};

struct HgSums { double a00, a10, a11, a20, a21, a22, b0, b1, b2, chisq; };

// h(g) = (1 - g^2) / (1 + g^2 - 2 g cos)^1.5 (henyey :2163)
__device__ __forceinline__ double hg_term(double g, double ca)
{
#pragma clang fp contract(off)
    return (1.0 - g * g) / pow(1.0 + g * g - 2 * g * ca, 1.5);
}

struct HgPoint { double f, g1, g2, ft, g1t, g2t, dx0, dx1, dx2; };

// the three perturbed points of subhgphas (:2138-2147), with the sign flips
__device__ __forceinline__ HgPoint hg_point(double f, double g1, double g2)
{
#pragma clang fp contract(off)
    HgPoint p;
    p.f = f; p.g1 = g1; p.g2 = g2;
    p.ft = f + 0.01;
    if (p.ft > 0.99) p.ft = f - 0.01;
    p.g1t = g1 + 0.01;
    if (p.g1t > 0.98) p.g1t = g1 - 0.01;
    p.g2t = g2 + 0.01;
    p.dx0 = p.ft - f; p.dx1 = p.g1t - g1; p.dx2 = p.g2t - g2;
    return p;
}

// one angle's terms of mrqcofl's sums (:2105-2115), added to s
__device__ __forceinline__ void hg_angle(const HgPoint &p, double ca, double lph, HgSums &s)
{
#pragma clang fp contract(off)
    const double h1 = hg_term(p.g1, ca), h2 = hg_term(p.g2, ca);
    const double h1t = hg_term(p.g1t, ca), h2t = hg_term(p.g2t, ca);
    const double cph = p.f * h1 + (1.0 - p.f) * h2;
    double k0 = ((p.ft * h1 + (1.0 - p.ft) * h2) - cph) / p.dx0;
    double k1 = ((p.f * h1t + (1.0 - p.f) * h2) - cph) / p.dx1;
    double k2 = ((p.f * h1 + (1.0 - p.f) * h2t) - cph) / p.dx2;
    k0 = k0 / cph; k1 = k1 / cph; k2 = k2 / cph;
    const double dy = lph - log(cph);
    s.a00 += k0 * k0; s.a10 += k1 * k0; s.a11 += k1 * k1;
    s.a20 += k2 * k0; s.a21 += k2 * k1; s.a22 += k2 * k2;
    s.b0 += dy * k0; s.b1 += dy * k1; s.b2 += dy * k2;
    s.chisq += dy * dy;
}

__device__ __forceinline__ double hg_wave_sum(double v)
{
#pragma clang fp contract(off)
    for (int st = kHgLanes / 2; st >= 1; st >>= 1) v += __shfl_down(v, st, kHgLanes);   // lanes >= st: not part of lane 0's tree
    return __shfl(v, 0, kHgLanes);
}

// mrqcofl at (f, g1, g2): every lane returns the same ten sums
__device__ __forceinline__ HgSums hg_sums(int lane, int nphase, const double *calpha, const double *lphase, double ca0, double lph0,
                                          double f, double g1, double g2)
{
#pragma clang fp contract(off)
    const HgPoint p = hg_point(f, g1, g2);
    HgSums s = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    if (lane < nphase) hg_angle(p, ca0, lph0, s);
    for (int i = lane + kHgLanes; i < nphase; i += kHgLanes) hg_angle(p, calpha[i], lphase[i], s);
    s.a00 = hg_wave_sum(s.a00); s.a10 = hg_wave_sum(s.a10); s.a11 = hg_wave_sum(s.a11);
    s.a20 = hg_wave_sum(s.a20); s.a21 = hg_wave_sum(s.a21); s.a22 = hg_wave_sum(s.a22);
    s.b0 = hg_wave_sum(s.b0); s.b1 = hg_wave_sum(s.b1); s.b2 = hg_wave_sum(s.b2);
    s.chisq = hg_wave_sum(s.chisq);
    return s;
}

// (alpha with its diagonal times (1 + alamda)) da = beta (:2036-2047) by Gaussian elimination; column by column the row of
// the largest magnitude becomes the pivot (the first of equals; a NaN never displaces).  false: an exact zero pivot.
__device__ __forceinline__ bool hg_solve3(const HgSums &s, double alamda, double &d0, double &d1, double &d2)
{
#pragma clang fp contract(off)
    double m00 = s.a00 * (1.0 + alamda), m01 = s.a10, m02 = s.a20, r0 = s.b0;
    double m10 = s.a10, m11 = s.a11 * (1.0 + alamda), m12 = s.a21, r1 = s.b1;
    double m20 = s.a20, m21 = s.a21, m22 = s.a22 * (1.0 + alamda), r2 = s.b2;
    double t;
#define HG_SWAP(a, b) do { t = a; a = b; b = t; } while (0)
    double big = fabs(m00);
    const bool p1 = fabs(m10) > big;
    if (p1) big = fabs(m10);
    const bool p2 = fabs(m20) > big;
    if (p2) { HG_SWAP(m00, m20); HG_SWAP(m01, m21); HG_SWAP(m02, m22); HG_SWAP(r0, r2); }
    else if (p1) { HG_SWAP(m00, m10); HG_SWAP(m01, m11); HG_SWAP(m02, m12); HG_SWAP(r0, r1); }
    if (m00 == 0.0) return false;
    double l = m10 / m00;
    m11 = m11 - l * m01; m12 = m12 - l * m02; r1 = r1 - l * r0;
    l = m20 / m00;
    m21 = m21 - l * m01; m22 = m22 - l * m02; r2 = r2 - l * r0;
    if (fabs(m21) > fabs(m11)) { HG_SWAP(m11, m21); HG_SWAP(m12, m22); HG_SWAP(r1, r2); }
#undef HG_SWAP
    if (m11 == 0.0) return false;
    l = m21 / m11;
    m22 = m22 - l * m12; r2 = r2 - l * r1;
    if (m22 == 0.0) return false;
    d2 = r2 / m22;
    d1 = (r1 - m12 * d2) / m11;
    d0 = (r0 - m01 * d1 - m02 * d2) / m00;
    return true;
}

__global__ void __launch_bounds__(kHgLanes * kHgWaves) k_hg_fit(HgFitParams p)
{
#pragma clang fp contract(off)
    const int lane = threadIdx.x & (kHgLanes - 1);
    const int fit = blockIdx.x * kHgWaves + threadIdx.x / kHgLanes;
    if (fit >= p.nfit) return;                          // the whole wavefront
    double *lphase = p.lphase + (size_t)fit * p.nphase;
    double ca0 = 0.0, lph0 = 0.0;
    if (lane < p.nphase) { ca0 = p.calpha[lane]; lph0 = log(lphase[lane]); }
    for (int i = lane + kHgLanes; i < p.nphase; i += kHgLanes) lphase[i] = log(lphase[i]);   // read back by this lane only

    // subfithgm (:1981-2006) with mrqminl's first-call branch (:2025-2033) ahead of the loop
    double f = 0.5, g1 = 0.5, g2 = -0.5;
    HgSums cur = hg_sums(lane, p.nphase, p.calpha, lphase, ca0, lph0, f, g1, g2);
    double ochisq = cur.chisq, alamda = 1000.0;
    double chisq = 0.0;                                 // what prev_chisq sees before the first call
    int calls = 0, accepted = 0, nc = 0, failed = 0;
    for (int it = 0; it < kHgCalls; ++it) {
        const double prev = chisq;
        double d0, d1, d2;
        if (!hg_solve3(cur, alamda, d0, d1, d2)) { failed = 1; break; }
        double ft = f + d0, g1t = g1 + d1, g2t = g2 + d2;
        // the reference's comparisons (:2055-2070), not fmin / fmax: a NaN passes through
        if (ft > 0.999999) ft = 0.999999;
        if (ft < 0.000001) ft = 0.000001;
        if (g1t > 0.98) g1t = 0.98;
        if (g1t < 0.0) g1t = 0.0;
        if (g2t < -0.98) g2t = -0.98;
        if (g2t > -0.1) g2t = -0.1;
        const HgSums trial = hg_sums(lane, p.nphase, p.calpha, lphase, ca0, lph0, ft, g1t, g2t);
        ++calls;
        if (trial.chisq <= ochisq) {
            ++accepted;
            alamda = 0.9 * alamda;
            chisq = trial.chisq; ochisq = trial.chisq;
            cur = trial;
            f = ft; g1 = g1t; g2 = g2t;
            const double rel = fabs(chisq - prev) / (chisq + prev + 1e-30);
            if (rel < 1e-8) {
                if (++nc > 5) break;
            } else {
                nc = 0;
            }
        } else {
            alamda = 1.5 * alamda;
            chisq = ochisq;
            if (alamda > 1e36) alamda = 1e36;
        }
    }
    if (lane == 0) {
        p.out[fit] = f;
        p.out[(size_t)p.nfit + fit] = g1;
        p.out[(size_t)2 * p.nfit + fit] = g2;
        p.out[(size_t)3 * p.nfit + fit] = sqrt(chisq);
        p.counts[2 * (size_t)fit] = calls;
        p.counts[2 * (size_t)fit + 1] = accepted;
        p.fail[fit] = failed;
    }
}

}  // namespace ansfm

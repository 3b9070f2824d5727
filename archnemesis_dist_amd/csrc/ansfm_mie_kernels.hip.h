// ansfm_mie_kernels.hip.h -- Mie theory over a particle size distribution on gfx950 (fp64).
//
// Restates Scatter_0.makephase (Scatter_0.py:1828) = miescat (:1600) over dmie (:1399) for iscat 1 .. 4; the arithmetic is
// written down in tests/mie_cases.py (makephase_np), operation by operation in the reference's order.  Every
// (wavelength, radius) pair is independent up to one sequential test per wavelength, the cut-off of an open range:
//   k_mie_coeff    one thread per (wavelength, radius) of a block of radii: x = 2 pi r / lambda, the logarithmic derivative
//                  D_n(m x) downwards from nmx1 = max(150, int(1.1 |m| x)), the Riccati-Bessel functions upwards, a_n and b_n
//                  until |a_n|^2 + |b_n|^2 < 1e-14 -> Q_ext, Q_sca, the term count, n(r), a failure code, and a_n, b_n in HBM
//   k_mie_cutoff   one thread per wavelength: the reference's walk over the block's radii (running maximum of n Q_sca; the
//                  first radius with r >= r_peak and n Q_sca <= 1e-6 max ends an open range and is still summed); a failure
//                  code counts only when the walk reaches its radius
//   k_mie_angles   one wavefront per (wavelength, chunk of 64 radii, angle), one lane per radius: pi_n / tau_n, the four
//                  amplitude sums at theta and at 180 - theta, (M1 + M2)/2 times n(r) and the Simpson weight, then the sum
//                  over the chunk's 64 lanes; the wavefront after the last angle sums k_sca, k_ext and the norm
//   k_mie_accum    adds the block's chunk sums onto the running totals in ascending chunk order
//   k_mie_finish   cross-sections in cm^2, phase = lambda^2 sum / (pi k_sca), the angles beyond 90 degrees mirrored
// The sum over radii has one order whatever the block size: chunks of 64 radii aligned at radius 0, inside a chunk the
// halving tree lane i += lane i + s (s = 32 .. 1), the chunks one after the other -- radii beyond the end of the integration
// add +0.0.  No atomics.  D_n and the coefficients of a thread live in the context's workspace, [order][component][thread]
// (a thread's neighbours in the wavefront are the neighbouring radii): no per-thread array is indexed at run time.
// Nothing is contracted into fma: what is left to differ from NumPy are sin, cos, exp, log and pow.
#pragma once
#include <hip/hip_runtime.h>
#include <limits.h>
#include <stdint.h>

namespace ansfm {

constexpr int kMieChunk = 64;         // radii per chunk of the sum = lanes of a wavefront
constexpr int kMieAngleWaves = 4;     // wavefronts (angles) per workgroup of k_mie_angles
constexpr int kMieNcap = 29999;       // the reference gives up at nmx1 >= ncap - 1 (:1437, :1458)

struct MieParams {
    const double *wavel, *refindx;    // [nwave], [nwave][2]
    const double *cstht, *si2tht;     // [ntheta] cos and sin^2 of the angles
    int nwave, ntheta, nphas, iscat;
    double d0, d1, d2;                // dsize
    double r1, delr, rmax, sqrt2pi;   // first radius, step, r_peak of the open range's test, sqrt(2 pi)
    int inr;                          // radii of a closed range; 0: open
    int mend;                         // no radius at or above it is computed: inr, or the cap of an open range
    int m0, nrad, NH;                 // the block: radii m0 .. m0 + nrad - 1 (nrad a multiple of 64); rows of acap / coef
    // per thread t = wave * nrad + radius in the block, T = nwave * nrad
    double *acap;                     // [NH][2][T]  D_n in row n - 1
    double *coef;                     // [NH][4][T]  Re a_n, Im a_n, Re b_n, Im b_n in row n - 1 (row 0 times 3/2, as the reference holds it)
    double *qext, *qsca, *anr;        // [T]
    int *nterm, *fail;                // [T] terms summed (0: not computed); 0, 1: nmx1 >= 29999, 2: more than nmx2 terms, 3: NH too small
    // per wavelength
    int *mcut;                        // last radius of the integration, INT_MAX until it is known
    int *failcode, *failm;            // the failure the walk met, and its radius
    double *nqmax;                    // running maximum of n Q_sca
    double *partial;                  // [nrad / 64][nwave][ntheta + 1][3] chunk sums (theta, 180 - theta, -; row ntheta: k_sca, k_ext, norm)
    double *total;                    // [nwave][ntheta + 1][3]
    double *xscat, *xext, *phas;      // [nwave], [nwave], [nwave][nphas]
};

struct MieC { double r, i; };

__device__ __forceinline__ MieC mie_cmul(MieC a, MieC b)
{
#pragma clang fp contract(off)
    return {a.r * b.r - a.i * b.i, a.r * b.i + a.i * b.r};
}

// NumPy's complex division (Smith's form with a reciprocal)
__device__ __forceinline__ MieC mie_cdiv(MieC a, MieC b)
{
#pragma clang fp contract(off)
    if (fabs(b.r) >= fabs(b.i)) {
        const double rat = b.i / b.r, scl = 1.0 / (b.r + b.i * rat);
        return {(a.r + a.i * rat) * scl, (a.i - a.r * rat) * scl};
    }
    const double rat = b.r / b.i, scl = 1.0 / (b.i + b.r * rat);
    return {(a.r * rat + a.i) * scl, (a.i * rat - a.r) * scl};
}

// a_n or b_n: (tc psi_n - psi_{n-1}) / (tc xi_n - xi_{n-1})
__device__ __forceinline__ MieC mie_coeff(MieC tc, MieC wfn2, MieC wfn1)
{
#pragma clang fp contract(off)
    const MieC num = {tc.r * wfn2.r - wfn1.r, tc.i * wfn2.r};
    const MieC q = mie_cmul(tc, wfn2);
    return mie_cdiv(num, {q.r - wfn1.r, q.i - wfn1.i});
}

__device__ __forceinline__ double mie_simpson(int m, int inr, double delr)
{
#pragma clang fp contract(off)
    if (m == 0 || m == inr - 1) return delr / 3.0;
    return (m % 2 == 0) ? 2.0 * delr / 3.0 : 4.0 * delr / 3.0;
}

__global__ void __launch_bounds__(256) k_mie_coeff(MieParams p)
{
#pragma clang fp contract(off)
    const int T = p.nwave * p.nrad;
    const int tid = blockIdx.x * blockDim.x + threadIdx.x;
    if (tid >= T) return;
    const int j = tid % p.nrad, w = tid / p.nrad, m = p.m0 + j;
    p.nterm[tid] = 0; p.fail[tid] = 0;
    p.qext[tid] = 0.0; p.qsca[tid] = 0.0; p.anr[tid] = 0.0;
    if (m >= p.mend || p.mcut[w] < p.m0) return;          // beyond the range, or this wavelength has ended
    const double xlam = p.wavel[w], rfr = p.refindx[2 * w], rfi = p.refindx[2 * w + 1];
    const double rr = p.r1 + (double)m * p.delr;
    const double x = 2.0 * M_PI * rr / xlam;

    double anr = 1.0;
    if (p.d1 != 0.0 && p.iscat != 4) {
        if (p.iscat == 1) {
            anr = pow(rr, p.d2) * exp(-rr / (p.d0 * p.d1));
        } else if (p.iscat == 2) {
            const double d = log(rr) - log(p.d0);
            anr = 1.0 / (rr * p.d1 * p.sqrt2pi) * exp(-(d * d) / (2.0 * (p.d1 * p.d1)));
        } else {
            anr = pow(rr, p.d0) * exp(-p.d1 * pow(rr, p.d2));
        }
    }
    p.anr[tid] = anr;

    const MieC rf = {rfr, -rfi};
    const MieC rrf = mie_cdiv({1.0, 0.0}, rf);
    const double rx = 1.0 / x;
    const MieC rrfx = {rrf.r * rx, rrf.i * rx};
    const double t0 = sqrt(x * x * (rfr * rfr + rfi * rfi));
    if (!(1.1 * t0 < (double)kMieNcap)) { p.fail[tid] = 1; return; }      // int(1.1 t0) >= 29999, or not a number
    int nmx1 = (int)(1.1 * t0), nmx2 = (int)t0;
    if (!(nmx1 > 150)) { nmx1 = 150; nmx2 = 135; }
    if (nmx2 > p.NH) { p.fail[tid] = 3; return; }

    // D_n downwards from D_{nmx1 + 1} = 0; the series reads D_1 .. D_nmx2 at most
    MieC cur = {0.0, 0.0};
    for (int nn = nmx1; nn >= 1; --nn) {
        const double k = (double)(nn + 1);
        const MieC a = {k * rrfx.r, k * rrfx.i};
        const MieC inv = mie_cdiv({1.0, 0.0}, {a.r + cur.r, a.i + cur.i});
        cur = {a.r - inv.r, a.i - inv.i};
        if (nn <= nmx2) {
            p.acap[((size_t)(nn - 1) * 2 + 0) * T + tid] = cur.r;
            p.acap[((size_t)(nn - 1) * 2 + 1) * T + tid] = cur.i;
        }
    }

    const double cx = cos(x), sx = sin(x);
    MieC wm1 = {cx, -sx}, wfn1 = {sx, cx};
    MieC wfn2 = {rx * wfn1.r - wm1.r, rx * wfn1.i - wm1.i};
    MieC D = {p.acap[tid], p.acap[(size_t)T + tid]};
    MieC q1 = mie_cmul(D, rrf), q2 = mie_cmul(D, rf);
    MieC fna = mie_coeff({q1.r + rx, q1.i}, wfn2, wfn1);
    MieC fnb = mie_coeff({q2.r + rx, q2.i}, wfn2, wfn1);
    double tb0 = 1.5 * fna.r, tb1 = 1.5 * fna.i, tc0 = 1.5 * fnb.r, tc1 = 1.5 * fnb.i;
    p.coef[(size_t)0 * T + tid] = tb0; p.coef[(size_t)1 * T + tid] = tb1;
    p.coef[(size_t)2 * T + tid] = tc0; p.coef[(size_t)3 * T + tid] = tc1;
    double qext = 2.0 * (tb0 + tc0);
    double qsca = (tb0 * tb0 + tb1 * tb1 + tc0 * tc0 + tc1 * tc1) / 0.75;
    int n = 2, code = 0;
    for (;;) {
        const double u0 = (double)(2 * n - 1), u2 = (double)(2 * n + 1);
        wm1 = wfn1; wfn1 = wfn2;
        const double f = u0 * rx;
        wfn2 = {f * wfn1.r - wm1.r, f * wfn1.i - wm1.i};
        D = {p.acap[((size_t)(n - 1) * 2 + 0) * T + tid], p.acap[((size_t)(n - 1) * 2 + 1) * T + tid]};
        q1 = mie_cmul(D, rrf); q2 = mie_cmul(D, rf);
        const double nrx = (double)n * rx;
        fna = mie_coeff({q1.r + nrx, q1.i}, wfn2, wfn1);
        fnb = mie_coeff({q2.r + nrx, q2.i}, wfn2, wfn1);
        tb0 = fna.r; tb1 = fna.i; tc0 = fnb.r; tc1 = fnb.i;
        double *row = p.coef + (size_t)(n - 1) * 4 * T + tid;
        row[0] = tb0; row[(size_t)T] = tb1; row[(size_t)2 * T] = tc0; row[(size_t)3 * T] = tc1;
        qext += u2 * (tb0 + tc0);
        const double t3 = tb0 * tb0 + tc0 * tc0 + tb1 * tb1 + tc1 * tc1;
        qsca += u2 * t3;
        if (t3 < 1e-14) break;
        ++n;
        if (n > nmx2) { code = 2; break; }
    }
    if (code) { p.fail[tid] = code; return; }
    const double t = 2.0 * rx * rx;
    p.qext[tid] = qext * t;
    p.qsca[tid] = qsca * t;
    p.nterm[tid] = n;
}

__global__ void __launch_bounds__(64) k_mie_cutoff(MieParams p)
{
#pragma clang fp contract(off)
    const int w = blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= p.nwave || p.mcut[w] < p.m0) return;
    double nqmax = p.nqmax[w];
    for (int j = 0; j < p.nrad; ++j) {
        const int m = p.m0 + j, tid = w * p.nrad + j;
        if (m >= p.mend) break;
        if (p.fail[tid]) { p.failcode[w] = p.fail[tid]; p.failm[w] = m; p.mcut[w] = m - 1; break; }
        const double nq = p.anr[tid] * p.qsca[tid];
        if (nq > nqmax) nqmax = nq;
        if (p.inr == 0) {
            const double rr = p.r1 + (double)m * p.delr;
            if (!(rr < p.rmax || nq > 1e-06 * nqmax)) { p.mcut[w] = m; break; }
        } else if (m == p.inr - 1) {
            p.mcut[w] = m;
            break;
        }
    }
    p.nqmax[w] = nqmax;
}

__global__ void __launch_bounds__(kMieChunk * kMieAngleWaves) k_mie_angles(MieParams p)
{
#pragma clang fp contract(off)
    __shared__ double s[kMieAngleWaves][3][kMieChunk];
    const int lane = threadIdx.x & (kMieChunk - 1), wf = threadIdx.x / kMieChunk;
    const int a = blockIdx.z * kMieAngleWaves + wf, w = blockIdx.y;
    const int j = blockIdx.x * kMieChunk + lane, m = p.m0 + j;
    const int T = p.nwave * p.nrad, tid = w * p.nrad + j;
    double v0 = 0.0, v1 = 0.0, v2 = 0.0;
    const int nterm = (a <= p.ntheta && m < p.mend && m <= p.mcut[w]) ? p.nterm[tid] : 0;
    if (nterm > 0) {
        const double anr = p.anr[tid], vv = mie_simpson(m, p.inr, p.delr);
        if (a == p.ntheta) {
            const double rr = p.r1 + (double)m * p.delr;
            v0 = M_PI * rr * rr * p.qsca[tid] * anr * vv;
            v1 = M_PI * rr * rr * p.qext[tid] * anr * vv;
            v2 = anr * vv;
        } else {
            const double c = p.cstht[a], s2 = p.si2tht[a];
            const double *row = p.coef + tid;
            double tb0 = row[0], tb1 = row[(size_t)T], tc0 = row[(size_t)2 * T], tc1 = row[(size_t)3 * T];
            double pi0 = 0.0, pi1 = 1.0, tau0 = 0.0, tau1 = c;
            double e0 = tb0 * pi1 + tc0 * tau1, e1 = tb1 * pi1 + tc1 * tau1;
            double e2 = tc0 * pi1 + tb0 * tau1, e3 = tc1 * pi1 + tb1 * tau1;
            double b0 = tb0 * pi1 - tc0 * tau1, b1 = tb1 * pi1 - tc1 * tau1;
            double b2 = tc0 * pi1 - tb0 * tau1, b3 = tc1 * pi1 - tb1 * tau1;
            for (int n = 2; n <= nterm; ++n) {
                const double u0 = (double)(2 * n - 1), u1 = (double)(n - 1), u2 = (double)(2 * n + 1);
                const double pi2 = (u0 * pi1 * c - (double)n * pi0) / u1;
                const double tau2 = c * (pi2 - pi0) - u0 * s2 * pi1 + tau0;
                row += (size_t)4 * T;
                tb0 = row[0]; tb1 = row[(size_t)T]; tc0 = row[(size_t)2 * T]; tc1 = row[(size_t)3 * T];
                const double wn = u2 / (double)(n * (n + 1));
                e0 += wn * (tb0 * pi2 + tc0 * tau2); e1 += wn * (tb1 * pi2 + tc1 * tau2);
                e2 += wn * (tc0 * pi2 + tb0 * tau2); e3 += wn * (tc1 * pi2 + tb1 * tau2);
                if (n % 2 == 0) {
                    b0 += wn * (-tb0 * pi2 + tc0 * tau2); b1 += wn * (-tb1 * pi2 + tc1 * tau2);
                    b2 += wn * (-tc0 * pi2 + tb0 * tau2); b3 += wn * (-tc1 * pi2 + tb1 * tau2);
                } else {
                    b0 += wn * (tb0 * pi2 - tc0 * tau2); b1 += wn * (tb1 * pi2 - tc1 * tau2);
                    b2 += wn * (tc0 * pi2 - tb0 * tau2); b3 += wn * (tc1 * pi2 - tb1 * tau2);
                }
                pi0 = pi1; pi1 = pi2; tau0 = tau1; tau1 = tau2;
            }
            const double h = 0.5 * anr * vv;
            v0 = h * ((e2 * e2 + e3 * e3) + (e0 * e0 + e1 * e1));
            v1 = h * ((b2 * b2 + b3 * b3) + (b0 * b0 + b1 * b1));
        }
    }
    s[wf][0][lane] = v0; s[wf][1][lane] = v1; s[wf][2][lane] = v2;
    __syncthreads();
    for (int st = kMieChunk / 2; st >= 1; st >>= 1) {
        if (lane < st) {
            s[wf][0][lane] += s[wf][0][lane + st];
            s[wf][1][lane] += s[wf][1][lane + st];
            s[wf][2][lane] += s[wf][2][lane + st];
        }
        __syncthreads();
    }
    if (lane < 3 && a <= p.ntheta)
        p.partial[(((size_t)blockIdx.x * p.nwave + w) * (p.ntheta + 1) + a) * 3 + lane] = s[wf][lane][0];
}

__global__ void __launch_bounds__(256) k_mie_accum(MieParams p)
{
    const int n = p.nwave * (p.ntheta + 1) * 3;
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    double t = p.total[i];
    for (int c = 0; c < p.nrad / kMieChunk; ++c) t += p.partial[(size_t)c * n + i];
    p.total[i] = t;
}

__global__ void __launch_bounds__(256) k_mie_finish(MieParams p)
{
#pragma clang fp contract(off)
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= p.nwave * p.nphas) return;
    const int w = i / p.nphas, jq = i % p.nphas, A = p.ntheta;
    const double *tot = p.total + (size_t)w * (A + 1) * 3;
    double kscat = tot[A * 3 + 0];
    const double kext = tot[A * 3 + 1], anorm = tot[A * 3 + 2];
    double xscat = 0.0, xext = 0.0;
    if (anorm > 0.0) {
        xscat = kscat / anorm * 1e-08;
        xext = kext / anorm * 1e-08;
    } else {
        kscat = 1.0;
    }
    if (jq == 0) { p.xscat[w] = xscat; p.xext[w] = xext; }
    const double sum = jq < A ? tot[jq * 3] : tot[(p.nphas - 1 - jq) * 3 + 1];
    const double xlam = p.wavel[w];
    p.phas[i] = xlam * xlam * (sum / (M_PI * kscat));
}

}  // namespace ansfm

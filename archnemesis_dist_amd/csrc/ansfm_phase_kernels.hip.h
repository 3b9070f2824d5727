// ansfm_phase_kernels.hip.h -- aerosol phase functions on the calculation grid: Scatter_0.calc_phase (Scatter_0.py:760) for the
// three IMIE modes and calc_phase_ray (:834).  Included by ansfm_phase.hip only.
//
// calc_phase forms phase1 [NWS][nth][NDUST] on the aerosol grid -- the double Henyey-Greenstein function (calc_hgphase :699), the
// tabulated function interpolated in angle (interp_phase :732) or the Legendre series (calc_lpphase :1060) -- and interpolates
// it linearly along the wavenumbers, end intervals extrapolating.  Both interpolations are scipy's interp1d._call_linear:
//   i = clip(searchsorted(x, x_new, 'left'), 1, n - 1);  slope = (y[i] - y[i - 1]) / (x[i] - x[i - 1]);
//   y = slope * (x_new - x[i - 1]) + y[i - 1]
// Every expression below keeps the reference's order of operations and nothing contracts into an fma, so that the results can
// differ from NumPy's only where cos and pow do; the tabulated mode has neither and is the reference bit for bit.
//
//   k_phase_prep     once per wavenumber: the bracket (lo, x_lo, x_hi); once per angle: cos(theta) or the angle's bracket
//   k_phase_hg_grid  F, G1, G2 on the grid by np.interp's rule (ansfm_upload_phase, IMIE 0)
//   k_phase_fn       one lane per (wavenumber, angle), the populations in an inner loop; two builds, by the layout written
//   k_phase_ray      calc_phase_ray
// Nothing here is tiled or staged in LDS: per lane a handful of loads from tables of a few kB that stay in the caches, a few
// dozen flops and one store per population.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ansfm {

constexpr int kPhaseBlock = 256;       // lanes of a block: four wavefronts
constexpr int kPhaseChunk = 8;         // populations whose Legendre sums a lane carries side by side

struct PhaseParams {
    int imie, NWS, NDUST, NTAB, nth, W, Wpad;
    const double *swave;        // [NWS] Scatter.WAVE, strictly ascending
    const double *theta_tab;    // [NTAB] Scatter.THETA (IMIE 1)
    const double *tab;          // IMIE 0: F, G1, G2 [3][NWS][NDUST]; 1: PHASE [NWS][NTAB][NDUST]; 2: WLPOL [NWS][NTAB][NDUST]
    const double *x;            // [W] the calculation wavenumbers
    int32_t *wlo;               // [W] lower node of a wavenumber's interval
    double *xlo, *xhi;          // [W] its ends
    const double *theta;        // [nth] degrees
    double *ca;                 // [nth] cos(theta / 180. * pi) (IMIE 0, 2)
    int32_t *tlo;               // [nth] lower node of an angle's interval (IMIE 1)
    const double *mu;           // [nth] row 1 of the scattering layout
    const double *hg;           // f_w, g1_w, g2_w [3][NDUST][Wpad] (scattering layout, IMIE 0)
    double *out;
    int ostride, ray;           // plain layout: doubles per (wavenumber, angle); 1: calc_phase_ray behind the populations
};

// clip(searchsorted(x, v, 'left'), 1, n - 1) - 1
__device__ __forceinline__ int phase_bracket(const double *x, int n, double v)
{
    int lo = 0, hi = n;
    while (lo < hi) { const int mid = (lo + hi) >> 1; if (x[mid] < v) lo = mid + 1; else hi = mid; }
    return (lo < 1 ? 1 : (lo > n - 1 ? n - 1 : lo)) - 1;
}

__device__ __forceinline__ double phase_cos_deg(double theta)
{
#pragma clang fp contract(off)
    return cos(theta / 180.0 * 3.141592653589793);
}

// interp1d._call_linear on one interval
__device__ __forceinline__ double phase_lin(double ylo, double yhi, double xlo, double xhi, double x)
{
#pragma clang fp contract(off)
    const double slope = (yhi - ylo) / (xhi - xlo);
    return slope * (x - xlo) + ylo;
}

// brackets != 0: the wavenumbers' brackets too (a resident source keeps those of the table's grid)
__global__ __launch_bounds__(kPhaseBlock) void k_phase_prep(PhaseParams p, int brackets)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (brackets && i < p.W) {
        const int lo = phase_bracket(p.swave, p.NWS, p.x[i]);
        p.wlo[i] = lo; p.xlo[i] = p.swave[lo]; p.xhi[i] = p.swave[lo + 1];
    }
    if (i < p.nth) {
        if (p.imie == 1) p.tlo[i] = phase_bracket(p.theta_tab, p.NTAB, p.theta[i]);
        else p.ca[i] = phase_cos_deg(p.theta[i]);
    }
}

// np.interp(x, swave, y[:, d]) for y = F, G1, G2: a node returns its tabulated value, the ends clamp, and in between
// slope * (x - x_j) + y_j with numpy's two fall-backs for a result that is not a number.  hg [3][NDUST][Wpad], zero beyond W.
__global__ __launch_bounds__(kPhaseBlock) void k_phase_hg_grid(PhaseParams p, double *__restrict__ hg)
{
#pragma clang fp contract(off)
    const int w = blockIdx.x * blockDim.x + threadIdx.x, d = blockIdx.y, k = blockIdx.z;
    if (w >= p.Wpad) return;
    double r = 0.0;
    if (w < p.W) {
        const double x = p.x[w];
        const double *y = p.tab + (size_t)k * p.NWS * p.NDUST + d;
        const int n = p.NWS;
        if (x != x) r = x;
        else if (x > p.swave[n - 1]) r = y[(size_t)(n - 1) * p.NDUST];
        else if (x < p.swave[0]) r = y[0];
        else {
            int lo = 0, hi = n;                     // the last node that is <= x
            while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (p.swave[mid] <= x) lo = mid; else hi = mid; }
            const int j = lo;
            const double yj = y[(size_t)j * p.NDUST];
            if (j == n - 1 || p.swave[j] == x) r = yj;
            else {
                const double y1 = y[(size_t)(j + 1) * p.NDUST];
                const double slope = (y1 - yj) / (p.swave[j + 1] - p.swave[j]);
                r = slope * (x - p.swave[j]) + yj;
                if (r != r) {
                    r = slope * (x - p.swave[j + 1]) + y1;
                    if (r != r && yj == y1) r = yj;
                }
            }
        }
    }
    hg[((size_t)k * p.NDUST + d) * p.Wpad + w] = r;
}

// calc_hgphase at one node of the aerosol grid
__device__ __forceinline__ double phase_hg(double f, double g1, double g2, double c)
{
#pragma clang fp contract(off)
    const double t1 = (1.0 - g1 * g1) / pow(1.0 - 2.0 * g1 * c + g1 * g1, 1.5);
    const double t2 = (1.0 - g2 * g2) / pow(1.0 - 2.0 * g2 * c + g2 * g2, 1.5);
    return (f * t1 + (1.0 - f) * t2) / (4.0 * 3.141592653589793);
}

// SCAT = false: out [W][nth][ostride], the reference's layout (ostride = NDUST, or NDUST + 1 with calc_phase_ray last: phase_fn
// of the single-scattering batch).  SCAT = true: phasarr [NDUST][W][2][nth] of the scattering entries, the angles reversed: row 0
// the phase function (IMIE 0: f_w, g1_w, g2_w in the first three slots and zeros behind), row 1 mu.
template <bool SCAT>
__global__ __launch_bounds__(kPhaseBlock) void k_phase_fn(PhaseParams p)
{
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.W * p.nth) return;
    const int w = (int)(idx / p.nth), t = (int)(idx - (size_t)w * p.nth);
    const int ND = p.NDUST, nth = p.nth;
    if (SCAT && p.imie == 0) {
        for (int d = 0; d < ND; ++d) {
            double *o = p.out + ((size_t)d * p.W + w) * 2 * nth;
            o[t] = t < 3 ? p.hg[((size_t)t * ND + d) * p.Wpad + w] : 0.0;
            o[nth + (nth - 1 - t)] = p.mu[t];
        }
        return;
    }
    const int lo = p.wlo[w];
    const double x = p.x[w], xlo = p.xlo[w], xhi = p.xhi[w];
    double *o = SCAT ? p.out + (size_t)w * 2 * nth + (nth - 1 - t) : p.out + idx * p.ostride;
    const size_t od = SCAT ? (size_t)p.W * 2 * nth : 1;         // from one population to the next
    if (p.imie == 0) {
        const double c = p.ca[t];
        const size_t plane = (size_t)p.NWS * ND;
        const double *a = p.tab + (size_t)lo * ND, *b = a + ND;
        for (int d = 0; d < ND; ++d) {
            const double ylo = phase_hg(a[d], a[plane + d], a[2 * plane + d], c);
            const double yhi = phase_hg(b[d], b[plane + d], b[2 * plane + d], c);
            o[d * od] = phase_lin(ylo, yhi, xlo, xhi, x);
        }
    } else if (p.imie == 1) {
        const int j = p.tlo[t];
        const double th = p.theta[t], tl = p.theta_tab[j], tu = p.theta_tab[j + 1];
        const double *a = p.tab + ((size_t)lo * p.NTAB + j) * ND, *b = a + (size_t)p.NTAB * ND;
        for (int d = 0; d < ND; ++d) {
            const double ylo = phase_lin(a[d], a[ND + d], tl, tu, th);
            const double yhi = phase_lin(b[d], b[ND + d], tl, tu, th);
            o[d * od] = phase_lin(ylo, yhi, xlo, xhi, x);
        }
    } else {
        const double c = p.ca[t];
        const double *a = p.tab + (size_t)lo * p.NTAB * ND, *b = a + (size_t)p.NTAB * ND;
        for (int d0 = 0; d0 < ND; d0 += kPhaseChunk) {          // one pass while NDUST <= kPhaseChunk
            double slo[kPhaseChunk], shi[kPhaseChunk];
#pragma unroll
            for (int k = 0; k < kPhaseChunk; ++k) { slo[k] = 0.0; shi[k] = 0.0; }
            double p0 = 1.0, p1 = c;                            // P_{l-2}, P_{l-1} from l = 2 on
            for (int l = 0; l < p.NTAB; ++l) {
                double pl;
                if (l == 0) pl = 1.0;
                else if (l == 1) pl = c;
                else {
                    pl = ((double)(2 * l - 1) * c * p1 - (double)(l - 1) * p0) / (double)l;       // legendre_p :2236
                    p0 = p1; p1 = pl;
                }
#pragma unroll
                for (int k = 0; k < kPhaseChunk; ++k)
                    if (d0 + k < ND) {
                        slo[k] = slo[k] + pl * a[(size_t)l * ND + d0 + k];
                        shi[k] = shi[k] + pl * b[(size_t)l * ND + d0 + k];
                    }
            }
#pragma unroll
            for (int k = 0; k < kPhaseChunk; ++k)
                if (d0 + k < ND) o[(d0 + k) * od] = phase_lin(slo[k], shi[k], xlo, xhi, x);
        }
    }
    if (SCAT) {
        for (int d = 0; d < ND; ++d) o[d * od + nth] = p.mu[t];
    } else if (p.ray) {
        const double c = phase_cos_deg(p.theta[t]);
        o[ND] = 0.75 * (1.0 + c * c) / (4.0 * 3.141592653589793);
    }
}

// calc_phase_ray (:852)
__global__ __launch_bounds__(kPhaseBlock) void k_phase_ray(int nth, const double *__restrict__ theta, double *__restrict__ out)
{
#pragma clang fp contract(off)
    const int t = blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nth) return;
    const double c = phase_cos_deg(theta[t]);
    out[t] = 0.75 * (1.0 + c * c) / (4.0 * 3.141592653589793);
}

}  // namespace ansfm

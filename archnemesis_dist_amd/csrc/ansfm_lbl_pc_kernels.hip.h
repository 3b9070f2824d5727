// ansfm_lbl_pc_kernels.hip.h -- pseudo-continuum of the weak lines (Irwin+19) of the runtime line-by-line opacity on gfx950.
//
// Restates LineData_0.add_pseudo_continuum_monochromatic_absorption (LineData_0.py:486-572) = the parameters of the bins
// (stimulated_emission :124 at t_ref, line_strength :206, doppler_width :144, lorentz_width :159; no pressure shift) and
// add_pseudo_continuum_monochromatic_spectrum (:361-483): every source bin in [first, last) spreads its strength over its
// 2 nb + 1 neighbours with the line shape at the bin centres, normalised by the sum of those shapes; the bins are divided by
// their widths and interpolated to the grid.
//
// The reference scatters twice (source bin -> neighbours, bin -> grid points).  Here every sum has one owner and the
// reference's order, so nothing needs a floating-point atomic and a repeat gives the same bits:
//   k_pc_params   one thread per (layer, bin)         strength, alpha_d, gamma_l
//   k_pc_shapes   one thread per (layer, source bin)  the 2 nb + 1 shapes in ascending k and their sum
//   k_pc_gather   one thread per (layer, target bin)  its sources in ascending i, then the division by the width
//   k_pc_interp   one thread per grid point, kPcLayers layers in registers: its bins in ascending i
// The three sums are evaluated without contraction into fma, as NumPy evaluates them: what is left to differ from the
// reference are exp, pow and the Voigt function (see ansfm_lbl_kernels.hip.h).
//
// The bin geometry does not depend on the layer: first, last, the largest touched grid point and the largest width are
// found once per call on the host with the reference's expressions (PcParams).  The lower edges c - w/2 are non-decreasing
// and the widths positive (the entry point refuses anything else): the bins that can touch a grid point wn then lie in
// lo^-1([wn - wmax, wn]), found by bisection and widened by a margin far above the rounding of the edges; inside it the
// reference's own test -0.5 <= (wn - c)/w < 0.5 decides.
#pragma once
#include "ansfm_lbl_kernels.hip.h"

namespace ansfm {

constexpr int kPcMaxNeighbours = 8;   // n_neighbour_bins 0 .. 8 (the reference's call sites pass 3)
constexpr int kPcLayers = 4;          // layers per thread of k_pc_interp: the bin tests are paid once per kPcLayers layers

struct PcParams {
    const double *wn_grid;                       // [nw] ascending
    const double *centers, *widths, *sw, *e_lower;  // [N]
    const double *lo;                            // [N] centers - widths / 2, non-decreasing
    const double *bparams;                       // [3M][N]
    const double *mmf;                           // [M], or [L][M] with mmf_stride = M
    const double *t_calc, *p_calc, *q_ratio;     // [L]
    double *store;                               // [L][3][N] strength, alpha_d, gamma_l
    double *y;                                   // [L][N][2 nb + 1] shapes of source bin i at its neighbours
    double *ysum;                                // [L][N] their sum in ascending k (0 for a bin that does not spread)
    double *x;                                   // [L][N] spread continuum per unit wavenumber
    double *out;                                 // [L][nw] (added to)
    int nw, N, M, L, lineshape_id, nb;
    int mmf_stride;                              // 0: one mmf[M] for all points
    int first, last;                             // source bins [first, last) spread (:399-416)
    int jmax;                                    // largest touched grid point: points below it receive (:476)
    double t_ref, p_ref, iso_abundance, iso_mass, wmax;
};

__global__ void k_pc_params(PcParams p)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.L * p.N) return;
    const int i = (int)(idx % p.N), l = (int)(idx / p.N);
    const double t_calc = p.t_calc[l];
    const LblTp c = lbl_tp(t_calc, p.t_ref, p.p_calc[l], p.p_ref);
    const double nu = p.centers[i];
    const double stim_ref = 1 - exp(-c.c2_cgs * nu / p.t_ref);                                  // :521
    double sh;
    double *st = p.store + (size_t)l * 3 * p.N + i;
    st[0] = lbl_strength(c, t_calc, p.q_ratio[l], nu, p.sw[i], p.e_lower[i], stim_ref);
    st[p.N] = lbl_doppler_width(c, t_calc, p.iso_mass, nu);
    st[2 * (size_t)p.N] = lbl_lorentz_width(c, p.bparams, p.mmf + (size_t)l * p.mmf_stride, p.M, p.N, i, &sh);
}

__global__ void k_pc_shapes(PcParams p)
{
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.L * p.N) return;
    const int i = (int)(idx % p.N), l = (int)(idx / p.N);
    double sum = 0.0;
    if (i >= p.first && i < p.last) {
        const double *st = p.store + (size_t)l * 3 * p.N + i;
        const double alpha_d = st[p.N], gamma_l = st[2 * (size_t)p.N], ci = p.centers[i];
        double *y = p.y + idx * (size_t)(2 * p.nb + 1);
        for (int k = 0; k <= 2 * p.nb; ++k) {                                                  // :422-434
            const int ii = i + k - p.nb;
            double v = 0.0;
            if (0 <= ii && ii < p.N) {
                v = lbl_lineshape(p.lineshape_id, p.centers[ii] - ci, alpha_d, gamma_l);
                sum += v;
            }
            y[k] = v;
        }
    }
    p.ysum[idx] = sum;
}

__global__ void k_pc_gather(PcParams p)
{
#pragma clang fp contract(off)
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)p.L * p.N) return;
    const int t = (int)(idx % p.N), l = (int)(idx / p.N);
    const size_t row = (size_t)l * p.N;
    const int ia = max(max(t - p.nb, p.first), 0), ib = min(min(t + p.nb, p.last - 1), p.N - 1);
    double x = 0.0;
    for (int i = ia; i <= ib; ++i) {                                                          // :436-441, by target
        const double s = p.ysum[row + i];
        if (s != 0) x += p.store[(size_t)l * 3 * p.N + i] * p.y[(row + i) * (size_t)(2 * p.nb + 1) + (t - i + p.nb)] / s;
    }
    p.x[idx] = x / p.widths[t];                                                               // :443
}

// Memory bound: per (layer, grid point) one read and one write of out and, from cache, the two or three bins around the
// point; the bisection and the divisions of the bin tests are shared by kPcLayers layers.
__global__ __launch_bounds__(256) void k_pc_interp(PcParams p)
{
#pragma clang fp contract(off)
    const int j = blockIdx.x * 256 + (int)threadIdx.x;
    if (j >= p.nw || j >= p.jmax) return;
    const int l0 = blockIdx.y * kPcLayers;
    const double wn = p.wn_grid[j];
    const double margin = 1e-9 * (fabs(wn) + p.wmax) + 1e-300;
    const double lo_wn = wn - p.wmax - margin, hi_wn = wn + margin;
    int a = 0, b = p.N;
    while (a < b) { int mid = (a + b) >> 1; if (p.lo[mid] < lo_wn) a = mid + 1; else b = mid; }
    const int ilo = a;
    b = p.N;
    while (a < b) { int mid = (a + b) >> 1; if (p.lo[mid] <= hi_wn) a = mid + 1; else b = mid; }
    const int ihi = a;
    double z0[kPcLayers];
#pragma unroll
    for (int k = 0; k < kPcLayers; ++k) z0[k] = 0.0;
    double z1 = 0.0;
    const double factor = p.iso_abundance;
    for (int i = ilo; i < ihi; ++i) {
        const double delta = (wn - p.centers[i]) / p.widths[i];                                // :453
        if (delta < -0.5 || delta >= 0.5) continue;
        const double n = 1.0 - fabs(delta);
        const int nbr = (delta < 0 && i > 0) ? i - 1 : (delta > 0 && i < p.N - 1) ? i + 1 : -1;
        const double fn = (1 - n) * factor, fc = n * factor;
#pragma unroll
        for (int k = 0; k < kPcLayers; ++k) {
            if (l0 + k < p.L) {
                const double *x = p.x + (size_t)(l0 + k) * p.N;
                if (nbr >= 0) z0[k] += fn * x[nbr];                                            // :467-470
                z0[k] += fc * x[i];                                                            // :471
            }
        }
        z1 += 1.0;
    }
    if (z1 == 0.0) return;
#pragma unroll
    for (int k = 0; k < kPcLayers; ++k)
        if (l0 + k < p.L) p.out[(size_t)(l0 + k) * p.nw + j] += z0[k] / z1;                   // :479
}

}  // namespace ansfm

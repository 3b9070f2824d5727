// ansfm_ms_optics_kernels.hip.h -- around the chains: the Fourier sum (k_ms_fourier) and the optics, layer-identity, row and
// g-quadrature kernels of CIRSrad's scattering branch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_ms_chain_steps.h"

namespace ansfm {

// ---- Fourier sum with the reference's convergence early-out :903-958 -----------------------------------------
__global__ void k_ms_fourier(MsParams p)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t total = (size_t)p.nwave * p.ng * p.ngeom;
    if (idx >= total) return;
    const int ipath = (int)(idx % p.ngeom);
    const int ig = (int)((idx / p.ngeom) % p.ng);
    const int widx = (int)(idx / ((size_t)p.ngeom * p.ng));
    const double *d = p.drad + (((size_t)widx * p.ng + ig) * (p.nf + 1)) * p.ngeom + ipath;
    double rad = 0.0;
    bool conv1 = false;
    for (int ic = 0; ic <= p.nf; ++ic)
        if (ms_fourier_step(d[(size_t)ic * p.ngeom], rad, conv1)) break;
    p.rad[((size_t)ipath * p.ng + ig) * p.nwave + widx] = rad;
}


// ---- scattering branch of CIRSrad on the device -----------------------------------------------------------------------
// calculate_layer_opacity (ForwardModel_0.py:3989) and the host preparation of scloud11wave (:5099-5119) for the arrays that
// have a g axis: TAUTOT = TAUGAS + TAUCIA + TAUDUST + TAURAY, OMEGA = (TAURAY + TAUSCAT) / TAUTOT where TAUTOT > 0, and
// BB = planck(TEMP) -- from the merge kernel's [rows][G][Wpad] gas opacities straight into the layouts the chain kernels
// read, so that TAUGAS / TAUTOT / OMEGA (NWAVE x NG x NLAY each) never leave HBM.
// For the models [m0, m0 + nm) of a batch on the wavenumbers [w0, w0 + wcount): the gas opacity of (model, layer) is row
// slot[model][layer] of the merge kernel's output (rows shared with model 0 where the layer inputs are identical), the outputs
// are laid out [model of the launch][wavenumber of the slab][..].  One model per call is the batch of one over the whole
// axis: slot = model_ids = nullptr, w0 = m0 = 0, wcount = W, nm = 1.
// The continuum is dense, [n][W][L], or (ROWS) handed over once per distinct layer (ansfm_cirsrad_ck_scatter_batch_rows): rows
// [R][W] of TAUCIA / TAUDUST / TAURAY / TAUSCAT and [R][ncont][W] of the aerosol fractions, wavenumber fastest, and cont_row
// [n][L], the row of layer l of model m.  The ROWS build also writes the slab's copies of TAURAY and the fractions the chain
// kernels read (MsParams::cont_local).

// planck_wave (ForwardModel_0.py:6214-6215): v a wavenumber (ispace = 0) or a wavelength in micron
__device__ __forceinline__ double ms_planck(int ispace, double v, double T)
{
    const double c1 = 1.1911e-12, c2 = 1.439;
    double y, a;
    if (ispace == 0) { y = v; a = c1 * (y * y * y); }
    else { y = 1.0e4 / v; a = c1 * (y * y * y * y * y) / 1.0e4; }
    return a / (exp(c2 * y / T) - 1.0);
}

// One thread per wavenumber of the slab, one block row per layer, one block plane per model of the launch.  Dense: a thread
// reads [m][W][L] at stride L.  ROWS: the row index is uniform per (model, layer), so a wavefront reads 64 consecutive doubles
// of every row.
template <bool ROWS> __global__ __launch_bounds__(128) void k_ms_optics(MsOpticsParams p)
{
    const int wl = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, ml = blockIdx.z;
    if (wl >= p.wcount) return;
    const int w = p.w0 + wl, m = p.model_ids ? p.model_ids[p.m0 + ml] : p.m0 + ml;
    const size_t ml_l = (size_t)m * p.L + l;
    const size_t cr = ROWS ? (size_t)p.cont_row[ml_l] : 0;
    const size_t in = ROWS ? cr * p.W + w : ((size_t)m * p.W + w) * p.L + l;
    const double cia = p.taucia ? p.taucia[in] : 0.0, dust = p.taudust ? p.taudust[in] : 0.0;
    const double ray = p.tauray ? p.tauray[in] : 0.0, sca = p.tauscat ? p.tauscat[in] : 0.0;
    const size_t row = p.slot ? (size_t)p.slot[ml_l] : (size_t)l;
    const size_t wrow = (size_t)ml * p.wcount + wl;
    for (int g = 0; g < p.G; ++g) {
        const double tt = ((p.taugas[(row * p.G + g) * p.Wpad + w] + cia) + dust) + ray;             // the sum order of :3989
        const size_t o = (wrow * p.G + g) * p.L + l;
        p.taus[o] = tt;
        p.omegas[o] = (tt > 0.0) ? (ray + sca) / tt : 0.0;
    }
    if constexpr (ROWS) {
        p.tauray_l[wrow * p.L + l] = ray;
        for (int c = 0; c < p.ncont; ++c) p.lfrac_l[(wrow * p.ncont + c) * p.L + l] = p.lfrac[(cr * p.ncont + c) * p.W + w];
    }
    p.bnu[wrow * p.L + l] = ms_planck(p.ispace, p.wave[w], p.lay_temp[ml_l]);
}

// same[m][l] = 1 when every input of layer l of model m is model 0's.  From the index maps: the gas-opacity row is shared
// (which covers pressure, temperature and the gas amounts) and, with cont_row, so is the continuum row -- no data is compared
// there: equal content under two indices counts as different (the layer is recomputed, with the bits of a separate call).
// cont_row = nullptr, the dense continuum: k_ms_same_cols compares its columns next.
__global__ void k_ms_same_index(int n_models, int L, const int32_t *__restrict__ slot, const int32_t *__restrict__ cont_row,
                                unsigned char *__restrict__ same)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n_models * L) same[i] = (slot[i] == i % L && (!cont_row || cont_row[i] == cont_row[i % L])) ? 1 : 0;
}
// arr [n][W][X][L] (X = 1 for the continuum opacities, ncont for the aerosol fractions).  One thread per (model, wavenumber, x);
// a differing element clears the layer's flag.
__global__ void k_ms_same_cols(int n_models, int W, int X, int L, const double *__restrict__ arr, unsigned char *__restrict__ same)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)W * X;
    if (i >= (size_t)(n_models - 1) * per) return;
    const size_t m = 1 + i / per, r = i % per;
    const double *a = arr + (m * per + r) * L, *b = arr + r * L;
    for (int l = 0; l < L; ++l)
        if (__double_as_longlong(a[l]) != __double_as_longlong(b[l])) same[m * L + l] = 0;
}

// Per-model phase functions (ansfm_set_phase_variants): a layer of model m stays model 0's only if none of the populations
// whose phase function differs between m's variant and variant 0 (diff [V][ncomp]) is present in it, i.e. its fraction is 0 at
// every wavenumber -- ms_phase_mix then adds fs pf(c) 0 = +-0 to the sum, which leaves every bit of a non-zero sum as it is as
// long as the phase matrices are finite.  Where the sum is itself an exact zero before the term (no Rayleigh term, or one that
// is +-0) the sign of the result could differ between variants; no test has shown it, and the rule would be narrowed if one
// did.  lfrac [n][W][ncont][L] or, with cont_row, the rows [R][ncont][W].  One thread per (model, wavenumber, population); a
// non-zero fraction (a NaN included) clears the layer's flag.
__global__ void k_ms_same_phase(int n_models, int W, int ncont, int L, const int *__restrict__ pvar, const unsigned char *__restrict__ diff,
                                const double *__restrict__ lfrac, const int32_t *__restrict__ cont_row, unsigned char *__restrict__ same)
{
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    const size_t per = (size_t)W * ncont;
    if (i >= (size_t)(n_models - 1) * per) return;
    const size_t m = 1 + i / per, w = (i % per) / ncont;
    const int c = (int)(i % ncont);
    if (!diff[(size_t)pvar[m] * (ncont + 1) + c]) return;
    for (int l = 0; l < L; ++l) {
        const double f = cont_row ? lfrac[((size_t)cont_row[m * L + l] * ncont + c) * W + w] : lfrac[((m * W + w) * ncont + c) * L + l];
        if (!(f == 0.0)) same[m * L + l] = 0;
    }
}

// The components of variants 1 .. V-1 that do not differ from variant 0's (Rayleigh always): their phase matrices and Hansen
// factors are variant 0's, bit for bit (the walk keeps one history per scatterer), copied here.  Every array of a variant is
// [..][ncomp][nn], so element idx of a variant belongs to component (idx / nn) % ncomp.  base: variant 0's ppl.
__global__ void k_ms_variant_fill(int V, int ncomp, int nn, size_t vstride, const unsigned char *__restrict__ diff, double *__restrict__ base)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= vstride) return;
    const int c = (int)((idx / nn) % ncomp);
    const double x = base[idx];
    for (int v = 1; v < V; ++v)
        if (!diff[(size_t)v * ncomp + c]) base[(size_t)v * vstride + idx] = x;
}

// One model's dense array from the rows, for the model-by-model route: dst [W][X][L] = rows [R][X][W] at cont_row[l] (X = 1:
// an opacity, ncont: the fractions).  One thread per (wavenumber, layer, x).
__global__ __launch_bounds__(128) void k_ms_rows_expand(int W, int X, int L, const int32_t *__restrict__ cont_row_m,
                                                       const double *__restrict__ rows, double *__restrict__ dst)
{
    const int w = blockIdx.x * blockDim.x + threadIdx.x, l = blockIdx.y, x = blockIdx.z;
    if (w >= W) return;
    dst[((size_t)w * X + x) * L + l] = rows[((size_t)cont_row_m[l] * X + x) * W + w];
}

// CIRSrad's g-quadrature of the scattering branch (:4504): SPECOUT[w][path] = xfac[w] * sum_g rad[path][g][w] * DELG[g];
// the radiances before the quadrature go out as well when wanted (spec_g[w][g][path], what scloud11wave returns).
__global__ void k_ms_gquad(const double *__restrict__ rad, const double *__restrict__ delg, const double *__restrict__ xfac,
                           double *__restrict__ specout, double *__restrict__ spec_g, int W, int G, int P)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)W * P) return;
    const int ip = (int)(idx % P), w = (int)(idx / P);
    const double xf = xfac ? xfac[w] : 1.0;
    double acc = 0.0;
    for (int g = 0; g < G; ++g) {
        const double r = rad[((size_t)ip * G + g) * W + w] * xf;
        if (spec_g) spec_g[((size_t)w * G + g) * P + ip] = r;
        acc += r * delg[g];
    }
    specout[idx] = acc;
}

}  // namespace ansfm

// ansfm_ms_params.h -- the parameter blocks and sizes the multiple-scattering kernels and their launchers share.  No HIP
// header: a plain C++17 compiler builds it (tests/host/ms_steps_main.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace ansfm {

constexpr int kMsMaxMu = 32;
constexpr int kMsMaxPath = 16;

struct MsParams {
    // reference-layout inputs (device pointers)
    const double *phasarr;   // [ncont][nwave][2][nth]
    const double *radg;      // [nwave][nmu]
    const double *solar;     // [nwave]
    const double *brdf;      // [nwave][nmu][nmu][nf+1]
    const double *bnu;       // [nwave][nlay]
    const double *taus;      // [nwave][ng][nlay]
    const double *tauray;    // [nwave][nlay]
    const double *omegas;    // [nwave][ng][nlay]
    const double *lfrac;     // [nwave][ncont][nlay]
    // workspaces / outputs
    double *ppl, *pmi;       // [nwin][nf+1][ncomp][nmu*nmu]    raw azimuth integrals   (wavenumbers pw0 .. pw0 + nwin - 1)
    double *fc;              // [ng][nwin][ncomp][nmu*nmu]      Hansen factors in the reference's loop order
    double *drad;            // [nwave][ng][nf+1][ngeom]
    double *rad;             // [ngeom][ng][nwave]
    int ncont, ncomp, nwave, nth, ngeom, lowbc, nmu, nf, ng, nlay, nphi, iray, imie;
    double mu[kMsMaxMu], wtmu[kMsMaxMu];          // already reversed (:725-726)
    double sol_ang[kMsMaxPath], emiss_ang[kMsMaxPath], aphi[kMsMaxPath];
    double xfac;
    int hansen_comp0, phase_comp0;
    int lookup;              // all emission angles > 90: layers top to bottom, surface brought in with idown (:366-420)
    int ig0, ng_launch;      // k_ms_hansen_seq / k_ms_chain16: the g-ordinates [ig0, ig0 + ng_launch) of this launch
    int phase_tab;           // k_ms_phase: the cos(ic phi) table fits in LDS (else the cosines are evaluated in place)
    int phase_lds;           // k_ms_chain16: the phase matrices of the components in use fit in LDS beside the operators
    // Batched Jacobian of the scattering branch (ansfm_cirsrad_ck_scatter_batch; k_ms_chain16<.., CACHE>).  A launch covers
    // the wavenumbers [w0, w0 + wcount) (0 / nwave outside the batch path); taus / omegas / bnu of such a launch are laid out
    // [model of the launch][wcount][..] relative to w0, every other per-wavenumber array keeps the whole axis.
    int w0, wcount;
    int m0, n_launch;        // CACHE = 2: models [m0, m0 + n_launch) of the batch, one block per (model, wavenumber, g)
    double *cache;           // [wcount][ng][nf+1][nlay][528]: doubled (r, t, j) of every scattering layer of model 0
    int *cache_orders;       // [wcount][ng]: Fourier orders model 0 worked through (those are in the cache)
    const unsigned char *same;   // [n_models][nlay]: the layer's inputs are bit-identical to model 0's
    double *pcache;          // [wcount][ng][nf+1][npre][528]: model 0's STACK (rc, tc, jc) after every kMsPrefixStep-th layer of the sweep
    const int *lstart;       // [n_models]: sweep index (multiple of kMsPrefixStep) a model's adding sweep may start from
    const int *model_ids;    // CACHE = 2: the models in launch order (sorted by lstart: the blocks of one launch then walk the same
                             // layers at about the same time and find model 0's cache lines in L2); model of block ml = ids[m0 + ml]
    int npre;
    size_t st_wl, st_wcl, st_wm, st_rad;   // strides between models: tauray [W][L], lfrac [W][ncont][L], radg [W][nmu], rad
    size_t st_drad;                        // ... and drad (k_ms_chain_lane<N, CACHE> leaves the orders to k_ms_fourier)
    // The continuum by rows (ansfm_cirsrad_ck_scatter_batch_rows): tauray / lfrac are the slab's copies k_ms_optics<true> wrote
    // beside taus / omegas / bnu, [model of the launch][wcount][..] relative to w0, st_wl / st_wcl the strides between launch
    // positions.  0: the batch's input arrays, by model over the whole axis.
    int cont_local;
    // 7 .. 15 streams on the 16-stream kernels: nmu = 16, nmu_real = the quadrature's size (0 = nmu).  mu / wtmu beyond it are
    // 1 / 0, the phase matrices, the surface operator and the boundary radiance zero there: every operator is block diagonal with
    // the quadrature's block in front and a block that couples to nothing behind it
    int nmu_real;
    // Spectral window (G = 1, ms_single): ppl / pmi / fc hold the wavenumbers [pw0, pw0 + nwin) only and every reader indexes
    // them relative to pw0 (pw0 = 0, nwin = nwave: the whole axis).  k_ms_hansen_seq continues from carry [ncomp][nmu*nmu] --
    // the factors of the last step of the previous window -- when carry_in is set, and leaves its own last factors there when
    // carry is set.
    int pw0, nwin, carry_in;
    double *carry;
    // Store range of the walk (ansfm_cirsrad_ck_scatter_batch_slice at G > 1): stn > 0 -- only the steps of the window's
    // wavenumbers [st0, st0 + stn) keep their factors, at fc[g][w - st0] (stride stn); the other steps run the same arithmetic
    // and store to sink [ncomp][nmu*nmu].  stn = 0: every step, stride nwin.
    int st0, stn;
    double *sink;
    // Per-model phase functions in the batch (ansfm_set_phase_variants; the layout is MsVariantPlan's, ansfm_ms_variants.h):
    // variant v's ppl / pmi / fc lie v * vstride doubles behind variant 0's.  pairs [..][2] = (variant, component): block y of
    // k_ms_phase / block x of k_ms_hansen_seq works on that pair instead of component y / x, npairs blocks (null: variant 0 alone);
    // phasarr_var [V - 1][ncont][nwave][2][nth], st_phas doubles apart: the phase functions of variants 1 .. V-1.
    // The chain kernels know nothing of variants: a launch of the cached chains covers models of ONE variant and gets that
    // variant's ppl / pmi / fc from the host (ms_run_slabs).
    const int *pairs;
    int npairs;
    const double *phasarr_var;
    size_t st_phas, vstride;
};

constexpr int kMsCacheEntry = 528;   // doubles per cached layer: r (256) and t (256) in the MFMA accumulator layout, j (16)
constexpr int kMsPrefixStep = 4;     // the stack below is kept after sweep layers 3, 7, 11, ...
constexpr int kMsHansenDepth = 8;    // steps the Hansen walk fetches its matrices ahead (k_ms_hansen_seq)

// Arguments of k_ms_optics (ansfm_ms_optics_kernels.hip.h, "scattering branch of CIRSrad on the device")
struct MsOpticsParams {
    const double *taugas;       // [rows][G][Wpad]
    const int32_t *slot;        // [n][L], or null: layer l reads row l
    const int32_t *cont_row;    // ROWS: [n][L]
    const double *taucia, *taudust, *tauray, *tauscat;   // [n][W][L], ROWS: [R][W]; or null
    const double *lfrac;        // ROWS: [R][ncont][W] (ncont > 0)
    const double *wave;         // [W]
    const double *lay_temp;     // [n][L]
    double *taus, *omegas;      // [nm][wcount][G][L]
    double *bnu;                // [nm][wcount][L]
    double *tauray_l;           // ROWS: [nm][wcount][L]
    double *lfrac_l;            // ROWS: [nm][wcount][ncont][L]
    const int *model_ids;       // launch position -> model (null: position m0 + ml is the model)
    int W, Wpad, G, L, ncont, ispace, w0, wcount, m0, nm;
};

}  // namespace ansfm

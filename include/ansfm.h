/*
 * ansfm.h -- C-ABI of libansfm.so: the MI355X (gfx950) forward-model engine for the
 * archNEMESIS radiative-transfer hot path.
 *
 * The reference (pure Python + numba) has no FFI; its seams are Python-level.
 * Every entry point below replaces one of those seams and cites it (paths relative to the
 * reference tree).  INTEGRATION.md shows the ctypes stub a maintainer adds on the reference side.
 *
 * Conventions
 *  - plain pointers + sizes, row-major (C order) float64 unless stated; int32 index arrays
 *  - enum-like ints carry the reference's IntEnum values (ISPACE: 0 wavenumber, 1 wavelength)
 *  - every function returns ANSFM_OK (0) or an error code; ansfm_last_error(ctx) gives the text
 *  - caller owns every array it passes; outputs are caller-allocated; the library never frees
 *    caller memory; device buffers (k-table, workspaces) are owned by the opaque ctx
 *  - one ctx per GPU; a ctx is not re-entrant, different ctx may be used from different threads
 *  - functions without suffix take HOST pointers (drop-in for the NumPy seams); `_dev` variants
 *    take DEVICE pointers (HBM-resident batches, what bench.py times) and run asynchronously on
 *    the ctx stream
 *  - there is NO CPU fallback: without a usable HIP device ansfm_create() fails
 */
#ifndef ANSFM_H
#define ANSFM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ANSFM_ABI_VERSION 1

#define ANSFM_OK 0
#define ANSFM_ERR_INVALID 1     /* bad argument / shape                                  */
#define ANSFM_ERR_HIP 2         /* HIP runtime error (text in ansfm_last_error)          */
#define ANSFM_ERR_NOTABLE 3     /* k-table not uploaded                                  */
#define ANSFM_ERR_UNSORTED 4    /* k-distribution not non-decreasing in g*/
#define ANSFM_ERR_UNSUPPORTED 5 /* valid in the reference, not built yet                 */

#define ANSFM_MAX_NG 32
/* ansfm_cirsradg_ck_thermal_cont(_dev): NVMR + 2, the gradient slots of calc_tau_cia a thread keeps in LDS (128 threads x 48 x 8
 * bytes = 48 KiB of a block at the cap; 8 KiB at NVMR = 6), may not exceed this, i.e. NVMR <= 46 */
#define ANSFM_MAX_CONT_GRAD_SLOTS 48

typedef struct ansfm_ctx ansfm_ctx;

int ansfm_abi_version(void);

/* Create / destroy the per-GPU context (device ordinal as in hipSetDevice). */
int ansfm_create(int device, ansfm_ctx **ctx);
void ansfm_destroy(ansfm_ctx *ctx);
const char *ansfm_last_error(const ansfm_ctx *ctx);

/* Use an external hipStream_t (e.g. torch's current stream) for all subsequent work; NULL
 * restores the ctx-owned stream. */
int ansfm_set_stream(ansfm_ctx *ctx, void *hip_stream);
int ansfm_synchronize(ansfm_ctx *ctx);

/* dtype semantics of the reference's NumPy arithmetic.  Spectroscopy_0.PRESS/TEMP ("grid") and DELG
 * are float32 arrays when the tables come from .kta files (read_ktahead, Spectroscopy_0.py:2544-2559);
 * NumPy (and numba) then evaluate np.log(PRESS[i]), phi-plo, thi-tlo, 1./(thi-tlo) (calc_k(g),
 * :2373-2389, :2236) and del_g[i]*del_g[j], np.cumsum(del_g) (k_overlap/rank, ForwardModel_0.py:6087,
 * :6142) in float32 -- a 4e-5 effect on tau.  Values are still passed as float64 (exactly the float32
 * values); these flags select the rounding.  Applies to every later call on this ctx. */
int ansfm_set_f32_semantics(ansfm_ctx *ctx, int grid_f32, int delg_f32);

/* ---- k-table ------------------------------------------------------------------------------
 * Replaces the state filled by Spectroscopy_0.read_tables (Spectroscopy_0.py:1448-1516):
 * K[W][G][NP][NT][S] (:213), PRESS[NP] (atm), TEMP[NT] (K), WAVE[W], DELG[G].
 * The table is re-laid out in HBM as ln k, [p][T][gas][g][wave] (wave fastest), float64.
 * `_dev`: K is a device pointer (same reference layout); the small vectors stay host pointers. */
int ansfm_upload_ktable(ansfm_ctx *ctx, int W, int G, int NP, int NT, int S, const double *K,
                        const double *PRESS, const double *TEMP, const double *WAVE,
                        const double *DELG);
int ansfm_upload_ktable_dev(ansfm_ctx *ctx, int W, int G, int NP, int NT, int S,
                            const double *K_dev, const double *PRESS, const double *TEMP,
                            const double *WAVE, const double *DELG);
/* dims = {W,G,NP,NT,S}; monotone = 1 when every k(g) column of the table is >=0 and
 * non-decreasing in g (precondition of the merge kernel's fast path). */
int ansfm_ktable_info(const ansfm_ctx *ctx, int64_t dims[5], int *monotone);
/* has_boxed = 1 when some entry of the table is <= 0 or NaN (such entries are stored NaN-boxed and every interpolation
 * tests for them); 0 for an all-positive table, whose forward merge reads it without those tests. */
int ansfm_ktable_has_boxed(const ansfm_ctx *ctx, int *has_boxed);
/* How the last forward merge (k_overlap, cirsrad_ck_thermal, ...) was launched: waves per block (1: one-wave blocks) and the
 * trims of the division-free fast path its kernel carried, as bits (1 weight product table, 2 two-instruction key repack,
 * 4 retired, never set, 8 list pass that ends at the insertion point, 16 per-lane choice of the row operand;
 * 0: the code without them, or another path of the merge). */
int ansfm_last_merge_launch(const ansfm_ctx *ctx, int *waves_per_block, int *trims);
/* Further bits of trims that are launch parameters, not code variants: 32 a wave's lanes are grouped over rows; 64 a wave whose
 * lanes' merges all sort row by row walks them without the head list (kernels with bit 1 only; ANSFM_MERGE_ROWMAJOR=0 clears it).
 * ansfm_last_merge_rowmajor: the (wave, merge) pairs of the last forward merge launch that took that walk, and all pairs that
 * merged; both 0 for a kernel without bit 1, which does not count.  Copies the two totals from the device (synchronises). */
int ansfm_last_merge_rowmajor(const ansfm_ctx *ctx, int64_t *merges, int64_t *merges_total);
/* A merge of such a launch that does not sort row by row from its first row may still do so from a row i0 on, above everything
 * in the rows below: the wave then runs the head list for the G * i0 elements of those rows and walks the rows i0 .. G-1
 * (at least two of them; results are the same bit for bit; ANSFM_MERGE_SUFFIX=0 at the call keeps the list to the end).
 * rows: the rows walked behind a list phase, summed over the (wave, merge) pairs of the last forward merge launch;
 * rows_of_list_merges: G times the pairs that ansfm_last_merge_rowmajor does not count as walked.  Both 0 for a kernel
 * without bit 1.  Copies the totals from the device (synchronises). */
int ansfm_last_merge_suffix(const ansfm_ctx *ctx, int64_t *rows, int64_t *rows_of_list_merges);
/* A merge that is walked whole meets the same weights in the same order in every lane, so where its bins close is known from
 * del_g alone: such a launch (float32 weights, G > 10) takes the crossings from a schedule formed once on the host and keeps the
 * closed bins on chip (results are the same bit for bit; ANSFM_MERGE_STATIC=0 at the call keeps the per-lane step).
 * merges: the (wave, merge) pairs of the last forward merge launch walked on the schedule, counted as ansfm_last_merge_rowmajor
 * counts; valid: 1 when the launch carried a valid schedule (0: del_g gave none, or a kernel that does not carry the form).
 * Copies the total from the device (synchronises). */
int ansfm_last_merge_static(const ansfm_ctx *ctx, int64_t *merges, int *valid);
/* The wavenumbers a wave of the last forward merge launch held with bit 32: 1 (64 rows of one wavenumber, the library's choice)
 * or 2 (2 wavenumbers x 32 rows, ANSFM_MERGE_LANES=pairs); 0 without bit 32 (64 wavenumbers of one row).  Reads the context only. */
int ansfm_last_merge_group_width(const ansfm_ctx *ctx, int *width);
/* The g-fastest copy of the k-table, ln k as [p][T][gas][wave][g] with g padded to an even count, that an upload builds from
 * the wave-fastest table (not with ANSFM_TABLE_GFAST=0 set at the upload, for G = 1 or an LBL table; a failed allocation
 * leaves the context without it and is no error): present = 1 and its size, or 0 and 0.  It takes the table's memory again. */
int ansfm_ktable_gfast(const ansfm_ctx *ctx, int *present, int64_t *bytes);
/* gfast = 1 when the last forward merge launch read the table from that copy (a launch with bit 32 on a context that holds
 * it; ANSFM_TABLE_LAYOUT=wave at the call keeps the wave-fastest reads), else 0.  Reads the context only. */
int ansfm_last_merge_table_layout(const ansfm_ctx *ctx, int *gfast);
/* The wavenumber order of the forward merge.  A launch with bits 1, 32 and 64 at group width 1 and G > 10 (a head list of 16
 * entries or more; shorter merges do not repay it) writes one byte per wavenumber,
 * the row-major verdicts of its first eight merges at the middle row, and hands the 64 wavenumbers of a block out sorted by
 * the bytes that the launch before wrote, so that a wave that holds the end of one wavenumber's rows and the start of the
 * next ones' mostly holds two of a kind (results do not depend on it, bit for bit).  The bytes are valid while the next such
 * launch has the same source (the same table upload, or the array-level seam), W, rows n_models * L, S and G; otherwise it
 * clears them and runs in wavenumber order.  ANSFM_MERGE_ORDER=0 at the call: wavenumber order, nothing written or kept.
 * applied = 1 when the last forward merge launch read valid bytes, and how many of them were not 0 (all 0: wavenumber order
 * still); 0 and 0 for every other launch.  Copies the count from the device (synchronises). */
int ansfm_last_merge_order(const ansfm_ctx *ctx, int *applied, int64_t *valid_bytes_nonzero);

/* ---- LBL tables (ILBL = LINE_BY_LINE_TABLES) ------------------------------------------------------
 * State of Spectroscopy_0 after read_tables on .lta / HDF5 LBL tables: K[W][NP][|NT|][S] (NG = 1),
 * PRESS[NP] (atm), TEMP[|NT|] or -- temp2d != 0, the reference's NT < 0 -- TEMP[NP][|NT|] (one
 * temperature grid per pressure, Spectroscopy_0.py:1664-1669).  After this upload the fused
 * cirsrad entry points run the ILBL=2 branch of calculate_gaseous_line_opacity (ForwardModel_0.py
 * :3795-3817: calc_klbl(g), tau = sum_gas k * amount) instead of the k-distribution merge. */
int ansfm_upload_lbltable(ansfm_ctx *ctx, int W, int NP, int NT, int S, const double *K,
                          const double *PRESS, const double *TEMP, int temp2d, const double *WAVE);
/* Spectroscopy_0.calc_klbl (:1768) / calc_klblg (:1601, when dkdT_out != NULL; note its missing
 * it<0 clamp is reproduced): press[L] atm, temp[L] K -> k_out[W][L][S] (, dkdT_out[W][L][S]). */
int ansfm_calc_klbl(ansfm_ctx *ctx, int L, const double *press, const double *temp, double *k_out,
                    double *dkdT_out);

/* ---- native .kta reader ------------------------------------------------------------------
 * Spectroscopy_0.read_ktahead (Spectroscopy_0.py:2492) / read_ktable (:2733) / read_tables (:1448) for binary
 * k-tables: header irec0, nwave, vmin, delv, fwhm, npress, ntemp, ng, gasID, isoID (vmin / delv rounded to 7 decimals
 * like the reference), g_ord, del_g, two pad floats, P, T, the wavenumber list when delv <= 0, then k * 1e20 as
 * float32 [wave][press][temp][g] from record irec0.
 * ansfm_ktable_file_header needs no GPU: dims = {nwave, ng, npress, ntemp}, ids = {gasID, isoID},
 * hdr = {vmin, delv, fwhm}; the array outputs may be NULL.
 * ansfm_upload_ktable_files reads S tables that share one grid, cuts the wavenumbers to [wavemin, wavemax] with
 * read_tables' searchsorted rule, and streams each file's float32 block to the GPU where it is divided by 1e20 in
 * float32 (as NumPy does) and re-laid out -- the float64 K (NWAVE,NG,NP,NT,NGAS) array of the reference is never
 * formed on the host.  Sets the float32 semantics of ansfm_set_f32_semantics (the file's grids are float32 arrays in
 * the reference).  ansfm_ktable_grids returns the host copies of WAVE / PRESS / TEMP / DELG of the table in HBM. */
int ansfm_ktable_file_header(const char *path, int64_t dims[4], int32_t ids[2], double hdr[3], double *wave,
                             float *g_ord, float *del_g, float *press, float *temp);
int ansfm_upload_ktable_files(ansfm_ctx *ctx, int S, const char *const *paths, double wavemin, double wavemax);
int ansfm_ktable_grids(const ansfm_ctx *ctx, double *WAVE, double *PRESS, double *TEMP, double *DELG);
/* The same for binary LBL tables: Spectroscopy_0.read_ltahead (:2451) / read_lbltable (:2626) -- header irec0, nwave,
 * vmin, delv, npress, ntemp, gasID, isoID, P, T, then k * 1e20 as float32 [wave][press][temp]; the reference unpacks
 * them with a Python loop over (wavenumber, pressure), minutes for a 10^6-point table.  dims = {nwave, npress, ntemp},
 * hdr = {vmin, delv}.  Tables with one temperature grid per pressure level (ntemp < 0) are not streamed
 * (ANSFM_ERR_INVALID; read them with the reference and use ansfm_upload_lbltable).  After the upload the context is in
 * the LBL-table state of ansfm_upload_lbltable; ansfm_ktable_grids returns WAVE / PRESS / TEMP (DELG = {1}). */
int ansfm_lbltable_file_header(const char *path, int64_t dims[3], int32_t ids[2], double hdr[2], double *wave,
                               float *press, float *temp);
int ansfm_upload_lbltable_files(ansfm_ctx *ctx, int S, const char *const *paths, double wavemin, double wavemax);

/* The k-table GENERATOR's numerical core, Spectroscopy_0.calc_ktable_chunk (Spectroscopy_0.py:3620-3652): from a
 * line-by-line spectrum kabs[ncalc] on the uniform grid wavecalc[ncalc], for each of nbin bins [vbinmin, vbinmax] the
 * points inside are sorted by k, weighted by the instrument function (np.interp of afil over dfil = VFIL - VCONV at the
 * distance from the bin centre wcen; nfil == NULL: weight 1), g = cumsum(w dv) / sum(w dv), and k is read at the
 * g-ordinates: kout[nbin][NG] = np.interp(g_ord, g_sorted, k_sorted).  dfil / afil are [nfilmax][nbin] with nfil[bin]
 * valid rows.  A bin without points is ANSFM_ERR_INVALID (np.interp raises there).  The sort is one segmented radix
 * sort over all bins (rocPRIM). */
int ansfm_kdist_bins(ansfm_ctx *ctx, int ncalc, const double *wavecalc, const double *kabs, int nbin,
                     const double *vbinmin, const double *vbinmax, const double *wcen, int nfilmax,
                     const int32_t *nfil, const double *dfil, const double *afil, int NG, const double *g_ord,
                     double *kout);

/* ---- array-level seams (host pointers), one per numba/NumPy kernel of the reference ------- */

/* Spectroscopy_0.calc_k (Spectroscopy_0.py:2298) / calc_kg (:2147), WAVECALC=None.
 * press[L] in atm, temp[L] in K -> k_out[W][G][L][S]; dkdT_out may be NULL (calc_k). */
int ansfm_calc_k(ansfm_ctx *ctx, int L, const double *press, const double *temp, double *k_out,
                 double *dkdT_out);

/* ForwardModel_0.k_overlap (ForwardModel_0.py:6029): del_g[G], k[W][G][L][S], amount[S][L]
 * -> tau[W][G][L].  Does not need an uploaded table. */
int ansfm_k_overlap(ansfm_ctx *ctx, int W, int G, int L, int S, const double *del_g,
                    const double *k, const double *amount, double *tau);

/* ForwardModel_0.calc_thermal_emission_spectrum (ForwardModel_0.py:6287).
 * TAUTOT_PATH[W][G][Li], EMITOT_PATH[W][Li] or NULL, TEMP[Li], PRESS[Li], EMISSIVITY/SOLFLUX/
 * REFLECTANCE[W] -> SPECOUT[W][G]. */
int ansfm_thermal_emission(ansfm_ctx *ctx, int ISPACE, int W, int G, int NLAYIN,
                           const double *WAVE, const double *TAUTOT_PATH,
                           const double *EMITOT_PATH, const double *TEMP, const double *PRESS,
                           double TSURF, const double *EMISSIVITY, const double *SOLFLUX,
                           const double *REFLECTANCE, double SOL_ANG, double EMISS_ANG,
                           double *SPECOUT);

/* ForwardModel_0.calc_thermal_emission_spectrumg (ForwardModel_0.py:6380-6504), array level: TAUTOT_PATH[W][G][Li],
 * dTAUTOT_PATH[W][G][NPAR][Li], NVMR = index of the temperature parameter, TEMP / PRESS[Li], EMISSIVITY[W] (needed
 * when TSURF > 0) -> SPECOUT[W][G], dSPECOUT[W][G][NPAR][Li], dTSURF[W][G].  The reference's O(NPAR Li^2) recursion is
 * evaluated as one backward sweep (the fused CIRSrad entry below does the same, with the g-quadrature folded in). */
int ansfm_thermal_emission_g(ansfm_ctx *ctx, int ISPACE, int W, int G, int NPAR, int NLAYIN, const double *WAVE,
                             const double *TAUTOT_PATH, const double *dTAUTOT_PATH, int NVMR, const double *TEMP,
                             const double *PRESS, double TSURF, const double *EMISSIVITY, double *SPECOUT,
                             double *dSPECOUT, double *dTSURF);

/* ForwardModel_0.calc_singlescatt_plane_spectrum (ForwardModel_0.py:6509-6600), array level: plane-parallel thermal
 * emission + singly scattered sunlight (ssfac * omega * phase * SOLFLUX / 4 pi per layer) + lower boundary (always added) +
 * sunlight reflected by the ground (BRDF).  TAUTOT_PATH / OMEGA[W][G][Li], PHASE[W][Li], TEMP[Li], EMISSIVITY / BRDF /
 * SOLFLUX[W] -> SPECOUT[W][G]. */
int ansfm_singlescatt_plane_spectrum(ansfm_ctx *ctx, int ISPACE, int W, int G, int NLAYIN, const double *WAVE,
                                     const double *TAUTOT_PATH, const double *TEMP, const double *OMEGA, const double *PHASE,
                                     double TSURF, const double *EMISSIVITY, const double *BRDF, const double *SOLFLUX,
                                     double SOL_ANG, double EMISS_ANG, double *SPECOUT);

/* CIRSrad, single-scattering branch (IMOD & SINGLE_SCATTERING_PLANE_PARALLEL; ForwardModel_0.py:4493 ->
 * calculate_single_scattering_plane_parallel_spectrum :4251-4336) fused with the opacity assembly: the albedo
 * OMEGA = (TAURAY + TAUSCAT) / TAUTOT of every (wavenumber, g, layer) is formed in the RT kernel from the vertical opacities.
 * Host pointers: taucont[W][L] = TAUCIA + TAUDUST + TAURAY, tausca[W][L] = TAURAY + TAUSCAT, phase[P][W][L] = the layer-mean
 * phase function at each path's scattering angle (:4318-4322), BRDF[W][P], SOLFLUX[W], angles [P] -> SPECOUT[W][P].
 * The uploaded table is a k-table (calc_k + k_overlap) or an LBL table (ILBL = LINE_BY_LINE_TABLES: calc_klbl, G = 1). */
int ansfm_cirsrad_ck_singlescatt(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, const double *tausca, const double *phase, int P,
                                 int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                 const double *EMTEMP, double TSURF, const double *EMISSIVITY, const double *BRDF,
                                 const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                 double *SPECOUT);

/* The same branch for the n_models states of a numerical Jacobian (jacobian_nemesis takes the numerical route whenever ISCAT is
 * not thermal emission, ForwardModel_0.py:2251-2252).  Arrays that depend on the state carry a leading model axis:
 * lay_press_pa / lay_temp [n][L], amount [n][S][L], taucont / tausca [n][W][L], phase [n][P][W][L], SCALE / EMTEMP
 * [n][LIMAX][P], TSURF [n]; the paths, EMISSIVITY, BRDF, SOLFLUX, the angles and xfac are shared -> SPECOUT [n][W][P].
 * Only the distinct (model, layer) gas opacities are computed (ansfm_set_layer_dedup, ansfm_last_layer_rows), and with at
 * least 4 states every state starts each path from the record state 0 left after the last layer whose opacity row, continuum,
 * scattering opacity, phase function of that path, SCALE and EMTEMP are all state 0's (ansfm_last_rt_shared).  The same
 * numbers as n_models calls of ansfm_cirsrad_ck_singlescatt, bit for bit, with and without the sharing.  n_models * P <= 65535. */
int ansfm_cirsrad_ck_singlescatt_batch(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, const double *taucont, const double *tausca,
                                       const double *phase, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *BRDF, const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG,
                                       const double *xfac, double *SPECOUT);
/* The same batch with taucont, tausca and phase formed inside the call, once per distinct layer, from the context's resident
 * sources (ansfm_upload_cia, ansfm_upload_dust, which keeps the scattering cross sections too) and the Rayleigh
 * parametrisations: nothing of size n W L exists on the host or crosses PCIe.  In their place the entry takes the continuum
 * block of ansfm_cirsrad_ck_thermal_cont_dev as host arrays (use_cia with lay_q [n][L][NVMR], lay_frac, lay_delh [n][L];
 * use_dust with lay_cont [n][L][ncont]; ray_mode 0 or IRAY 1, 2, 4, 12 with f4 [n][L][4] for mode 4; lay_totam [n][L] for CIA
 * and Rayleigh) and phase_fn [W][P][ncont + 1]: the phase function of every population and, last, of Rayleigh scattering at
 * the scattering angle of each path (ScatterX.calc_phase / calc_phase_ray, ForwardModel_0.py:4269-4271 before the transpose).
 * Per distinct row (k_ss_cont_rows), every term rounded as ansfm_calc_tau_cia / ansfm_calc_tau_dust / ansfm_calc_tau_rayleigh
 * round it: taucont = (TAUCIA + TAUDUST) + TAURAY with TAUDUST = sum_d clip(nan_to_num(e_d), 0, 1e20); tausca = TAURAY +
 * TAUSCAT with TAUSCAT = sum_d s_d (raw), s_d = (ksca 1e-4) CONT; phase of path ip = num / (TAURAY + TAUSCAT) where num > 0,
 * else num, num = sum_d phase_fn[w][ip][d] s_d + phase_fn[w][ip][ncont] TAURAY, added in that order (:4316-4321); a term that
 * is not used is the reference's zeros.  The result is bit-identical to ansfm_cirsrad_ck_singlescatt_batch on dense arrays
 * formed that way, with and without ansfm_set_layer_dedup.  One row map serves gas opacities and continuum: a layer is
 * distinct when it differs from state 0's in pressure, temperature, an amount or a column an opacity is formed from (lay_totam;
 * f4; lay_q, lay_delh and, for a CIA table with a para-H2 axis, lay_frac; lay_cont), and with at least 4 states a layer counts
 * as state 0's exactly when its row is state 0's row of that layer -- no array is compared.  ANSFM_ERR_INVALID, before anything
 * is launched: a source that is used has not been uploaded since the last table, the CIA source was uploaded for the other
 * ISPACE, ncont is not the number of populations uploaded (0 without use_dust), neither use_dust nor ray_mode (no scattering
 * opacity), an array of a used term or phase_fn is NULL, NLAYIN outside 1 .. LIMAX or a LAYINC entry outside 0 .. L - 1, and for
 * the dense entry's reasons.  ANSFM_ERR_UNSUPPORTED: more than 7 populations, n_models * P > 65535.  ansfm_last_layer_rows and
 * ansfm_last_rt_shared report as for the dense entry. */
int ansfm_cirsrad_ck_singlescatt_batch_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                            const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                            const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                            const double *lay_cont, int ray_mode, const double *f4, int ncont, const double *phase_fn,
                                            int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                            const double *EMTEMP, const double *TSURF, const double *EMISSIVITY, const double *BRDF,
                                            const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                            double *SPECOUT);
/* The same with phase_fn formed on the device (phase_fn [W][P][ncont + 1] is the one per-wavenumber input the entry above still
 * takes from the host): in its place alpha_deg [P], the scattering angle of each path in degrees, arccos(calpha) / pi * 180 by
 * the expression of ForwardModel_0.py:4265-4270.  phase_fn[w][ip][0 .. ncont) is the resident phase-function source
 * (ansfm_upload_phase) at alpha_deg, [ncont] is calc_phase_ray; k_phase_fn writes both into the buffer k_ss_cont_rows reads.
 * Bit-identical to the entry above called with phase_fn put together from ansfm_phase_from_source and ansfm_calc_phase_ray at
 * the same angles, with and without ansfm_set_layer_dedup.  ANSFM_ERR_INVALID, before anything is launched, also when no
 * phase-function source has been uploaded since the last table, when its NDUST is not ncont, or (IMIE 1) for an angle outside
 * the tabulated ones. */
int ansfm_cirsrad_ck_singlescatt_batch_src(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                           const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                           const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                           const double *lay_cont, int ray_mode, const double *f4, int ncont, const double *alpha_deg,
                                           int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                                           const double *EMTEMP, const double *TSURF, const double *EMISSIVITY, const double *BRDF,
                                           const double *SOLFLUX, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                           double *SPECOUT);

/* ---- fused seam: CIRSrad, ILBL=K_TABLES, IMOD=THERMAL_EMISSION ------------------------------
 * ForwardModel_0.CIRSrad (ForwardModel_0.py:4376-4511) =
 *   calculate_gaseous_line_opacity (:3850-3877: calc_k -> k_overlap)
 *   -> calculate_layer_opacity (:3989 TAUTOT = TAUGAS+TAUCIA+TAUDUST+TAURAY; :4006 LAYINC*SCALE)
 *   -> calculate_thermal_emission_spectrum (:4216-4244) -> g-quadrature (:4504)
 * for a BATCH of n_models atmospheres sharing the uploaded k-table and the path structure
 * (the fan-out of jacobian_nemesis, ForwardModel_0.py:2305-2337).
 *
 *   lay_press_pa[n][L]   LayerX.PRESS (Pa; divided by 101325 internally, :3855)
 *   lay_temp[n][L]       LayerX.TEMP
 *   amount[n][S][L]      f_gas = LayerX.AMOUNT[:,IGAS]*1e-4 (cm-2, :3861)
 *   taucont[n][W][L]     TAUCIA+TAUDUST+TAURAY (vertical), or NULL (=0)
 *   NLAYIN[P], LAYINC[LIMAX][P] (int32), SCALE[n][LIMAX][P], EMTEMP[n][LIMAX][P]   PathX (:4006,:4218)
 *   TSURF[n]; EMISSIVITY/SOLFLUX/REFLECTANCE/xfac [W] or NULL (0,0,0,1); SOL_ANG/EMISS_ANG [P]
 *   SPECOUT[n][W][P]
 * n_models strides are contiguous.  Host-pointer version copies in/out; `_dev` takes device
 * pointers for every array (int32 arrays too) and is asynchronous on the ctx stream. */
int ansfm_cirsrad_ck_thermal(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                             const double *lay_press_pa, const double *lay_temp,
                             const double *amount, const double *taucont, int P, int LIMAX,
                             const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                             const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                             const double *SOLFLUX, const double *REFLECTANCE,
                             const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                             double *SPECOUT);
int ansfm_cirsrad_ck_thermal_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                                 const double *lay_press_pa, const double *lay_temp,
                                 const double *amount, const double *taucont, int P, int LIMAX,
                                 const int32_t *NLAYIN, const int32_t *LAYINC,
                                 const double *SCALE, const double *EMTEMP, const double *TSURF,
                                 const double *EMISSIVITY, const double *SOLFLUX,
                                 const double *REFLECTANCE, const double *SOL_ANG,
                                 const double *EMISS_ANG, const double *xfac, double *SPECOUT);

/* The same for a batch whose only continuum is Rayleigh scattering (calc_tau_rayleigh, ForwardModel_0.py:4869; ray_mode =
 * IRAY 1, 2, 4, or 12 for calc_tau_rayleighv): TAURAY = k(wavenumber[, composition]) * TOTAM is formed inside the call from
 * the DEVICE arrays TOTAM[n][L] (m-2) and, ray_mode 4, f4[n][L][4] (mixing ratios of H2, He, CH4, NH3) -- once per DISTINCT
 * layer of the batch (TOTAM and f4 are part of a layer's identity next to pressure, temperature and amounts) and straight in
 * the layout the RT kernel reads.  The n * NWAVE * L array ansfm_calc_tau_rayleigh_batch_dev would fill (1.6 GB for the 201
 * states of BASELINE configs[2]) is neither written, transposed nor compared.  Same bits as the two-call route. */
int ansfm_cirsrad_ck_thermal_ray_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                     const double *lay_temp, const double *amount, int ray_mode, const double *TOTAM,
                                     const double *f4, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                     const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                     const double *SOLFLUX, const double *REFLECTANCE, const double *SOL_ANG,
                                     const double *EMISS_ANG, const double *xfac, double *SPECOUT);

/* The same for a batch whose continuum is collision-induced absorption, aerosol extinction and Rayleigh scattering, any of
 * the three: cont = (TAUCIA + TAUDUST) + TAURAY (calculate_layer_opacity :3989; an absent term is left out, not added as
 * zero) is formed inside the call from the context's resident sources (ansfm_upload_cia, ansfm_upload_dust) -- once per
 * DISTINCT layer of the batch and straight in the layout the RT kernel reads.  DEVICE arrays: use_cia: lay_q[n][L][NVMR] =
 * PP / PRESS (NVMR as uploaded), lay_frac[n][L] (para-H2 fraction), lay_totam[n][L] (m-2), lay_delh[n][L] (km); use_dust:
 * lay_cont[n][L][NDUST] (particles m-2 after any DUST_RENORMALISATION, NDUST as uploaded); ray_mode 0 or as in
 * ansfm_cirsrad_ck_thermal_ray_dev, from lay_totam and f4[n][L][4].  All of them are part of a layer's identity: a state that
 * perturbs He changes no spectroscopic amount, yet it changes CIA.  Same bits as ansfm_calc_tau_cia + ansfm_calc_tau_dust
 * (nan_to_num, clip to [0, 1e20], summed over the populations in order) + ansfm_calc_tau_rayleigh_batch_dev over all n * L
 * layers, summed in that order and passed as taucont.  ANSFM_ERR_INVALID when a source that is used has not been uploaded
 * since the last table, or the CIA source was uploaded for the other ISPACE. */
int ansfm_cirsrad_ck_thermal_cont_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                      const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                      const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                      const double *lay_cont, int ray_mode, const double *f4, int P, int LIMAX,
                                      const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP,
                                      const double *TSURF, const double *EMISSIVITY, const double *SOLFLUX,
                                      const double *REFLECTANCE, const double *SOL_ANG, const double *EMISS_ANG, const double *xfac,
                                      double *SPECOUT);

/* CIRSrad, pure-transmission branch (IMOD without ABSORBTION / THERMAL_EMISSION / scattering flags; ForwardModel_0.py:
 * 4478-4481 -> calculate_transmission_spectrum :4110-4131): SPECOUT[n][W][P] = xfac[W] * sum_g DELG[g] exp(-sum_layers
 * TAUTOT_LAYINC) -- the same opacity assembly as the thermal branch, the RT kernel's epilogue switched.  xfac = the
 * solar flux when IFORM = Atmospheric_transmission, else NULL.  (The reference's absorption branch,
 * calculate_absorption_spectrum :4133, is declared without `self` and cannot be called; it has no counterpart.) */
int ansfm_cirsrad_ck_transmission(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa, const double *lay_temp,
                                  const double *amount, const double *taucont, int P, int LIMAX, const int32_t *NLAYIN,
                                  const int32_t *LAYINC, const double *SCALE, const double *xfac, double *SPECOUT);

/* The same branch with return_grad (calculate_transmission_spectrum :4128-4131 followed by CIRSrad's g-quadrature and
 * nan_to_num :4507): dSPECOUT[n][W][NPAR][LIMAX][P] = - sum_g DELG[g] xfac exp(-tau_path(g)) dTAUTOT_LAYINC[g], with
 * dTAUTOT_LAYINC assembled as in ansfm_cirsradg_ck_thermal (gas slots x 1e-4 through igas_map, temperature slot at NVMR,
 * dtaucon, x SCALE).  dTSURF of this branch is identically zero and not returned. */
int ansfm_cirsradg_ck_transmission(ansfm_ctx *ctx, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, const double *taucont,
                                   const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                                   const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *xfac,
                                   double *SPECOUT, double *dSPECOUT);

/* Primary-transit depth with analytic gradients of ONE model (nemesisPTfm, ForwardModel_0.py:1838-1995), collapsed over the
 * paths on the device instead of through dSPECOUT (W, NPAR, LIMAX, P).  All pointers are host pointers.  With
 * Sm[l][p] = sum of SCALE[j][p] over j < NLAYIN[p] with LAYINC[j][p] = l (padding beyond NLAYIN[p] is never read) and the annulus
 * weights path_weight[P] = c_p of the trapezoid of :1949-1954:
 *   tau_path[w][g][p] = sum_l Sm[l][p] (TAUGAS[w][g][l] + taucont[w][l])      TRANS[w][p] = sum_g DELG[g] exp(-tau_path)
 *   AREA[w] = sum_p c_p (1 - TRANS[w][p])
 *   dAREA[w][k][l] = sum_g DELG[g] (sum_p c_p exp(-tau_path) Sm[l][p]) dTAUTOT[w][g][k][l]
 * with dTAUTOT assembled as in ansfm_cirsradg_ck_thermal before its x SCALE (gas slots x 1e-4 through igas_map, temperature slot
 * at NVMR, dtaucon, a pending ansfm_set_shared_gas_gradient, ansfm_set_gradient_gases honoured).  nan_to_num (:4507) acts on
 * each dAREA element (the reference applies it per path entry; the two agree whenever its dSPECOUT is finite).
 * TRANS[W][P] and dAREA[W][NPAR][L] may be NULL; dAREA always stays on the device as a (W, NPAR, L, 1) result for
 * ansfm_map2pro(dSPECIN = NULL) with LAYINC = 0 .. L - 1.  Device scratch beyond the gas stage is 8 (L + P) G Wpad bytes plus
 * the outputs; ANSFM_ERR_UNSUPPORTED above 320 layers or 320 paths (a 64-lane LDS tile with one row per layer or path, 160 KiB).
 * ANSFM_ERR_INVALID for NLAYIN[p] > LIMAX or a LAYINC[j][p], j < NLAYIN[p], outside 0 .. L - 1.
 * ansfm_transit_last: info[0] the bytes of that scratch in the last call, info[1] / info[2] the milliseconds of k_transit_sens /
 * k_transit_grad. */
int ansfm_cirsradg_ck_transit(ansfm_ctx *ctx, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                              const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P,
                              int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                              const double *path_weight, double *AREA, double *TRANS, double *dAREA);
int ansfm_transit_last(const ansfm_ctx *ctx, double info[3]);

/* Solar occultation with analytic gradients of ONE model (nemesisSOfmg, ForwardModel_0.py:983-1249): the limb paths are mixed to
 * the Q geometries of the measurement on the device -- the interpolation to the tangent heights (:1208-1232) as a sparse matrix
 * C (Q, P), rows mix_ptr[q] .. mix_ptr[q + 1] of (mix_path, mix_val) -- instead of through dSPECOUT (W, NPAR, LIMAX, P).  All
 * pointers are host pointers.  With Sm and tau_path as for ansfm_cirsradg_ck_transit and xfac[W] the solar flux of :4119-4127
 * (NULL: 1):
 *   TRANS[w][p] = sum_g DELG[g] exp(-tau_path[w][g][p])          MOD[w][q] = xfac[w] sum_p C[q][p] TRANS[w][p]
 *   dMOD[w][k][l][q] = - xfac[w] sum_g DELG[g] (sum_p C[q][p] Sm[l][p] exp(-tau_path[w][g][p])) dTAUTOT[w][g][k][l]
 * with dTAUTOT assembled as in ansfm_cirsradg_ck_thermal before its x SCALE (gas slots x 1e-4 through igas_map, temperature slot
 * at NVMR, dtaucon, a pending ansfm_set_shared_gas_gradient, ansfm_set_gradient_gases honoured).  dMOD has the layout of the
 * reference's dSPECOUT with LIMAX -> L and NPATH -> Q; nan_to_num (:4507) acts on each dMOD element (the reference applies it per
 * path entry; the two agree whenever its dSPECOUT is finite).  A geometry with an empty row gives zeros.  TRANS[W][P] and
 * dMOD[W][NPAR][L][Q] may be NULL; dMOD always stays on the device as a (W, NPAR, L, Q) result for ansfm_map2pro(dSPECIN = NULL)
 * with NLAYIN = L and LAYINC = 0 .. L - 1 for every geometry.  dMOD is held as a whole, 8 W NPAR L Q bytes (the spectral axis is
 * not slabbed): ANSFM_ERR_UNSUPPORTED when that cannot be reserved, so that the caller can take the un-collapsed route.  Device
 * scratch beyond the gas stage and dMOD is 8 P G Wpad bytes plus MOD and TRANS.  ANSFM_ERR_UNSUPPORTED above 320 layers or 320
 * paths (a 64-lane LDS tile with one row per layer, 160 KiB).  ANSFM_ERR_INVALID for NLAYIN[p] > LIMAX, a LAYINC[j][p],
 * j < NLAYIN[p], outside 0 .. L - 1, a mix_ptr that does not start at 0 or decreases, a mix_path outside 0 .. P - 1.
 * ansfm_occultation_last: info[0] the bytes of that scratch in the last call, info[1] / info[2] the milliseconds of k_occ_paths /
 * k_occ_grad. */
int ansfm_cirsradg_ck_occultation(ansfm_ctx *ctx, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                                  const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P,
                                  int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, int Q,
                                  const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val, const double *xfac,
                                  double *MOD, double *TRANS, double *dMOD);
int ansfm_occultation_last(const ansfm_ctx *ctx, double info[3]);

/* Limb thermal emission with analytic gradients of ONE model (nemesisLfmg, ForwardModel_0.py:1372-1521): the limb paths are mixed
 * to the Q geometries of the measurement on the device -- the interpolation to the tangent heights (:1475-1496) as a sparse matrix
 * C (Q, P), rows mix_ptr[q] .. mix_ptr[q + 1] of (mix_path, mix_val) -- instead of through dSPECOUT (W, NPAR, LIMAX, P).  All
 * pointers are host pointers.  Path p has the entries j < NLAYIN[p] (padding beyond is never read) with l_j = LAYINC[j][p],
 * s_j = SCALE[j][p], B and dB/dT the Planck function of :6274-6281 at EMTEMP[j][p] in the units of ISPACE (0 wavenumber, 1
 * wavelength), xfac[W] the factor of :4158-4168 (NULL: 1):
 *   tau_j[w][g] = s_j (TAUGAS[w][g][l_j] + taucont[w][l_j])      T_-1 = 1, T_j = T_{j-1} exp(-tau_j)
 *   spec[w][g][p] = sum_j (T_{j-1} - T_j) B_j                     SPEC[w][p] = sum_g DELG[g] spec[w][g][p]
 *   MOD[w][q] = xfac[w] sum_p C[q][p] SPEC[w][p]
 *   A_j = T_j B_j - sum_{m > j} (T_{m-1} - T_m) B_m               E[w][g][l][q] = sum_p C[q][p] sum_{j: l_j = l} s_j A_j
 *   Z[w][l][q] = sum_g DELG[g] sum_p C[q][p] sum_{j: l_j = l} (T_{j-1} - T_j) dB/dT_j
 *   dMOD[w][k][l][q] = xfac[w] (sum_g DELG[g] E[w][g][l][q] dTAUTOT[w][g][k][l] + [k == NVMR] Z[w][l][q])
 * with dTAUTOT assembled as in ansfm_cirsradg_ck_thermal before its x SCALE (gas slots x 1e-4 through igas_map, temperature slot
 * at NVMR, dtaucon, a pending ansfm_set_shared_gas_gradient, ansfm_set_gradient_gases honoured).  dMOD has the layout of the
 * reference's dSPECOUT with LIMAX -> L and NPATH -> Q; nan_to_num (:4507) acts on each dMOD element (the reference applies it per
 * path entry; the two agree whenever its dSPECOUT is finite).  A geometry with an empty row gives zeros.  SPEC[W][P] and
 * dMOD[W][NPAR][L][Q] may be NULL; dMOD always stays on the device as a (W, NPAR, L, Q) result for ansfm_map2pro(dSPECIN = NULL)
 * with NLAYIN = L and LAYINC = 0 .. L - 1 for every geometry.  Limb paths only: a path whose last layer lies at a higher pressure
 * than its middle one (the lower boundary would contribute, :6479-6496) is ANSFM_ERR_UNSUPPORTED, so that the caller can take the
 * un-collapsed route; so are more than 160 layers (two 64-lane LDS rows per layer, 160 KiB) and a dMOD (8 W NPAR L Q bytes, held
 * as a whole) or a scratch that cannot be reserved.  Device scratch beyond the gas stage and dMOD is 8 Wpad (Q L (G + min(G, 4)) +
 * P G + 2 NT) bytes, NT the number of bit-distinct EMTEMP values, plus MOD and SPEC.  That is less than the 8 W NPAR LIMAX P bytes of
 * the dSPECOUT the call replaces where NPAR LIMAX P W exceeds (G + 4) Q L Wpad or so (W 1024, G 20, L 100, P 20, LIMAX 200,
 * NPAR 10, Q 10: 202 MB against 328 MB); it is not for a handful of wavenumbers (Wpad pads W to a multiple of 64) or few parameters,
 * and the entry does not refuse such shapes.  ANSFM_ERR_INVALID for NLAYIN[p] > LIMAX, a
 * LAYINC[j][p], j < NLAYIN[p], outside 0 .. L - 1, a mix_ptr that does not start at 0 or decreases, a mix_path outside
 * 0 .. P - 1.  ansfm_limb_last: info[0] the bytes of that scratch in the last call, info[1] / info[2] the milliseconds of
 * k_limb_planck with k_limb_sens / of k_limb_grad. */
int ansfm_cirsradg_ck_limb(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                           const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                           const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE, const double *EMTEMP, int Q,
                           const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val, const double *xfac, double *MOD,
                           double *SPEC, double *dMOD);
int ansfm_limb_last(const ansfm_ctx *ctx, double info[3]);

/* Disc-averaged thermal emission with analytic gradients of ONE model (nemesisdiscfmg, ForwardModel_0.py:1719-1834): the P
 * averaging points of an unresolved planet are mixed to Q geometries on the device -- the weighted sum with WGEOM (:1789-1794) as
 * a sparse matrix C (Q, P), rows mix_ptr[q] .. mix_ptr[q + 1] of (mix_path, mix_val) -- instead of through one dSPECOUT
 * (W, NPAR, NLAYIN, 1) per point.  All pointers are host pointers.  The points are paths through ONE layer sequence of N entries j
 * with l_j = LAYINC[j] and B, dB/dT the Planck function of :6274-6281 at EMTEMP[j] in the units of ISPACE; they differ in
 * s_jp = SCALE[j][p] only.  Unlike ansfm_cirsradg_ck_limb the sequence may end at the lower boundary (:6479-6498):
 *   tau_jp[w][g] = s_jp (TAUGAS[w][g][l_j] + taucont[w][l_j])     T_-1,p = 1, T_jp = T_{j-1,p} exp(-tau_jp)
 *   ground = lay_press_pa[l_{N-1}] > lay_press_pa[l_{int(N/2)-1}]   (index -1 is N - 1)
 *   R, dR = TSURF <= 0 ? B, dB/dT at EMTEMP[N-1] : EMISSIVITY[w] x (B, dB/dT at TSURF)
 *   spec[w][g][p] = sum_j (T_{j-1,p} - T_jp) B_j + [ground] T_{N-1,p} R       SPEC[w][p] = sum_g DELG[g] spec[w][g][p]
 *   MOD[w][q] = xfac[w] sum_p C[q][p] SPEC[w][p]
 *   dTSMOD[w][q] = xfac[w] sum_g DELG[g] sum_p C[q][p] [ground] T_{N-1,p} dR
 *   A_jp = T_jp B_j - sum_{m > j} (T_{m-1,p} - T_mp) B_m - [ground] T_{N-1,p} R
 *   E[w][g][l][q] = sum_p C[q][p] sum_{j: l_j = l} s_jp A_jp
 *   Z[w][l][q] = sum_g DELG[g] sum_p C[q][p] sum_{j: l_j = l} (T_{j-1,p} - T_jp) dB/dT_j
 *   dMOD[w][k][l][q] = xfac[w] (sum_g DELG[g] E[w][g][l][q] dTAUTOT[w][g][k][l] + [k == NVMR] Z[w][l][q])
 * with dTAUTOT, nan_to_num, the layout of dMOD and its stay on the device for ansfm_map2pro(dSPECIN = NULL) as for
 * ansfm_cirsradg_ck_limb.  As in the reference, dTSMOD with TSURF <= 0 is still T_end dB/dT at EMTEMP[N-1], and the bottom
 * layer's temperature column of dMOD gets no dR term.  SPEC[W][P], dTSMOD[W][Q] and dMOD[W][NPAR][L][Q] may be NULL; EMISSIVITY[W]
 * may be NULL where TSURF <= 0.  ANSFM_ERR_UNSUPPORTED above 160 layers (two 64-lane LDS rows per layer, 160 KiB) and for a dMOD
 * (8 W NPAR L Q bytes, held as a whole) or a scratch that cannot be reserved.  Device scratch beyond the gas stage and dMOD is
 *   8 Wpad (Q L (G + GS) + (P + Q) G + 2 (NT + 1)) + 8 W (2 Q + P) bytes,
 *   GS = min(G, max(4, ceil(256 / ((Wpad / 64) (Q + u))))),  u = 1 if some path is named by no geometry, else 0,
 * NT the number of bit-distinct EMTEMP values and GS the groups of g-ordinates the sensitivity kernel puts on its grid.
 * ANSFM_ERR_INVALID for N, P or Q <= 0, a LAYINC[j] outside 0 .. L - 1, TSURF > 0 with EMISSIVITY == NULL, a mix_ptr that does not
 * start at 0 or decreases, a mix_path outside 0 .. P - 1.  ansfm_disc_last: info[0] the bytes of that scratch in the last call,
 * info[1] / info[2] the milliseconds of k_disc_planck with k_disc_sens / of k_disc_grad. */
int ansfm_cirsradg_ck_disc(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp, const double *amount,
                           const double *taucont, const double *dtaucon, int NVMR, int NPAR, const int32_t *igas_map, int N,
                           const int32_t *LAYINC, const double *EMTEMP, int P, const double *SCALE, double TSURF,
                           const double *EMISSIVITY, int Q, const int32_t *mix_ptr, const int32_t *mix_path, const double *mix_val,
                           const double *xfac, double *MOD, double *SPEC, double *dTSMOD, double *dMOD);
int ansfm_disc_last(const ansfm_ctx *ctx, double info[3]);

/* ---- analytic-gradient seams ---------------------------------------------------------------
 * ForwardModel_0.k_overlapg (ForwardModel_0.py:5842): + dkdT[W][G][L][S] -> tau[W][G][L],
 * dk[W][G][L][S+1] (slots 0..S-1 = d tau/d amount_gas, slot S = d tau/dT). */
int ansfm_k_overlapg(ansfm_ctx *ctx, int W, int G, int L, int S, const double *del_g,
                     const double *k, const double *dkdT, const double *amount, double *tau,
                     double *dk);

/* A continuum gradient that is the same for every gas parameter: dTAU_WL[W][L] (host) is added to dTAUCON[:, v, :] of all
 * v < NVMR in the NEXT ansfm_cirsradg_ck_thermal call of one model (then forgotten) -- what calculate_layer_opacity does with
 * dTAURAY (ForwardModel_0.py:3955-3957), without NVMR copies of the array crossing PCIe inside `dtaucon`.  NULL cancels. */
int ansfm_set_shared_gas_gradient(ansfm_ctx *ctx, int L, const double *dTAU_WL);

/* Which spectroscopic gases' amount gradients the k-table gradient path (ansfm_cirsradg_ck_*) computes: bit s of `mask` for
 * gas s of the uploaded table (default: all).  The reference always carries every gas through rankg (ForwardModel_0.py:
 * 5842-6026) and lets map2xvec drop what the state vector does not name; a caller that knows its state vector saves the replay
 * passes of the other gases (C2: 49 -> 21 passes for one gas).  The parameters of a gas that is switched off come back as the
 * continuum part only (dTAUCON), i.e. zero without one.  Bit 31: the temperature slot of the merge (d tau / dT through the
 * k-tables, two passes per merge); without it the temperature parameter keeps its continuum and Planck-function parts only.
 * Sticky until changed. */
int ansfm_set_gradient_gases(ansfm_ctx *ctx, unsigned int mask);

/* CIRSrad(return_grad=True), ILBL=K_TABLES, IMOD=THERMAL_EMISSION (ForwardModel_0.py:4376-4511
 * with :3853-3872 calc_kg/k_overlapg/dTAUGAS, :3993 dTAUTOT, :4012 LAYINC*SCALE, :4233
 * calc_thermal_emission_spectrumg, :4244-4247 xfac, :4504-4508 g-quadrature + nan_to_num).
 *   dtaucon[n][W][NPAR][L]  dTAUCON of calculate_layer_opacity (:3916-3981) or NULL
 *   NVMR, NPAR = NVMR+2+NDUST; igas_map[S] (HOST int32) = AtmosphereX.locate_gas(ID[i],ISO[i])
 *   SPECOUT[n][W][P], dSPECOUT[n][W][NPAR][LIMAX][P], dTSURF[n][W][P]
 * The reference's O(NPAR*Li^2) recursion is evaluated as one backward sweep.  * dSPECOUT may be NULL for n_models = 1: the gradients then stay on the device (no 8 W NPAR LIMAX P byte copy) for
 * ansfm_map2pro(dSPECIN = NULL); likewise ansfm_map2pro(dSPECOUT = NULL) keeps its result for ansfm_map2xvec(dSPECIN = NULL). */
int ansfm_cirsradg_ck_thermal(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                              const double *lay_press_pa, const double *lay_temp,
                              const double *amount, const double *taucont, const double *dtaucon,
                              int NVMR, int NPAR, const int32_t *igas_map, int P, int LIMAX,
                              const int32_t *NLAYIN, const int32_t *LAYINC, const double *SCALE,
                              const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                              const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF);
int ansfm_cirsradg_ck_thermal_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L,
                                  const double *lay_press_pa, const double *lay_temp,
                                  const double *amount, const double *taucont,
                                  const double *dtaucon, int NVMR, int NPAR,
                                  const int32_t *igas_map_host, int P, int LIMAX,
                                  const int32_t *NLAYIN, const int32_t *LAYINC,
                                  const double *SCALE, const double *EMTEMP, const double *TSURF,
                                  const double *EMISSIVITY, const double *xfac, double *SPECOUT,
                                  double *dSPECOUT, double *dTSURF);

/* The same with the continuum and its gradients formed inside the call from the context's resident sources (ansfm_upload_cia,
 * ansfm_upload_dust) and the Rayleigh parametrisations, any of the three -- the continuum block of
 * ansfm_cirsrad_ck_thermal_cont_dev in place of taucont / dtaucon; over all n * L layers (no de-duplication: a gradient call is
 * one state, or a few).  cont = (TAUCIA + TAUDUST) + TAURAY as there, and dTAUCON of calculate_layer_opacity (:3940-3981)
 * straight in the layout the gradient RT kernel reads ([n][NPAR][L][Wpad]), NPAR = NVMR + 2 + NDUST:
 *   kpar < NVMR            (dTAUCIA[kpar] of calc_tau_cia, i.e. its sum * xfac) / TOTAM, a true division, + dTAURAY (the Rayleigh
 *                          cross section per unit column) when ray_mode != 0.  As in the reference, calc_tau_cia's dk/dT term
 *                          lands in slot NVMR - 2 (:4741), on top of whatever that gas contributes as a partner
 *   kpar == NVMR           dTAUCIA[NVMR], which calc_tau_cia never fills: zero
 *   kpar == NVMR + 1 + i   dTAUDUST1 of population i = kext * 1e-4, raw: nan_to_num and the clip to [0, 1e20] (:3966) act on
 *                          the opacity only, so a negative population is clipped in cont and not here
 *   kpar == NPAR - 1       zero (para-H2)
 * An absent term adds nothing.  Same bits as ansfm_calc_tau_cia (with gradients) + ansfm_calc_tau_dust +
 * ansfm_calc_tau_rayleigh assembled on the host that way and passed as taucont / dtaucon -- without the 8 W NPAR L bytes per
 * state crossing PCIe twice.  The Rayleigh term is summed into the dense gradients, not handed over as a shared gas gradient
 * (which the RT adds as a second product, with other bits): a pending ansfm_set_shared_gas_gradient is ANSFM_ERR_INVALID and is
 * cancelled.  ANSFM_ERR_INVALID also when a source that is used has not been uploaded since the last table, the CIA source
 * was uploaded for the other ISPACE, NVMR is not the NVMR of the uploaded CIA source (or < 2) when CIA is used, or NPAR is not
 * NVMR + 2 + the NDUST of the uploaded aerosol source when aerosols are used.  ANSFM_ERR_UNSUPPORTED for NVMR + 2 >
 * ANSFM_MAX_CONT_GRAD_SLOTS.  None of the refusals launches a kernel.
 * Host-pointer version: every array a host pointer, dSPECOUT may be NULL for n_models = 1 as in ansfm_cirsradg_ck_thermal;
 * `_dev`: device pointers for every array but igas_map, asynchronous on the ctx stream. */
int ansfm_cirsradg_ck_thermal_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                   const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                   const double *lay_cont, int ray_mode, const double *f4, int NVMR, int NPAR,
                                   const int32_t *igas_map, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                   const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                   const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF);
int ansfm_cirsradg_ck_thermal_cont_dev(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                       const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                       const double *lay_cont, int ray_mode, const double *f4, int NVMR, int NPAR,
                                       const int32_t *igas_map_host, int P, int LIMAX, const int32_t *NLAYIN, const int32_t *LAYINC,
                                       const double *SCALE, const double *EMTEMP, const double *TSURF, const double *EMISSIVITY,
                                       const double *xfac, double *SPECOUT, double *dSPECOUT, double *dTSURF);

/* ---- multiple scattering ---------------------------------------------------------------------
 * Multiple_Scattering_Core.scloud11wave_core (Multiple_Scattering_Core.py:651-960): plane-parallel
 * matrix-operator doubling/adding with azimuth Fourier expansion.  Arguments, layouts and meaning
 * are the reference's (host pointers):
 *   phasarr[ncont][nwave][2][nth] (HG: f,g1,g2 in the first 3 slots of [..][0][:] when imie == 0),
 *   radg[nwave][nmu], sol_angs/emiss_angs/aphis[ngeom] (deg), solar[nwave], lowbc (0 thermal, >0 surface),
 *   brdf_matrix[nwave][nmu][nmu][nf+1], mu1/wt1[nmu], bnu[nwave][nlay], taus[nwave][ng][nlay],
 *   tauray[nwave][nlay], omegas_s[nwave][ng][nlay], lfrac[nwave][ncont][nlay]  ->  rad[ngeom][ng][nwave].
 * Mixed emission angles above/below 90 deg -> ANSFM_ERR_INVALID (the reference raises ValueError :776);
 * look-up geometry (all > 90) -> ANSFM_ERR_UNSUPPORTED for now. */
int ansfm_scloud11wave_core(ansfm_ctx *ctx, int ncont, int nwave, int nth, const double *phasarr,
                            const double *radg, int ngeom, const double *sol_angs,
                            const double *emiss_angs, const double *solar, const double *aphis,
                            int lowbc, const double *brdf_matrix, int nmu, const double *mu1,
                            const double *wt1, int nf, const double *bnu, int ng, int nlay,
                            const double *taus, const double *tauray, const double *omegas_s,
                            int nphi, int iray, int imie, const double *lfrac, double *rad);

/* CIRSrad, scattering branch (ILBL = K_TABLES or LINE_BY_LINE_TABLES, IMOD & MULTIPLE_SCATTERING; ForwardModel_0.py:4478-4501
 * -> calculate_multiple_scattering_spectrum :4343 -> scloud11wave :5018-5165) with everything that has a g axis on the
 * device: calc_k + k_overlap (k-tables) or calc_klbl (LBL tables, G = 1, DELG = {1}; :3795-3817) give the VERTICAL gas
 * opacities (not LAYINC-scaled: scloud11wave reads LayerX.TAUTOT),
 * TAUTOT = TAUGAS + TAUCIA + TAUDUST + TAURAY (:3989), OMEGA = (TAURAY + TAUSCAT) / TAUTOT and BB = planck(TEMP) (:5099-5119)
 * are formed in HBM and feed the doubling / adding kernels directly; the g-quadrature with DELG (:4504) ends the call.
 * Host pointers, reference layouts: taucia / taudust (summed over populations) / tauray / tauscat [W][L] (NULL = zeros),
 * lfrac[W][ncont][L] = TAUCLSCAT / TAUSCAT, the remaining scloud11wave_core arguments as above (W = the table's wavenumber
 * grid, ng = its g-ordinates), xfac[W] or NULL -> SPECOUT[W][ngeom]; SPEC_G[W][G][ngeom] (what scloud11wave returns, before
 * the quadrature) when not NULL.  ansfm_get_taugas returns the TAUGAS side product afterwards.
 * G = 1 (every LBL table): the phase matrices and Hansen factors are held for a window of wavenumbers at a time (default the
 * larger of 4096 and W / 16, rounded up to 64, one window's buffers under 2 GB; ANSFM_MS_WINDOW=<wavenumbers> overrides);
 * the walk of window k + 1 runs beside the chains of window k.  The window size changes no bit of the result. */
int ansfm_cirsrad_ck_scatter(ansfm_ctx *ctx, int ISPACE, int L, const double *lay_press_pa, const double *lay_temp,
                             const double *amount, const double *taucia, const double *taudust, const double *tauray,
                             const double *tauscat, int ncont, int nth, const double *phasarr, const double *lfrac,
                             const double *radg, int ngeom, const double *sol_angs, const double *emiss_angs,
                             const double *aphis, const double *solar, int lowbc, const double *brdf_matrix, int nmu,
                             const double *mu1, const double *wt1, int nf, int nphi, int iray, int imie, const double *xfac,
                             double *SPECOUT, double *SPEC_G);

/* The same branch for the n_models forward models of a numerical Jacobian: jacobian_nemesis forces the numerical route
 * whenever ISCAT != THERMAL_EMISSION (ForwardModel_0.py:2251-2252), i.e. NX + 1 multiple-scattering forward models that
 * differ from the first in the few layers one state-vector element touches.  Arrays that depend on the state carry a
 * leading model axis: lay_press_pa / lay_temp [n][L], amount [n][S][L], taucia / taudust / tauray / tauscat [n][W][L] (NULL =
 * zeros), lfrac [n][W][ncont][L], radg [n][W][nmu]; phasarr, solar, brdf_matrix, xfac and the geometry are shared
 * -> SPECOUT [n][W][ngeom].
 * 16 streams: the doubled (R, T, J) of a layer (calc_rtj_matrix, Multiple_Scattering_Core.py:566-650) depend on that
 * layer's inputs only and are ~92 % of a chain's work; model 0's pass keeps them per (wavenumber, g, Fourier order,
 * layer) in HBM (slabs of the spectral axis sized to the free memory), every other model re-runs the adding sweep
 * (addp :481-533) over them and recomputes only the layers whose inputs differ from model 0's in any bit -- the same
 * numbers as n_models separate calls, bit for bit.  ansfm_set_layer_dedup(ctx, 0) (or another stream count) runs the
 * models one after the other through ansfm_cirsrad_ck_scatter.  ansfm_last_scatter_cache: (model, layer) pairs taken
 * from the cache / all pairs of models 1..n-1 in the last call; ansfm_last_layer_rows: gas opacity rows computed.
 * LBL tables: the distinct (model, layer) rows through calc_klbl; at G = 1 the slabs of the spectral axis are the windows
 * of phase matrices and Hansen factors (as in ansfm_cirsrad_ck_scatter), the walk continuing from slab to slab. */
int ansfm_cirsrad_ck_scatter_batch(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                   const double *lay_temp, const double *amount, const double *taucia, const double *taudust,
                                   const double *tauray, const double *tauscat, int ncont, int nth, const double *phasarr,
                                   const double *lfrac, const double *radg, int ngeom, const double *sol_angs,
                                   const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                   const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                   int iray, int imie, const double *xfac, double *SPECOUT);
/* The same batch on a slice of the spectral axis (one rank of a wavenumber-sharded Jacobian): the context holds the slice
 * [w_begin, w_begin + W_local) of a W_full axis (W_local = the uploaded table's width).  phasarr covers the whole axis,
 * [ncont][W_full][2][nth]; taucia / taudust / tauray / tauscat, lfrac, radg, solar, brdf_matrix, xfac and SPECOUT
 * [n][W_local][ngeom] cover the slice.  The Hansen factors depend on every earlier (g, wavenumber) of the walk, so the walk
 * runs over the whole axis (up to the slice's end at G = 1) and keeps the slice's factors: the slices, side by side, are
 * bit-identical to ansfm_cirsrad_ck_scatter_batch over the whole axis; W_full = W_local, w_begin = 0 is that call.  A slice
 * needs the layer cache (n_models > 1, layer de-duplication on): ANSFM_ERR_UNSUPPORTED otherwise.  ANSFM_ERR_INVALID when
 * w_begin < 0, w_begin + W_local > W_full or phasarr is NULL with ncont > 0. */
int ansfm_cirsrad_ck_scatter_batch_slice(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                         const double *lay_temp, const double *amount, const double *taucia, const double *taudust,
                                         const double *tauray, const double *tauscat, int ncont, int nth, const double *phasarr,
                                         const double *lfrac, const double *radg, int ngeom, const double *sol_angs,
                                         const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                         const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                         int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin);
/* The same batch (whole axis: W_full = W_local, w_begin = 0; or one slice) with the continuum handed over once per distinct
 * layer instead of once per (model, layer): cont_row [n][L] (host) is the continuum row of layer l of model m,
 * 0 <= cont_row < R; taucia_rows / taudust_rows / tauray_rows / tauscat_rows [R][W_local] (host, wavenumber fastest, NULL =
 * zeros) and lfrac_rows [R][ncont][W_local] hold the rows -- one map serves all five, a row is "the continuum of one distinct
 * layer".  Every other argument is ansfm_cirsrad_ck_scatter_batch_slice's.  The result is bit-identical to that entry called
 * with the expanded arrays, dense[m][w][l] = rows[cont_row[m][l]][w]: the arithmetic per (wavenumber, g, layer) is the same.
 * Layer (m, l) counts as model 0's -- and is taken from the layer cache -- when its gas-opacity row is model 0's and
 * cont_row[m][l] == cont_row[0][l]; no array is compared.  Equal content under two different indices therefore loses cache
 * hits for that layer, never bits: a recomputed layer gives the bits of a separate call.  The dense arrays exist nowhere:
 * the rows are uploaded, and the chain kernels read copies of TAURAY and the fractions of one launch's models on one slab;
 * the model-by-model route (n_models = 1, ansfm_set_layer_dedup(ctx, 0), ANSFM_MS_LAYER_CACHE=0) forms one model's arrays
 * on the device at a time.  ANSFM_ERR_INVALID, before anything is launched, when cont_row is NULL, R <= 0 or an index is
 * outside [0, R), and for the slice entry's reasons.  ansfm_last_scatter_cache / ansfm_last_layer_rows /
 * ansfm_last_scatter_windows report as for the dense call. */
int ansfm_cirsrad_ck_scatter_batch_rows(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                        const double *lay_temp, const double *amount, int R, const int32_t *cont_row,
                                        const double *taucia_rows, const double *taudust_rows, const double *tauray_rows,
                                        const double *tauscat_rows, int ncont, int nth, const double *phasarr,
                                        const double *lfrac_rows, const double *radg, int ngeom, const double *sol_angs,
                                        const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                        const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                        int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin);
/* The same batch with the rows formed inside the call from the context's resident sources (ansfm_upload_cia,
 * ansfm_upload_dust, which keeps the scattering cross sections too) and the Rayleigh parametrisations: nothing of the
 * continuum crosses PCIe.  In place of R, cont_row and the five row arrays the entry takes the continuum block of
 * ansfm_cirsrad_ck_thermal_cont_dev, as host arrays like every other argument: use_cia with lay_q [n][L][NVMR] (NVMR as
 * uploaded), lay_frac, lay_delh [n][L]; use_dust with lay_cont [n][L][ncont]; ray_mode (0, or IRAY 1, 2, 4, 12) with f4
 * [n][L][4] for mode 4; lay_totam [n][L] for CIA and Rayleigh.  Per distinct row (k_ms_cont_rows) TAUCIA and TAURAY are what
 * ansfm_calc_tau_cia / ansfm_calc_tau_rayleigh give; per population d, e_d = (kext 1e-4) CONT and s_d = (ksca 1e-4) CONT as
 * ansfm_calc_tau_dust rounds them, TAUDUST = sum_d clip(nan_to_num(e_d), 0, 1e20), TAUSCAT = sum_d s_d (raw) and the fraction
 * of d is s_d / TAUSCAT where TAUSCAT > 0, else 0 (ForwardModel_0.py:3963-3972, :5107-5113) -- the result is bit-identical to
 * ansfm_cirsrad_ck_scatter_batch_rows on rows formed that way.  A term that is not used is absent (NULL to the optics), not
 * zeros.  One row map serves gas opacities and continuum: a layer is distinct when it differs from model 0's in pressure,
 * temperature, an amount or a column its continuum is formed from (lay_totam; f4; lay_q, lay_delh and, for a CIA table with
 * a para-H2 axis, lay_frac; lay_cont), and counts as model 0's exactly when its row is model 0's row of that layer.  The
 * model-by-model route (n_models = 1, ansfm_set_layer_dedup(ctx, 0), ANSFM_MS_LAYER_CACHE=0) forms the L rows of one model at
 * a time.  ANSFM_ERR_INVALID, before anything is launched: a source that is used has not been uploaded since the last table,
 * the CIA source was uploaded for the other ISPACE, ncont is not the number of populations uploaded (0 without use_dust), no
 * term is used or one of its arrays is NULL, and for the slice entry's reasons.  ansfm_last_scatter_cache /
 * ansfm_last_layer_rows / ansfm_last_scatter_windows report as for the rows entry. */
int ansfm_cirsrad_ck_scatter_batch_cont(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                        const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                        const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                        const double *lay_cont, int ray_mode, const double *f4, int ncont, int nth,
                                        const double *phasarr, const double *radg, int ngeom, const double *sol_angs,
                                        const double *emiss_angs, const double *aphis, const double *solar, int lowbc,
                                        const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf, int nphi,
                                        int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin);
/* The same with phasarr formed on the device from the resident phase-function source (ansfm_upload_phase): in its place
 * theta_deg [nth] (Scatter.THETA, strictly ascending) and mu_theta [nth] = np.cos(THETA * pi / 180) from the host, so that row 1
 * carries NumPy's bits.  k_phase_fn writes PHASE_ARRAY[:, :, :, ::-1] of ForwardModel_0.py:5128-5142 straight into the buffer
 * the phase-matrix kernels read: with imie == 0 row 0 holds f_w, g1_w, g2_w (np.interp of F, G1, G2 on the table's grid) in its
 * first three slots and zeros behind, otherwise the source at theta_deg, reversed; row 1 is mu_theta, reversed.
 * ansfm_phasarr_from_source returns the same array to the host, and the result is bit-identical to the entry above called with
 * it, for every stream count, with the layer cache on and off.  use_dust must be set.  ANSFM_ERR_UNSUPPORTED: W_full is not the
 * table's W or w_begin != 0 (a slice's context does not hold the whole grid).  ANSFM_ERR_INVALID, before anything is launched,
 * also when no phase-function source has been uploaded since the last table, when its NDUST is not ncont, when imie is 0 and
 * the source's is not (or the reverse), for theta_deg not ascending or (IMIE 1) outside the tabulated angles. */
int ansfm_cirsrad_ck_scatter_batch_src(ansfm_ctx *ctx, int ISPACE, int n_models, int L, const double *lay_press_pa,
                                       const double *lay_temp, const double *amount, int use_cia, const double *lay_q,
                                       const double *lay_frac, const double *lay_totam, const double *lay_delh, int use_dust,
                                       const double *lay_cont, int ray_mode, const double *f4, int ncont, int nth,
                                       const double *theta_deg, const double *mu_theta, const double *radg, int ngeom,
                                       const double *sol_angs, const double *emiss_angs, const double *aphis, const double *solar,
                                       int lowbc, const double *brdf_matrix, int nmu, const double *mu1, const double *wt1, int nf,
                                       int nphi, int iray, int imie, const double *xfac, double *SPECOUT, int W_full, int w_begin);
/* Per-model phase functions inside the batch: the states of a Jacobian that change an aerosol population's phase function
 * (a size distribution or a refractive index, Models/PreRTModels/model_444.py) join the batch instead of running on their own.
 * A pending setting in the style of ansfm_set_shared_gas_gradient: phase_of [n_models] (host) names the variant of every model,
 * 0 <= phase_of < V; variant 0 is the phasarr argument of the consuming call and phase_of[0] must be 0; phasarr_variants
 * [V - 1][ncont][W][2][nth] (host, W = the uploaded table's width) holds variants 1 .. V-1.  THE LIBRARY COPIES BOTH ARRAYS AT
 * SET TIME: the caller may free them as soon as this returns.  The setting arms the NEXT ansfm_cirsrad_ck_scatter_batch or
 * ansfm_cirsrad_ck_scatter_batch_rows call on the whole axis and is then forgotten, whether that call succeeds or fails; V <= 1
 * or a NULL array cancels it.  Every spectrum has the bits of a separate ansfm_cirsrad_ck_scatter call of that model with its
 * variant's phasarr.
 * Per variant the components whose [W][2][nth] block differs from variant 0's in any bit are found on the host; only those
 * (variant, component) pairs are integrated (k_ms_phase) and walked (k_ms_hansen_seq), in the same two launches as variant 0's
 * components -- the walk keeps one history per scatterer, so an unchanged component, Rayleigh always, has variant 0's matrices
 * and factors bit for bit and is copied on the device.  A variant's matrices and factors keep variant 0's layout, one variant
 * behind the other (V times the bytes of one; ansfm_last_scatter_variants reports the pairs beyond variant 0's and the bytes
 * of variants 1 .. V-1 in the last batched call, and in walk_ms the time between two events around the phase-matrix launch,
 * the walk and the copy of that call -- with or without variants; -1 when the call had none, as at G = 1), reserved before
 * the layer cache is sized.
 * A layer of model m counts as model 0's only if, besides the rules above, no population whose phase function differs between
 * m's variant and variant 0 is present in it: its fraction lfrac is 0 at every wavenumber (the layer's lfrac row in the rows
 * form).  The mixing sum then gains a term fs P 0 = +-0, which changes no bit of a non-zero sum; where the sum before the term
 * is an exact zero its sign could differ between variants -- not observed in any test; the rule would be narrowed if it were.
 * THE RULE ASSUMES FINITE PHASE MATRICES (0 times an infinity or a NaN is a NaN).  A model that shares every layer is legal.
 * The model-by-model route (ansfm_set_layer_dedup(ctx, 0), ANSFM_MS_LAYER_CACHE=0) hands each model its variant's phasarr.
 * The consuming call returns, before anything is launched,
 *   ANSFM_ERR_INVALID      n_models, ncont or nth differ from the call's (or the table's width changed since the setting),
 *                          a phase_of entry is outside [0, V), phase_of[0] != 0;
 *   ANSFM_ERR_UNSUPPORTED  the call is a slice (W_full != W_local), the table has one g-ordinate (G = 1: the windowed walk with
 *                          carries), or the entry is ansfm_cirsrad_ck_scatter_batch_cont / _src (their resident aerosol
 *                          source has no model axis for the cross sections, so a size-distribution state cannot be expressed);
 * and ANSFM_ERR_UNSUPPORTED later when the variants' buffers cannot be reserved: the caller then groups its states by phase
 * function as before.  ansfm_set_phase_variants itself: ANSFM_ERR_INVALID without a table or for n_models <= 0, ncont <= 0,
 * nth < 3. */
int ansfm_set_phase_variants(ansfm_ctx *ctx, int n_models, int V, const int32_t *phase_of, int ncont, int nth,
                             const double *phasarr_variants);
int ansfm_last_scatter_variants(const ansfm_ctx *ctx, int64_t *pairs, int64_t *bytes, double *walk_ms);
int ansfm_last_scatter_cache(const ansfm_ctx *ctx, int64_t *layers_from_cache, int64_t *layers_total);
/* Spectral windows of phase matrices / Hansen factors in the last scattering call (ansfm_cirsrad_ck_scatter(_batch),
 * ansfm_scloud11wave_core) and the wavenumbers per window: 1 and W when one window covers the axis (always at G > 1). */
int ansfm_last_scatter_windows(const ansfm_ctx *ctx, int64_t *windows, int64_t *window_wavenumbers);

/* ---- runtime line-by-line (ILBL = LINE_BY_LINE_RUNTIME) -------------------------------------------
 * LineData_0.add_line_set_monochromatic_absorption (LineData_0.py:280-357), batched over L (T,p) points
 * (L = 1 is the reference's signature).  lineshape_id = SpectroscopicLineProfileEnum value: 0 VOIGT
 * (scipy.special.voigt_profile), 4 LORENTZ, 12 DOPPLER; the rest -> ANSFM_ERR_UNSUPPORTED (the reference's
 * enum map raises NotImplementedError for them too).
 *   wn_grid[nw] ascending; t_calc/p_calc/q_ratio[L]; mol_mix_frac[M]; broadening_params[3M][N]
 *   (gamma, n, delta per broadener); nu/sw/e_lower/stim_ref[N];
 *   out[L][nw] is ADDED to (like the reference); store[L][4][N] (strength, alpha_d, gamma_l, shift) or NULL. */
int ansfm_add_line_set_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance,
    double isotopic_mass, int M, const double *mol_mix_frac, int N, const double *broadening_params,
    const double *nu, const double *sw, const double *e_lower, const double *stim_ref, double *out,
    double *store, double s_floor, double wn_calc_window, double wn_approx_window);

/* LineData_0.add_pseudo_continuum_monochromatic_absorption (LineData_0.py:486-572): the pseudo-continuum of the weak
 * lines in N bins, batched over L (T,p) points like the line entry (same line shapes, same error codes).  The
 * stimulated-emission factor at t_ref is computed at the bin centres; there is no pressure shift.
 *   lsw_mean_broadening_params[3M][N]; wn_bin_centers/wn_bin_widths/sw_sum/lsw_mean_e_lower[N];
 *   out[L][nw] is ADDED to; store[L][3][N] (strength, alpha_d, gamma_l) or NULL; store_x[L][N] (the spread continuum per
 *   unit wavenumber) or NULL.  The reference's scratch arrays store_y / store_z are not filled: they hold the last source
 *   bin's shapes and the interpolation's sums and counts, which no caller reads.
 *   n_neighbour_bins 0 .. 8 (the reference's call sites pass 3); more -> ANSFM_ERR_UNSUPPORTED.
 * The widths must be positive and the lower edges centre - width/2 ascending (the reference's j_start shortcut
 * :451-457 equals the plain definition of a touched grid point exactly then), else ANSFM_ERR_INVALID, as for a descending
 * grid.  N == 0 is a no-op. */
int ansfm_add_pseudo_continuum_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance,
    double isotopic_mass, int M, const double *mol_mix_frac, int N, const double *lsw_mean_broadening_params,
    const double *wn_bin_centers, const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
    double *out, double *store, double *store_x, int n_neighbour_bins);

/* The opacity of a gas summed in HBM: the context owns a zeroed [L][nw] accumulator between `begin` and the next `begin`.
 * The two add calls take the arguments of the host entries without grid, (T,p) points and `out`, run the same kernels and
 * leave the sum on the device: after any sequence of adds it equals the same sequence of host-`out` calls started from
 * zeros, bit for bit.  An add, read or device_ptr before begin -> ANSFM_ERR_INVALID; a second begin starts over.
 * device_ptr: the buffer ([*L][*nw] float64, valid until the next begin or ansfm_destroy), synchronised. */
int ansfm_lbl_accum_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int L, const double *t_calc, const double *p_calc);
int ansfm_lbl_accum_add_lines(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                              double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                              const double *broadening_params, const double *nu, const double *sw, const double *e_lower,
                              const double *stim_ref, double *store, double s_floor, double wn_calc_window,
                              double wn_approx_window);
int ansfm_lbl_accum_add_pseudo_continuum(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                                         double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac,
                                         int N, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                         const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                         double *store, double *store_x, int n_neighbour_bins);
int ansfm_lbl_accum_read(ansfm_ctx *ctx, double *out);
int ansfm_lbl_accum_device_ptr(ansfm_ctx *ctx, double **dev, int *L, int *nw);

/* Side product of the last gradient CIRSrad call (ansfm_cirsradg_ck_thermal / _transmission), like ansfm_get_taugas of a
 * forward call: the derivatives of the vertical gas opacity of model `model`, dTAUGAS[W][G][S + 1][L] -- slot s = the
 * derivative with respect to the amount of gas s as the kernels keep it (the reference's dTAUGAS[:, :, IGAS, :] is this times
 * SQ_CM_TO_SQ_METER = 1e-4, :3813, :3844), slot S = d tau / dT (:3814, :3845).  No gradient call yet, or a gas-overlap seam since -> ANSFM_ERR_INVALID. */
int ansfm_get_dtaugas(ansfm_ctx *ctx, int model, double *dTAUGAS);

/* ---- runtime line-by-line as the context's opacity source ------------------------------------------------------------
 * The ILBL = LINE_BY_LINE_RUNTIME branch of ForwardModel_0.calculate_gaseous_line_opacity (ForwardModel_0.py:3819-3848) with
 * Spectroscopy_0.calc_klbl_online (:2046) / calc_klblg_online (:1922): the line data of S gases stay in HBM, and every entry
 * that computes gas opacities (thermal and its gradient, transmission and its gradient, single and multiple scattering,
 * ansfm_get_taugas) takes them from the lines instead of a table.
 *
 * begin: wn_grid[nw] ascending (else ANSFM_ERR_INVALID), S gases, M broadeners ("self" first, then the ambient gases).  A
 * source committed earlier is taken apart.
 * add_isotopologue: everything of one isotopologue of gas `gas` that stays fixed over a retrieval, in the order the
 * reference walks LineData_0.line_data / continuum_data.  The caller has applied the reference's host-side selections: the
 * inclusive wn_calc_range masks (LineData_0.py:882, :1376) and the zeroed shift rows of include_pressure_shift = False
 * (:886-888).  Lines: N, t_ref, p_ref, broadening_params[3M][N], nu / sw / e_lower / stim_ref[N] in any order (sorted here,
 * once), s_floor and the two windows, as in ansfm_add_line_set_monochromatic_absorption.  Bins: N_bins, t_cont, p_cont,
 * lsw_mean_broadening_params[3M][N_bins], wn_bin_centers / wn_bin_widths / sw_sum / lsw_mean_e_lower[N_bins],
 * n_neighbour_bins, as in ansfm_add_pseudo_continuum_monochromatic_absorption.  include_lines / include_continuum: the
 * reference's switches.  Error codes are those entries': a shape that is not built -> ANSFM_ERR_UNSUPPORTED, bin widths
 * that are not positive or lower edges that do not ascend -> ANSFM_ERR_INVALID, more than 8 neighbour bins ->
 * ANSFM_ERR_UNSUPPORTED.  N == 0, or sw_sum all zero, is the reference's has_data == False: that part adds nothing.
 * commit: every gas has an isotopologue, else ANSFM_ERR_INVALID.  The context then answers like an uploaded LBL table with
 * G = 1 and W = nw (ansfm_ktable_info), and stays so until a table is uploaded; a commit after an upload takes the table's
 * place.  Layer de-duplication and the scattering batch's layer cache are not applied in this mode (their comparison of
 * pressure, temperature and amounts does not see the mix fractions; the distinct rows of set_state take their place), so
 * ansfm_cirsrad_ck_scatter_batch runs its models one by one and ansfm_cirsrad_ck_scatter_batch_slice is
 * ANSFM_ERR_UNSUPPORTED.  ansfm_calc_k / ansfm_calc_klbl -> ANSFM_ERR_NOTABLE. */
int ansfm_lblrt_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int S, int M);
int ansfm_lblrt_add_isotopologue(ansfm_ctx *ctx, int gas, int lineshape_id, double isotopic_abundance, double isotopic_mass,
                                 int include_lines, int N, double t_ref, double p_ref, const double *broadening_params,
                                 const double *nu, const double *sw, const double *e_lower, const double *stim_ref, double s_floor,
                                 double wn_calc_window, double wn_approx_window, int include_continuum, int N_bins, double t_cont,
                                 double p_cont, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                 const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                 int n_neighbour_bins);
int ansfm_lblrt_commit(ansfm_ctx *ctx);

/* The state of the next CIRSrad calls, by distinct k-row: the cross-section of gas s in a layer depends on (p, T, the mix
 * fractions of gas s) only, so the caller hands over the R distinct rows and krow[n][S][L] (int32), the row of every (model,
 * gas, layer) -- as cont_row does in ansfm_cirsrad_ck_scatter_batch_rows.
 *   row_gas[R] (int32, ascending: the rows are grouped by gas); row_p_atm[R] (atm: PRESS / ATM_TO_PASCAL as the reference
 *   divides); row_t[R]; row_mix[R][M] (1 - sum amb_frac, amb_frac...: LineData_0.py:2342-2345); row_q_lines / row_q_cont: the
 *   partition-function ratios Q(t_ref) / Q(T) and Q(t_cont) / Q(T) of the isotopologues of the row's gas, one row after the
 *   other ([R][isotopologues of that gas]); row_q_*_dT: the same at T + 5 K, both or neither -- NULL when no gradient is
 *   asked for.  The ratios come from the caller because the reference's partition_fn_data[i] is a Python callable.
 * The maps are checked on the host before anything launches: a krow entry outside [0, R) or naming a row of another gas, a
 * row_gas outside [0, S) or descending -> ANSFM_ERR_INVALID.  The rows' spectra are computed here, per gas as one batch of
 * (T, p) points with the (T + 5 K, p) points in the same launches, in chunks of rows whose scratch fits
 * ansfm_lblrt_set_scratch_bytes (default 256 MiB; the chunk size changes no bit of the result).  Per row the
 * isotopologues add lines_0, continuum_0, lines_1, ... onto one zeroed buffer: calc_klblg_online's order and the order of
 * ansfm_lbl_accum_*, to which the rows are bit-identical.  calc_klbl_online forms (sum lines) + (sum continuum)
 * (LineData_0.py:2255-2279): the forward seam agrees with the reference to rounding only.
 * The state stands until the next set_state, commit, table upload or ansfm_calc_klbl(g)_online.  A CIRSrad call whose
 * (n_models, L) differs from the state's, a call before any state, and a gradient call on a state without the _dT ratios
 * -> ANSFM_ERR_INVALID.  tau = sum_s k[krow] * amount in ascending s (:3841, :3848); the temperature slot of the gradient is
 * sum_s dkdt_s * amount (:3845) with the reference's dkdt: calc_klblg_online clears its T + 5 K buffer once per gas, not per
 * point (Spectroscopy_0.py:1987), so dkdt of layer l is (sum_{j <= l} k(T_j + 5) - k(T_l)) / 5 (:2041), and so it is here.
 * last: the rows and (T, p) points of the last computation and the chunks they ran in. */
int ansfm_lblrt_set_state(ansfm_ctx *ctx, int n_models, int L, int R, const int32_t *krow, const int32_t *row_gas,
                          const double *row_p_atm, const double *row_t, const double *row_mix, const double *row_q_lines,
                          const double *row_q_cont, const double *row_q_lines_dT, const double *row_q_cont_dT);
int ansfm_lblrt_set_scratch_bytes(ansfm_ctx *ctx, int64_t bytes);
int ansfm_lblrt_last(const ansfm_ctx *ctx, int *rows, int *points, int *chunks);

/* Array-level seams, mirroring ansfm_calc_klbl: Spectroscopy_0.calc_klbl_online / calc_klblg_online on the committed source.
 *   press[L] (atm), temp[L]; mol_mix_frac[S][M] per gas; q_lines / q_cont (and _dT at T + 5 K): [isotopologues of gas 0, of
 *   gas 1, ...][L] -> k_out[nw][L][S], dkdT_out[nw][L][S] = (sum_{j <= l} k(T_j + 5) - k(T_l)) / 5 (see above).
 * Both run the order of calc_klblg_online (see above).  No committed source -> ANSFM_ERR_NOTABLE.  A pending state of
 * ansfm_lblrt_set_state is dropped. */
int ansfm_calc_klbl_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                           const double *q_lines, const double *q_cont, double *k_out);
int ansfm_calc_klblg_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                            const double *q_lines, const double *q_cont, const double *q_lines_dT, const double *q_cont_dT,
                            double *k_out, double *dkdT_out);

/* ---- layering ---------------------------------------------------------------------------------------
 * Layer_0.layer_average (Layer_0.py:755-1030), batched over n_models atmospheric states (the states of a
 * numerical Jacobian): LAYINT 0 = MID_PATH, 1 = ABSORBER_WEIGHTED_AVERAGE (Curtis-Godson, :949-1010).
 *   H,P,T[n][NPRO]; VMR[n][NPRO][NVMR]; DUST[n][NPRO][NDUST] or NULL; PARAH2[n][NPRO] or NULL;
 *   BASEH[n][NLAY] (layer_split output); DUST_UNITS[NDUST] (int32) / XMOLWT[n][NPRO] (kg/mol) or NULL
 *   -> HEIGHT,PRESS,TEMP,TOTAM,FRAC,DELH,BASET,LAYSF [n][NLAY]; AMOUNT,PP [n][NLAY][NVMR]; CONT [n][NLAY][NDUST].
 * 2 <= NINT <= 256 (even NINT: scipy.integrate.simpson's last-interval correction, as the reference gets). */
int ansfm_layer_average(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H,
                        const double *P, const double *T, int NVMR, const double *VMR, int NDUST,
                        const double *DUST, const double *PARAH2, int NLAY, const double *BASEH,
                        double LAYANG, int LAYINT, double LAYHT, int NINT, const int32_t *DUST_UNITS,
                        const double *XMOLWT, double *HEIGHT, double *PRESS, double *TEMP, double *TOTAM,
                        double *AMOUNT, double *PP, double *CONT, double *FRAC, double *DELH,
                        double *BASET, double *LAYSF);

/* The same with every array argument resident on the DEVICE (DUST_UNITS stays a host array) and the results left there:
 * out_dev = HEIGHT,PRESS,TEMP,TOTAM,FRAC,DELH,BASET,LAYSF [n][NLAY] one after the other, then AMOUNT [n][NLAY][NVMR],
 * PP [n][NLAY][NVMR], CONT [n][NLAY][NDUST] -- n * NLAY * (8 + 2 NVMR + NDUST) doubles.  Asynchronous on the context's
 * stream: the states of a numerical Jacobian go from profiles to layers to CIRSrad without crossing PCIe.  With more than
 * one state, a layer whose sub-points read only levels at which a state holds state 0's numbers takes state 0's result
 * (bit-identical; also in ansfm_layer_average; ANSFM_LAYER_SHARE=0 integrates every layer). */
int ansfm_layer_average_dev(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H,
                            const double *P, const double *T, int NVMR, const double *VMR, int NDUST,
                            const double *DUST, const double *PARAH2, int NLAY, const double *BASEH,
                            double LAYANG, int LAYINT, double LAYHT, int NINT, const int32_t *DUST_UNITS,
                            const double *XMOLWT, double *out_dev);

/* Layer_0.layer_averageg (Layer_0.py:1032-1398): the same plus DTE, DAM, DCO, DPH [n][NLAY][NPRO], the matrices
 * relating layer temperature / gas amounts / dust amounts / para-H2 fraction to the profile levels (consumed by
 * map2pro).  T, PARAH2, VMR and DUST go through the reference's own `interpg` bracket (:716-751) here, so the layer
 * values differ from ansfm_layer_average's in the last bits exactly as the reference's two functions do.
 * ANSFM_ERR_INVALID for an even NINT (ValueError :1188) and for MID_PATH with DUST_UNITS == -1 (the reference
 * fails there, :1255-1257). */
int ansfm_layer_averageg(ansfm_ctx *ctx, int n_models, double RADIUS, int NPRO, const double *H,
                         const double *P, const double *T, int NVMR, const double *VMR, int NDUST,
                         const double *DUST, const double *PARAH2, int NLAY, const double *BASEH,
                         double LAYANG, int LAYINT, double LAYHT, int NINT, const int32_t *DUST_UNITS,
                         const double *XMOLWT, double *HEIGHT, double *PRESS, double *TEMP, double *TOTAM,
                         double *AMOUNT, double *PP, double *CONT, double *FRAC, double *DELH,
                         double *BASET, double *LAYSF, double *DTE, double *DAM, double *DCO, double *DPH);

/* ---- gradient maps ------------------------------------------------------------------------------------
 * ForwardModel_0.map2pro (ForwardModel_0.py:5319-5383): layer gradients -> profile-level gradients,
 *   dSPECOUT[W][NPAR][NPRO][P] = sum_j dSPECIN[W][NPAR][LIMAX][P] * M[LAYINC[j][p]][NPRO], M = DAM for gas
 *   parameters (index < NVMR), DTE for temperature (== NVMR), DCO for dust (NVMR < index <= NVMR+NDUST);
 *   NPAR = NVMR+2+NDUST.  INCPAR[n_incpar] = the parameters to map (n_incpar = 0: all); unlisted slots stay 0.
 *   The para-H2 slot (NVMR+NDUST+1) receives the PREVIOUS listed parameter's result, as in the reference
 *   (:5373-5377 assign the stale dSPECOUT1); listing it first is the reference's UnboundLocalError ->
 *   ANSFM_ERR_INVALID.   LAYINC[LIMAX][P] int32, DTE/DAM/DCO[NLAY][NPRO].
 * ForwardModel_0.map2xvec (:5387-5424): dSPECOUT[W][P][NX] = sum_{par,pro} dSPECIN[W][NPAR][NPRO][P] * xmap[NX][NPAR][NPRO].
 * Device chaining: dSPECIN == NULL takes the device-resident result of the previous step of this ctx
 * (map2pro: the dSPECOUT of the last single-model ansfm_cirsradg_ck_thermal; map2xvec: the last map2pro) and
 * fails with ANSFM_ERR_INVALID if its dimensions differ.  dSPECOUT == NULL (map2pro only) keeps the result
 * on the device for the following map2xvec. */
int ansfm_map2pro(ansfm_ctx *ctx, int W, int NPAR, int LIMAX, int P, int NPRO, int NLAY, int NVMR, int NDUST,
                  const double *dSPECIN, const int32_t *LAYINC, const double *DTE, const double *DAM,
                  const double *DCO, int n_incpar, const int32_t *INCPAR, double *dSPECOUT);
int ansfm_map2xvec(ansfm_ctx *ctx, int W, int NPAR, int NPRO, int P, int NX, const double *dSPECIN,
                   const double *xmap, double *dSPECOUT);

/* ---- instrument line shape (the step after the path) ---------------------------------------
 * Measurement_0.lblconv (Measurement_0.py:3335; nx = 0) / lblconvg (:3799; nx > 0): convolution of the monochromatic
 * spectrum y[nwave] (and gradients dydx[nwave][nx]) with the ILS given by ISHAPE (0 square, 1 triangular, 2 gaussian,
 * 3 Hamming, 4 Hanning) and FWHM > 0 at the convolution wavenumbers vconv[nconv] -> yout[nconv], gradout[nconv][nx].
 * Reference behaviour kept: only weights > 0 count; the Hamming window of lblconv is the single point
 * vcen - 1.1 FWHM (:3391-3393) while lblconvg uses vcen -+ FWHM (:3866-3868); Hanning assigns no weight, so the
 * result is 0/0 = NaN like the reference's.  vwave must be ascending (ANSFM_ERR_UNSORTED otherwise).
 * lblconv_fil (:3549) / lblconvg_fil (:3992): the ILS is tabulated per convolution point, nfil[nconv] points in
 * column j of vfil / afil [nfilmax][nconv], weights by linear interpolation (np.interp). */
int ansfm_lblconv(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx, const double *dydx,
                  int nconv, const double *vconv, int ishape, double fwhm, double *yout, double *gradout);
int ansfm_lblconv_fil(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx,
                      const double *dydx, int nconv, const double *vconv, int nfilmax, const int32_t *nfil,
                      const double *vfil, const double *afil, double *yout, double *gradout);
/* lblconv_ngeom (:3444) / lblconvg_ngeom (:3685) / lblconv_fil_ngeom (:3614) / lblconvg_fil_ngeom (:3912): NGEOM spectra
 * on one grid, y[nwave][ngeom], dydx[nwave][ngeom][nx] (nx = 0: none) -> yout[nconv][ngeom], gradout[nconv][ngeom][nx].
 * Same arithmetic per column; the Hamming window of both ISHAPE variants is the single point vcen - FWHM (:3501-3503,
 * :3753-3755).  (The reference's lblconv_ngeom is an un-jitted Python loop.) */
int ansfm_lblconv_ngeom(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                        const double *dydx, int nconv, const double *vconv, int ishape, double fwhm, double *yout,
                        double *gradout);
int ansfm_lblconv_fil_ngeom(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                            const double *dydx, int nconv, const double *vconv, int nfilmax, const int32_t *nfil,
                            const double *vfil, const double *afil, double *yout, double *gradout);

/* integrate_filter (:4079) / integrate_filterg (:4188) and their *_ngeom variants (:4131, :4251): np.trapz of
 * (filter x spectrum) over the calculation points inside each filter, no normalisation.  y[nwave][ngeom],
 * dydx[nwave][ngeom][nx] (ngeom = 1 for the single-geometry functions) -> yout[nconv][ngeom], gradout[nconv][ngeom][nx]. */
int ansfm_integrate_filter(ansfm_ctx *ctx, int nwave, const double *vwave, int ngeom, const double *y, int nx,
                           const double *dydx, int nconv, const double *vconv, int nfilmax, const int32_t *nfil,
                           const double *vfil, const double *afil, double *yout, double *gradout);

/* Measurement_0.conv (:2288) / convg (:2467), k-table runs, FWHM < 0 branch (:2425-2461, :2655-2691): the filter
 * average of lblconv_fil, but over the window from the last calculation point BELOW vfil[0][j] to the first ABOVE
 * vfil[nfil[j]-1][j] (both must exist: the reference raises IndexError otherwise -> ANSFM_ERR_INVALID), np.interp
 * clamping to the edge values outside the filter. */
int ansfm_conv_fil(ansfm_ctx *ctx, int nwave, const double *vwave, const double *y, int nx, const double *dydx,
                   int nconv, const double *vconv, int nfilmax, const int32_t *nfil, const double *vfil,
                   const double *afil, double *yout, double *gradout);

/* ---- continuum ---------------------------------------------------------------------------
 * ForwardModel_0.calc_tau_cia (ForwardModel_0.py:4516-4760), wavenumber space (the caller converts and re-orders a
 * wavelength grid as the reference does, :4565-4568 / :4741-4743).  WAVEN[W] ascending; the CIA table
 * K_CIA[NPAIR][NPE][NT][NWC] on cia_waven / cia_temp / cia_frac[nfrac] (NPE = size of the para axis of K_CIA, NPARA =
 * CIA.NPARA, 0 for tables without ortho/para dependence); igas1 / igas2[NPAIR] = index of each partner among the NVMR
 * atmospheric gases, -1 when the pair is not to be used (gas missing or ambiguous :4676-4684, or the pair's INORMALT
 * differs from CIA.INORMAL :4696-4701); per layer temperature, para-H2 fraction, mixing ratios q[L][NVMR] = PP/PRESS
 * and xfac[L] = (TOTAM*1e-4)^2 / (DELH*1e2); ico2 / in2 / ih2 = index of CO2 / N2 / H2 (or -1) with the reference's
 * co2cia / n2n2cia / n2h2cia(WAVEN) vectors (wavenumber-only parametrisations; NULL when the index is -1).
 * -> TAUCIA[W][L], dTAUCIA[W][L][NVMR+2] (NULL to skip).  Reference quirks kept (temp1 overwritten by the upper
 * para-fraction clamp :4623; temperature gradient in slot NVMR-2 :4695). */
int ansfm_calc_tau_cia(ansfm_ctx *ctx, int W, const double *WAVEN, int NWC, const double *cia_waven, int NPAIR,
                       int NPE, int NT, const double *K_CIA, const double *cia_temp, int nfrac,
                       const double *cia_frac, int NPARA, const int32_t *igas1, const int32_t *igas2, int L,
                       int NVMR, const double *lay_temp, const double *lay_frac, const double *q,
                       const double *xfac, int ico2, const double *k_co2, int in2, const double *k_n2n2, int ih2,
                       const double *k_n2h2, double *TAUCIA, double *dTAUCIA);

/* ForwardModel_0.calc_tau_rayleigh (ForwardModel_0.py:4869): mode = IRAY -- 1 calc_tau_rayleighj (:5525, gas giants),
 * 2 calc_tau_rayleighv2 (:5647, CO2), 4 calc_tau_rayleighls (:5712, Jovian air; f4[L][4] = mixing ratios of H2, He, CH4,
 * NH3 per layer, 0 where absent) -- or 12 for calc_tau_rayleighv (:5598, not selected by any IRAY).  WAVEC[W] in the
 * units of ISPACE, TOTAM[L] in m-2 -> TAURAY[W][L], dTAURAY[W][L] (= dTAURAY/dTOTAM). */
int ansfm_calc_tau_rayleigh(ansfm_ctx *ctx, int mode, int ISPACE, int W, const double *WAVEC, int L,
                            const double *TOTAM, const double *f4, double *TAURAY, double *dTAURAY);

/* calc_tau_rayleigh for the n states of a Jacobian batch, on the uploaded table's wavenumber grid, left in HBM:
 * TOTAM[n][L] and (mode 4) f4[n][L][4] are host arrays (a few kB per state), TAURAY_dev[n][W][L] is a DEVICE pointer in
 * the layout ansfm_cirsrad_ck_thermal_dev takes as taucont (8 MB per state at C2 that never cross PCIe). */
int ansfm_calc_tau_rayleigh_batch_dev(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L, const double *TOTAM,
                                      const double *f4, double *TAURAY_dev);
/* ... and with TOTAM / f4 resident on the device too (what ansfm_layer_average_dev left there); asynchronous. */
int ansfm_calc_tau_rayleigh_batch_dev_in(ansfm_ctx *ctx, int mode, int ISPACE, int n_models, int L,
                                         const double *TOTAM_dev, const double *f4_dev, double *TAURAY_dev);

/* ForwardModel_0.calc_tau_dust (ForwardModel_0.py:4790): KEXT / KSCA[NWS][NDUST] tabulated on SWAVE[NWS] (Scatter.WAVE,
 * strictly ascending) interpolated to WAVEC[W] like scipy interp1d(kind='cubic') (not-a-knot spline; linear when
 * NWS == 2; NWS == 3 is refused as scipy refuses it), out-of-range values replaced by the linear interpolant
 * (:4849-4859); CONT[L][NDUST] in particles m-2 (after any DUST_RENORMALISATION, which the caller applies).
 * -> TAUDUST, TAUCLSCAT, dTAUDUSTdq, dTAUCLSCATdq [W][L][NDUST].  A WAVEC outside SWAVE is ANSFM_ERR_INVALID (the
 * reference's interp1d raises ValueError). */
int ansfm_calc_tau_dust(ansfm_ctx *ctx, int W, const double *WAVEC, int NWS, const double *SWAVE, int NDUST,
                        const double *KEXT, const double *KSCA, int L, const double *CONT, double *TAUDUST,
                        double *TAUCLSCAT, double *dTAUDUSTdq, double *dTAUCLSCATdq);

/* Continuum sources resident in the context, like the table and on its wavenumber grid, for
 * ansfm_cirsrad_ck_thermal_cont_dev.  Uploading a k-table or LBL table (or committing a line source) clears both.
 * ansfm_upload_cia: everything of ansfm_calc_tau_cia that does not depend on the layers.  The CIA table is evaluated at
 * x = WAVE[w] (ISPACE 0) or 1e4 / WAVE[w] (ISPACE 1; interp1d is pointwise, so the reference's sort and un-sort :4565-4568 /
 * :4741-4743 change no value); k_co2 / k_n2n2 / k_n2h2[W] are co2cia / n2n2cia / n2h2cia at that x, in the order of the
 * table's grid.  The `covers` test (:4671) is made here on the range of x.  ANSFM_ERR_UNSUPPORTED for a table whose para-H2
 * bracket could leave K_CIA for some layer (NPARA > 0 without NPARA == nfrac == NPE >= 2): the per-layer IndexError of
 * ansfm_calc_tau_cia cannot arise on the device. */
int ansfm_upload_cia(ansfm_ctx *ctx, int ISPACE, int NWC, const double *cia_waven, int NPAIR, int NPE, int NT,
                     const double *K_CIA, const double *cia_temp, int nfrac, const double *cia_frac, int NPARA,
                     const int32_t *igas1, const int32_t *igas2, int NVMR, int ico2, const double *k_co2, int in2,
                     const double *k_n2n2, int ih2, const double *k_n2h2);
/* ansfm_upload_dust: the extinction cross sections KEXT[NWS][NDUST] on SWAVE evaluated on the table's grid exactly as
 * ansfm_calc_tau_dust evaluates them (KSCA[NWS][NDUST] decides with KEXT where the linear interpolant replaces the spline,
 * :4849-4859; NULL: zeros) and kept as kext_w[NDUST][Wpad]; the scattering cross sections, evaluated by the same body in the
 * same launch, are kept beside them as ksca_w[NDUST][Wpad] for ansfm_cirsrad_ck_scatter_batch_cont.  NDUST > 7 is ANSFM_ERR_UNSUPPORTED: NumPy sums eight and more
 * populations pairwise, fewer in order, and the fused entry sums in order. */
int ansfm_upload_dust(ansfm_ctx *ctx, int NWS, const double *SWAVE, int NDUST, const double *KEXT, const double *KSCA);
int ansfm_clear_continuum_sources(ansfm_ctx *ctx);

/* Layer de-duplication inside a batch (n_models > 1) of the cirsrad_ck_thermal entry points.  The states of a
 * numerical Jacobian (ForwardModel_0.jacobian_nemesis :2234-2242) differ from the unperturbed one in two or three
 * layers; every layer (m, l) whose pressure, temperature and S amounts equal those of layer l of model 0 to the last
 * bit shares its gas opacity with it instead of being merged again.  Results are bit-identical with and without;
 * on by default; costs one stream synchronisation per batched call.  ansfm_last_layer_rows reports how many layer
 * opacities the last call computed out of n_models * L. */
int ansfm_set_layer_dedup(ansfm_ctx *ctx, int enable);
int ansfm_last_layer_rows(const ansfm_ctx *ctx, int *rows_computed, int *rows_total);

/* *shared = 1 when the last thermal-emission or single-scattering batch started the paths of its states from the records state 0 left behind
 * (a de-duplicated batch of at least 4 states: every state shares the top of each path with state 0 up to the first layer
 * whose opacity row, continuum, SCALE or EMTEMP differs; bit-identical; ANSFM_RT_PREFIX=0 switches it off). */
int ansfm_last_rt_shared(const ansfm_ctx *ctx, int *shared);

/* Row-head list of the forward random-overlap merge (k_overlap / rank, ForwardModel_0.py:6029-6173): bits = 64 (default)
 * orders the heads on double keys (k_ck_overlap: values closer than 2^-41 count as ties); bits = 32 on float32 keys
 * (k_ck_overlap32: heads whose float32 values coincide are settled by their exact double sums, every merge carries a
 * check that the sums were consumed in non-decreasing order and is rerun exactly when it was not).  Both produce the
 * reference's merged order.  Measured on MI355X: the 32-bit kernel issues fewer instructions but
 * exposes more LDS latency and is the slower of the two at C2, hence opt-in.  Input that is unsorted or negative runs
 * on the generic 64-bit path either way. */
int ansfm_set_merge_keys(ansfm_ctx *ctx, int bits);
/* Statistics of the 32-bit-key kernel: (wave, gas) merges whose fast pass did not consume the sums in non-decreasing
 * order and were rerun with every step popping the exact minimum; counted since the last table upload. */
int ansfm_merge_redo_count(ansfm_ctx *ctx, int64_t *count);

/* Vertical gas opacity of the last cirsrad call's first model, TAUGAS[W][G][L]
 * (what CIRSrad leaves in LayerX.TAUGAS, ForwardModel_0.py:3925) -- host pointer out. */
int ansfm_get_taugas(ansfm_ctx *ctx, int model, double *TAUGAS);

/* ---- Mie theory over a particle size distribution ------------------------------------------------------------------------
 * Scatter_0.makephase (module level, Scatter_0.py:1828) = miescat (:1600) over dmie (:1399) for iscat 1 gamma, 2 log-normal,
 * 3 MCS modified gamma, 4 single size: what model 444 recomputes in every forward model.  wavel_um[nwave], dsize[3], rs[3] =
 * first radius, last radius, step (um; rs[1] < rs[0]: open range, ended -- that radius included -- by the first radius at or
 * beyond the distribution's peak whose n(r) Q_sca is at most 1e-6 of its running maximum), refindx[nwave][2] = real and
 * imaginary part, theta_deg[ntheta] within [0, 90] ascending -> xscat / xext[nwave] (cm2) and phas[nwave][nphas] =
 * lambda^2 sum / (pi k_sca) over the angles theta followed by 180 - theta in ascending order (nphas = 2 ntheta - 1 when
 * 90 degrees is among them, else 2 ntheta): what miescat returns, before the class method divides by 4 pi.
 * n_radii[nwave] (may be NULL): the radii each wavelength integrated over.
 * The radii are processed in blocks (ansfm_mie_set_radius_block: a multiple of 64, 0 = the default 512); the sum over radii
 * has one order -- chunks of 64 radii from radius 0, a fixed tree inside a chunk, chunks in ascending order -- so the block
 * size changes no bit.  An open range that has not ended after the cap (ansfm_mie_set_radius_cap, 0 = the default 2^20
 * radii) is ANSFM_ERR_INVALID "size integration did not terminate" (the reference would loop to 10^9).
 * ANSFM_ERR_INVALID with the wavelength and radius in the text also where the reference gives up: nmx1 = int(1.1 |m| x) >=
 * 29999, or a series that needs more than nmx2 = max(135, int(|m| x)) terms; and for an angle outside [0, 90] or iscat
 * outside 1 .. 4.  ansfm_mie_last: kernel milliseconds, blocks and the largest block of the last call. */
int ansfm_mie_makephase(ansfm_ctx *ctx, int nwave, const double *wavel_um, int iscat, const double dsize[3], const double rs[3],
                        const double *refindx, int ntheta, const double *theta_deg, double *xscat, double *xext, double *phas,
                        int32_t *n_radii);
int ansfm_mie_set_radius_block(ansfm_ctx *ctx, int radii);
int ansfm_mie_set_radius_cap(ansfm_ctx *ctx, int radii);
int ansfm_mie_last(const ansfm_ctx *ctx, double *kernel_ms, int32_t *blocks, int32_t *block_radii);

/* ---- Double Henyey-Greenstein fit of a phase function --------------------------------------------------------------------
 * Scatter_0.subfithgm (Scatter_0.py:1948): what the class method Scatter_0.makephase runs after the Mie integration when
 * IMIE = 0 (:1366).  theta_deg[nphase], phase[nfit][nphase] (normalised to 4 pi, as makephase hands it over) -> f, g1, g2,
 * rms[nfit]: per fit a Levenberg-Marquardt chain from (0.5, 0.5, -0.5) against log(phase), with the reference's finite
 * differences (dx = 0.01 and its sign flips), clips (f in [1e-6, 0.999999], g1 in [0, 0.98], g2 in [-0.98, -0.1]), damping
 * (alamda from 1000, times 0.9 when accepted, times 1.5 up to 1e36 when not) and stopping rule (more than 5 accepted calls in
 * a row with a relative change of chisq below 1e-8, or 1000 calls); rms = sqrt(chisq).  counts[nfit][2] (may be NULL): the
 * calls of mrqminl a fit took and how many were accepted.
 * One wavefront per fit; the sums over the angles have one order (per lane the angles i, i + 64, ... ascending, then a fixed
 * tree over the lanes), so a fit's bits do not depend on the fits beside it.  The normal equations are solved by Gaussian
 * elimination with partial pivoting where the reference inverts the matrix: the results agree to the 1e-8 the stopping rule
 * defines them to, the counts need not.  A phase function with a 0 or a NaN gives what the reference gives (the start point
 * and rms = inf or NaN); nothing is checked about the values.
 * ANSFM_ERR_INVALID, before anything is launched, for nfit outside 1 .. 2^20, nphase outside 1 .. 8192 or a null pointer;
 * and, naming the fit, where the elimination meets an exact zero pivot (the reference ends in "Singular matrix" there).
 * ansfm_hg_fit_last: kernel milliseconds of the last call. */
int ansfm_hg_fit(ansfm_ctx *ctx, int nfit, int nphase, const double *theta_deg, const double *phase, double *f, double *g1,
                 double *g2, double *rms, int32_t *counts);
int ansfm_hg_fit_last(const ansfm_ctx *ctx, double *kernel_ms);

/* ---- Aerosol phase functions on the calculation grid --------------------------------------------------------------------
 * Scatter_0.calc_phase (Scatter_0.py:760) and calc_phase_ray (:834).  imie selects what tab holds on SWAVE [NWS] (Scatter.WAVE,
 * strictly ascending, in the units of the calculation grid):
 *   0 HENYEY_GREENSTEIN     F, G1, G2 as [3][NWS][NDUST]; NTAB and THETA_TAB are ignored (calc_hgphase :699)
 *   1 MIE_THEORY            PHASE [NWS][NTAB][NDUST] on THETA_TAB [NTAB] (Scatter.THETA), interpolated in angle (interp_phase :732)
 *   2 LEGENDRE_POLYNOMIALS  WLPOL [NWS][NTAB = NLPOL][NDUST]; THETA_TAB is ignored (calc_lpphase :1060)
 * ansfm_calc_phase: theta_deg [nth], WAVEC [W] -> phase [W][nth][NDUST].  phase1 on the aerosol grid, then linear along the
 * wavenumbers with the end intervals extrapolating; both interpolations are interp1d's (searchsorted 'left' clipped to
 * 1 .. n - 1, slope * (x - x_lo) + y_lo).  One lane per (wavenumber, angle); no expression contracts into an fma, so that the
 * results differ from NumPy's only where cos and pow do, and imie = 1, which has neither, is the reference bit for bit.
 * ANSFM_ERR_INVALID, before anything is launched: a null pointer; NWS < 2, nth < 1, W < 1, NDUST < 1, NTAB < 1 (< 2 for imie
 * 1); SWAVE not strictly ascending; imie 1 with THETA_TAB not strictly ascending or a theta_deg outside it (the reference's
 * interp1d raises); the reference's range test, SWAVE[0] > (1 + 1e-6) min(WAVEC) or SWAVE[NWS - 1] < (1 - 1e-6) max(WAVEC);
 * an imie outside 0 .. 2.
 * ansfm_calc_phase_ray: 0.75 (1 + cos^2 theta) / (4 pi) at theta_deg [nth].
 * ansfm_phase_last: kernel milliseconds of the last ansfm_calc_phase, ansfm_calc_phase_ray or ansfm_phase_from_source.
 *
 * ansfm_upload_phase makes the tables a resident source on the uploaded table's grid, beside ansfm_upload_dust: the tables go
 * to HBM, every wavenumber's interval (lo, x_lo, x_hi) is found once, and for imie 0 f_w, g1_w, g2_w [NDUST][Wpad] are formed
 * by np.interp's rule (a node returns its tabulated value, the ends clamp, slope * (x - x_j) + y_j in between: np.interp's
 * bits).  The range test is made on the table's grid.  NDUST > 7 is ANSFM_ERR_UNSUPPORTED, as for ansfm_upload_dust.  A new
 * table, a committed line source and ansfm_clear_continuum_sources clear the source.
 * ansfm_phase_from_source: phase [W][nth][NDUST] on the table's grid, bit-identical to ansfm_calc_phase with WAVEC = that grid.
 * ansfm_phasarr_from_source: the array ansfm_cirsrad_ck_scatter_batch_src forms (described there), [NDUST][W][2][nth], nth >= 3.
 * Both: ANSFM_ERR_INVALID without a source, and for the angles as above.
 * ansfm_phase_source_info: imie and NDUST of the source that stands (-1 and 0: none); a caller sizes the results by it. */
int ansfm_calc_phase(ansfm_ctx *ctx, int imie, int NWS, const double *SWAVE, int NDUST, int NTAB, const double *THETA_TAB,
                     const double *tab, int nth, const double *theta_deg, int W, const double *WAVEC, double *phase);
int ansfm_calc_phase_ray(ansfm_ctx *ctx, int nth, const double *theta_deg, double *phase);
int ansfm_phase_last(const ansfm_ctx *ctx, double *kernel_ms);
int ansfm_upload_phase(ansfm_ctx *ctx, int imie, int NWS, const double *SWAVE, int NDUST, int NTAB, const double *THETA_TAB,
                       const double *tab);
int ansfm_phase_source_info(const ansfm_ctx *ctx, int *imie, int *NDUST);
int ansfm_phase_from_source(ansfm_ctx *ctx, int nth, const double *theta_deg, double *phase);
int ansfm_phasarr_from_source(ansfm_ctx *ctx, int nth, const double *theta_deg, const double *mu_theta, double *phasarr);

/* ---- Surface reflection ----------------------------------------------------------------------------------------------------
 * lowbc takes the values of LowerBoundaryConditionEnum and decides the rows of params[npar][nwave]:
 *   1 LAMBERTIAN  the albedo
 *   2 HAPKE       the ten arguments of calc_Hapke_BRDF (Surface_0.py:1292) in its order: w, K, BS0, hs, BC0, hc, ROUGHNESS,
 *                 G1, G2, F
 *   3 OREN_NAYAR  A, ROUGHNESS (calc_OrenNayar_BRDF :1743)
 * -- the parameters on the calculation wavenumbers, i.e. after the np.interp of Surface_0.calc_BRDF (:944-971).
 *
 * ansfm_surface_brdf: Surface_0.calc_BRDF (:916) at ntheta angle triples (solar zenith, emission, azimuth; degrees, the
 * azimuth in the reference's convention: 180 is backscattering) -> brdf[nwave][ntheta].  Hapke: 0 where an angle is >= 90.
 *
 * ansfm_brdf_matrix: ForwardModel_0.calc_brdf_matrix (ForwardModel_0.py:5168) -> brdf_mat[nwave][nmu][nmu][nf + 1], indexed
 * [w][emission i][solar j][Fourier order]: for HAPKE the sum over the azimuth nodes k = 0 .. nphi, in that order, of
 * wphi[k] BRDF(ang[j], ang[i], azi[k]) cos(ic k dphi); for LAMBERTIAN plane 0 = albedo / pi and zeros above; for 0 and 3 zeros
 * (params and the tables may be NULL then), as the reference returns.  The tables are the caller's, in the reference's own
 * expressions, so that the exact comparisons of the point function see the reference's bits:
 *   ang_deg[nmu]         arccos(MU[::-1]) * 180 / pi
 *   azi_deg[nphi + 1]    (k dphi) * 180 / pi, dphi = 2 pi / nphi  (with nphi = 100 the last one is 360.00000000000006)
 *   phix_deg[nphi + 1]   180 - azi_deg folded into [0, 180] (:1363-1381); checked against azi_deg
 *   wphi[nphi + 1]       dphi / (2 pi), (0.5 dphi) / (2 pi) at both ends
 *   cosk[nf + 1][nphi + 1]  cos(ic (k dphi))
 * nf <= 32.  ANSFM_ERR_INVALID, before anything is launched, for an unknown lowbc, sizes out of range, a null pointer or a
 * phix that is not the fold of its azimuth.  ansfm_brdf_last: kernel milliseconds of the last call of either. */
int ansfm_surface_brdf(ansfm_ctx *ctx, int lowbc, int nwave, const double *params, int ntheta, const double *sol_ang,
                       const double *emiss_ang, const double *azi_ang, double *brdf);
int ansfm_brdf_matrix(ansfm_ctx *ctx, int lowbc, int nwave, const double *params, int nmu, const double *ang_deg, int nphi, int nf,
                      const double *azi_deg, const double *phix_deg, const double *wphi, const double *cosk, double *brdf_mat);
int ansfm_brdf_last(const ansfm_ctx *ctx, double *kernel_ms);

/* ---- measurement helpers (bench.py / profiling) -------------------------------------------
 * Time of the dominant kernel (ck_overlap) measured with hipEvents on the ctx stream around
 * the launches of the last cirsrad call: total milliseconds and number of launches. */
int ansfm_last_kernel_ms(const ansfm_ctx *ctx, double *overlap_ms, int *overlap_launches,
                         double *rt_ms, int *rt_launches);

#ifdef __cplusplus
}
#endif
#endif /* ANSFM_H */

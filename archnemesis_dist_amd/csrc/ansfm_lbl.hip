// ansfm_lbl.hip -- runtime line-by-line of libansfm.so: line sets and pseudo-continuum on a grid, the accumulator of a gas,
// the line source resident in the context.  gfx950 only.
#include "ansfm_lbl_kernels.hip.h"
#include "ansfm_lbl_pc_kernels.hip.h"
#include "ansfm_lblrt_kernels.hip.h"
#include "ansfm_ctx.hip.h"

using namespace ansfm;

void ansfm::launch_lblrt_tau(ansfm_ctx *ctx, int n, int L, int m0, const double *amount, double *dk)
{
    hipLaunchKernelGGL(k_lblrt_tau, dim3(nblk((size_t)n * L * ctx->Wpad, 256)), dim3(256), 0, ctx->stream, ctx->rt_k.as<double>(),
                       ctx->st_H, ctx->W, ctx->Wpad, ctx->S, L, n, ctx->rt_krow.as<int32_t>() + (size_t)m0 * ctx->S * L, amount,
                       ctx->tau.as<double>(), dk);
}

static int lbl_shape_built(ansfm_ctx *ctx, int lineshape_id)
{
    if (lineshape_id != 0 && lineshape_id != 4 && lineshape_id != 12)
        FAIL(ANSFM_ERR_UNSUPPORTED, "lineshape: VOIGT (0), LORENTZ (4), DOPPLER (12) are built");   // enum map raises NotImplementedError
    return ANSFM_OK;
}

static int lbl_grid_ascending(ansfm_ctx *ctx, int nw, const double *wn_grid)
{
    for (int j = 1; j < nw; ++j)
        if (wn_grid[j] < wn_grid[j - 1]) FAIL(ANSFM_ERR_INVALID, "wn_grid must be ascending (LineData_0.py:230)");
    return ANSFM_OK;
}

// Lines sorted by wavenumber for the windowed gather (the reference accepts any order; summation order then differs from it
// only in rounding): h = nu, sw, e_lower, stim_ref [N], bparams [3M][N] in sorted order, ord[i] = the caller's index of line i
static void lbl_pack_lines(int M, int N, const double *broadening_params, const double *nu, const double *sw,
                           const double *e_lower, const double *stim_ref, std::vector<int> &ord, std::vector<double> &h)
{
    ord.resize(N);
    for (int i = 0; i < N; ++i) ord[i] = i;
    bool sorted = true;
    for (int i = 1; i < N; ++i) if (nu[i] < nu[i - 1]) { sorted = false; break; }
    if (!sorted) std::stable_sort(ord.begin(), ord.end(), [&](int a, int b) { return nu[a] < nu[b]; });
    h.resize((size_t)(4 + 3 * M) * N);
    double *hnu = h.data(), *hsw = hnu + N, *hel = hsw + N, *hsr = hel + N, *hbp = hsr + N;
    for (int i = 0; i < N; ++i) {
        const int o = ord[i];
        hnu[i] = nu[o]; hsw[i] = sw[o]; hel[i] = e_lower[o]; hsr[i] = stim_ref[o];
        for (int r = 0; r < 3 * M; ++r) hbp[(size_t)r * N + i] = broadening_params[(size_t)r * N + o];
    }
}

// The geometry of the pseudo-continuum bins on a grid, with the reference's expressions: first / last (:399-416), the largest
// touched grid point (j_max :463; the touched points of a bin are a run, because (wn - c)/w does not decrease along an
// ascending grid), the lower edges and the largest width
struct PcGeometry {
    std::vector<double> lo;
    int first = -1, last = -1, jmax = 0;
    double wmax = 0.0;
};
static int lbl_pc_geometry(ansfm_ctx *ctx, int nw, const double *h_grid, int N, const double *centers, const double *widths,
                           PcGeometry &g)
{
    g.lo.resize(N);
    for (int i = 0; i < N; ++i) {
        const double c = centers[i], w = widths[i];
        if (!(w > 0.0)) FAIL(ANSFM_ERR_INVALID, "pseudo-continuum: bin widths must be positive");
        const double bin_min = c - w / 2.0, bin_max = c + w / 2.0;
        if (i > 0 && !(bin_min >= g.lo[i - 1]))
            FAIL(ANSFM_ERR_INVALID, "pseudo-continuum: the lower bin edges centre - width / 2 must be ascending");
        g.lo[i] = bin_min;
        if (g.first == -1 && bin_min <= h_grid[0]) g.first = i;
        if (g.last == -1 && bin_max > h_grid[nw - 1]) g.last = i;
        if (w > g.wmax) g.wmax = w;
        int a = 0, b = nw;      // first j with (wn_j - c)/w >= 0.5
        while (a < b) { const int mid = (a + b) >> 1; if ((h_grid[mid] - c) / w < 0.5) a = mid + 1; else b = mid; }
        if (a > 0 && (h_grid[a - 1] - c) / w >= -0.5 && a - 1 > g.jmax) g.jmax = a - 1;
    }
    if (g.first == -1) g.first = N;
    if (g.last == -1) g.last = N;
    return ANSFM_OK;
}

// The launches of a filled LblParams: the records of its L points x N lines into p.store / p.shift, then their sum onto p.out
static int lbl_launch_lines(ansfm_ctx *ctx, const LblParams &p)
{
    const int nw = p.nw, N = p.N, L = p.L;
    hipLaunchKernelGGL(k_lbl_line_params, dim3(nblk((size_t)L * N, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_lbl_accumulate, dim3(nblk(nw, 256 * kLblPts), (unsigned)L), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    return ANSFM_OK;
}

// The launches of a filled PcParams: the records of its L points x N bins into p.store / p.x / p.ysum / p.y, then the
// interpolation of the grid points below jmax onto p.out
static int lbl_launch_pc(ansfm_ctx *ctx, const PcParams &p)
{
    const int L = p.L, jmax = p.jmax;
    const size_t LN = (size_t)L * p.N;
    hipLaunchKernelGGL(k_pc_params, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pc_shapes, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    hipLaunchKernelGGL(k_pc_gather, dim3(nblk(LN, 256)), dim3(256), 0, ctx->stream, p);
    HIPCHK(hipGetLastError());
    if (jmax > 0) {
        hipLaunchKernelGGL(k_pc_interp, dim3(nblk((size_t)jmax, 256), nblk((size_t)L, kPcLayers)), dim3(256), 0, ctx->stream, p);
        HIPCHK(hipGetLastError());
    }
    return ANSFM_OK;
}

// The lines of one isotopologue onto d_out[L][nw] in HBM.  d_grid / d_t / d_p: device copies of the grid and the (T, p)
// points (h_p: the pressures on the host); everything else is staged here, from st's next slot on.  Arguments are checked.
static int lbl_lines_dev(ansfm_ctx *ctx, Stager &st, int nw, const double *d_grid, int lineshape_id, int L, const double *d_t,
                         double t_ref, const double *d_p, const double *h_p, double p_ref, const double *q_ratio,
                         double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                         const double *broadening_params, const double *nu, const double *sw, const double *e_lower,
                         const double *stim_ref, double *d_out, double *store, double s_floor, double wn_calc_window,
                         double wn_approx_window)
{
    std::vector<int> ord;
    std::vector<double> h;
    lbl_pack_lines(M, N, broadening_params, nu, sw, e_lower, stim_ref, ord, h);
    double dmax = 0.0;
    for (int o = 0; o < N; ++o) {
        double d = 0.0;
        for (int j = 0; j < M; ++j) d += fabs(broadening_params[(size_t)(3 * j + 2) * N + o] * mol_mix_frac[j]);
        if (d > dmax) dmax = d;
    }
    double pmax = 0.0;
    for (int l = 0; l < L; ++l) if (fabs(h_p[l] / p_ref) > pmax) pmax = fabs(h_p[l] / p_ref);
    const size_t D = sizeof(double);
    LblParams p;
    memset(&p, 0, sizeof p);
    const double *dl = st.up(h.data(), h.size());
    p.mmf = st.up(mol_mix_frac, M);
    p.q_ratio = st.up(q_ratio, L);
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h is a local buffer
    HIPCHK(ctx->misc.reserve((size_t)L * (kLblRows + 1) * N * D));
    p.wn_grid = d_grid; p.t_calc = d_t; p.p_calc = d_p; p.out = d_out;
    p.nu = dl; p.sw = dl + N; p.e_lower = dl + 2 * (size_t)N; p.stim_ref = dl + 3 * (size_t)N; p.bparams = dl + 4 * (size_t)N;
    p.store = ctx->misc.as<double>();
    p.shift = p.store + (size_t)L * kLblRows * N;
    p.nw = nw; p.N = N; p.M = M; p.L = L; p.lineshape_id = lineshape_id;
    p.t_ref = t_ref; p.p_ref = p_ref; p.iso_abundance = isotopic_abundance; p.iso_mass = isotopic_mass; p.s_floor = s_floor;
    p.wn_calc_window = wn_calc_window; p.wn_approx_window = wn_approx_window;
    p.max_shift = dmax * pmax * 1.0000001 + 1e-12;
    const int rc = lbl_launch_lines(ctx, p);
    if (rc) return rc;
    if (store) {   // store[L][4][N] = strength, alpha_d, gamma_l, shift in the caller's line order
        std::vector<double> hst((size_t)L * (kLblRows + 1) * N);
        HIPCHK(hipMemcpyAsync(hst.data(), p.store, hst.size() * D, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        static const int src[3] = {0, 6, 7};
        const double *hsh = hst.data() + (size_t)L * kLblRows * N;
        for (int l = 0; l < L; ++l)
            for (int i = 0; i < N; ++i) {
                const double *rec = hst.data() + ((size_t)l * N + i) * kLblRows;
                for (int r = 0; r < 3; ++r) store[((size_t)l * 4 + r) * N + ord[i]] = rec[src[r]];
                store[((size_t)l * 4 + 3) * N + ord[i]] = hsh[(size_t)l * N + i];
            }
    }
    return ANSFM_OK;
}

// The pseudo-continuum of one isotopologue onto d_out[L][nw] in HBM; h_grid: the grid on the host, for the bin geometry.
static int lbl_pc_dev(ansfm_ctx *ctx, Stager &st, int nw, const double *d_grid, const double *h_grid, int lineshape_id, int L,
                      const double *d_t, double t_ref, const double *d_p, double p_ref, const double *q_ratio,
                      double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                      const double *bparams, const double *centers, const double *widths, const double *sw_sum,
                      const double *e_lower, double *d_out, double *store, double *store_x, int nb)
{
    PcGeometry g;
    const int grc = lbl_pc_geometry(ctx, nw, h_grid, N, centers, widths, g);
    if (grc) return grc;
    const std::vector<double> &lo = g.lo;
    const int first = g.first, last = g.last, jmax = g.jmax;
    const double wmax = g.wmax;
    const size_t D = sizeof(double), LN = (size_t)L * N;
    PcParams p;
    memset(&p, 0, sizeof p);
    p.centers = st.up(centers, N); p.widths = st.up(widths, N); p.sw = st.up(sw_sum, N); p.e_lower = st.up(e_lower, N);
    p.lo = st.up(lo.data(), N); p.bparams = st.up(bparams, (size_t)3 * M * N);
    p.mmf = st.up(mol_mix_frac, M); p.q_ratio = st.up(q_ratio, L);
    if (st.rc) return st.rc;
    HIPCHK(hipStreamSynchronize(ctx->stream));   // lo is a local buffer
    HIPCHK(ctx->misc.reserve(LN * (size_t)(3 + (2 * nb + 1) + 2) * D));
    p.wn_grid = d_grid; p.t_calc = d_t; p.p_calc = d_p; p.out = d_out;
    p.store = ctx->misc.as<double>();
    p.x = p.store + 3 * LN; p.ysum = p.x + LN; p.y = p.ysum + LN;
    p.nw = nw; p.N = N; p.M = M; p.L = L; p.lineshape_id = lineshape_id; p.nb = nb;
    p.first = first; p.last = last; p.jmax = jmax;
    p.t_ref = t_ref; p.p_ref = p_ref; p.iso_abundance = isotopic_abundance; p.iso_mass = isotopic_mass; p.wmax = wmax;
    const int rc = lbl_launch_pc(ctx, p);
    if (rc) return rc;
    if (store) HIPCHK(hipMemcpyAsync(store, p.store, 3 * LN * D, hipMemcpyDeviceToHost, ctx->stream));
    if (store_x) HIPCHK(hipMemcpyAsync(store_x, p.x, LN * D, hipMemcpyDeviceToHost, ctx->stream));
    if (store || store_x) HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

static int lbl_pc_args(ansfm_ctx *ctx, int lineshape_id, int M, int N, const double *q_ratio, const double *mol_mix_frac,
                       const double *bparams, const double *centers, const double *widths, const double *sw_sum,
                       const double *e_lower, int nb)
{
    if (M <= 0 || N < 0 || nb < 0 || !q_ratio || !mol_mix_frac || (N > 0 && (!bparams || !centers || !widths || !sw_sum || !e_lower)))
        FAIL(ANSFM_ERR_INVALID, "add_pseudo_continuum_monochromatic_absorption: bad argument");
    if (nb > kPcMaxNeighbours) FAIL(ANSFM_ERR_UNSUPPORTED, "pseudo-continuum: n_neighbour_bins 0 .. 8 are built");
    return lbl_shape_built(ctx, lineshape_id);
}

extern "C" {

int ansfm_add_line_set_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance, double isotopic_mass, int M,
    const double *mol_mix_frac, int N, const double *broadening_params, const double *nu, const double *sw,
    const double *e_lower, const double *stim_ref, double *out, double *store, double s_floor, double wn_calc_window,
    double wn_approx_window)
{
    CHECK_CTX(ctx);
    if (nw <= 0 || L <= 0 || M <= 0 || N < 0 || !wn_grid || !t_calc || !p_calc || !q_ratio || !mol_mix_frac || !out ||
        (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)))
        FAIL(ANSFM_ERR_INVALID, "add_line_set_monochromatic_absorption: bad argument");
    int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc || (rc = lbl_grid_ascending(ctx, nw, wn_grid))) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_grid = st.up(wn_grid, nw), *d_t = st.up(t_calc, L), *d_p = st.up(p_calc, L);
    double *d_out = const_cast<double *>(st.up(out, (size_t)L * nw));     // accumulated onto
    if (st.rc) return st.rc;
    rc = lbl_lines_dev(ctx, st, nw, d_grid, lineshape_id, L, d_t, t_ref, d_p, p_calc, p_ref, q_ratio, isotopic_abundance,
                       isotopic_mass, M, mol_mix_frac, N, broadening_params, nu, sw, e_lower, stim_ref, d_out, store, s_floor,
                       wn_calc_window, wn_approx_window);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)L * nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_add_pseudo_continuum_monochromatic_absorption(
    ansfm_ctx *ctx, int nw, const double *wn_grid, int lineshape_id, int L, const double *t_calc, double t_ref,
    const double *p_calc, double p_ref, const double *q_ratio, double isotopic_abundance, double isotopic_mass, int M,
    const double *mol_mix_frac, int N, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
    const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower, double *out, double *store,
    double *store_x, int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (nw <= 0 || L <= 0 || !wn_grid || !t_calc || !p_calc || !out)
        FAIL(ANSFM_ERR_INVALID, "add_pseudo_continuum_monochromatic_absorption: bad argument");
    int rc = lbl_pc_args(ctx, lineshape_id, M, N, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers,
                         wn_bin_widths, sw_sum, lsw_mean_e_lower, n_neighbour_bins);
    if (rc || (rc = lbl_grid_ascending(ctx, nw, wn_grid))) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const double *d_grid = st.up(wn_grid, nw), *d_t = st.up(t_calc, L), *d_p = st.up(p_calc, L);
    double *d_out = const_cast<double *>(st.up(out, (size_t)L * nw));     // accumulated onto
    if (st.rc) return st.rc;
    rc = lbl_pc_dev(ctx, st, nw, d_grid, wn_grid, lineshape_id, L, d_t, t_ref, d_p, p_ref, q_ratio, isotopic_abundance,
                    isotopic_mass, M, mol_mix_frac, N, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                    lsw_mean_e_lower, d_out, store, store_x, n_neighbour_bins);
    if (rc) return rc;
    HIPCHK(hipMemcpyAsync(out, d_out, (size_t)L * nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

/* ---- the opacity of a gas in HBM: the sum over its isotopologues of lines and pseudo-continuum -------------------------- */
int ansfm_lbl_accum_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int L, const double *t_calc, const double *p_calc)
{
    CHECK_CTX(ctx);
    ctx->acc_nw = ctx->acc_L = 0;
    if (nw <= 0 || L <= 0 || !wn_grid || !t_calc || !p_calc) FAIL(ANSFM_ERR_INVALID, "lbl_accum_begin: bad argument");
    const int rc = lbl_grid_ascending(ctx, nw, wn_grid);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    const size_t D = sizeof(double);
    HIPCHK(ctx->acc.reserve((size_t)L * nw * D));
    HIPCHK(ctx->acc_grid.reserve((size_t)nw * D));
    HIPCHK(ctx->acc_tp.reserve((size_t)2 * L * D));
    ctx->acc_h_grid.assign(wn_grid, wn_grid + nw);
    ctx->acc_h_p.assign(p_calc, p_calc + L);
    HIPCHK(hipMemsetAsync(ctx->acc.p, 0, (size_t)L * nw * D, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_grid.p, ctx->acc_h_grid.data(), (size_t)nw * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_tp.p, t_calc, (size_t)L * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipMemcpyAsync(ctx->acc_tp.as<double>() + L, p_calc, (size_t)L * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // t_calc / p_calc are the caller's
    ctx->acc_nw = nw; ctx->acc_L = L;
    return ANSFM_OK;
}

int ansfm_lbl_accum_add_lines(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                              double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac, int N,
                              const double *broadening_params, const double *nu, const double *sw, const double *e_lower,
                              const double *stim_ref, double *store, double s_floor, double wn_calc_window,
                              double wn_approx_window)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_lines: call ansfm_lbl_accum_begin first");
    if (M <= 0 || N < 0 || !q_ratio || !mol_mix_frac || (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)))
        FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_lines: bad argument");
    const int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const int L = ctx->acc_L;
    return lbl_lines_dev(ctx, st, ctx->acc_nw, ctx->acc_grid.as<double>(), lineshape_id, L, ctx->acc_tp.as<double>(), t_ref,
                         ctx->acc_tp.as<double>() + L, ctx->acc_h_p.data(), p_ref, q_ratio, isotopic_abundance, isotopic_mass, M,
                         mol_mix_frac, N, broadening_params, nu, sw, e_lower, stim_ref, ctx->acc.as<double>(), store, s_floor,
                         wn_calc_window, wn_approx_window);
}

int ansfm_lbl_accum_add_pseudo_continuum(ansfm_ctx *ctx, int lineshape_id, double t_ref, double p_ref, const double *q_ratio,
                                         double isotopic_abundance, double isotopic_mass, int M, const double *mol_mix_frac,
                                         int N, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                         const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                         double *store, double *store_x, int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_add_pseudo_continuum: call ansfm_lbl_accum_begin first");
    const int rc = lbl_pc_args(ctx, lineshape_id, M, N, q_ratio, mol_mix_frac, lsw_mean_broadening_params, wn_bin_centers,
                               wn_bin_widths, sw_sum, lsw_mean_e_lower, n_neighbour_bins);
    if (rc) return rc;
    if (N == 0) return ANSFM_OK;
    HIPCHK(hipSetDevice(ctx->device));
    Stager st{ctx};
    const int L = ctx->acc_L;
    return lbl_pc_dev(ctx, st, ctx->acc_nw, ctx->acc_grid.as<double>(), ctx->acc_h_grid.data(), lineshape_id, L,
                      ctx->acc_tp.as<double>(), t_ref, ctx->acc_tp.as<double>() + L, p_ref, q_ratio, isotopic_abundance,
                      isotopic_mass, M, mol_mix_frac, N, lsw_mean_broadening_params, wn_bin_centers, wn_bin_widths, sw_sum,
                      lsw_mean_e_lower, ctx->acc.as<double>(), store, store_x, n_neighbour_bins);
}

int ansfm_lbl_accum_read(ansfm_ctx *ctx, double *out)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_read: call ansfm_lbl_accum_begin first");
    if (!out) FAIL(ANSFM_ERR_INVALID, "lbl_accum_read: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipMemcpyAsync(out, ctx->acc.p, (size_t)ctx->acc_L * ctx->acc_nw * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_lbl_accum_device_ptr(ansfm_ctx *ctx, double **dev, int *L, int *nw)
{
    CHECK_CTX(ctx);
    if (ctx->acc_nw <= 0) FAIL(ANSFM_ERR_INVALID, "lbl_accum_device_ptr: call ansfm_lbl_accum_begin first");
    if (!dev) FAIL(ANSFM_ERR_INVALID, "lbl_accum_device_ptr: bad argument");
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // the caller may read the buffer from another stream
    *dev = ctx->acc.as<double>();
    if (L) *L = ctx->acc_L;
    if (nw) *nw = ctx->acc_nw;
    return ANSFM_OK;
}


/* ---- the line source resident in the context: runtime line-by-line as the opacity source of CIRSrad -------------------- */
} // extern "C"

// k rows of R distinct (gas, p, T, mix) rows into ctx->rt_k [R][H][nw] (H = 2: the (T + 5 K, p) spectrum behind every row):
// per gas, its rows are one batch of (T, p) points through the line and pseudo-continuum kernels, isotopologue by
// isotopologue -- lines_0, continuum_0, lines_1, ... onto one zeroed buffer (calc_klblg_online's order, LineData_0.py
// :2395-2459).  The points run in chunks whose constants fit ctx->rt_budget; a point's sums do not depend on its neighbours
// in a launch, so the chunk size changes no bit.  Rows are grouped by gas (checked by the callers); q_*: [R][isotopologues
// of the row's gas], one row after the other.
static int lblrt_compute(ansfm_ctx *ctx, int R, const int32_t *row_gas, const double *row_p, const double *row_t,
                         const double *row_mix, const double *q_lines, const double *q_cont, const double *q_lines_dT,
                         const double *q_cont_dT)
{
    const int S = ctx->rt_S, M = ctx->rt_M, nw = ctx->rt_nw, H = q_lines_dT ? 2 : 1;
    const size_t D = sizeof(double);
    HIPCHK(ctx->rt_k.reserve((size_t)R * H * nw * D));
    HIPCHK(hipMemsetAsync(ctx->rt_k.p, 0, (size_t)R * H * nw * D, ctx->stream));
    // the points of every gas, staged in one copy: per gas t, p [npt], mix [npt][M], then q_lines, q_cont [npt] per isotopologue
    std::vector<int> r0(S + 1, 0);
    for (int r = 0; r < R; ++r) r0[row_gas[r] + 1]++;
    for (int s = 0; s < S; ++s) r0[s + 1] += r0[s];
    std::vector<size_t> off(S + 1, 0);
    for (int s = 0; s < S; ++s) off[s + 1] = off[s] + (size_t)(r0[s + 1] - r0[s]) * H * (2 + M + 2 * ctx->rt_gas[s].size());
    std::vector<double> h(off[S]);
    size_t qbase = 0;
    for (int s = 0; s < S; ++s) {
        const int nr = r0[s + 1] - r0[s], npt = nr * H, niso = (int)ctx->rt_gas[s].size();
        double *t = h.data() + off[s], *p = t + npt, *mix = p + npt, *q = mix + (size_t)npt * M;
        for (int k = 0; k < npt; ++k) {
            const int r = r0[s] + k / H, hh = k % H;
            t[k] = hh ? row_t[r] + 5.0 : row_t[r];                                  // Spectroscopy_0.py:2021
            p[k] = row_p[r];
            for (int j = 0; j < M; ++j) mix[(size_t)k * M + j] = row_mix[(size_t)r * M + j];
            const size_t qo = qbase + (size_t)(k / H) * niso;
            for (int i = 0; i < niso; ++i) {
                q[(size_t)(2 * i) * npt + k] = hh ? q_lines_dT[qo + i] : q_lines[qo + i];
                q[(size_t)(2 * i + 1) * npt + k] = hh ? q_cont_dT[qo + i] : q_cont[qo + i];
            }
        }
        qbase += (size_t)nr * niso;
    }
    HIPCHK(ctx->rt_pts.reserve(h.size() * D + 8));
    HIPCHK(hipMemcpyAsync(ctx->rt_pts.p, h.data(), h.size() * D, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h is a local buffer
    int chunks = 0;
    for (int s = 0; s < S; ++s) {
        const int nr = r0[s + 1] - r0[s], npt = nr * H, niso = (int)ctx->rt_gas[s].size();
        if (npt == 0) continue;
        const double *ht = h.data() + off[s], *hp = ht + npt, *hmix = hp + npt;
        const double *d_t = ctx->rt_pts.as<double>() + off[s], *d_p = d_t + npt, *d_mix = d_p + npt, *d_q = d_mix + (size_t)npt * M;
        size_t per_pt = 1;
        for (const auto &ip : ctx->rt_gas[s]) {
            per_pt = std::max(per_pt, (size_t)(kLblRows + 1) * ip->N);
            per_pt = std::max(per_pt, (size_t)(3 + (2 * ip->nb + 1) + 2) * ip->Nb);
        }
        const int C = (int)std::min<size_t>(std::min<size_t>((size_t)npt, 65535), std::max<size_t>(1, ctx->rt_budget / (per_pt * D)));
        HIPCHK(ctx->rt_scratch.reserve((size_t)C * per_pt * D));
        std::vector<double> mixmax(M, 0.0);
        for (int k = 0; k < npt; ++k)
            for (int j = 0; j < M; ++j) mixmax[j] = std::max(mixmax[j], fabs(hmix[(size_t)k * M + j]));
        for (int k0 = 0; k0 < npt; k0 += C, ++chunks) {
            const int Lc = std::min(C, npt - k0);
            double *d_out = ctx->rt_k.as<double>() + ((size_t)r0[s] * H + k0) * nw;
            for (int i = 0; i < niso; ++i) {
                const LblrtIso &iso = *ctx->rt_gas[s][i];
                if (iso.include_lines && iso.N > 0) {
                    // the shift of a line is at most sum_j |delta_j| mix_j |p / p_ref|; a wider bound only lengthens the line range
                    // that a block walks, and every line of it is tested against the windows again
                    double dmax = 0.0, pmax = 0.0;
                    for (int j = 0; j < M; ++j) dmax += iso.dabs[j] * mixmax[j];
                    for (int k = 0; k < npt; ++k) pmax = std::max(pmax, fabs(hp[k] / iso.p_ref));
                    const int N = iso.N;
                    const double *dl = iso.lines.as<double>();
                    LblParams p;
                    memset(&p, 0, sizeof p);
                    p.wn_grid = ctx->rt_grid.as<double>(); p.t_calc = d_t + k0; p.p_calc = d_p + k0; p.out = d_out;
                    p.q_ratio = d_q + (size_t)(2 * i) * npt + k0;
                    p.mmf = d_mix + (size_t)k0 * M; p.mmf_stride = M;
                    p.nu = dl; p.sw = dl + N; p.e_lower = dl + 2 * (size_t)N; p.stim_ref = dl + 3 * (size_t)N; p.bparams = dl + 4 * (size_t)N;
                    p.store = ctx->rt_scratch.as<double>();
                    p.shift = p.store + (size_t)Lc * kLblRows * N;
                    p.nw = nw; p.N = N; p.M = M; p.L = Lc; p.lineshape_id = iso.lineshape_id;
                    p.t_ref = iso.t_ref; p.p_ref = iso.p_ref; p.iso_abundance = iso.abundance; p.iso_mass = iso.mass; p.s_floor = iso.s_floor;
                    p.wn_calc_window = iso.wn_calc_window; p.wn_approx_window = iso.wn_approx_window;
                    p.max_shift = dmax * pmax * 1.0000001 + 1e-12;
                    const int rc = lbl_launch_lines(ctx, p);
                    if (rc) return rc;
                }
                if (iso.include_continuum && iso.Nb > 0) {
                    const int N = iso.Nb;
                    const size_t LN = (size_t)Lc * N;
                    const double *db = iso.bins.as<double>();
                    PcParams p;
                    memset(&p, 0, sizeof p);
                    p.centers = db; p.widths = db + N; p.sw = db + 2 * (size_t)N; p.e_lower = db + 3 * (size_t)N; p.lo = db + 4 * (size_t)N;
                    p.bparams = db + 5 * (size_t)N;
                    p.mmf = d_mix + (size_t)k0 * M; p.mmf_stride = M;
                    p.q_ratio = d_q + (size_t)(2 * i + 1) * npt + k0;
                    p.wn_grid = ctx->rt_grid.as<double>(); p.t_calc = d_t + k0; p.p_calc = d_p + k0; p.out = d_out;
                    p.store = ctx->rt_scratch.as<double>();
                    p.x = p.store + 3 * LN; p.ysum = p.x + LN; p.y = p.ysum + LN;
                    p.nw = nw; p.N = N; p.M = M; p.L = Lc; p.lineshape_id = iso.lineshape_id; p.nb = iso.nb;
                    p.first = iso.first; p.last = iso.last; p.jmax = iso.jmax;
                    p.t_ref = iso.t_cont; p.p_ref = iso.p_cont; p.iso_abundance = iso.abundance; p.iso_mass = iso.mass; p.wmax = iso.wmax;
                    const int rc = lbl_launch_pc(ctx, p);
                    if (rc) return rc;
                }
            }
        }
    }
    ctx->rt_last_rows = R; ctx->rt_last_points = R * H; ctx->rt_last_chunks = chunks;
    return ANSFM_OK;
}

extern "C" {

int ansfm_lblrt_begin(ansfm_ctx *ctx, int nw, const double *wn_grid, int S, int M)
{
    CHECK_CTX(ctx);
    ctx->rt_stage = 0; ctx->st_n = 0;
    if (ctx->lblrt) { ctx->lblrt = 0; ctx->have_table = false; }     // the committed source is taken apart
    if (nw <= 0 || S <= 0 || M <= 0 || !wn_grid) FAIL(ANSFM_ERR_INVALID, "lblrt_begin: bad argument");
    const int rc = lbl_grid_ascending(ctx, nw, wn_grid);
    if (rc) return rc;
    HIPCHK(hipSetDevice(ctx->device));
    ctx->rt_h_grid.assign(wn_grid, wn_grid + nw);
    HIPCHK(ctx->rt_grid.reserve((size_t)nw * sizeof(double)));
    HIPCHK(hipMemcpyAsync(ctx->rt_grid.p, ctx->rt_h_grid.data(), (size_t)nw * sizeof(double), hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    ctx->rt_gas.clear();
    ctx->rt_gas.resize(S);
    ctx->rt_nw = nw; ctx->rt_S = S; ctx->rt_M = M; ctx->rt_stage = 1;
    return ANSFM_OK;
}

int ansfm_lblrt_add_isotopologue(ansfm_ctx *ctx, int gas, int lineshape_id, double isotopic_abundance, double isotopic_mass,
                                 int include_lines, int N, double t_ref, double p_ref, const double *broadening_params,
                                 const double *nu, const double *sw, const double *e_lower, const double *stim_ref, double s_floor,
                                 double wn_calc_window, double wn_approx_window, int include_continuum, int N_bins, double t_cont,
                                 double p_cont, const double *lsw_mean_broadening_params, const double *wn_bin_centers,
                                 const double *wn_bin_widths, const double *sw_sum, const double *lsw_mean_e_lower,
                                 int n_neighbour_bins)
{
    CHECK_CTX(ctx);
    if (ctx->rt_stage != 1) FAIL(ANSFM_ERR_INVALID, "lblrt_add_isotopologue: call ansfm_lblrt_begin first (and add before the commit)");
    if (gas < 0 || gas >= ctx->rt_S || N < 0 || N_bins < 0 || n_neighbour_bins < 0 ||
        (N > 0 && (!broadening_params || !nu || !sw || !e_lower || !stim_ref)) ||
        (N_bins > 0 && (!lsw_mean_broadening_params || !wn_bin_centers || !wn_bin_widths || !sw_sum || !lsw_mean_e_lower)))
        FAIL(ANSFM_ERR_INVALID, "lblrt_add_isotopologue: bad argument");
    if (n_neighbour_bins > kPcMaxNeighbours) FAIL(ANSFM_ERR_UNSUPPORTED, "pseudo-continuum: n_neighbour_bins 0 .. 8 are built");
    int rc = lbl_shape_built(ctx, lineshape_id);
    if (rc) return rc;
    const int M = ctx->rt_M;
    const size_t D = sizeof(double);
    std::unique_ptr<LblrtIso> iso(new LblrtIso());
    iso->lineshape_id = lineshape_id; iso->abundance = isotopic_abundance; iso->mass = isotopic_mass;
    iso->include_lines = include_lines ? 1 : 0; iso->include_continuum = include_continuum ? 1 : 0;
    iso->t_ref = t_ref; iso->p_ref = p_ref; iso->s_floor = s_floor; iso->wn_calc_window = wn_calc_window;
    iso->wn_approx_window = wn_approx_window; iso->t_cont = t_cont; iso->p_cont = p_cont; iso->nb = n_neighbour_bins;
    iso->dabs.assign(M, 0.0);
    HIPCHK(hipSetDevice(ctx->device));
    std::vector<double> h, hb;
    if (N > 0) {     // no lines: LineSetSpecData.has_data == False, nothing is added (LineData_0.py:845)
        std::vector<int> ord;
        lbl_pack_lines(M, N, broadening_params, nu, sw, e_lower, stim_ref, ord, h);
        for (int j = 0; j < M; ++j)
            for (int i = 0; i < N; ++i) iso->dabs[j] = std::max(iso->dabs[j], fabs(broadening_params[(size_t)(3 * j + 2) * N + i]));
        HIPCHK(iso->lines.reserve(h.size() * D));
        HIPCHK(hipMemcpyAsync(iso->lines.p, h.data(), h.size() * D, hipMemcpyHostToDevice, ctx->stream));
        iso->N = N;
    }
    bool any = false;
    for (int i = 0; i < N_bins; ++i) any = any || sw_sum[i] != 0;
    if (any) {       // all sums zero: PseudoContSpecData.has_data == False (:1244, :1336)
        PcGeometry g;
        if ((rc = lbl_pc_geometry(ctx, ctx->rt_nw, ctx->rt_h_grid.data(), N_bins, wn_bin_centers, wn_bin_widths, g))) return rc;
        const size_t n = N_bins;
        hb.resize((5 + 3 * (size_t)M) * n);
        for (size_t i = 0; i < n; ++i) {
            hb[i] = wn_bin_centers[i]; hb[n + i] = wn_bin_widths[i]; hb[2 * n + i] = sw_sum[i]; hb[3 * n + i] = lsw_mean_e_lower[i];
            hb[4 * n + i] = g.lo[i];
        }
        memcpy(hb.data() + 5 * n, lsw_mean_broadening_params, 3 * (size_t)M * n * D);
        HIPCHK(iso->bins.reserve(hb.size() * D));
        HIPCHK(hipMemcpyAsync(iso->bins.p, hb.data(), hb.size() * D, hipMemcpyHostToDevice, ctx->stream));
        iso->Nb = N_bins; iso->first = g.first; iso->last = g.last; iso->jmax = g.jmax; iso->wmax = g.wmax;
    }
    HIPCHK(hipStreamSynchronize(ctx->stream));   // h / hb are local buffers
    ctx->rt_gas[gas].push_back(std::move(iso));
    return ANSFM_OK;
}

int ansfm_lblrt_commit(ansfm_ctx *ctx)
{
    CHECK_CTX(ctx);
    if (ctx->rt_stage < 1) FAIL(ANSFM_ERR_INVALID, "lblrt_commit: call ansfm_lblrt_begin first");
    for (const auto &g : ctx->rt_gas)
        if (g.empty()) FAIL(ANSFM_ERR_INVALID, "lblrt_commit: every gas needs at least one isotopologue (ansfm_lblrt_add_isotopologue)");
    HIPCHK(hipSetDevice(ctx->device));
    // the context answers like an LBL table with G = 1 and W = nw: the table's bookkeeping (wave grid, the single
    // g-ordinate, paddings) comes from the table uploader on a 2 x 2 table of zeros that no kernel reads in this mode
    const int W = ctx->rt_nw, S = ctx->rt_S;
    const size_t n = (size_t)W * 4 * S;
    HIPCHK(ctx->tmp_in.reserve(n * sizeof(double)));
    HIPCHK(hipMemsetAsync(ctx->tmp_in.p, 0, n * sizeof(double), ctx->stream));
    const double pt[2] = {1.0, 2.0}, one = 1.0;
    const int rc = ansfm_upload_ktable_dev(ctx, W, 1, 2, 2, S, ctx->tmp_in.as<double>(), pt, pt, ctx->rt_h_grid.data(), &one);
    ctx->tmp_in.release();
    if (rc) return rc;
    ctx->is_lbl = 1; ctx->temp2d = 0; ctx->monotone = 1;
    ctx->lblrt = 1; ctx->rt_stage = 2; ctx->st_n = 0;
    return ANSFM_OK;
}

int ansfm_lblrt_set_scratch_bytes(ansfm_ctx *ctx, int64_t bytes)
{
    CHECK_CTX(ctx);
    if (bytes <= 0) FAIL(ANSFM_ERR_INVALID, "lblrt_set_scratch_bytes: bad argument");
    ctx->rt_budget = (size_t)bytes;
    return ANSFM_OK;
}

int ansfm_lblrt_last(const ansfm_ctx *ctx, int *rows, int *points, int *chunks)
{
    if (!ctx) return ANSFM_ERR_INVALID;
    if (rows) *rows = ctx->rt_last_rows;
    if (points) *points = ctx->rt_last_points;
    if (chunks) *chunks = ctx->rt_last_chunks;
    return ANSFM_OK;
}

int ansfm_lblrt_set_state(ansfm_ctx *ctx, int n_models, int L, int R, const int32_t *krow, const int32_t *row_gas,
                          const double *row_p_atm, const double *row_t, const double *row_mix, const double *row_q_lines,
                          const double *row_q_cont, const double *row_q_lines_dT, const double *row_q_cont_dT)
{
    CHECK_CTX(ctx);
    ctx->st_n = 0;
    if (!ctx->lblrt) FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: commit a line source first (ansfm_lblrt_commit)");
    if (n_models <= 0 || L <= 0 || R <= 0 || !krow || !row_gas || !row_p_atm || !row_t || !row_mix || !row_q_lines || !row_q_cont ||
        (row_q_lines_dT == nullptr) != (row_q_cont_dT == nullptr))
        FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: bad argument");
    const int S = ctx->rt_S;
    // the maps, before anything is launched
    for (int r = 0; r < R; ++r)
        if (row_gas[r] < 0 || row_gas[r] >= S || (r > 0 && row_gas[r] < row_gas[r - 1]))
            FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: row_gas[" + std::to_string(r) + "] = " + std::to_string(row_gas[r]) +
                                        " is outside [0, S = " + std::to_string(S) + ") or below its predecessor (rows are grouped by gas)");
    const size_t nk = (size_t)n_models * S * L;
    for (size_t i = 0; i < nk; ++i) {
        const int s = (int)((i / L) % S);
        if (krow[i] < 0 || krow[i] >= R || row_gas[krow[i]] != s)
            FAIL(ANSFM_ERR_INVALID, "lblrt_set_state: krow[" + std::to_string(i / ((size_t)S * L)) + "][" + std::to_string(s) + "][" +
                                        std::to_string(i % L) + "] = " + std::to_string(krow[i]) + " is outside [0, R = " + std::to_string(R) +
                                        ") or a row of another gas");
    }
    HIPCHK(hipSetDevice(ctx->device));
    HIPCHK(ctx->rt_krow.reserve(nk * sizeof(int32_t)));
    HIPCHK(hipMemcpyAsync(ctx->rt_krow.p, krow, nk * sizeof(int32_t), hipMemcpyHostToDevice, ctx->stream));
    const int rc = lblrt_compute(ctx, R, row_gas, row_p_atm, row_t, row_mix, row_q_lines, row_q_cont, row_q_lines_dT, row_q_cont_dT);
    if (rc) return rc;           // (lblrt_compute synchronises after its staging copy: krow is the caller's)
    ctx->st_n = n_models; ctx->st_L = L; ctx->st_R = R; ctx->st_H = row_q_lines_dT ? 2 : 1;
    return ANSFM_OK;
}

static int calc_klbl_online_impl(ansfm_ctx *ctx, const char *fn, int L, const double *press, const double *temp,
                                 const double *mol_mix_frac, const double *q_lines, const double *q_cont,
                                 const double *q_lines_dT, const double *q_cont_dT, double *k_out, double *dkdT_out)
{
    CHECK_CTX(ctx);
    if (!ctx->lblrt) { ctx->err = std::string(fn) + ": commit a line source first (ansfm_lblrt_commit)"; return ANSFM_ERR_NOTABLE; }
    if (L <= 0 || !press || !temp || !mol_mix_frac || !q_lines || !q_cont || !k_out || (dkdT_out && (!q_lines_dT || !q_cont_dT))) {
        ctx->err = std::string(fn) + ": bad argument";
        return ANSFM_ERR_INVALID;
    }
    HIPCHK(hipSetDevice(ctx->device));
    ctx->st_n = 0;                                  // the rows of a pending state are overwritten
    const int S = ctx->rt_S, M = ctx->rt_M, W = ctx->rt_nw, R = S * L;
    size_t niso_all = 0;
    for (const auto &g : ctx->rt_gas) niso_all += g.size();
    std::vector<int32_t> row_gas(R);
    std::vector<double> rp(R), rt(R), rmix((size_t)R * M), q[4];
    const double *qsrc[4] = {q_lines, q_cont, dkdT_out ? q_lines_dT : nullptr, dkdT_out ? q_cont_dT : nullptr};
    for (int a = 0; a < 4; ++a) if (qsrc[a]) q[a].resize(niso_all * L);
    size_t qo = 0, ib = 0;
    for (int s = 0; s < S; ++s) {
        const size_t niso = ctx->rt_gas[s].size();
        for (int l = 0; l < L; ++l) {
            const int r = s * L + l;
            row_gas[r] = s; rp[r] = press[l]; rt[r] = temp[l];
            for (int j = 0; j < M; ++j) rmix[(size_t)r * M + j] = mol_mix_frac[(size_t)s * M + j];
            for (size_t i = 0; i < niso; ++i, ++qo)
                for (int a = 0; a < 4; ++a) if (qsrc[a]) q[a][qo] = qsrc[a][(ib + i) * L + l];
        }
        ib += niso;
    }
    int rc = lblrt_compute(ctx, R, row_gas.data(), rp.data(), rt.data(), rmix.data(), q[0].data(), q[1].data(),
                           qsrc[2] ? q[2].data() : nullptr, qsrc[3] ? q[3].data() : nullptr);
    if (rc) return rc;
    const size_t n = (size_t)W * L * S;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double) * (dkdT_out ? 2 : 1)));
    double *dk = dkdT_out ? ctx->tmp_out.as<double>() + n : nullptr;
    hipLaunchKernelGGL(k_lblrt_seam, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream, ctx->rt_k.as<double>(), dkdT_out ? 2 : 1, W, S, L,
                       ctx->tmp_out.as<double>(), dk);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(k_out, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    if (dkdT_out) HIPCHK(hipMemcpyAsync(dkdT_out, dk, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

int ansfm_calc_klbl_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                           const double *q_lines, const double *q_cont, double *k_out)
{
    return calc_klbl_online_impl(ctx, "calc_klbl_online", L, press, temp, mol_mix_frac, q_lines, q_cont, nullptr, nullptr, k_out,
                                 nullptr);
}

int ansfm_calc_klblg_online(ansfm_ctx *ctx, int L, const double *press, const double *temp, const double *mol_mix_frac,
                            const double *q_lines, const double *q_cont, const double *q_lines_dT, const double *q_cont_dT,
                            double *k_out, double *dkdT_out)
{
    if (ctx && !dkdT_out) { ctx->err = "calc_klblg_online: bad argument"; return ANSFM_ERR_INVALID; }
    return calc_klbl_online_impl(ctx, "calc_klblg_online", L, press, temp, mol_mix_frac, q_lines, q_cont, q_lines_dT, q_cont_dT,
                                 k_out, dkdT_out);
}

int ansfm_get_dtaugas(ansfm_ctx *ctx, int model, double *dTAUGAS)
{
    CHECK_CTX(ctx);
    if (!ctx->have_table || ctx->dk_n == 0) FAIL(ANSFM_ERR_INVALID, "get_dtaugas: no gradient cirsrad call yet");
    if (model < 0 || model >= ctx->dk_n || !dTAUGAS) FAIL(ANSFM_ERR_INVALID, "get_dtaugas: bad model index");
    HIPCHK(hipSetDevice(ctx->device));
    const int W = ctx->W, Wpad = ctx->Wpad, G = ctx->G, L = ctx->dk_L, NP1 = ctx->S + 1;
    const size_t n = (size_t)W * G * NP1 * L;
    HIPCHK(ctx->tmp_out.reserve(n * sizeof(double)));
    hipLaunchKernelGGL(k_dtaugas_to_ref, dim3(nblk(n, 256)), dim3(256), 0, ctx->stream,
                       ctx->dkbuf.as<double>() + (size_t)model * L * NP1 * G * Wpad, ctx->tmp_out.as<double>(), W, Wpad, G, NP1, L);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(dTAUGAS, ctx->tmp_out.p, n * sizeof(double), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(hipStreamSynchronize(ctx->stream));
    return ANSFM_OK;
}

}  // extern "C"

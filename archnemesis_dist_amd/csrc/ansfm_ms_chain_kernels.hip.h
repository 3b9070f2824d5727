// ansfm_ms_chain_kernels.hip.h -- the (R,T,J) chain of one (wave, g, ic) on one wavefront, the matrices in LDS: the small dense
// helpers and k_ms_chain<N, CACHE>.
#pragma once
#include "ansfm_ms_chain_steps.h"
#include "ansfm_ms_phase_kernels.hip.h"

namespace ansfm {

// ---- small dense helpers on LDS matrices (one wavefront = one block), any nmu <= kMsMaxMu = 32 -------------------
typedef double ms_v4f64 __attribute__((ext_vector_type(4)));
// element (i, j) of a matrix with the kernel's leading dimension ld (k_ms_chain, k_ms_chain16); the elements a lane of
// k_ms_chain owns (a lane of k_ms_chain16 owns rows q, q + 4, q + 8, q + 12 of column c)
#define MS_AT(M, i, j) M[(i) * ld + (j)]
#define MS_FOR_IJ for (int e = lane, i = e / n, j = e % n; e < nn; e += 64, i = e / n, j = e % n)

// (the blocks of k_ms_chain are ONE wavefront: a compiler fence orders its lanes' LDS accesses -- MS_WAVE_SYNC, as in the
//  Hansen walk; __syncthreads() would also wait for every global access in flight at each of the ~30 points of a layer)
__device__ __forceinline__ void ms_mm(int n, int ld, const double *A, const double *B, double *C, int lane)
{   // C = A B   (C distinct from A and B)
    for (int e = lane; e < n * n; e += 64) {
        const int i = e / n, j = e % n;
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += A[i * ld + k] * B[k * ld + j];
        C[i * ld + j] = s;
    }
    MS_WAVE_SYNC();
}
__device__ __forceinline__ void ms_mv(int n, int ld, const double *A, const double *x, double *y, int lane)
{   // y = A x   (y distinct from x)
    if (lane < n) {
        double s = 0.0;
        for (int k = 0; k < n; ++k) s += A[lane * ld + k] * x[k];
        y[lane] = s;
    }
    MS_WAVE_SYNC();
}
__device__ __forceinline__ double ms_frob(int n, int ld, const double *r, int lane)
{
    double s = 0.0;
    for (int e = lane; e < n * n; e += 64) { const double v = r[(e / n) * ld + (e % n)]; s += v * v; }
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off, 64);
    return sqrt(s);
}
// Ainv = inverse(A) by Gauss-Jordan with partial pivoting (first largest |.|, like LAPACK's idamax); A is
// destroyed.  col = scratch[n].  The pivot search is a wavefront arg-max over the n candidate rows.
__device__ __forceinline__ void ms_inv(int n, int ld, double *A, double *Ainv, double *col, int lane)
{
    for (int e = lane; e < n * n; e += 64) { const int i = e / n, j = e % n; Ainv[i * ld + j] = (i == j) ? 1.0 : 0.0; }
    MS_WAVE_SYNC();
    for (int c = 0; c < n; ++c) {
        double best = (lane >= c && lane < n) ? fabs(A[lane * ld + c]) : -1.0;
        int piv = lane;
#pragma unroll
        for (int off = 16; off > 0; off >>= 1) {     // n <= 32: lanes 0..31 hold every candidate
            const double ob = __shfl_xor(best, off, 64);
            const int op = __shfl_xor(piv, off, 64);
            if (ob > best || (ob == best && op < piv)) { best = ob; piv = op; }
        }
        piv = __builtin_amdgcn_readfirstlane(piv);
        if (lane < n) {
            double ac = A[c * ld + lane], wc = Ainv[c * ld + lane];
            if (piv != c) {
                const double ap = A[piv * ld + lane], wp = Ainv[piv * ld + lane];
                A[piv * ld + lane] = ac; Ainv[piv * ld + lane] = wc;
                ac = ap; wc = wp;
            }
            // pivot element after the swap, read by every lane from the (not yet scaled) row
            const double d = 1.0 / __shfl(ac, c, 64);
            A[c * ld + lane] = ac * d;
            Ainv[c * ld + lane] = wc * d;
        }
        MS_WAVE_SYNC();
        if (lane < n) col[lane] = A[lane * ld + c];
        MS_WAVE_SYNC();
        for (int e = lane; e < n * n; e += 64) {
            const int r = e / n, j = e % n;
            if (r != c) {
                const double f = col[r];
                A[r * ld + j] -= f * A[c * ld + j];
                Ainv[r * ld + j] -= f * Ainv[c * ld + j];
            }
        }
        MS_WAVE_SYNC();
    }
}

// ---- (R,T,J) chain of one (wave, g, ic) -------------------------------------------------------------------
// N: the stream count at compile time (5 = the reference's default quadrature, Scatter_0.py:59; 8), 0 = any nmu <= kMsMaxMu at
// run time.  With N known the element -> (row, column) divisions become multiplications and the k-loops of the small products
// unroll (C4 size at 5 streams: 0.26 -> 0.21 s).  127 registers = four waves per SIMD; capped at 85 / 64 registers (six / eight
// waves, 0 / 55 spilled) the kernel is no faster (0.21 / 0.24 s): it is not occupancy that binds it.
// CACHE (the batched numerical Jacobian, ansfm_cirsrad_ck_scatter_batch; see k_ms_chain16): 1 = model 0's pass over the slab
// [w0, w0 + wcount) stores the doubled (r1, t1, j1) of every scattering layer, [wavenumber of the slab][g][order][layer]
// [2 n^2 + n]; 2 = the models [m0, m0 + n_launch) of a launch (grid x n_launch) take the layers flagged `same` from there and
// run the adding sweep only.  Same numbers either way.
template <int N, int CACHE = 0>
__global__ __launch_bounds__(64) void k_ms_chain(MsParams p)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    const int n = N ? N : p.nmu, nn = n * n;
    const int ld = n;
    const int msz = n * ld;
    const unsigned per_model = (unsigned)p.wcount * (unsigned)p.ng_launch * (unsigned)(p.nf + 1);
    const int ml = (CACHE == 2) ? (int)(blockIdx.x / per_model) : 0;           // position in the launch
    const unsigned rest = (CACHE == 2) ? blockIdx.x % per_model : blockIdx.x;
    const int mg = (CACHE == 2) ? p.model_ids[p.m0 + ml] : p.m0;               // model (0 outside the batch path)
    const int ic = rest % (p.nf + 1);
    const int ig = p.ig0 + (int)((rest / (p.nf + 1)) % p.ng_launch);      // the g-ordinates [ig0, ig0 + ng_launch) of this launch
    const int wl = rest / ((p.nf + 1) * p.ng_launch);                      // wavenumber within the slab (w0 = 0 outside the batch path)
    const int widx = p.w0 + wl;
    const auto [taus_w, omegas_w, bnu_w, tauray_w, lfrac_m, PPL, PMI, FC, wcn] = ms_chain_inputs(p, ml, mg, wl, widx, ig, ic, nn);
    const double *radg_m = p.radg + (size_t)mg * p.st_wm;
    const size_t centry = (size_t)(2 * nn + n);
    // LDS carve-up
    double *rc = sm, *tc = rc + msz, *r1 = tc + msz, *t1 = r1 + msz, *pp = t1 + msz, *pm = pp + msz;
    double *m0 = pm + msz, *m1 = m0 + msz, *m2 = m1 + msz, *m3 = m2 + msz, *m4 = m3 + msz, *m5 = m4 + msz;
    double *jc = m5 + msz, *j1 = jc + kMsMaxMu, *v0 = j1 + kMsMaxMu, *v1 = v0 + kMsMaxMu, *col = v1 + kMsMaxMu;
    double *radg = col + kMsMaxMu;
    (void)m5;
    if (lane < n) radg[lane] = radg_m[(size_t)widx * n + (n - 1 - lane)];   // radg[:, ::-1] :765
    MS_WAVE_SYNC();
    bool defined = false;
    const bool lookup = p.lookup != 0;
    if (p.lowbc > 0 && !lookup) {  // surface operator first :824-836
        MS_FOR_IJ {
            MS_AT(rc, i, j) = ms_surface_element(p.brdf, widx, n, i, j, p.nf, ic, p.mu[j], p.wtmu[j], p.xfac);
            MS_AT(tc, i, j) = 0.0;
        }
        if (lane < n) jc[lane] = radg[lane];
        defined = true;
        MS_WAVE_SYNC();
    }
    for (int l = 0; l < p.nlay; ++l) {
        const int k = lookup ? p.nlay - 1 - l : l;  // look-down: bottom layer first (:842-845)
        const double taut = taus_w[k];
        const double bc = bnu_w[k];
        const double taur = tauray_w[k];
        const auto [tauscat, omega, kind] = ms_layer_scalars(taut, omegas_w[k], taur);
        // ---- calc_rtj_matrix :566-647 -> (r1, t1, j1), iscl ------------------------------------------------
        int iscl = 0;
        if (kind == kMsLayerEmpty) {
            MS_FOR_IJ { MS_AT(r1, i, j) = 0.0; MS_AT(t1, i, j) = (i == j) ? 1.0 : 0.0; }
            if (lane < n) j1[lane] = 0.0;
            MS_WAVE_SYNC();
        } else if (kind == kMsLayerAbsorbing) {
            MS_FOR_IJ { MS_AT(r1, i, j) = 0.0; MS_AT(t1, i, j) = 0.0; }
            MS_WAVE_SYNC();
            if (lane < n) {
                const double tex = -(1. / p.mu[lane]) * taut;
                const double tt = (tex > -200.0) ? exp(tex) : 0.0;
                MS_AT(t1, lane, lane) = tt;
                j1[lane] = bc * (1.0 - tt);
            }
            MS_WAVE_SYNC();
        } else if (CACHE == 2 && p.same[(size_t)mg * p.nlay + k]) {
            // the layer of model 0, as its own pass left it (block-uniform branch)
            iscl = 1;
            const double *ce = p.cache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.nlay + k) * centry;
            MS_FOR_IJ { MS_AT(r1, i, j) = ce[e]; MS_AT(t1, i, j) = ce[nn + e]; }
            if (lane < n) j1[lane] = ce[2 * nn + lane];
            MS_WAVE_SYNC();
        } else {
            iscl = 1;
            const auto [con, tau0, fr, fs, nd] = ms_doubling_start(taut, omega, tauscat, taur, ic, [](double x) { return log2(x); },
                                                                   [](double x) { return exp2(x); });
            MS_FOR_IJ {
                double a, b;
                ms_phase_mix(MsPhaseGlobal{PPL, PMI, FC, nn, e}, fr, fs, p.iray, p.ncont, lfrac_m, wcn, p.nlay, k, a, b);
                MS_AT(pp, i, j) = a;
                MS_AT(pm, i, j) = b;
            }
            MS_WAVE_SYNC();
            // ---- double1 :321-362 --------------------------------------------------------------------------
            // Gamma++ = M^-1 (E - con P++ C) ;  Gamma+- = M^-1 con P+- C   (C, M^-1 diagonal)
            MS_FOR_IJ {
                const double gpp = (1. / p.mu[i]) * (((i == j) ? 1.0 : 0.0) - (MS_AT(pp, i, j) * p.wtmu[j]) * con);
                const double gpm = (1. / p.mu[i]) * ((MS_AT(pm, i, j) * p.wtmu[j]) * con);
                MS_AT(t1, i, j) = ((i == j) ? 1.0 : 0.0) - tau0 * gpp;
                MS_AT(r1, i, j) = tau0 * gpm;
            }
            if (lane < n) j1[lane] = (ic == 0) ? (1.0 - omega) * bc * tau0 * (1. / p.mu[lane]) : 0.0;
            MS_WAVE_SYNC();
            for (int it = 0; it < nd; ++it) {   // add :275-297
                ms_mm(n, ld, r1, r1, m0, lane);               // bcom
                if (ms_frob(n, ld, r1, lane) > 0.1) {
                    MS_FOR_IJ MS_AT(m1, i, j) = ((i == j) ? 1.0 : 0.0) - MS_AT(m0, i, j);
                    MS_WAVE_SYNC();
                    ms_inv(n, ld, m1, m2, col, lane);             // acom = inv(e - bcom)
                } else {
                    MS_FOR_IJ MS_AT(m2, i, j) = ((i == j) ? 1.0 : 0.0) + MS_AT(m0, i, j);
                    MS_WAVE_SYNC();
                }
                ms_mm(n, ld, t1, m2, m3, lane);               // ccom = t1 acom
                ms_mm(n, ld, m3, r1, m0, lane);               // rans = ccom r1
                ms_mm(n, ld, m0, t1, m1, lane);               // acom = rans t1
                ms_mm(n, ld, m3, t1, m4, lane);               // tans = ccom t1
                if (ic == 0) {
                    ms_mv(n, ld, r1, j1, v0, lane);               // jcom = r1 j1 + j1
                    if (lane < n) v0[lane] = v0[lane] + j1[lane];
                    MS_WAVE_SYNC();
                    ms_mv(n, ld, m3, v0, v1, lane);               // jans = ccom jcom + j1
                    if (lane < n) j1[lane] = v1[lane] + j1[lane];
                }
                MS_FOR_IJ { MS_AT(r1, i, j) = MS_AT(r1, i, j) + MS_AT(m1, i, j); MS_AT(t1, i, j) = MS_AT(m4, i, j); }
                MS_WAVE_SYNC();
            }
            if constexpr (CACHE == 1) {
                double *ce = p.cache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.nlay + k) * centry;
                MS_FOR_IJ { ce[e] = MS_AT(r1, i, j); ce[nn + e] = MS_AT(t1, i, j); }
                if (lane < n) ce[2 * nn + lane] = j1[lane];
            }
        }
        // ---- combine with the stack below :868-875 ------------------------------------------------------------
        if (l == 0 && !defined) {
            MS_FOR_IJ { MS_AT(rc, i, j) = MS_AT(r1, i, j); MS_AT(tc, i, j) = MS_AT(t1, i, j); }
            if (lane < n) jc[lane] = j1[lane];
            MS_WAVE_SYNC();
        } else if (iscl == 1) {   // addp, scattering layer :486-511 (rsub,tsub,jsub) = (rc,tc,jc)
            ms_mm(n, ld, rc, r1, m0, lane);                   // rsq = rsub r1
            if (ms_frob(n, ld, m0, lane) > 0.01) {
                MS_FOR_IJ MS_AT(m1, i, j) = ((i == j) ? 1.0 : 0.0) - MS_AT(m0, i, j);
                MS_WAVE_SYNC();
                ms_inv(n, ld, m1, m2, col, lane);
            } else {
                MS_FOR_IJ MS_AT(m2, i, j) = ((i == j) ? 1.0 : 0.0) + MS_AT(m0, i, j);
                MS_WAVE_SYNC();
            }
            ms_mm(n, ld, t1, m2, m3, lane);                   // ccom = t1 acom
            ms_mm(n, ld, m3, rc, m0, lane);                   // rans = ccom rsub
            ms_mm(n, ld, m0, t1, m1, lane);                   // bcom = rans t1
            ms_mm(n, ld, m3, tc, m4, lane);                   // tans = ccom tsub
            ms_mv(n, ld, rc, j1, v0, lane);                       // jcom = rsub j1 + jsub
            if (lane < n) v0[lane] += jc[lane];
            MS_WAVE_SYNC();
            ms_mv(n, ld, m3, v0, v1, lane);                       // jans = ccom jcom + j1
            if (lane < n) jc[lane] = v1[lane] + j1[lane];
            MS_FOR_IJ { MS_AT(rc, i, j) = MS_AT(r1, i, j) + MS_AT(m1, i, j); MS_AT(tc, i, j) = MS_AT(m4, i, j); }
            MS_WAVE_SYNC();
        } else {                  // addp, non-scattering layer :513-530
            ms_mv(n, ld, rc, j1, v0, lane);
            if (lane < n) v0[lane] += jc[lane];
            MS_WAVE_SYNC();
            MS_FOR_IJ {
                const double ta = MS_AT(t1, i, i), tb = MS_AT(t1, j, j);
                MS_AT(m0, i, j) = MS_AT(tc, i, j) * ta;
                MS_AT(m1, i, j) = MS_AT(rc, i, j) * ta * tb;
            }
            if (lane < n) v1[lane] = j1[lane] + MS_AT(t1, lane, lane) * v0[lane];
            MS_WAVE_SYNC();
            MS_FOR_IJ { MS_AT(tc, i, j) = MS_AT(m0, i, j); MS_AT(rc, i, j) = MS_AT(m1, i, j); }
            if (lane < n) jc[lane] = v1[lane];
            MS_WAVE_SYNC();
        }
    }
    if (ic != 0 && lane < n) jc[lane] = 0.0;   // :881-882
    MS_WAVE_SYNC();
    if (lookup && p.lowbc > 0) {
        // idown (:366-420) with rb = rs, tb = 0, jb = radg (js is set for every ic, :822):
        //   upl = (E - rc rs)^-1 (tc u0+ + (rc radg + jc));   m3 = the inverse, v0 = rc radg + jc
        MS_FOR_IJ MS_AT(m0, i, j) = ms_surface_element(p.brdf, widx, n, i, j, p.nf, ic, p.mu[j], p.wtmu[j], p.xfac);
        MS_WAVE_SYNC();
        ms_mm(n, ld, rc, m0, m1, lane);
        MS_FOR_IJ MS_AT(m2, i, j) = ((i == j) ? 1.0 : 0.0) - MS_AT(m1, i, j);
        MS_WAVE_SYNC();
        ms_inv(n, ld, m2, m3, col, lane);
        ms_mv(n, ld, rc, radg, v0, lane);
        if (lane < n) v0[lane] = v0[lane] + jc[lane];
        MS_WAVE_SYNC();
    }
    // ---- per path: the four (mu0, mu) samples and the bilinear interpolation :886-945 ---------------------------
    if (lane < p.ngeom) {
        const int ipath = lane;
        const double drad = ms_path_drad_ld(p, [](double x) { return cos(x); }, lookup, widx, ic, ipath, n, n, ld, p.mu, p.wtmu, rc, tc, jc,
                                            radg, m3, v0);
        p.drad[(size_t)mg * p.st_drad + (((size_t)widx * p.ng + ig) * (p.nf + 1) + ic) * p.ngeom + ipath] = drad;
    }
}

}  // namespace ansfm

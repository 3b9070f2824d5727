// ansfm_ms_chain16_kernels.hip.h -- the same chain for 16 streams on the matrix cores: Ms16, the inverses, the out-of-line libm
// wrappers and k_ms_chain16<PHASE_LDS, CACHE>.
#pragma once
#include "ansfm_ms_chain_kernels.hip.h"

namespace ansfm {

// ---- nmu == 16: the same chain on the matrix cores ----------------------------------------------------------
// Every 16x16 float64 matrix lives in LDS (leading dimension 17) and, while it is being worked on, in the
// MFMA accumulator layout ("D layout": lane (c = l&15, q = l>>4) holds rows q, q+4, q+8, q+12 of column c).
// v_mfma_f64_16x16x4_f64 takes B operands in exactly that layout, so products chain in registers; only a
// LEFT operand has to be read back from LDS transposed-wise (a[kb] = M[c][q+4kb]).  Mat-vec products reuse
// the a-operand registers (4 FMAs + a reduction over q).  One wavefront per block: LDS is in-order per
// wave, so a compiler fence replaces the barriers.
#define MS16_FENCE() __atomic_signal_fence(__ATOMIC_SEQ_CST)
struct Ms16 {
    int c, q;
    __device__ __forceinline__ void load_a(const double *M, double a[4]) const
    {
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) a[kb] = M[c * 17 + q + 4 * kb];
    }
    __device__ __forceinline__ ms_v4f64 load_d(const double *M) const
    {
        ms_v4f64 v;
#pragma unroll
        for (int r = 0; r < 4; ++r) v[r] = M[(q + 4 * r) * 17 + c];
        return v;
    }
    __device__ __forceinline__ void store_d(double *M, ms_v4f64 v) const
    {
#pragma unroll
        for (int r = 0; r < 4; ++r) M[(q + 4 * r) * 17 + c] = v[r];
    }
    __device__ __forceinline__ static ms_v4f64 mm(const double a[4], ms_v4f64 b)
    {
        ms_v4f64 acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kb], b[kb], acc, 0, 0, 0);
        return acc;
    }
    // (M x)[c] for the matrix whose a-operands are given; x in LDS.  Same value in the four lanes of column c.
    __device__ __forceinline__ double mv(const double a[4], const double *x) const
    {
        double s = 0.0;
#pragma unroll
        for (int kb = 0; kb < 4; ++kb) s += a[kb] * x[q + 4 * kb];
        return ms_xor32_sum(ms_xor16_sum(s));
    }
    // |v|_F^2, and the smallest doubles whose (correctly rounded) square root exceeds 0.1 / 0.01: `frob(v) > 0.1` is
    // `sumsq(v) >= kFrobSq01` without the square root in the chain
    static constexpr double kFrobSq01 = 0x1.47ae147ae147dp-7, kFrobSq001 = 0x1.a36e2eb1c432fp-14;
    __device__ __forceinline__ static double sumsq(ms_v4f64 v)
    {
        double s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        s += ms_dpp_f64<0x128>(s);
        s += ms_dpp_f64<0x124>(s);
        s += ms_dpp_f64<0x122>(s);
        s += ms_dpp_f64<0x121>(s);
        return ms_xor32_sum(ms_xor16_sum(s));
    }
    __device__ __forceinline__ static double frob(ms_v4f64 v)
    {
        double s = v[0] * v[0] + v[1] * v[1] + v[2] * v[2] + v[3] * v[3];
        s += ms_dpp_f64<0x128>(s);      // row_ror:8, 4, 2, 1: every lane ends with its row's sum
        s += ms_dpp_f64<0x124>(s);
        s += ms_dpp_f64<0x122>(s);
        s += ms_dpp_f64<0x121>(s);
        return sqrt(ms_xor32_sum(ms_xor16_sum(s)));
    }
    __device__ __forceinline__ ms_v4f64 eye_plus(ms_v4f64 v, double sgn) const
    {   // E + sgn * v
        ms_v4f64 o;
#pragma unroll
        for (int r = 0; r < 4; ++r) o[r] = ((q + 4 * r == c) ? 1.0 : 0.0) + sgn * v[r];
        return o;
    }
};

// inverse of the 16x16 matrix in LDS A (ld 17) -> Ainv; Gauss-Jordan, partial pivoting (first largest |.|).
// A is destroyed.  Lane (c0,q) updates rows q+4r of column c0 in both matrices.  Out of line (it is the rare fallback of
// the series inverse; inlined three times it cost the chain kernel 11 registers), pointers in the LDS address space.
typedef __attribute__((address_space(3))) double ms_lds_double;
__device__ __attribute__((noinline)) void ms_inv16_lds(ms_lds_double *A, ms_lds_double *Ainv, int lane)
{
    const int c0 = lane & 15, q = lane >> 4;
#pragma unroll
    for (int r = 0; r < 4; ++r) Ainv[(q + 4 * r) * 17 + c0] = (q + 4 * r == c0) ? 1.0 : 0.0;
    MS16_FENCE();
    for (int c = 0; c < 16; ++c) {
        double best = (c0 >= c) ? fabs(A[c0 * 17 + c]) : -1.0;    // every 16-lane row group searches alike
        int piv = c0;
#pragma unroll
        for (int off = 8; off > 0; off >>= 1) {
            const double ob = __shfl_xor(best, off, 64);
            const int op = __shfl_xor(piv, off, 64);
            if (ob > best || (ob == best && op < piv)) { best = ob; piv = op; }
        }
        piv = __builtin_amdgcn_readfirstlane(piv);
        // rows c and piv of both matrices: swap, then scale the pivot row
        const double ac = A[c * 17 + c0], wc = Ainv[c * 17 + c0];
        const double ap = A[piv * 17 + c0], wp = Ainv[piv * 17 + c0];
        const double d = 1.0 / A[piv * 17 + c];
        const double pa = ap * d, pw = wp * d;
        MS16_FENCE();
        if (q == 0) {
            A[piv * 17 + c0] = ac; Ainv[piv * 17 + c0] = wc;      // no-op content when piv == c, overwritten next
            A[c * 17 + c0] = pa; Ainv[c * 17 + c0] = pw;
        }
        MS16_FENCE();
        double f[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) f[r] = A[(q + 4 * r) * 17 + c];
        MS16_FENCE();
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = q + 4 * r;
            if (row != c) {
                A[row * 17 + c0] -= f[r] * pa;
                Ainv[row * 17 + c0] -= f[r] * pw;
            }
        }
        MS16_FENCE();
    }
}
__device__ __forceinline__ void ms_inv16(double *A, double *Ainv, int lane)
{
    ms_inv16_lds((ms_lds_double *)A, (ms_lds_double *)Ainv, lane);
}

// (E - B)^-1 for a 16x16 B given in D layout, on the matrix cores: the product form of the Neumann series,
//     (E - B)^-1 = (E + B)(E + B^2)(E + B^4)...,
// two MFMA products per factor; it stops when the next power is below 1e-17 in Frobenius norm (B = R R' of physical
// reflection operators has spectral radius < 1: 6 factors at |B| = 0.5, 9 at 0.9).  Returns false when it has not
// converged after 12 squarings (the caller then falls back on Gauss-Jordan).  mA / mB: LDS scratch matrices.
__device__ __forceinline__ bool ms_inv16_series(const Ms16 &L, ms_v4f64 B, double *mA, double *mB, ms_v4f64 &X)
{
    X = L.eye_plus(B, 1.0);
    ms_v4f64 Pw = B;
    double fP = Ms16::frob(B);
    for (int it = 0; it < 12; ++it) {
        double aP[4], aX[4];
        if (fP * fP < 1e-17) return true;                      // |P^2|_F <= |P|_F^2: the next power would be dropped anyway
        L.store_d(mA, Pw);
        L.store_d(mB, X);
        MS16_FENCE();
        L.load_a(mA, aP);
        const ms_v4f64 P2 = Ms16::mm(aP, Pw);                  // B^(2^(it+1))
        fP = Ms16::frob(P2);
        if (!(fP >= 1e-17)) return true;                       // also leaves on NaN
        L.load_a(mB, aX);
        const ms_v4f64 XP = Ms16::mm(aX, P2);
#pragma unroll
        for (int r = 0; r < 4; ++r) X[r] = X[r] + XP[r];       // X (E + P2)
        Pw = P2;
        MS16_FENCE();
    }
    return false;
}

// libm calls of the chain kernel, kept out of line: inlined, their polynomial constants and temporaries count towards the
// kernel's register allocation (log2 / exp2: 14 registers, exp: 14, cos: more) and it is the allocation, not the pressure inside
// the product loops, that decides how many waves share a SIMD.
__device__ __attribute__((noinline)) double ms_log2_ni(double x) { return log2(x); }
__device__ __attribute__((noinline)) double ms_exp2_ni(double x) { return exp2(x); }
__device__ __attribute__((noinline)) double ms_exp_ni(double x) { return exp(x); }
__device__ __attribute__((noinline)) double ms_cos_ni(double x) { return cos(x); }

// Register allocation and LDS decide how many waves share a SIMD, and a wave of this kernel spends half of its time waiting
// to issue (dependent products on a shared MFMA pipe).  History at C4 (1e4 wavenumbers): 280 registers after the Fourier-order
// loop moved into the block = ONE wave per SIMD, 1.05 s; capped at 256 = two, 0.73 s; libm calls and the Gauss-Jordan fallback
// out of line (they count towards the allocation: log2 / exp2 14 registers, exp 14, cos more), the inverse's scratch aliased
// onto r1 / t1 (4 instead of 6 LDS matrices) and a cap of 168 = three waves per SIMD, 0.59-0.60 s.  PHASE_LDS = true keeps the
// phase matrices of the Fourier order in LDS (17.5 KB: nine blocks per CU, no spills); PHASE_LDS = false reads them from HBM / L2
// in every layer (9.3 KB: twelve blocks, 65 registers spilled in the layer set-up) and is 2-4 % faster: the default.
// CACHE (the batched numerical Jacobian of the scattering configuration, ForwardModel_0.py:2251-2252: NX + 1 forward models
// that differ from the first in a few layers): the doubled (r, t, j) of a layer (calc_rtj_matrix :566-650) depend on that
// layer's inputs only and are 92 % of a chain's work (about twelve doublings of five products and an inverse each, against
// one adding step).  CACHE = 1: model 0's pass stores them per (wavenumber, g, Fourier order, layer) -- in the accumulator
// layout, 64 lanes x 8 doubles, coalesced -- and the number of orders it worked through.  CACHE = 2: one block per (model,
// wavenumber, g) re-runs the adding sweep (addp :481-533) and takes every layer whose inputs are bit-identical to model 0's
// from that cache; a changed layer, or an order beyond the cached ones, is computed as usual.  Same numbers either way.
template <bool PHASE_LDS, int CACHE = 0>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(3, 3))) void k_ms_chain16(MsParams p)
{
    extern __shared__ double sm[];
    const int lane = threadIdx.x;
    constexpr int n = 16, nn = 256, ld = 17, msz = 16 * 17;
    const Ms16 L{lane & 15, lane >> 4};
    const int c = L.c, q = L.q;
    int ig, widx, ml = 0;
    if constexpr (CACHE == 2) {
        // blocks of one (wavenumber, g) pair -- they read the same cache lines -- sit 8 apart in the launch order: consecutive
        // workgroups go round the 8 XCDs, so the models of a pair share ONE XCD's L2
        const long grp = (long)(blockIdx.x >> 3), slot = (long)(blockIdx.x & 7);
        const long pair = (grp / p.n_launch) * 8 + slot;
        ml = (int)(grp % p.n_launch);
        if (pair >= (long)p.wcount * p.ng) return;
        ig = (int)(pair % p.ng);
        widx = p.w0 + (int)(pair / p.ng);
    } else {
        ig = p.ig0 + (int)(blockIdx.x % p.ng_launch);
        widx = p.w0 + (int)(blockIdx.x / p.ng_launch);
    }
    int mg = p.m0 + ml;
    if constexpr (CACHE == 2) mg = p.model_ids[p.m0 + ml];
    const int wl = widx - p.w0;
    int ncached = 0;
    if constexpr (CACHE == 2) ncached = p.cache_orders[(size_t)wl * p.ng + ig];
    int ndone = 0;
    const double pi = 3.141592653589793;
    // rc / tc: the stack below; r1 / t1: the layer's operators as LEFT operands (their right-operand form stays in registers).
    // The same two matrices are the scratch of the inverse and of the chained products (mA / mB): every step reads its left
    // operands out of r1 / t1 first and stores the new r1 / t1 last.
    double *rc = sm, *tc = rc + msz, *r1 = tc + msz, *t1 = r1 + msz, *mA = r1, *mB = t1;
    double *jc = t1 + msz, *j1 = jc + 16, *v0 = j1 + 16, *mus = v0 + 16, *wts = mus + 16;
    // radg[:, ::-1] (:765) sits in j1 once the layer loop is done
    double *radg = j1;
    // phase matrices of this Fourier order (P++ times the Hansen factor, P+-) by component, lane-private [comp][2][4][64]:
    // they do not depend on the layer (PHASE_LDS only)
    double *phl = wts + 16;

    // quadrature points / weights for per-lane indexing: a kernel-argument array indexed per lane would be copied to scratch
    // memory (and a second copy of this loop further down costs 64 registers: the scalar loads are hoisted and kept)
    for (int kk = 0; kk < n; ++kk)
        if (lane == kk) { mus[kk] = p.mu[kk]; wts[kk] = p.wtmu[kk]; }
    MS16_FENCE();
    const bool lookup = p.lookup != 0;
    const double mu_c = mus[c], wt_c = wts[c];
    const double rmu_c = 1. / mu_c;
    double rmu_i[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) rmu_i[r] = 1. / mus[q + 4 * r];
    // Fourier sum of every path with the reference's early-out (:903-958), kept by lane `ipath`: the orders are worked
    // through one after the other by this block, and it stops as soon as every path has converged -- the reference builds the
    // operators of all NF + 1 orders first (:790) and never reads the ones beyond the break.
    double frad = 0.0;
    bool fconv1 = false, fdone = (lane >= p.ngeom);
    for (int ic = 0; ic <= p.nf; ++ic) {
    bool defined = false;
    if (p.lowbc > 0 && !lookup) {  // surface operator first :824-836
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = q + 4 * r, j = c;
            MS_AT(rc, i, j) = ms_surface_element(p.brdf, widx, n, i, j, p.nf, ic, mu_c, wt_c, p.xfac);
            MS_AT(tc, i, j) = 0.0;
        }
        if (lane < n) jc[lane] = p.radg[(size_t)mg * p.st_wm + (size_t)widx * n + (n - 1 - lane)];
        defined = true;
    }
    MS16_FENCE();
    // (mirrors ms_chain_inputs, with the five pointers below in front of the layer loop)
    const size_t wpw = (size_t)(widx - p.pw0);                              // in the window of phase matrices / factors
    const double *PPL = p.ppl + ((wpw * (p.nf + 1) + ic) * p.ncomp) * nn;
    const double *PMI = p.pmi + ((wpw * (p.nf + 1) + ic) * p.ncomp) * nn;
    const double *FC = p.fc + (((size_t)ig * p.nwin + wpw) * p.ncomp) * nn;   // ppl *= fc (:232)
    const int ncu = p.ncont + (p.iray > 0 ? 1 : 0);      // components in use: the aerosols, then Rayleigh
    if constexpr (PHASE_LDS) {
        for (int cc = 0; cc < ncu; ++cc)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = (q + 4 * r) * 16 + c;
                phl[((cc * 2 + 0) * 4 + r) * 64 + lane] = PPL[(size_t)cc * nn + e] * FC[(size_t)cc * nn + e];
                phl[((cc * 2 + 1) * 4 + r) * 64 + lane] = PMI[(size_t)cc * nn + e];
            }
        MS16_FENCE();
    }

    // the layer's scalars are fetched one layer ahead
    const size_t wrow = (size_t)ml * p.wcount + wl;       // taus / omegas / bnu: [model of the launch][wavenumber of the slab]
    const double *taus_w = p.taus + (wrow * p.ng + ig) * p.nlay, *omegas_w = p.omegas + (wrow * p.ng + ig) * p.nlay;
    const int mc = p.cont_local ? ml : mg, wcn = p.cont_local ? wl : widx;     // tauray / lfrac: by model, or by launch position
    const double *bnu_w = p.bnu + wrow * p.nlay, *tauray_w = p.tauray + (size_t)mc * p.st_wl + (size_t)wcn * p.nlay;
    const double *lfrac_m = p.lfrac + (size_t)mc * p.st_wcl;
    // CACHE = 2: every layer of the sweep below lstart is model 0's, and so is the stack they add up to (the lower boundary
    // included: the host leaves lstart at 0 when the boundary radiance differs) -- take it from model 0's pass and start there
    int lbeg = 0;
    if constexpr (CACHE == 2) {
        if (ic < ncached) lbeg = p.lstart[mg];
        if (lbeg > 0) {
            const double *pe = p.pcache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.npre + (lbeg / kMsPrefixStep - 1)) * kMsCacheEntry;
            ms_v4f64 sR, sT;
#pragma unroll
            for (int r = 0; r < 4; ++r) { sR[r] = pe[r * 64 + lane]; sT[r] = pe[(4 + r) * 64 + lane]; }
            const double sj = pe[512 + c];
            MS16_FENCE();
            L.store_d(rc, sR); L.store_d(tc, sT);
            if (q == 0) jc[c] = sj;
            MS16_FENCE();
            defined = true;
        }
    }
    // (a model that shares every layer with model 0 starts at lbeg = nlay when nlay is a multiple of kMsPrefixStep: no layer is
    // left, and kfirst would be one element outside the rows)
    const int kfirst = lookup ? p.nlay - 1 - lbeg : lbeg;
    double n_taut = 0.0, n_bc = 0.0, n_omega = 0.0, n_taur = 0.0;
    if (lbeg < p.nlay) { n_taut = taus_w[kfirst]; n_bc = bnu_w[kfirst]; n_omega = omegas_w[kfirst]; n_taur = tauray_w[kfirst]; }
    for (int l = lbeg; l < p.nlay; ++l) {
        const int k = lookup ? p.nlay - 1 - l : l;  // look-down: bottom layer first (:842-845)
        const double taut = n_taut, bc = n_bc;
        double omega = n_omega;
        const double taur_l = n_taur;
        if (l + 1 < p.nlay) {
            const int k1 = lookup ? k - 1 : k + 1;
            n_taut = taus_w[k1]; n_bc = bnu_w[k1]; n_omega = omegas_w[k1]; n_taur = tauray_w[k1];
        }
        if (omega < 0) omega = 0.0;                 // (the scalars and the three-way decision mirror ms_layer_scalars)
        if (omega > 1) omega = 1.0;
        double tauscat = taut * omega;
        const double taur = taur_l;
        tauscat = tauscat - taur;
        if (tauscat < 0) tauscat = 0.0;
        // ---- calc_rtj_matrix :566-647 -> (r1, t1, j1), iscl ------------------------------------------------
        int iscl = 0;
        omega = (tauscat + taur) / taut;
        if (taut == 0) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { MS_AT(r1, q + 4 * r, c) = 0.0; MS_AT(t1, q + 4 * r, c) = (q + 4 * r == c) ? 1.0 : 0.0; }
            if (lane < n) j1[lane] = 0.0;
            MS16_FENCE();
        } else if (omega == 0) {
            const double tex = -rmu_c * taut;
            const double tt = (tex > -200.0) ? ms_exp_ni(tex) : 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) { MS_AT(r1, q + 4 * r, c) = 0.0; MS_AT(t1, q + 4 * r, c) = (q + 4 * r == c) ? tt : 0.0; }
            if (lane < n) j1[lane] = bc * (1.0 - tt);
            MS16_FENCE();
        } else if (CACHE == 2 && ic < ncached && p.same[(size_t)mg * p.nlay + k]) {
            // the layer of model 0, as its own pass left it (wave-uniform branch)
            iscl = 1;
            const double *ce = p.cache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.nlay + k) * kMsCacheEntry;
            ms_v4f64 bR, bT;
#pragma unroll
            for (int r = 0; r < 4; ++r) { bR[r] = ce[r * 64 + lane]; bT[r] = ce[(4 + r) * 64 + lane]; }
            const double jv = ce[512 + c];
            L.store_d(r1, bR); L.store_d(t1, bT);
            if (q == 0) j1[c] = jv;
            MS16_FENCE();
        } else {
            iscl = 1;
            // ---- double1 :321-362: starting (r,t,j) of the 2^-nd sub-layer, built straight in D layout -----
            const auto [con, tau0, fr, fs, nd] = ms_doubling_start(taut, omega, tauscat, taur, ic, [](double x) { return ms_log2_ni(x); },
                                                                   [](double x) { return ms_exp2_ni(x); });
            ms_v4f64 bR, bT;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = q + 4 * r, j = c, e = i * 16 + j;
                double a, b;
                if constexpr (PHASE_LDS) {
                    ms_phase_mix(MsPhaseLds{phl, r, lane}, fr, fs, p.iray, p.ncont, lfrac_m, wcn, p.nlay, k, a, b);
                } else {
                    ms_phase_mix(MsPhaseGlobal32{PPL, PMI, FC, nn, (unsigned)e * 8u}, fr, fs, p.iray, p.ncont, lfrac_m, wcn, p.nlay, k, a, b);
                }
                // Gamma++ = M^-1 (E - con P++ C) ;  Gamma+- = M^-1 con P+- C   (C, M^-1 diagonal)
                const double gpp = rmu_i[r] * (((i == j) ? 1.0 : 0.0) - (a * wt_c) * con);
                const double gpm = rmu_i[r] * ((b * wt_c) * con);
                bT[r] = ((i == j) ? 1.0 : 0.0) - tau0 * gpp;
                bR[r] = tau0 * gpm;
            }
            double jv = (ic == 0) ? (1.0 - omega) * bc * tau0 * rmu_c : 0.0;    // j1[c], same in the 4 lanes of c
            L.store_d(r1, bR); L.store_d(t1, bT);
            if (q == 0) j1[c] = jv;
            MS16_FENCE();
            for (int it = 0; it < nd; ++it) {   // add :275-297
                double aR[4], aT[4], aC[4];
                L.load_a(r1, aR);
                L.load_a(t1, aT);                                             // before r1 / t1 serve as scratch
                const ms_v4f64 bcom = Ms16::mm(aR, bR);                       // r1 r1
                // rans t1 = (ccom r1) t1 is formed as ccom (r1 t1): r1 t1 needs nothing of the inverse and keeps the matrix
                // cores busy while it is worked out, and ccom is the only intermediate that has to change layout (one LDS
                // round trip instead of two).  Same products, other association: the last bits differ from the reference's order.
                const ms_v4f64 r1t1 = Ms16::mm(aR, bT);                       // r1 t1
                ms_v4f64 acom;
                if (Ms16::sumsq(bR) >= Ms16::kFrobSq01) {                     // |r1|_F > 0.1: inv(e - bcom)
                    if (!ms_inv16_series(L, bcom, mA, mB, acom)) {
                        L.store_d(mA, L.eye_plus(bcom, -1.0));
                        MS16_FENCE();
                        ms_inv16(mA, mB, lane);
                        acom = L.load_d(mB);
                    }
                } else
                    acom = L.eye_plus(bcom, 1.0);
                const ms_v4f64 ccom = Ms16::mm(aT, acom);                     // t1 acom
                L.store_d(mB, ccom);
                double jcom = 0.0;
                if (ic == 0) {
                    jcom = L.mv(aR, j1) + jv;                                 // r1 j1 + j1
                    if (q == 0) v0[c] = jcom;
                }
                MS16_FENCE();
                L.load_a(mB, aC);
                const ms_v4f64 tans = Ms16::mm(aC, bT);                       // ccom t1
                const ms_v4f64 acc = Ms16::mm(aC, r1t1);                      // ccom (r1 t1) = rans t1
                if (ic == 0) jv = L.mv(aC, v0) + jv;                          // ccom jcom + j1
#pragma unroll
                for (int r = 0; r < 4; ++r) bR[r] = bR[r] + acc[r];
                bT = tans;
                MS16_FENCE();
                L.store_d(r1, bR); L.store_d(t1, bT);
                if (q == 0) j1[c] = jv;
                MS16_FENCE();
            }
            if constexpr (CACHE == 1) {
                double *ce = p.cache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.nlay + k) * kMsCacheEntry;
#pragma unroll
                for (int r = 0; r < 4; ++r) { ce[r * 64 + lane] = bR[r]; ce[(4 + r) * 64 + lane] = bT[r]; }
                if (q == 0) ce[512 + c] = jv;
            }
        }
        // ---- combine with the stack below :868-875 ------------------------------------------------------------
        if (l == 0 && !defined) {
#pragma unroll
            for (int r = 0; r < 4; ++r) { MS_AT(rc, q + 4 * r, c) = MS_AT(r1, q + 4 * r, c); MS_AT(tc, q + 4 * r, c) = MS_AT(t1, q + 4 * r, c); }
            if (lane < n) jc[lane] = j1[lane];
            MS16_FENCE();
        } else if (iscl == 1) {   // addp, scattering layer :486-511 (rsub,tsub,jsub) = (rc,tc,jc)
            double aRc[4], aT[4], aC[4];
            const ms_v4f64 bR1 = L.load_d(r1), bT1 = L.load_d(t1), bTc = L.load_d(tc);
            const double j1v = j1[c];
            L.load_a(rc, aRc);
            L.load_a(t1, aT);                                                 // before r1 / t1 serve as scratch
            const ms_v4f64 rsq = Ms16::mm(aRc, bR1);                          // rsub r1
            const ms_v4f64 rst1 = Ms16::mm(aRc, bT1);                         // rsub t1: rans t1 = ccom (rsub t1), as in the doubling
            ms_v4f64 acom;
            if (Ms16::sumsq(rsq) >= Ms16::kFrobSq001) {                       // |rsq|_F > 0.01
                if (!ms_inv16_series(L, rsq, mA, mB, acom)) {
                    L.store_d(mA, L.eye_plus(rsq, -1.0));
                    MS16_FENCE();
                    ms_inv16(mA, mB, lane);
                    acom = L.load_d(mB);
                }
            } else
                acom = L.eye_plus(rsq, 1.0);
            const ms_v4f64 ccom = Ms16::mm(aT, acom);                         // t1 acom
            L.store_d(mB, ccom);
            const double jcom = L.mv(aRc, j1) + jc[c];                        // rsub j1 + jsub
            if (q == 0) v0[c] = jcom;
            MS16_FENCE();
            L.load_a(mB, aC);
            const ms_v4f64 tans = Ms16::mm(aC, bTc);                          // ccom tsub
            const ms_v4f64 bcomm = Ms16::mm(aC, rst1);                        // ccom (rsub t1) = rans t1
            const double jans = L.mv(aC, v0) + j1v;                           // ccom jcom + j1
            ms_v4f64 rnew;
#pragma unroll
            for (int r = 0; r < 4; ++r) rnew[r] = bR1[r] + bcomm[r];
            MS16_FENCE();
            L.store_d(rc, rnew); L.store_d(tc, tans);
            if (q == 0) jc[c] = jans;
            MS16_FENCE();
        } else {                  // addp, non-scattering layer :513-530
            double aRc[4];
            L.load_a(rc, aRc);
            const double jcom = L.mv(aRc, j1) + jc[c];
            const double tcc = MS_AT(t1, c, c);
            const double jn = j1[c] + tcc * jcom;
            ms_v4f64 tn, rn;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int i = q + 4 * r;
                const double ta = MS_AT(t1, i, i);
                tn[r] = MS_AT(tc, i, c) * ta;
                rn[r] = MS_AT(rc, i, c) * ta * tcc;
            }
            MS16_FENCE();
            L.store_d(tc, tn); L.store_d(rc, rn);
            if (q == 0) jc[c] = jn;
            MS16_FENCE();
        }
        if constexpr (CACHE == 1) {
            if ((l % kMsPrefixStep) == kMsPrefixStep - 1 && l / kMsPrefixStep < p.npre) {
                double *pe = p.pcache + ((((size_t)wl * p.ng + ig) * (p.nf + 1) + ic) * p.npre + l / kMsPrefixStep) * kMsCacheEntry;
                const ms_v4f64 sR = L.load_d(rc), sT = L.load_d(tc);
#pragma unroll
                for (int r = 0; r < 4; ++r) { pe[r * 64 + lane] = sR[r]; pe[(4 + r) * 64 + lane] = sT[r]; }
                if (q == 0) pe[512 + c] = jc[c];
            }
        }
    }
    if (ic != 0 && lane < n) jc[lane] = 0.0;   // :881-882
    if (lane < n) radg[lane] = p.radg[(size_t)mg * p.st_wm + (size_t)widx * n + (n - 1 - lane)];   // j1 is free until the next order's first layer
    __syncthreads();
    if (lookup && p.lowbc > 0) {
        // idown (:366-420) with rb = rs, tb = 0, jb = radg (js is set for every ic, :822):
        //   upl = (E - rc rs)^-1 (tc u0+ + (rc radg + jc));   mB = the inverse, v0 = rc radg + jc
        ms_v4f64 rs;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = q + 4 * r, j = c;
            rs[r] = ms_surface_element(p.brdf, widx, n, i, j, p.nf, ic, mu_c, wt_c, p.xfac);
        }
        double aRc[4];
        L.load_a(rc, aRc);
        L.store_d(mA, L.eye_plus(Ms16::mm(aRc, rs), -1.0));
        MS16_FENCE();
        ms_inv16(mA, mB, lane);
        const double wv = L.mv(aRc, radg) + jc[c];
        if (q == 0) v0[c] = wv;
        __syncthreads();
    }
    // ---- per path: the four (mu0, mu) samples and the bilinear interpolation :886-945 (mirrors ms_path_drad_ld) --------
    if (lane < p.ngeom) {
        const int ipath = lane;
        const double sol_ang = p.sol_ang[ipath];
        const double emiss_ang = lookup ? 180. - p.emiss_ang[ipath] : p.emiss_ang[ipath];   // new_emi :900-903
        double zmu0, solar1;
        if (sol_ang > 90.0) { zmu0 = ms_cos_ni((180 - sol_ang) * pi / 180.0); solar1 = p.solar[widx] * 0.0; }
        else { zmu0 = ms_cos_ni(sol_ang * pi / 180.0); solar1 = p.solar[widx]; }
        const double zmu = ms_cos_ni(emiss_ang * pi / 180.0);
        int isol = 0, iemm = 0;
        const int nq = p.nmu_real ? p.nmu_real : n;     // the quadrature's points (a smaller quadrature padded to 16 streams)
        for (int j = 0; j < nq - 1; ++j) if (zmu0 <= mus[j] && zmu0 > mus[j + 1]) isol = j;
        if (zmu0 <= mus[nq - 1]) isol = nq - 2;
        for (int j = 0; j < nq - 1; ++j) if (zmu <= mus[j] && zmu > mus[j + 1]) iemm = j;
        if (zmu <= mus[nq - 1]) iemm = nq - 2;
        const double u = (mus[isol] - zmu0) / (mus[isol] - mus[isol + 1]);
        const double t = (mus[iemm] - zmu) / (mus[iemm] - mus[iemm + 1]);
        double yx[4];
        int ico = 0;
        for (int imu0 = isol; imu0 < isol + 2; ++imu0) {
            const double s0 = solar1 / (2.0 * pi * wts[imu0]);
            for (int imu = iemm; imu < iemm + 2; ++imu) {
                if (!lookup) {
                    double bcom = 0.0;   // (T utmi)[imu], utmi = radg for ic == 0 else 0
                    if (ic == 0) for (int kk = 0; kk < n; ++kk) bcom += MS_AT(tc, imu, kk) * radg[kk];
                    yx[ico++] = (MS_AT(rc, imu, imu0) * s0 + bcom) + jc[imu];
                } else if (p.lowbc == 0) {   // bottom of the atmosphere: T u0+ + R u- + J  (:929-933)
                    double bcom = 0.0;
                    if (ic == 0) for (int kk = 0; kk < n; ++kk) bcom += MS_AT(rc, imu, kk) * radg[kk];
                    yx[ico++] = (MS_AT(tc, imu, imu0) * s0 + bcom) + jc[imu];
                } else {
                    double upl = 0.0;
                    for (int kk = 0; kk < n; ++kk) upl += MS_AT(mB, imu, kk) * (MS_AT(tc, kk, imu0) * s0 + v0[kk]);
                    yx[ico++] = upl;
                }
            }
        }
        double drad = ((1 - t) * (1 - u) * yx[0] + t * (1 - u) * yx[1] + t * u * yx[3] + (1 - t) * u * yx[2]) *
                      ms_cos_ni(ic * p.aphi[ipath] * pi / 180.0);
        if (ic > 0) drad *= 2;
        if (!fdone) fdone = ms_fourier_step(drad, frad, fconv1);   // :945-958
    }
    ++ndone;
    if (__builtin_amdgcn_ballot_w64(!fdone) == 0) break;
    __syncthreads();                                    // the LDS matrices are rebuilt by the next order
    }
    if constexpr (CACHE == 1) { if (lane == 0) p.cache_orders[(size_t)wl * p.ng + ig] = ndone; }
    if (lane < p.ngeom) p.rad[(size_t)mg * p.st_rad + ((size_t)lane * p.ng + ig) * p.nwave + widx] = frad;
}

}  // namespace ansfm

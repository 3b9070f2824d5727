// ansfm_ms_phase_kernels.hip.h -- what comes before the chains: padding to 16 streams, the azimuth-integrated phase matrices
// (k_ms_phase), the cross-lane sums without the LDS crossbar, the sequential Hansen walk (k_ms_hansen_seq).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ansfm_ms_params.h"

namespace ansfm {

// radg [rows][nr] -> [rows][16]: the chain kernels read it back to front (radg[:, ::-1], :765), so the quadrature's values go to
// the END of a padded row.  brdf [W][nr][nr][nf1] -> [W][16][16][nf1], zero outside the block.
__global__ void k_ms_pad_radg(size_t rows, int nr, const double *__restrict__ src, double *__restrict__ dst)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= rows * 16) return;
    const int k = (int)(idx % 16);
    const size_t r = idx / 16;
    dst[idx] = (k >= 16 - nr) ? src[r * nr + (k - (16 - nr))] : 0.0;
}
__global__ void k_ms_pad_brdf(size_t W, int nr, int nf1, const double *__restrict__ src, double *__restrict__ dst)
{
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= W * 256 * nf1) return;
    const int ic = (int)(idx % nf1), j = (int)((idx / nf1) % 16), i = (int)((idx / ((size_t)nf1 * 16)) % 16);
    const size_t w = idx / ((size_t)nf1 * 256);
    dst[idx] = (i < nr && j < nr) ? src[((w * nr + i) * nr + j) * nf1 + ic] : 0.0;
}

__device__ __forceinline__ double ms_interp(double x, const double *xp, const double *fp, int n)
{   // np.interp
    if (x <= xp[0]) return fp[0];
    if (x >= xp[n - 1]) return fp[n - 1];
    int lo = 0, hi = n - 1;
    while (hi - lo > 1) { int mid = (lo + hi) >> 1; if (xp[mid] <= x) lo = mid; else hi = mid; }
    double slope = (fp[lo + 1] - fp[lo]) / (xp[lo + 1] - xp[lo]);
    return slope * (x - xp[lo]) + fp[lo];
}

// ---- phase matrices -----------------------------------------------------------------------------
// raw azimuth integrals (phasint2 :141-197), one block per (wave, scatterer), all ic.
// A thread owns matrix elements (i, j) and walks the azimuth grid ONCE for all Fourier orders: the phase function at
// (i, j, phi) does not depend on the order (the first version evaluated it per (order, element): nf + 1 times), and
// cos(ic phi) depends on neither i nor j -- a table in LDS, filled by the same expression.  Same sums in the same order.
constexpr int kMsPhaseOrders = 9;     // Fourier orders accumulated per pass over the azimuth grid (nf = 8: one pass)
__global__ __launch_bounds__(256) void k_ms_phase(MsParams p)
{
    extern __shared__ double ctab[];            // [nf + 2][nphi + 1]: cos(ic phi_k); the last row is cos(phi_k)
    const int wl = blockIdx.x, widx = p.pw0 + wl;                      // wl: in the window
    // comp == ncont -> Rayleigh.  With a pair list (per-model phase functions) block y is a (variant, component) pair: the
    // variant's phase function in, its matrices out, the same arithmetic
    const int var = p.pairs ? p.pairs[2 * blockIdx.y] : 0;
    const int comp = p.pairs ? p.pairs[2 * blockIdx.y + 1] : blockIdx.y + p.phase_comp0;
    const int n = p.nmu, nn = n * n, tid = threadIdx.x;
    const double pi = 3.141592653589793;
    const double dphi = 2.0 * pi / p.nphi;
    const int jc = comp < p.ncont ? comp : (p.ncont > 0 ? p.ncont - 1 : 0);
    const double *phas = var > 0 ? p.phasarr_var + (size_t)(var - 1) * p.st_phas : p.phasarr;
    const double *pfunc = phas + (((size_t)jc * p.nwave + widx) * 2 + 0) * p.nth;
    const double *xmu = phas + (((size_t)jc * p.nwave + widx) * 2 + 1) * p.nth;
    double *const oppl = p.ppl + (size_t)var * p.vstride, *const opmi = p.pmi + (size_t)var * p.vstride;
    const int iscat = (comp == p.ncont) ? 0 : (p.imie == 0 ? 2 : 4);
    const int nk = p.nphi + 1;
    const bool tab = p.phase_tab != 0;
    if (tab) {
        for (int t = tid; t < (p.nf + 2) * nk; t += blockDim.x) {
            const int ic = t / nk, k = t % nk;
            const double phi = k * dphi;
            ctab[t] = (ic <= p.nf) ? cos(ic * phi) : cos(phi);
        }
        __syncthreads();
    }
    const double *cphi_row = ctab + (size_t)(p.nf + 1) * nk;
    const int nr = p.nmu_real ? p.nmu_real : n;
    for (int e = tid; e < nn; e += blockDim.x) {
        const int i = e / n, j = e % n;
        if (i >= nr || j >= nr) {               // beyond the quadrature (a smaller one padded to 16 streams): nothing scatters there
            for (int ic = 0; ic <= p.nf; ++ic) {
                oppl[(((size_t)wl * (p.nf + 1) + ic) * p.ncomp + comp) * nn + e] = 0.0;
                opmi[(((size_t)wl * (p.nf + 1) + ic) * p.ncomp + comp) * nn + e] = 0.0;
            }
            continue;
        }
        const double sthi = sqrt(1.0 - p.mu[i] * p.mu[i]), sthj = sqrt(1.0 - p.mu[j] * p.mu[j]);
        const double ss = sthi * sthj, mmu = p.mu[i] * p.mu[j];
        for (int ic0 = 0; ic0 <= p.nf; ic0 += kMsPhaseOrders) {
            double spl[kMsPhaseOrders], smi[kMsPhaseOrders];
#pragma unroll
            for (int o = 0; o < kMsPhaseOrders; ++o) { spl[o] = 0.0; smi[o] = 0.0; }
            for (int k = 0; k <= p.nphi; ++k) {
                const double phi = k * dphi;
                const double cphi = tab ? cphi_row[k] : cos(phi);
                const double cpl = ss * cphi + mmu, cmi = ss * cphi - mmu;
                double pl, pm;
                if (iscat == 0) {
                    pl = 0.75 * (1.0 + cpl * cpl) / (4 * pi);
                    pm = 0.75 * (1.0 + cmi * cmi) / (4 * pi);
                } else if (iscat == 2) {
                    const double f1 = pfunc[0], f2 = 1.0 - f1;
                    const double hg11 = 1.0 - pfunc[1] * pfunc[1], hg12 = 2.0 - hg11;
                    const double hg21 = 1.0 - pfunc[2] * pfunc[2], hg22 = 2.0 - hg21;
                    double s1 = sqrt(hg12 - 2.0 * pfunc[1] * cpl), s2 = sqrt(hg22 - 2.0 * pfunc[2] * cpl);
                    pl = f1 * hg11 / (s1 * s1 * s1) + f2 * hg21 / (s2 * s2 * s2);
                    s1 = sqrt(hg12 - 2.0 * pfunc[1] * cmi); s2 = sqrt(hg22 - 2.0 * pfunc[2] * cmi);
                    pm = f1 * hg11 / (s1 * s1 * s1) + f2 * hg21 / (s2 * s2 * s2);
                    pl /= 4 * pi; pm /= 4 * pi;
                } else {
                    pl = ms_interp(cpl, xmu, pfunc, p.nth);
                    pm = ms_interp(cmi, xmu, pfunc, p.nth);
                }
                const double w = (k == 0 || k == p.nphi) ? 0.5 * dphi : dphi;
                const double w0 = w / (2.0 * pi), w1 = w / pi;
#pragma unroll
                for (int o = 0; o < kMsPhaseOrders; ++o) {
                    const int ic = ic0 + o;
                    if (ic <= p.nf) {
                        const double wphi = (ic == 0) ? w0 : w1;
                        const double cic = tab ? ctab[(size_t)ic * nk + k] : cos(ic * phi);
                        spl[o] += wphi * (pl * cic);
                        smi[o] += wphi * (pm * cic);
                    }
                }
            }
#pragma unroll
            for (int o = 0; o < kMsPhaseOrders; ++o) {
                const int ic = ic0 + o;
                if (ic <= p.nf) {
                    oppl[(((size_t)wl * (p.nf + 1) + ic) * p.ncomp + comp) * nn + e] = spl[o];
                    opmi[(((size_t)wl * (p.nf + 1) + ic) * p.ncomp + comp) * nn + e] = smi[o];
                }
            }
        }
    }
}

// Cross-lane sums without the LDS crossbar (__shfl_xor = ds_bpermute: an LDS round trip per stage, six dependent stages for a
// norm, in front of every product that waits for the result).  Within a 16-lane row: DPP row rotations (VALU); across the
// four rows: gfx950's v_permlane16_swap / v_permlane32_swap (vdst's odd rows / upper half <-> src's even rows / lower half;
// with both operands the same register the two results are the partner values).  tools/calib/lane_reduce_check.hip.
template <int CTRL> __device__ __forceinline__ double ms_dpp_f64(double v)
{
    const long long b = __double_as_longlong(v);
    const int lo = __builtin_amdgcn_update_dpp(0, (int)(unsigned)b, CTRL, 0xf, 0xf, false);
    const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), CTRL, 0xf, 0xf, false);
    return __longlong_as_double(((long long)hi << 32) | (unsigned long long)(unsigned)lo);
}
__device__ __forceinline__ double ms_xor16_sum(double s)      // s[l] + s[l ^ 16]
{
    const long long b = __double_as_longlong(s);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    return __longlong_as_double(((long long)rh[0] << 32) | (unsigned long long)rl[0]) +
           __longlong_as_double(((long long)rh[1] << 32) | (unsigned long long)rl[1]);
}
__device__ __forceinline__ double ms_xor32_sum(double s)      // s[l] + s[l ^ 32]
{
    const long long b = __double_as_longlong(s);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = __builtin_amdgcn_permlane32_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane32_swap(hi, hi, false, false);
    return __longlong_as_double(((long long)rh[0] << 32) | (unsigned long long)rl[0]) +
           __longlong_as_double(((long long)rh[1] << 32) | (unsigned long long)rl[1]);
}
// maximum over the 64 lanes, the same way (every lane gets it)
__device__ __forceinline__ double ms_wave_max(double x)
{
    x = fmax(x, ms_dpp_f64<0x128>(x));
    x = fmax(x, ms_dpp_f64<0x124>(x));
    x = fmax(x, ms_dpp_f64<0x122>(x));
    x = fmax(x, ms_dpp_f64<0x121>(x));
    const long long b = __double_as_longlong(x);
    const unsigned lo = (unsigned)b, hi = (unsigned)(b >> 32);
    const auto rl = __builtin_amdgcn_permlane16_swap(lo, lo, false, false);
    const auto rh = __builtin_amdgcn_permlane16_swap(hi, hi, false, false);
    x = fmax(__longlong_as_double(((long long)rh[0] << 32) | (unsigned long long)rl[0]),
             __longlong_as_double(((long long)rh[1] << 32) | (unsigned long long)rl[1]));
    const long long b2 = __double_as_longlong(x);
    const unsigned lo2 = (unsigned)b2, hi2 = (unsigned)(b2 >> 32);
    const auto sl = __builtin_amdgcn_permlane32_swap(lo2, lo2, false, false);
    const auto sh = __builtin_amdgcn_permlane32_swap(hi2, hi2, false, false);
    return fmax(__longlong_as_double(((long long)sh[0] << 32) | (unsigned long long)sl[0]),
                __longlong_as_double(((long long)sh[1] << 32) | (unsigned long long)sl[1]));
}

// Hansen renormalisation (hansen :200-233).  The reference keeps ONE fc array per scatterer for the whole
// call and hansen() updates it in place, so the factor found for (g, wave) is the starting point of the
// next (g, wave) in loop order (:780-815); the normalisation has no unique solution, so the result depends
// on that history (a 1e-4 effect on the radiance).  Reproduced: one wavefront per scatterer walks the
// (g outer, wave inner) sequence and stores fc[g][wave][comp][nmu*nmu].
// One wavefront per block: LDS instructions of a wave execute in order, so a compiler fence orders the lanes' LDS accesses.
// __syncthreads() also waits for every outstanding GLOBAL access (vmcnt(0)) -- here that is the prefetch of the matrices two
// steps ahead and the store of the factors, i.e. a full memory round trip in every step of a walk that is nothing but latency.
#define MS_WAVE_SYNC() __atomic_signal_fence(__ATOMIC_SEQ_CST)
template <int NMU>   // NMU = 16: compile-time size (unrolled sums, all LDS reads in flight); 0: any nmu <= kMsMaxMu
__global__ __launch_bounds__(64) void k_ms_hansen_seq(MsParams p)
{
    __shared__ double ppl_s[kMsMaxMu * kMsMaxMu], pmi_s[kMsMaxMu * kMsMaxMu], fc[kMsMaxMu * kMsMaxMu];
    __shared__ double rsum[kMsMaxMu], tsum[kMsMaxMu], xs[kMsMaxMu];
    // two waves on the whole chip walk while thousands of chain waves compute: the walk gates the chains of the next
    // g-ordinate, so its waves issue first wherever they share a SIMD
    __builtin_amdgcn_s_setprio(3);
    // with a pair list (per-model phase functions) block x walks a (variant, component) pair on the variant's matrices
    const int var = p.pairs ? p.pairs[2 * blockIdx.x] : 0;
    const int comp = p.pairs ? p.pairs[2 * blockIdx.x + 1] : blockIdx.x + p.hansen_comp0;
    const double *const vppl = p.ppl + (size_t)var * p.vstride, *const vpmi = p.pmi + (size_t)var * p.vstride;
    double *const vfc = p.fc + (size_t)var * p.vstride;
    const int n = NMU ? NMU : p.nmu, nn = n * n, tid = threadIdx.x;
    const double x1 = 2.0 * 3.141592653589793;
    const int nr = p.nmu_real ? p.nmu_real : n;              // the quadrature's size (a smaller one padded to 16 streams)
    constexpr int NE = NMU ? (NMU * NMU + 63) / 64 : (kMsMaxMu * kMsMaxMu + 63) / 64;   // matrix elements per lane
    // The walk is a chain of short steps (a converged start needs one pass over a 16 x 16 matrix) and every step needs two
    // matrices from HBM / L2: a microsecond away.  They are fetched kMsHansenDepth steps ahead into a ring of registers (the
    // loop is unrolled over the ring so that every slot is a fixed set of registers and the wait before a slot is used counts
    // the younger loads and stores still in flight instead of draining them); fetched ONE step ahead, as until round 3, the
    // step took the memory latency: 2.0-2.5 us, 20-25 ms per g-ordinate at 1e4 wavenumbers, which was the wall time of a C4
    // forward model (the chain kernels of g-ordinate ig wait for the factors of ig).
    constexpr int D = NMU ? kMsHansenDepth : 2;
    constexpr bool FULL = NMU != 0 && (NMU * NMU) % 64 == 0;     // every lane holds NE elements: no bounds tests on the accesses
    // a compile-time size that does not fill the lanes (5 x 5: the reference's default quadrature): the idle lanes repeat the
    // last element's access -- the same value to the same address -- so that the number of loads and stores stays fixed
    constexpr bool CLAMP = NMU != 0 && !FULL;
    double ring[D][2 * NE];
    auto fetch = [&](int d, int widx) {
        const double *gppl = vppl + (((size_t)widx * (p.nf + 1) + 0) * p.ncomp + comp) * nn;
        const double *gpmi = vpmi + (((size_t)widx * (p.nf + 1) + 0) * p.ncomp + comp) * nn;
#pragma unroll
        for (int r = 0; r < NE; ++r) {
            const int e = CLAMP ? min(tid + 64 * r, nn - 1) : tid + 64 * r;
            if (FULL || CLAMP || e < nn) { ring[d][r] = gppl[e]; ring[d][NE + r] = gpmi[e]; }
        }
    };
    auto stage = [&](int d) {
#pragma unroll
        for (int r = 0; r < NE; ++r) {
            const int e = CLAMP ? min(tid + 64 * r, nn - 1) : tid + 64 * r;
            if (FULL || CLAMP || e < nn) { ppl_s[e] = ring[d][r]; pmi_s[e] = ring[d][NE + r]; }
        }
    };
    // the walk of this launch: g-ordinates [ig0, ig0 + ng_launch) over the window's wavenumbers, continuing from the factors
    // the previous launch left for its last (g, wave) -- a launch per g-ordinate lets the chains of g run beside the walk of
    // g + 1; at G = 1 a launch per window, which continues from the carry of the previous window
    if (p.carry_in) {
        const double *pfc = p.carry + (size_t)comp * nn;
        for (int e = tid; e < nn; e += 64) fc[e] = pfc[e];
    } else if (p.ig0 == 0) { for (int e = tid; e < nn; e += 64) fc[e] = 1.0; }
    else {
        const double *pfc = vfc + (((size_t)(p.ig0 - 1) * p.nwin + (p.nwin - 1)) * p.ncomp + comp) * nn;
        for (int e = tid; e < nn; e += 64) fc[e] = pfc[e];
    }
    const long total = (long)p.ng_launch * p.nwin;
    const int sn = p.stn ? p.stn : p.nwin;
    int wf = 0;                                                 // wavenumber of the next fetch (wraps around: see below)
#pragma unroll
    for (int d = 0; d < D; ++d) { fetch(d, wf); if (++wf == p.nwin) wf = 0; }
    int ig = p.ig0, widx = 0;
    for (long iter0 = 0; iter0 < total; iter0 += D) {
#pragma unroll
    for (int d = 0; d < D; ++d) {
        const long iter = iter0 + d;
        if (iter >= total) break;
        const double *ppl = ppl_s, *pmi = pmi_s;
        stage(d);                                               // the previous step's readers are behind this wave's fence
        // always issued (beyond the end of the walk it re-reads a matrix that is there): a fetch under a condition leaves the
        // number of loads in flight unknown to the compiler, which then waits for all of them
        fetch(d, wf);
        if (++wf == p.nwin) wf = 0;
        MS_WAVE_SYNC();
        double rs = 0.0;
        if (tid < nr) {
            double s = 0.0;
#pragma unroll
            for (int i = 0; i < n; ++i) s += pmi[i * n + tid] * p.wtmu[i];
            rs = s * x1;
            rsum[tid] = rs;
        }
        for (int niter = 0; niter < 10000; ++niter) {
            double dev = 0.0;
            if (tid < nr) {
                double s = 0.0;
#pragma unroll
                for (int i = 0; i < n; ++i) s += ppl[i * n + tid] * p.wtmu[i] * fc[i * n + tid];
                const double ts = s * x1;
                tsum[tid] = ts;
                dev = fabs(rs + ts - 1.0);
            }
            dev = ms_wave_max(dev);                  // VALU lane exchanges (six dependent ds_bpermute stages before)
            MS_WAVE_SYNC();
            if (dev < 1e-14) break;
            if (tid < nr) xs[tid] = (1.0 - rsum[tid]) / tsum[tid];   // one division per column instead of two per element
            else if (tid < n) xs[tid] = 1.0;                         // columns beyond the quadrature keep their factor of 1
            MS_WAVE_SYNC();
            for (int e = tid; e < nn; e += 64) {
                const int i = e / n, j = e % n;
                if (i <= j) {
                    const double xj = xs[j], xi = xs[i];
                    const double v = 0.5 * (fc[i * n + j] * xj + fc[j * n + i] * xi);
                    fc[i * n + j] = v;
                    fc[j * n + i] = v;
                }
            }
            MS_WAVE_SYNC();
        }
        // outside the store range: the same store to the sink (an address select; the step's arithmetic does not change)
        const int ws = widx - p.st0;
        double *ofc = (unsigned)ws < (unsigned)sn ? vfc + (((size_t)ig * sn + ws) * p.ncomp + comp) * nn : p.sink + (size_t)comp * nn;
#pragma unroll
        for (int r = 0; r < NE; ++r) {           // a fixed number of stores per step (the waits before the ring's slots count them)
            const int e = CLAMP ? min(tid + 64 * r, nn - 1) : tid + 64 * r;
            if (FULL || CLAMP || e < nn) ofc[e] = fc[e];
        }
        if (++widx == p.nwin) { widx = 0; ++ig; }
        MS_WAVE_SYNC();
    }
    }
    if (p.carry) {                               // the last step's factors, bit for bit: the next window starts from them
        double *cfc = p.carry + (size_t)comp * nn;
        for (int e = tid; e < nn; e += 64) cfc[e] = fc[e];
    }
}

}  // namespace ansfm
